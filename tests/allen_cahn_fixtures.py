"""The recorded Allen-Cahn steps and solves (tests/golden/allen_cahn.*, written by tests/golden/make_golden_allen_cahn.py) and the bounds
the CPU and the GPU tests hold a step against them with. A plain helper like cases.py: no tests, no fixtures of pytest.

Tolerances of an IMEX step, none of them measured on the code under test:
  * ours: a product with an orthogonal n x n matrix is off by at most n eps (1 - n eps)^-1 times the vector's 2-norm, the spectral scale
    is <= 1, so four products give  norm_F(error) <= (4 nx + 8) eps norm_F(b)  per Phi (the 8: pointwise right-hand side and scale);
  * the reference's SuperLU solve: forward error <= cond * rho, cond = 1 + 8 dt / dx^2 (exact for I - dt L), rho its own relative
    residual as recorded in the fixture; allowed: 4 * cond * rho * norm_inf(x_ref);
  * reference_phi (allen_cahn_reference.py): EPS norm_F(b), the rounding of its long-double solution to float64.
"""
import numpy as np

import cases

META = cases.load_json("allen_cahn.json")
ARR = np.load(cases.GOLDEN + "/allen_cahn.npz")
EPS = cases.EPS


def ours_bound(app, u, dt):
    """(4 nx + 8) eps norm_F(b), b the right-hand side of the implicit solve"""
    b = u + dt / app.eps ** 2 * u * (1.0 - u ** app.nu)
    return (4 * app.nx + 8) * EPS * float(np.linalg.norm(b))


def step_input(app, rec):
    return np.asarray(app.initial_guess().get_values()) if rec["src"] == "init" else ARR[f"rand_nx{rec['nx']}"]


def reference_bound(rec, x_ref):
    cond = 1.0 + 8.0 * rec["dt"] * rec["nx"] ** 2
    return 4.0 * cond * rec["rho"] * float(np.abs(x_ref).max())


def apply_step(app, u, dt):
    from pymgrit_amd import VectorAllenCahn2D
    vec = VectorAllenCahn2D(app.nx, app.ny)
    vec.set_values(np.array(u, dtype=np.float64))
    return np.asarray(app.step(vec, 0.0, dt).get_values())


def check_history(name, conv, norm_u, ref=None):
    """|conv - reference| <= 1e-10 * reference + BLK_K * eps * norm(u) (tests/cases.py: histories whose Phi passes through SuperLU on
    the reference side); prints the multiple of eps * norm(u) each history needs. ref: the recorded history, META["solve"][name]["conv"]
    unless another record is given"""
    ref = np.asarray(META["solve"][name]["conv"] if ref is None else ref)
    assert len(conv) == len(ref), (name, conv, ref)
    dev = np.abs(np.asarray(conv) - ref)
    unit = EPS * norm_u
    print(f"{name}: largest deviation {np.max(dev / unit):.2f} units of eps*norm(u); beyond 1e-10 relative: "
          f"{np.max(np.maximum(dev - 1e-10 * ref, 0.0) / unit):.2f}")
    assert np.all(dev <= 1e-10 * ref + cases.BLK_K * unit), (name, conv, ref)
