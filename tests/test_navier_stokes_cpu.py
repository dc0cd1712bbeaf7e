"""NavierStokes2D on the host (no GPU): the IMEX step against an independent high-precision Phi that uses no transform
(tests/navier_stokes_reference.py: a bordered sparse solve for the stream function, the stencil in long double, the diffusion solve of
gray_scott_reference.solve_plane), the known answers of the scheme, the condition of the inputs, a plugin-path solve, the refusals, the
device description, the transfer and the exports.

The tolerance of one IMEX step, (C(nx) + ALLOWANCE) EPS M with C(nx) = 4 nx + 17 and the majorant M = M1 + M2, is derived in
tests/navier_stokes_reference.py beside the functions that evaluate it (C, lam_1, majorant); kolmogorov, the forcing of the tests, is there too.
"""
import logging

import numpy as np
import pytest

import cases
from navier_stokes_reference import ALLOWANCE, LD, C, kolmogorov, lam_1, majorant, reference_phi, right_hand_side, stream_function

EPS = cases.EPS


def make(nx, cls=None, **kw):
    from pymgrit_amd import NavierStokes2D
    kw.setdefault("t_start", 0), kw.setdefault("t_stop", 1), kw.setdefault("nt", 2)
    kw.setdefault("L", nx / 16)      # dx = 1 / 16 for every nx
    return (cls or NavierStokes2D)(nx=nx, **kw)


def apply_step(app, w, dt):
    from pymgrit_amd import VectorNavierStokes2D
    vec = VectorNavierStokes2D(app.nx, app.nx)
    vec.set_values(np.array(w, dtype=np.float64).reshape(app.nx, app.nx))
    return np.asarray(app.step(vec, 0.0, dt).get_values())


REF_NX = [4, 12, 33, 66]
NU, DT = 0.1, 1e-3
# name: (forcing, mean added)
REF_CASES = {"plain": (False, 0.0), "forcing": (True, 0.0), "mean 5": (False, 5.0), "forcing, mean 5": (True, 5.0)}


@pytest.mark.parametrize("nx", REF_NX)
def test_host_imex_step_matches_the_high_precision_phi(nx):
    """_step_imex (Hartley table, lam_k, the tables S and D, the float64 stencil) against reference_phi, which shares none of it: a
    wrong eigenvalue, swapped axes, a wrong sign of the Jacobian or a mean that reaches psi shows here"""
    rng = np.random.default_rng(1000 * nx)
    worst = 0.0
    for what, (forced, mean) in REF_CASES.items():
        f = kolmogorov(nx) if forced else None
        app = make(nx, nu=NU, forcing=f)
        assert DT * NU / app.dx ** 2 <= 50      # inside the reference solver's certificate
        w = rng.uniform(-1.0, 1.0, size=(nx, nx)) + mean
        got, ref = apply_step(app, w, DT), reference_phi(w, DT, nx, NU, app.L, f)
        assert got.shape == ref.shape == (nx, nx)
        err, tol = float(np.linalg.norm(got - ref)), (C(nx) + ALLOWANCE) * EPS * majorant(w, DT, nx, app.L, f)
        worst = max(worst, err / tol)
        print(f"RATIO host_imex[nx={nx}] {what}: error/allowed {err / tol:.4f}")
        assert err <= tol, (nx, what, err, tol)
    print(f"RATIO host_imex[nx={nx}]: worst error/allowed {worst:.4f}")


@pytest.mark.parametrize("nx", REF_NX + [6])
def test_inputs_are_conditioned_to_show_the_jacobian(nx):
    """from the reference's numbers alone: the transport term moves the state by at least 1000 times the relative per-Phi tolerance,
    norm(b - w) / norm(w) >= 1000 (C(nx) + ALLOWANCE) EPS M / norm(w), at the smallest step the GPU tests take (2.5e-4) and at this
    file's. A wrong sign or a swapped axis of the Jacobian changes b - w by its own size and misses by orders of magnitude"""
    rng = np.random.default_rng(2000 + nx)
    w = rng.uniform(-1.0, 1.0, size=(nx, nx))
    L = nx / 16
    for dt in (2.5e-4, DT):
        moved = float(np.linalg.norm((right_hand_side(w, dt, nx, L) - w.astype(LD)).astype(np.float64))) / float(np.linalg.norm(w))
        rel_tol = (C(nx) + ALLOWANCE) * EPS * majorant(w, dt, nx, L) / float(np.linalg.norm(w))
        print(f"RATIO condition[nx={nx},dt={dt}]: moved {moved:.3e}, relative tolerance {rel_tol:.3e}, quotient {moved / rel_tol:.3e}")
        assert moved >= 1000 * rel_tol, (nx, dt, moved, rel_tol)


@pytest.mark.parametrize("nx", [12, 33])
def test_taylor_green_decays_by_the_discrete_factor(nx):
    """w = 2 cos(k X) cos(k Y): an eigenfunction of the discrete Laplacian, psi = w / mu_k, so the discrete Jacobian of psi and w is
    that of w with itself: 0 to rounding. One step multiplies w by 1 / (1 + dt nu mu_k), mu_k = 2 (4 / dx^2) sin^2(pi k / nx) -- written
    here from the stencil, not taken from the application's eigenvalue function. The yardstick is exact up to a few EPS of |w|: the
    tolerance is the per-Phi bound"""
    k = 2
    app = make(nx, nu=NU)
    X = 2 * np.pi * np.arange(nx) / nx
    w = 2.0 * np.cos(k * X)[:, None] * np.cos(k * X)[None, :]
    mu_k = 2.0 * (4.0 / app.dx ** 2) * np.sin(np.pi * k / nx) ** 2
    got = apply_step(app, w, DT)
    want = w / (1.0 + DT * NU * mu_k)
    err, tol = float(np.linalg.norm(got - want)), (C(nx) + ALLOWANCE) * EPS * majorant(w, DT, nx, app.L)
    print(f"RATIO taylor_green[nx={nx}]: error/allowed {err / tol:.4f}")
    assert err <= tol, (err, tol)
    assert float(np.linalg.norm(want - w)) > 1e3 * tol      # (the step moves the state by far more than the bound)


@pytest.mark.parametrize("nx", [4, 33])
def test_a_state_depending_on_y_only_is_only_diffused(nx):
    """w = g(y): psi depends on y only up to the products' rounding, so px and wx are rounding and J = 0 within the bound. The step is
    the reference's step of the same state, and the result stays independent of x within the bound while the diffusion moves it by far
    more. A Jacobian that pairs py with wy (a swapped axis in one factor) is far from zero for this state"""
    app = make(nx, nu=NU)
    g = np.random.default_rng(nx).uniform(-1.0, 1.0, size=nx)
    w = np.repeat(g[None, :], nx, axis=0)
    got, ref = apply_step(app, w, DT), reference_phi(w, DT, nx, NU, app.L)
    tol = (C(nx) + ALLOWANCE) * EPS * majorant(w, DT, nx, app.L)
    err = float(np.linalg.norm(got - ref))
    print(f"RATIO y_only[nx={nx}]: error/allowed {err / tol:.4f}")
    assert err <= tol, (err, tol)
    assert float(np.linalg.norm(got - got[:1, :])) <= tol
    assert float(np.linalg.norm(got - w)) > 1e3 * tol


@pytest.mark.parametrize("nx", [4, 33])
def test_constant_state_is_a_fixed_point(nx):
    """w = 5: T w T has mode (0, 0) only up to the products' rounding, S[0][0] = 0 removes it: psi is rounding of size EPS |w| / lam_1,
    b = w within M2's reach, mode 0 has D = 1: Phi(w) = w within the per-Phi bound. A mean that reached psi through a non-zero S[0][0]
    would still give J = 0; what this pins is that S[0][0] is finite (1 / 0 = inf would poison the plane) and D[0][0] = 1"""
    app = make(nx, nu=NU)
    w = np.full((nx, nx), 5.0)
    app._tables()
    assert app._sinv()[0, 0] == 0.0 and np.all(np.isfinite(app._sinv()))
    got = apply_step(app, w, DT)
    assert np.all(np.isfinite(got))
    err, tol = float(np.linalg.norm(got - w)), C(nx) * EPS * majorant(w, DT, nx, app.L)
    print(f"RATIO fixed_point[nx={nx}]: error/allowed {err / tol:.4f}")
    assert err <= tol, (err, tol)


def test_the_mean_does_not_enter_the_stream_function():
    """psi(w + 5) = psi(w) within the products' rounding on the mean: 4 nx EPS norm_F(w + 5) / lam_1"""
    nx = 12
    app = make(nx, nu=NU)
    w = np.random.default_rng(4).uniform(-1.0, 1.0, size=(nx, nx))
    a, b = app.stream_function(w), app.stream_function(w + 5.0)
    tol = (4 * nx + 7) * EPS * float(np.linalg.norm(w + 5.0)) / lam_1(nx, app.L)
    assert float(np.linalg.norm(a - b)) <= 2 * tol
    assert abs(float(np.mean(a))) <= tol
    ref = stream_function(w, nx, app.L).astype(np.float64)
    assert float(np.linalg.norm(a - ref)) <= tol + EPS * float(np.linalg.norm(ref))


def test_right_hand_side_of_the_reference_is_the_formula():
    """the long-double b at one point, written out: axis 0 is x, u = psi_y multiplies the x difference of w"""
    nx, L, dt = 5, 5 / 16, 1e-3
    w = np.random.default_rng(3).uniform(-1.0, 1.0, size=(nx, nx))
    f = kolmogorov(nx)
    psi = stream_function(w, nx, L)
    b = right_hand_side(w, dt, nx, L, f)
    two_dx = LD(2) * LD(L) / LD(nx)
    i, j = 4, 0      # both wraps
    px, py = (psi[0][j] - psi[3][j]) / two_dx, (psi[i][1] - psi[i][4]) / two_dx
    wx, wy = (LD(w[0][j]) - LD(w[3][j])) / two_dx, (LD(w[i][1]) - LD(w[i][4])) / two_dx
    assert b[i][j] == LD(w[i][j]) - LD(dt) * (py * wx - px * wy) + LD(dt) * LD(f[i][j])
    # and psi solves the Poisson equation at that point, by the stencil written out
    lap = (psi[0][j] + psi[3][j] + psi[i][1] + psi[i][4] - LD(4) * psi[i][j]) / (LD(L) / LD(nx)) ** 2
    assert abs(float(lap + (LD(w[i][j]) - np.sum(w.astype(LD)) / LD(nx * nx)))) <= 8 * EPS


def _host_class():
    from pymgrit_amd import NavierStokes2D

    class HostNavierStokes2D(NavierStokes2D):     # overriding step sends the hierarchy to the plugin path
        def step(self, u_start, t_start, t_stop):
            return super().step(u_start, t_start, t_stop)
    return HostNavierStokes2D


def test_plugin_path_solve_converges_to_sequential_time_stepping():
    """two levels, nx = 12, nt = 17 (coarsening by 2): the residual falls below 1e-10 and the result is the sequential solution -- the
    fixed point of MGRIT -- within the residual's reach: the last C-point's error is at most the sum of the residuals amplified by the
    steps' Lipschitz factors, far below 1e-8 for a residual below 1e-10 on 16 steps of this mild flow"""
    from pymgrit_amd import Mgrit
    nx = 12
    logging.disable(logging.WARNING)
    try:
        mg = Mgrit([make(nx, cls=_host_class(), nu=0.05, L=2 * np.pi, forcing=0.1 * kolmogorov(nx), t_stop=1.0, nt=nt) for nt in (17, 9)],
                   tol=1e-10, max_iter=15, logging_lvl=30)
        assert type(mg.backend).__name__ == "PluginBackend"
        conv = np.asarray(mg.solve()["conv"])
    finally:
        logging.disable(logging.NOTSET)
    print(f"plugin solve: {len(conv)} iterations, conv {conv}")
    assert len(conv) < 15 and conv[-1] < 1e-10, conv
    app = mg.problem[0]
    u = app.vector_t_start
    seq = [np.asarray(u.get_values())]
    for a, z in zip(mg.t[0][:-1], mg.t[0][1:]):
        u = app.step(u, a, z)
        seq.append(np.asarray(u.get_values()))
    dev = max(float(np.linalg.norm(np.asarray(v.get_values()) - s)) for v, s in zip(mg.u[0], seq))
    print(f"RATIO plugin_solve: deviation from time stepping {dev:.3e} (allowed 1e-8)")
    assert dev <= 1e-8, dev
    assert float(np.linalg.norm(seq[-1] - seq[0])) > 1e-2      # (the flow moved)


def test_vector_interface():
    from pymgrit_amd import Vector, VectorNavierStokes2D
    nx = 5
    rng = np.random.default_rng(0)
    a, b = VectorNavierStokes2D(nx, nx), VectorNavierStokes2D(nx, nx)
    va, vb = rng.normal(size=(nx, nx)), rng.normal(size=(nx, nx))
    a.set_values(va.copy()), b.set_values(vb.copy())
    assert isinstance(a, Vector) and a.get_values().shape == (nx, nx)
    assert np.array_equal((a + b).get_values(), va + vb) and np.array_equal((a - b).get_values(), va - vb)
    assert np.array_equal((a * 2.5).get_values(), va * 2.5)
    assert a.norm() == np.linalg.norm(va.ravel())
    c = a.clone()
    c.get_values()[0, 0] += 1.0
    assert np.array_equal(a.get_values(), va)            # a clone owns its values
    z = a.clone_zero()
    assert isinstance(z, VectorNavierStokes2D) and z.get_values().shape == (nx, nx) and not z.get_values().any()
    r = a.clone_rand()
    assert r.get_values().shape == (nx, nx) and 0.0 <= r.get_values().min() and r.get_values().max() < 1.0
    z.unpack(np.asarray(a.pack()).copy())
    assert np.array_equal(z.get_values(), va)


def test_initial_guess_has_a_jacobian():
    """two wavenumber shells: the first step's transport term is far from zero (a single shell would give J = 0)"""
    nx = 16
    app = make(nx, L=2 * np.pi)
    w = np.asarray(app.vector_t_start.get_values())
    assert w.shape == (nx, nx)
    moved = (right_hand_side(w, 1.0, nx, app.L) - w.astype(LD)).astype(np.float64)      # dt = 1: -J
    assert float(np.linalg.norm(moved)) > 0.05 * float(np.linalg.norm(w))
    X = 2 * np.pi * np.arange(nx) / nx
    shell = np.cos(X)[:, None] * np.cos(X)[None, :]
    none = (right_hand_side(shell, 1.0, nx, app.L) - shell.astype(LD)).astype(np.float64)
    assert float(np.linalg.norm(none)) < 1e-12 * float(np.linalg.norm(shell))


def test_constructor_defaults_and_refusals():
    from pymgrit_amd import NavierStokes2D
    app = NavierStokes2D(t_start=0, t_stop=0.5, nt=3)
    assert (app.nx, app.nu, app.L, app.method, app.forcing) == (32, 1e-2, 2 * np.pi, "IMEX", None)
    assert app.dx == 2 * np.pi / 32 and app.inv_2dx == 1.0 / (2.0 * app.dx)
    with pytest.raises(Exception, match="Unknown method 'nope'"):
        make(8, method="nope")
    for bad in (3, 0, -4, 8.5):
        with pytest.raises(Exception, match="nx"):
            make(bad, L=1.0)
    for bad in (dict(nu=0.0), dict(nu=-1.0), dict(nu=float("nan")), dict(nu=float("inf")), dict(L=0.0), dict(L=-1.0), dict(L=float("inf"))):
        with pytest.raises(Exception, match="nu and L"):
            make(8, **bad)
    nan = np.zeros((8, 8))
    nan[3, 4] = np.nan
    for bad in (np.zeros((8, 7)), np.zeros(64), nan, "no", lambda x, y: np.zeros(3)):
        with pytest.raises(Exception, match="forcing"):
            make(8, forcing=bad)
    assert make(4).nx == 4 and make(8.0).nx == 8
    # a callable is evaluated once on the grid, axis 0 = x; a function of y alone broadcasts
    app = make(8, L=2.0, forcing=lambda x, y: np.sin(np.pi * x) + 2.0 * y)
    for i in range(8):
        for j in range(8):
            assert app.forcing[i, j] == np.sin(np.pi * i * 0.25) + 2.0 * (j * 0.25)
    assert make(8, forcing=lambda x, y: np.cos(y)).forcing.shape == (8, 8)
    given = np.arange(64.0).reshape(8, 8)
    app = make(8, forcing=given)
    given[0, 0] = 99.0
    assert app.forcing[0, 0] == 0.0      # the application keeps its own copy


def test_device_description():
    app = make(20, nu=0.05)
    assert app.device_stepper() == {"kind": "navierstokes2d", "n": 400, "nx": 20, "inv_dx2": 1.0 / app.dx ** 2,
                                    "inv_2dx": 1.0 / (2.0 * app.dx), "nu": 0.05, "forcing": None}
    f = kolmogorov(20)
    d = make(20, forcing=f).device_stepper()
    assert np.array_equal(d["forcing"], f) and d["forcing"].flags["C_CONTIGUOUS"] and d["forcing"].dtype == np.float64


def test_grid_transfer_is_the_allen_cahn_arithmetic():
    from pymgrit_amd import GridTransferAllenCahn, GridTransferNavierStokes, VectorAllenCahn2D, VectorNavierStokes2D
    from pymgrit_amd.core import hip_lib
    rng = np.random.default_rng(8)
    ns, ac = GridTransferNavierStokes(), GridTransferAllenCahn()
    assert ns.device_transfer() == hip_lib.TRANSFER_PERIODIC2D == ac.device_transfer()
    for nf in (4, 12, 66):
        fine, coarse = rng.uniform(-1.0, 1.0, size=(nf, nf)), rng.uniform(-1.0, 1.0, size=(nf // 2, nf // 2))
        for method, plane in (("restriction", fine), ("interpolation", coarse)):
            a, b = VectorNavierStokes2D(*plane.shape), VectorAllenCahn2D(*plane.shape)
            a.set_values(plane.copy()), b.set_values(plane.copy())
            got, want = getattr(ns, method)(a), getattr(ac, method)(b)
            assert isinstance(got, VectorNavierStokes2D)
            assert np.array_equal(got.get_values(), want.get_values()), (nf, method)
    odd = VectorNavierStokes2D(5, 5)
    with pytest.raises(Exception, match="GridTransferAllenCahn restricts even periodic fine grids"):
        ns.restriction(odd)


def test_package_exports():
    import pymgrit_amd
    from pymgrit_amd.core import hip_lib
    from pymgrit_amd.core.backend_hip import PERIODIC_2D
    for name in ("NavierStokes2D", "VectorNavierStokes2D", "GridTransferNavierStokes"):
        assert name in pymgrit_amd.__all__ and hasattr(pymgrit_amd, name)
    assert hip_lib.STEPPER_NAVIERSTOKES2D == 9 and "mgrit_hip_level_navierstokes2d" in hip_lib.EXPORTS
    assert PERIODIC_2D["navierstokes2d"][0] == "Navier-Stokes" and PERIODIC_2D["navierstokes2d"][2] is False
    from pymgrit_amd.navier_stokes.navier_stokes import NavierStokes2D
    assert pymgrit_amd.NavierStokes2D is NavierStokes2D
