"""CahnHilliard on the host (no GPU): the numpy step against an independent high-precision solve that uses no transform
(tests/cahn_hilliard_reference.py: sparse LU start, iterative refinement in long double, its own forward error bound asserted), the
constructor, the device description, the package exports, the grid transfer, and the properties of the scheme (mass, energy, fixed points).

The tolerance of one Phi in the Hartley form, C(nx) EPS bnorm with C(nx) = 4 nx + 36, is derived in tests/cahn_hilliard_reference.py beside
the functions that evaluate it (c_of, d2max, b_norm); reference_phi gets EPS bnorm, its asserted forward error bound.
"""
import numpy as np
import pytest

import cases
from cahn_hilliard_reference import b_norm, c_of

EPS = cases.EPS


def apply_step(app, u, dt):
    from pymgrit_amd import VectorCahnHilliard2D
    v = VectorCahnHilliard2D(app.nx, app.nx)
    v.set_values(u)
    return np.asarray(app.step(v, 0.0, dt).get_values())      # (t_stop - t_start is dt bit for bit)


def energy(u, dx, eps):
    """dx^2 sum((u^2 - 1)^2 / 4 + eps^2 |forward differences / dx|^2 / 2), this module's own code"""
    gx, gy = (np.roll(u, -1, 0) - u) / dx, (np.roll(u, -1, 1) - u) / dx
    return float(dx * dx * np.sum(0.25 * (u * u - 1.0) ** 2 + 0.5 * eps ** 2 * (gx * gx + gy * gy)))


# (nx, eps, stab, dt): absrow(A) = 1 + dt (64 eps^2 nx^4 + 8 s nx^2) stays below 60, inside the reference's certificate
STEP_CASES = [(4, 0.2, 2.0, 1e-2), (4, 0.3, 0.0, 5e-3), (9, 0.1, 0.0, 2e-3), (9, 0.1, 2.0, 1e-3), (9, 0.08, 0.5, 2.5e-3),
              (16, 0.05, 2.0, 1e-3), (16, 0.05, 0.0, 2e-3), (16, 0.1, 1.0, 1.25e-4), (33, 0.04, 2.0, 2e-4), (33, 0.04, 0.0, 3e-4),
              (33, 0.03, 3.0, 1e-5)]


@pytest.mark.parametrize("nx,eps,stab,dt", STEP_CASES)
def test_host_step_matches_the_high_precision_solve(nx, eps, stab, dt):
    """CahnHilliard.step (Hartley table, lam_k, D1, D2) against reference_phi, which shares none of it: a wrong eigenvalue, mode order,
    table or sign shows here. norm_F(error) <= C(nx) EPS bnorm for the step + EPS bnorm for the reference."""
    from pymgrit_amd import CahnHilliard
    from cahn_hilliard_reference import reference_phi
    app = CahnHilliard(nx=nx, eps=eps, stab=stab, t_start=0, t_stop=1, nt=2)
    rng = np.random.default_rng(1000 * nx + int(100 * stab))
    inputs = [(f"uniform[-{a}, {a}]", rng.uniform(-a, a, size=(nx, nx))) for a in (1.0, 1.5)]
    inputs += [(f"constant {v}", np.full((nx, nx), v)) for v in (0.0, 0.5, -0.5)]
    inputs.append(("initial state", np.asarray(app.vector_t_start.get_values())))
    worst = 0.0
    for what, u in inputs:
        got, ref = apply_step(app, u, dt), reference_phi(u, dt, nx, eps, stab)
        err, tol = float(np.linalg.norm(got - ref)), (c_of(nx) + 1) * EPS * b_norm(app, u.ravel(), dt)
        worst = max(worst, err / tol if tol > 0 else 0.0)
        assert got.shape == (nx, nx) and got.dtype == np.float64 and err <= tol, (what, err, tol)
    print(f"RATIO host_step[nx={nx},eps={eps},stab={stab},dt={dt}]: worst error/allowed {worst:.4f}")


def test_reference_solve_satisfies_its_own_system():
    """the reference against a dense float64 solve of the matrix written out from the equation (a check of the reference's stencil code)"""
    from cahn_hilliard_reference import reference_phi
    nx, eps, stab, dt = 6, 0.15, 1.5, 3e-3
    n, inv_dx2 = nx * nx, float(nx) ** 2
    lap = np.zeros((n, n))
    for i in range(nx):
        for j in range(nx):
            p = i * nx + j
            lap[p, p] -= 4.0 * inv_dx2
            for q in (((i + 1) % nx) * nx + j, ((i - 1) % nx) * nx + j, i * nx + (j + 1) % nx, i * nx + (j - 1) % nx):
                lap[p, q] += inv_dx2
    u = np.random.default_rng(3).uniform(-1, 1, size=n)
    A = np.eye(n) + dt * (eps ** 2 * lap @ lap - stab * lap)
    want = np.linalg.solve(A, u + dt * lap @ (u ** 3 - (1 + stab) * u))
    got = reference_phi(u, dt, nx, eps, stab).ravel()
    assert np.linalg.norm(got - want) <= 64 * np.linalg.cond(A) * EPS * np.linalg.norm(want)


def test_constructor_defaults_and_refusals():
    from pymgrit_amd import CahnHilliard, VectorCahnHilliard2D
    app = CahnHilliard(t_start=0, t_stop=1e-3, nt=3)
    assert (app.nx, app.ny, app.eps, app.stab, app.L, app.mean, app.amplitude, app.method) == (64, 64, 0.05, 2.0, 1.0, 0.0, 0.1, 'IMEX')
    assert app.dx == 1.0 / 64 and isinstance(app.vector_template, VectorCahnHilliard2D) and isinstance(app.vector_t_start, VectorCahnHilliard2D)
    x = np.arange(64) / 64.0
    want = 0.1 * (np.cos(4 * np.pi * x[:, None]) * np.cos(2 * np.pi * x[None, :]) + 0.5 * np.sin(2 * np.pi * x[:, None]) * np.sin(6 * np.pi * x[None, :]))
    assert np.allclose(app.vector_t_start.get_values(), want, rtol=0, atol=1e-15)
    shifted = CahnHilliard(nx=8, L=2.0, mean=0.25, amplitude=0.5, t_start=0, t_stop=1e-3, nt=3)
    assert shifted.dx == 0.25 and abs(np.mean(shifted.vector_t_start.get_values()) - 0.25) <= 4 * EPS
    grid = dict(t_start=0, t_stop=1e-3, nt=3)
    for bad, match in ((dict(method='IMPL'), "Unknown method"), (dict(method='CN'), "Unknown method"), (dict(eps=0.0), "eps=.*positive"),
                       (dict(eps=-0.1), "eps=.*positive"), (dict(stab=-1e-3), "stab=.*negative"), (dict(nx=3), "nx=3"),
                       (dict(eps=float("nan")), "finite"), (dict(stab=float("inf")), "finite"), (dict(L=float("inf")), "finite"),
                       (dict(mean=float("nan")), "finite"), (dict(amplitude=float("inf")), "finite"), (dict(L=0.0), "L=.*positive")):
        with pytest.raises(Exception, match=match):
            CahnHilliard(**bad, **grid)
    assert CahnHilliard(nx=4, stab=0.0, **grid).stab == 0.0


def test_device_description():
    from pymgrit_amd import CahnHilliard
    app = CahnHilliard(nx=12, eps=0.1, stab=1.5, L=3.0, t_start=0, t_stop=1e-3, nt=3)
    d = app.device_stepper()
    assert d == {"kind": "cahnhilliard2d", "n": 144, "nx": 12, "inv_dx2": 1.0 / app.dx ** 2, "eps2": 0.1 ** 2, "stab": 1.5}
    assert app.dx == 0.25 and sorted(d) == ["eps2", "inv_dx2", "kind", "n", "nx", "stab"]


def test_package_exports():
    import pymgrit_amd
    from pymgrit_amd.core import hip_lib
    for name in ("CahnHilliard", "VectorCahnHilliard2D", "GridTransferCahnHilliard"):
        assert name in pymgrit_amd.__all__ and hasattr(pymgrit_amd, name)
    assert hip_lib.STEPPER_CAHNHILLIARD2D == 7 and "mgrit_hip_level_cahnhilliard2d" in hip_lib.EXPORTS
    assert pymgrit_amd.GridTransferCahnHilliard().device_transfer() == hip_lib.TRANSFER_PERIODIC2D


def test_vector_arithmetic():
    from pymgrit_amd import VectorCahnHilliard2D
    a, b = VectorCahnHilliard2D(3, 3), VectorCahnHilliard2D(3, 3)
    a.set_values(np.arange(9.0).reshape(3, 3)); b.set_values(np.ones((3, 3)))
    assert np.array_equal((a + b).get_values(), np.arange(1.0, 10.0).reshape(3, 3)) and np.array_equal((a - b * 2.0).get_values(), np.arange(9.0).reshape(3, 3) - 2)
    assert a.norm() == np.linalg.norm(np.arange(9.0)) and np.array_equal(a.clone_zero().get_values(), np.zeros((3, 3)))
    c = a.clone(); c.unpack(a.pack() * 2)
    assert isinstance(c, VectorCahnHilliard2D) and np.array_equal(a.get_values(), np.arange(9.0).reshape(3, 3))
    assert a.clone_rand().get_values().shape == (3, 3)


@pytest.mark.parametrize("nc", [2, 5, 8])
def test_grid_transfer_has_the_arithmetic_of_the_allen_cahn_transfer(nc):
    from pymgrit_amd import GridTransferAllenCahn, GridTransferCahnHilliard, VectorAllenCahn2D, VectorCahnHilliard2D
    rng = np.random.default_rng(nc)
    fine, coarse = rng.uniform(-1, 1, size=(2 * nc, 2 * nc)), rng.uniform(-1, 1, size=(nc, nc))
    ours, theirs = GridTransferCahnHilliard(), GridTransferAllenCahn()
    for values, method in ((fine, "restriction"), (coarse, "interpolation")):
        a, b = VectorCahnHilliard2D(*values.shape), VectorAllenCahn2D(*values.shape)
        a.set_values(values.copy()); b.set_values(values.copy())
        got, want = getattr(ours, method)(a), getattr(theirs, method)(b)
        assert isinstance(got, VectorCahnHilliard2D) and (got.nx, got.ny) == np.shape(want.get_values())
        assert np.array_equal(got.get_values(), want.get_values())
    # full weighting and bilinear interpolation keep the mean of a periodic grid
    a = VectorCahnHilliard2D(2 * nc, 2 * nc); a.set_values(fine)
    assert abs(np.mean(ours.restriction(a).get_values()) - np.mean(fine)) <= 8 * EPS
    with pytest.raises(Exception, match="even periodic fine grids"):
        odd = VectorCahnHilliard2D(5, 5)
        ours.restriction(odd)


# the parameter sets the scheme was checked with before it was built: (nx, eps, stab, dt)
SCHEME_CASES = [(16, 0.05, 2.0, 1e-3), (33, 0.04, 2.0, 5e-4), (20, 0.05, 0.0, 1e-5), (12, 0.1, 2.0, 1e-2)]


@pytest.mark.parametrize("nx,eps,stab,dt", SCHEME_CASES)
def test_mass_is_conserved_and_energy_does_not_increase(nx, eps, stab, dt):
    """40 steps from the initial state, the product's step and the reference's solve side by side. The mean: mode (0, 0) has D1 = 1 and
    D2 = 0, so a step moves it by the rounding of the products only, C(nx) EPS bnorm / nx per step (norm_F / nx bounds the mean);
    the reference solves a system whose right-hand side dt Lh w has mean zero to rounding. The energy: the stabilised splitting is
    energy-stable for these sets (stab = 0 with dt = 1e-5 included); an increase beyond the rounding of the energy's own sum fails."""
    from pymgrit_amd import CahnHilliard
    from cahn_hilliard_reference import reference_solve
    app = CahnHilliard(nx=nx, eps=eps, stab=stab, t_start=0, t_stop=1, nt=2)
    u0 = np.asarray(app.vector_t_start.get_values())
    for name, phi in (("step", lambda u: apply_step(app, u, dt)), ("reference", lambda u: reference_solve(u, dt, nx, eps, stab)[0])):
        u, e, drift = u0.copy(), energy(u0, app.dx, eps), 0.0
        for k in range(1, 41):
            per_phi = (c_of(nx) + 1) * EPS * b_norm(app, u.ravel(), dt) / nx
            u = phi(u)
            drift += per_phi
            assert abs(np.mean(u) - np.mean(u0)) <= drift, (name, k, np.mean(u) - np.mean(u0), drift)
            e_new = energy(u, app.dx, eps)
            assert e_new <= e + nx * nx * EPS * e, (name, k, e_new - e)
            e = e_new
        assert e < energy(u0, app.dx, eps)
        print(f"{name}[nx={nx}]: mean drift {abs(np.mean(u) - np.mean(u0)):.2e} (allowed {drift:.2e}), energy {energy(u0, app.dx, eps):.6f} -> {e:.6f}")


@pytest.mark.parametrize("nx", [4, 9, 16])
def test_constants_are_fixed_points_and_zero_stays_zero(nx):
    """a constant has w constant, Lh w = 0: only mode (0, 0) is non-zero, D1 = 1 there and D2 = 0. u = 0 gives exact zeros"""
    from pymgrit_amd import CahnHilliard
    app = CahnHilliard(nx=nx, t_start=0, t_stop=1, nt=2)
    for c in (0.5, -0.5, 1.0, 0.3):
        u = np.full((nx, nx), c)
        assert np.linalg.norm(apply_step(app, u, 1e-3) - u) <= (c_of(nx) + 1) * EPS * b_norm(app, u.ravel(), 1e-3)
    out = apply_step(app, np.zeros((nx, nx)), 1e-3)
    assert np.array_equal(out, np.zeros((nx, nx)))


def test_three_level_hierarchy_converges_on_the_plugin_path():
    from pymgrit_amd import CahnHilliard, Mgrit

    class HostCahnHilliard(CahnHilliard):     # overriding step sends the hierarchy to the plugin path
        def step(self, u_start, t_start, t_stop):
            return super().step(u_start, t_start, t_stop)
    mg = Mgrit([HostCahnHilliard(nx=16, t_start=0, t_stop=0.04, nt=nt) for nt in (65, 17, 5)], logging_lvl=30, max_iter=8, tol=0.0)
    assert type(mg.backend).__name__ == "PluginBackend"
    conv = np.asarray(mg.solve()["conv"])
    assert len(conv) == 8 and conv[-1] <= 1e-9 * conv[0], conv
