"""AllenCahn on the host (no GPU): the three steppers against steps recorded from the reference (tests/golden/allen_cahn.*, written by
tests/golden/make_golden_allen_cahn.py), the Hartley table, the plugin-path solves against the reference's residual histories, the
device description and the package exports; and the host IMEX step against an independent high-precision solve that uses no transform
(tests/allen_cahn_reference.py: sparse LU start, iterative refinement in long double), itself checked against the recorded steps.

The tolerances of an IMEX step are derived in tests/allen_cahn_fixtures.py, which holds the recorded steps and the bounds the GPU
tests share.
"""
import logging

import numpy as np
import pytest

import cases
from allen_cahn_fixtures import ARR, EPS, META, apply_step, check_history, ours_bound, reference_bound, step_input


@pytest.mark.parametrize("name", sorted(META["steps"]))
def test_imex_step_matches_the_reference(name):
    from pymgrit_amd import AllenCahn
    rec = META["steps"][name]
    app = AllenCahn(nx=rec["nx"], nu=rec["nu"], eps=rec["eps"], method="IMEX", t_start=0, t_stop=1, nt=2)
    u, ref = step_input(app, rec), ARR["out_" + name]
    got = apply_step(app, u, rec["dt"])
    err, tol = float(np.abs(got - ref).max()), reference_bound(rec, ref) + ours_bound(app, u, rec["dt"])
    print(f"{name}: err {err:.3e} allowed {tol:.3e} ({err / (EPS * (1 + 8 * rec['dt'] * rec['nx'] ** 2)):.1f} eps*cond)")
    assert got.shape == ref.shape and err <= tol, (name, err, tol)


@pytest.mark.parametrize("name", sorted(META["steps"]))
def test_reference_phi_matches_the_recorded_steps(name):
    """the transform-free long-double solve against the reference's recorded SuperLU steps: the recorded side's own bound plus
    EPS norm_F(b) for the rounding of reference_phi's result"""
    from pymgrit_amd import AllenCahn
    from allen_cahn_reference import reference_phi
    rec = META["steps"][name]
    app = AllenCahn(nx=rec["nx"], nu=rec["nu"], eps=rec["eps"], method="IMEX", t_start=0, t_stop=1, nt=2)
    u, ref = step_input(app, rec), ARR["out_" + name]
    got = reference_phi(u, rec["dt"], rec["nx"], rec["nu"], rec["eps"])
    b = u + rec["dt"] / rec["eps"] ** 2 * u * (1.0 - u ** rec["nu"])
    err, tol = float(np.abs(got - ref).max()), reference_bound(rec, ref) + EPS * float(np.linalg.norm(b))
    print(f"{name}: err {err:.3e} allowed {tol:.3e}")
    assert got.shape == ref.shape and got.dtype == np.float64 and err <= tol, (name, err, tol)


REF_NX = [4, 9, 20, 33, 63, 64, 66, 96, 97, 129, 130, 200]   # the smallest grid, K steps and tiles of the device product +- 1, KP < P (96)
REF_DT = [1.25e-4, 3.1e-4, 1e-3]


@pytest.mark.parametrize("nu", [1, 2, 3, 4])
@pytest.mark.parametrize("nx", REF_NX)
def test_host_imex_step_matches_the_high_precision_solve(nx, nu):
    """_step_imex (Hartley table, lam_k, T((TbT) o D)T) against reference_phi, which shares none of it: a wrong eigenvalue, mode order
    or reaction term for this nu shows here. norm_F(error) <= (4 nx + 8) EPS norm_F(b) for the step + EPS norm_F(b) for the reference."""
    from pymgrit_amd import AllenCahn
    from allen_cahn_reference import reference_phi
    app = AllenCahn(nx=nx, nu=nu, method="IMEX", t_start=0, t_stop=1, nt=2)
    rng = np.random.default_rng(1000 * nx + nu)
    worst = 0.0
    for dt in REF_DT:
        inputs = [(f"uniform[-{a}, {a}]", rng.uniform(-a, a, size=(nx, nx))) for a in (1.0, 1.5)]
        inputs += [(f"constant {v}", np.full((nx, nx), v)) for v in (0.0, 1.0, -1.0)]
        for what, u in inputs:
            got, ref = apply_step(app, u, dt), reference_phi(u, dt, nx, nu, app.eps)
            b_norm = float(np.linalg.norm(u + dt / app.eps ** 2 * u * (1.0 - u ** nu)))
            err, tol = float(np.linalg.norm(got - ref)), ours_bound(app, u, dt) + EPS * b_norm
            ratio = err / tol if tol > 0.0 else 0.0
            worst = max(worst, ratio)
            print(f"nx={nx} nu={nu} dt={dt} {what}: error/bound {ratio:.4f}")
            assert got.shape == ref.shape == (nx, nx) and err <= tol, (nx, nu, dt, what, err, tol)
            if what.startswith("constant") and (u[0, 0] >= 0.0 or nu % 2 == 0):
                # constants are mode 0 with D = 1, and u (1 - u^nu) = 0 at 0, at 1 and (even nu) at -1: Phi(u) = b = u
                assert np.array_equal(ref, u), (nx, nu, dt, what)
    print(f"nx={nx} nu={nu}: worst error/bound {worst:.4f}")


@pytest.mark.parametrize("name", sorted(META["newton_steps"]))
def test_newton_step_matches_the_reference(name):
    """IMPL / CN: both sides stop Newton at norm_inf(g) < newton_tol = 1e-12. The Jacobian J = I - fac (L + diag((1 - (nu+1) u^nu) / eps^2))
    is symmetric with eigenvalues >= 1 - fac / eps^2 (L is negative semi-definite, the diagonal term at most 1 / eps^2), so two iterates
    whose residuals are below tol differ by at most  2 tol sqrt(N) / (1 - fac / eps^2)  in the 2-norm, N = nx^2 (second-order terms of
    the cubic are far below that at this distance)."""
    from pymgrit_amd import AllenCahn
    rec = META["newton_steps"][name]
    app = AllenCahn(nx=rec["nx"], nu=rec["nu"], eps=rec["eps"], method=rec["method"], t_start=0, t_stop=1, nt=2)
    got = apply_step(app, np.asarray(app.initial_guess().get_values()), rec["dt"])
    fac = rec["dt"] * (0.5 if rec["method"] == "CN" else 1.0)
    tol = 2 * app.newton_tol * rec["nx"] / (1.0 - fac / rec["eps"] ** 2)
    err = float(np.linalg.norm(got - ARR["out_" + name]))
    print(f"{name}: err {err:.3e} allowed {tol:.3e}")
    assert err <= tol, (name, err, tol)


@pytest.mark.parametrize("n", [4, 9, 32, 63, 64, 130])
def test_hartley_table_is_symmetric_and_its_own_inverse(n):
    from pymgrit_amd.allen_cahn.allen_cahn import hartley_matrix
    T = hartley_matrix(n)
    assert np.array_equal(T, T.T)
    assert np.abs(T @ T - np.eye(n)).max() <= n * EPS


def test_laplacian_matrix_is_diagonal_in_the_hartley_basis():
    from pymgrit_amd import AllenCahn
    from pymgrit_amd.allen_cahn.allen_cahn import hartley_matrix, periodic_laplacian_eigenvalues
    app = AllenCahn(nx=12, method="IMEX", t_start=0, t_stop=1, nt=2)
    T, lam = hartley_matrix(12), periodic_laplacian_eigenvalues(12, app.dx)
    K = np.kron(T, T)
    D = K @ app.space_disc.toarray() @ K
    want = -(lam[:, None] + lam[None, :]).ravel()
    assert np.abs(D - np.diag(want)).max() <= 144 * EPS * np.abs(want).max()


def _problem(rec, cls=None):
    from pymgrit_amd import AllenCahn
    cls = cls or AllenCahn
    return [cls(nx=rec["nx"], method=rec["method"], t_start=0, t_stop=META["t_stop"], nt=nt) for nt in rec["nts"]]


@pytest.mark.parametrize("name", sorted(META["solve"]))
def test_plugin_path_solves_match_the_reference_histories(name, caplog):
    """the host steppers under pymgrit_amd's Mgrit (plugin path: a subclass that overrides step, or IMPL which has no device form)"""
    from pymgrit_amd import AllenCahn, Mgrit

    class HostAllenCahn(AllenCahn):
        def step(self, u_start, t_start, t_stop):
            return super().step(u_start, t_start, t_stop)

    rec = META["solve"][name]
    with caplog.at_level(logging.WARNING):
        mg = Mgrit(_problem(rec, HostAllenCahn), logging_lvl=30, **rec["opts"])
    assert type(mg.backend).__name__ == "PluginBackend"
    conv = mg.solve()["conv"]
    u = np.array([np.asarray(v.get_values()) for v in mg.u[0]])
    check_history(name, conv, cases.spacetime_norm(u))
    last = ARR["last_" + name]
    assert np.abs(u[-1] - last).max() <= 1e-9 * np.abs(last).max()


def test_device_stepper_describes_imex_only():
    from pymgrit_amd import AllenCahn
    d = AllenCahn(nx=16, nu=4, method="IMEX", t_start=0, t_stop=1, nt=3).device_stepper()
    assert d["kind"] == "allencahn2d" and d["n"] == 256 and d["nx"] == 16 and d["nu"] == 4
    assert d["inv_dx2"] == 1.0 / (1.0 / 16) ** 2 and d["inv_eps2"] == 1.0 / 0.04 ** 2
    for method in ("IMPL", "CN"):
        assert AllenCahn(nx=16, method=method, t_start=0, t_stop=1, nt=3).device_stepper() is None
    assert AllenCahn(nx=16, t_start=0, t_stop=1, nt=3).method == "IMPL"


def test_impl_hierarchy_selects_the_plugin_path():
    from pymgrit_amd import AllenCahn, Mgrit
    prob = [AllenCahn(nx=8, method="IMPL", t_start=0, t_stop=0.001, nt=nt) for nt in (5, 3)]
    mg = Mgrit(prob, logging_lvl=30, max_iter=1)
    assert type(mg.backend).__name__ == "PluginBackend"


def test_unknown_method_raises_the_reference_text():
    from pymgrit_amd import AllenCahn
    with pytest.raises(Exception, match=r"Unknown method\. Choose IMPL \(implicit\), IMEX \(implicit-explicit\) or CN \(Crank-Nicolson"):
        AllenCahn(nx=8, method="RK4", t_start=0, t_stop=1, nt=3)


def test_package_exports():
    import pymgrit_amd
    from pymgrit_amd import AllenCahn, VectorAllenCahn2D, VectorHeat1D2Pts  # noqa: F401
    for name in ("AllenCahn", "VectorAllenCahn2D", "VectorHeat1D2Pts"):
        assert name in pymgrit_amd.__all__


def test_vector_and_attributes():
    from pymgrit_amd import AllenCahn, VectorAllenCahn2D
    app = AllenCahn(nx=16, method="IMEX", t_start=0, t_stop=1, nt=3)
    assert app.dx == 1.0 / 16 and app.ny == 16 and np.array_equal(app.x, np.linspace(-0.5, 0.5, 16))
    assert app.space_disc.shape == (256, 256) and app.exact_radius(0.02) == np.sqrt(0.25 ** 2 - 0.04) and app.exact_radius(1.0) == 0.0
    a, b = VectorAllenCahn2D(3, 3), VectorAllenCahn2D(3, 3)
    a.set_values(np.full((3, 3), 2.0)); b.set_values(np.ones((3, 3)))
    assert np.array_equal((a + b).get_values(), np.full((3, 3), 3.0)) and np.array_equal((a - b * 0.5).get_values(), np.full((3, 3), 1.5))
    assert a.norm() == 6.0 and a.clone_zero().norm() == 0.0 and a.clone().get_values() is not None
    assert a.clone_rand().get_values().shape == (3, 3) and a.pack() is a.get_values()


@pytest.mark.parametrize("nx", [64, 128])
def test_radius_of_the_initial_condition(nx):
    from pymgrit_amd import AllenCahn
    app = AllenCahn(nx=nx, method="IMEX", t_start=0, t_stop=1, nt=3)
    assert abs(app.compute_radius(app.initial_guess()) - app.radius) <= app.dx
    ref = ARR["out_imex_init_nx64_nu2_dt0.0001"]
    assert ref.shape == (64, 64)
