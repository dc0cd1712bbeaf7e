"""Burgers2D on the host (no GPU): the IMEX step against an independent high-precision Phi that uses no transform
(tests/burgers_reference.py: the right-hand side in long double, the solve of gray_scott_reference.solve_plane), the reference itself
against a dense solve written out from the equation, the fixed points and the 1-D reduction of the scheme, plugin-path solves over the
host step against the same solves over the reference step, the state vector, the initial guess, the refusals, the device description
and the exports.

Tolerance of one IMEX step, per plane c = u, v, nothing in it measured on the code under test:

    norm_F(error_c) <= (C(nx) + 1) EPS m_c,      C(nx) = 4 nx + 12
    m_c = norm_F(|c| + dt inv_2dx (|u| (|c[i+1]| + |c[i-1]|) + |v| (|c[j+1]| + |c[j-1]|)))

m_c is a majorant of b_c = c - dt (u ax_c + v ay_c): every term of b_c with its sign dropped, so |b_c| <= m_c point by point, and
every intermediate of the evaluation is bounded by the same expression.
  * 4 nx: a product with an orthogonal n x n matrix is off by at most n eps (1 - n eps)^-1 times the operand's 2-norm
    (test_allen_cahn_cpu.py derives the rule); the step has four such products, the table between them has |D| <= 1, and
    norm_F(b_c) <= m_c.
  * 12: b_c at one point goes through at most eight roundings, each relative to a partial result that the point's term of m_c bounds
    (two subtractions, two multiplications by inv_2dx, u * ax, v * ay and their sum -- one rounding less where the device fuses --,
    the product with dt and the sum with c -- again one less when fused): 8 EPS m_c in the Frobenius norm. inv_2dx itself is a rounded
    quotient (1 EPS on the transport term), the table entry is three roundings of a number <= 1 and the scale one more: 12 together.
  * 1: reference_phi is off by at most EPS norm_F(b_c) <= EPS m_c (burgers_reference.py).
The device form fuses two multiply-adds of b_c, which only removes roundings; numpy does not fuse, the bound covers both. A numpy
prototype of the step stayed below 0.054 of the bound over nx in 4 .. 129, four (nu, dt) pairs and states in [-1, 1] and [-2, 2].
"""
import logging

import numpy as np
import pytest

import cases
from burgers_reference import LD, ReferenceBurgers2D, reference_phi, right_hand_side

EPS = cases.EPS


def C(nx):
    return 4 * nx + 12


def make(nx, cls=None, **kw):
    from pymgrit_amd import Burgers2D
    kw.setdefault("t_start", 0), kw.setdefault("t_stop", 1), kw.setdefault("nt", 2)
    kw.setdefault("L", nx / 16)      # dx = 1 / 16 for every nx
    return (cls or Burgers2D)(nx=nx, **kw)


def apply_step(app, w, dt):
    from pymgrit_amd import VectorBurgers2D
    vec = VectorBurgers2D(app.nx)
    vec.set_values(np.array(w, dtype=np.float64).reshape(2, app.nx, app.nx))
    return np.asarray(app.step(vec, 0.0, dt).get_values())


def majorants(w, dt, inv_2dx):
    """m_u, m_v of the module docstring, evaluated by this file's own formula"""
    u, v = np.abs(w[0]), np.abs(w[1])
    return [float(np.linalg.norm(c + dt * inv_2dx * (u * (np.roll(c, -1, 0) + np.roll(c, 1, 0)) + v * (np.roll(c, -1, 1) + np.roll(c, 1, 1)))))
            for c in (u, v)]


REF_NX = [4, 20, 33, 66, 97, 129]      # the smallest grid, K steps (32) and tiles (64) of the device product + 1 / + 2
REF_NU_DT = [(0.1, 2e-3), (0.01, 5e-4), (1.0, 1e-2), (0.1, 2.0 ** -9)]


@pytest.mark.parametrize("nx", REF_NX)
def test_host_imex_step_matches_the_high_precision_phi(nx):
    """_step_imex (Hartley table, lam_k, the D table, the float64 stencil) against reference_phi, which shares none of it: a wrong
    eigenvalue, swapped axes or planes, or a wrong sign of the transport term shows here"""
    rng = np.random.default_rng(1000 * nx)
    worst = 0.0
    for nu, dt in REF_NU_DT:
        app = make(nx, nu=nu)
        assert dt * nu / app.dx ** 2 <= 50      # inside the reference solver's certificate
        inputs = [("initial guess", np.asarray(app.initial_guess().get_values()))]
        inputs += [(f"uniform [-{a}, {a}]", rng.uniform(-a, a, size=(2, nx, nx))) for a in (1, 2)]
        for what, w in inputs:
            got, ref = apply_step(app, w, dt), reference_phi(w, dt, nx, nu, app.L)
            assert got.shape == ref.shape == (2, nx, nx)
            for c, m in enumerate(majorants(w, dt, app.inv_2dx)):
                err, tol = float(np.linalg.norm(got[c] - ref[c])), (C(nx) + 1) * EPS * m
                worst = max(worst, err / tol)
                print(f"RATIO host_imex[nx={nx},nu={nu},dt={dt}] {what} plane {'uv'[c]}: error/bound {err / tol:.4f}")
                assert err <= tol, (nx, nu, dt, what, c, err, tol)
    print(f"RATIO host_imex[nx={nx}]: worst error/bound {worst:.4f}")


def test_the_bound_sees_a_relative_change_of_1e_10_in_nu():
    """what the comparison above can see: the host step with nu changed by 1e-10 relative misses the reference of the unchanged nu by
    more than the bound, in both planes"""
    nx, dt, nu = 20, 0.05, 0.1
    w = np.random.default_rng(7).uniform(-1.0, 1.0, size=(2, nx, nx))
    app = make(nx, nu=nu * (1.0 + 1e-10))
    got, ref = apply_step(app, w, dt), reference_phi(w, dt, nx, nu, app.L)
    for c, m in enumerate(majorants(w, dt, app.inv_2dx)):
        err, tol = float(np.linalg.norm(got[c] - ref[c])), (C(nx) + 1) * EPS * m
        print(f"RATIO sensitivity[nu] plane {'uv'[c]}: error/bound {err / tol:.1f}")
        assert err > tol, (c, err, tol)


def test_reference_matches_a_dense_solve_of_the_equation():
    """nx = 6: the scheme written out index by index in float64 -- b_c by loops, A = I - dt nu Lh as a dense 36 x 36 matrix -- and
    np.linalg.solve. A is symmetric with eigenvalues in [1, 1 + 8 r], r = dt nu / dx^2, so the solve is off by at most about
    8 n EPS cond(A) norm(x) (Gaussian elimination, n = 36) and b_c by 8 EPS m_c: allowed (8 n (1 + 8 r) + 8 + 1) EPS m_c"""
    nx, nu, L, dt = 6, 0.1, 6 / 16, 2e-3
    dx = L / nx
    r = dt * nu / dx ** 2
    w = np.random.default_rng(6).uniform(-1.0, 1.0, size=(2, nx, nx))
    A = np.zeros((nx * nx, nx * nx))
    for i in range(nx):
        for j in range(nx):
            p = i * nx + j
            A[p, p] += 1.0 + 4.0 * r
            for q in (((i + 1) % nx) * nx + j, ((i - 1) % nx) * nx + j, i * nx + (j + 1) % nx, i * nx + (j - 1) % nx):
                A[p, q] -= r
    ref = reference_phi(w, dt, nx, nu, L)
    u, v = w
    for c, m in enumerate(majorants(w, dt, 1.0 / (2.0 * dx))):
        b = np.zeros((nx, nx))
        for i in range(nx):
            for j in range(nx):
                ax = (w[c][(i + 1) % nx][j] - w[c][(i - 1) % nx][j]) / (2.0 * dx)
                ay = (w[c][i][(j + 1) % nx] - w[c][i][(j - 1) % nx]) / (2.0 * dx)
                b[i][j] = w[c][i][j] - dt * (u[i][j] * ax + v[i][j] * ay)
        x = np.linalg.solve(A, b.ravel()).reshape(nx, nx)
        err, tol = float(np.linalg.norm(x - ref[c])), (8 * nx * nx * (1.0 + 8.0 * r) + 9) * EPS * m
        print(f"RATIO reference_vs_dense plane {'uv'[c]}: error/bound {err / tol:.4f}")
        assert err <= tol, (c, err, tol)
        assert float(np.linalg.norm(x - w[c])) > 1e6 * tol      # (and the step is not the identity at this size)


@pytest.mark.parametrize("nx", [4, 33])
def test_constant_state_is_a_fixed_point(nx):
    """(u, v) = (p, q): every difference is exactly 0, so b = c exactly; mode 0 has D = 1, every other mode of a constant is 0 up to
    the products' rounding: Phi = (p, q) within the per-Phi bound"""
    app = make(nx, nu=0.1)
    p, q, dt = 0.75, -1.25, 2e-3
    w = np.stack((np.full((nx, nx), p), np.full((nx, nx), q)))
    b = app._rhs_imex(w[0], w[1], dt)
    assert np.array_equal(b[0], w[0]) and np.array_equal(b[1], w[1])
    got = apply_step(app, w, dt)
    for c, m in enumerate(majorants(w, dt, app.inv_2dx)):
        err, tol = float(np.linalg.norm(got[c] - w[c])), C(nx) * EPS * m
        print(f"RATIO fixed_point[nx={nx}] plane {'uv'[c]}: error/bound {err / tol:.4f}")
        assert err <= tol, (c, err, tol)


@pytest.mark.parametrize("nx", [4, 33])
def test_y_independent_state_steps_like_the_1d_scheme(nx):
    """u = f(x), v = 0: b_v = 0 exactly and so is its solve; u_y = 0 exactly, so b_u[i][j] = f_i - dt f_i (f_(i+1) - f_(i-1)) / (2 dx)
    for every j and the solve reduces to the 1-D periodic problem (I - dt nu L1) x = b, L1 = [1 -2 1] / dx^2. The 1-D problem is solved
    here densely with refinement in long double; its residual is asserted below EPS / 2 norm(b) as in solve_plane (the eigenvalues of
    the matrix are >= 1), so the yardstick is off by at most EPS norm_F(b) on the plane: (C(nx) + 1) EPS m_u as for the 2-D reference.
    Swapped axes give a state that depends on y; swapped planes a non-zero v."""
    app = make(nx, nu=0.1)
    dt = 2e-3
    f = np.random.default_rng(nx).uniform(-1.0, 1.0, size=nx)
    w = np.stack((np.repeat(f[:, None], nx, axis=1), np.zeros((nx, nx))))
    got = apply_step(app, w, dt)
    assert np.array_equal(got[1], np.zeros((nx, nx)))
    fl = f.astype(LD)
    b = fl - LD(dt) * fl * (np.roll(fl, -1) - np.roll(fl, 1)) / (LD(2) * LD(app.L) / LD(nx))
    r = LD(dt) * LD(app.nu) * (LD(nx) / LD(app.L)) ** 2
    A = (1.0 + 2.0 * float(r)) * np.eye(nx)
    for i in range(nx):
        A[i, (i + 1) % nx] -= float(r)
        A[i, (i - 1) % nx] -= float(r)

    def residual(x):
        return b - (x - r * (np.roll(x, 1) + np.roll(x, -1) - LD(2) * x))
    x = np.linalg.solve(A, b.astype(np.float64)).astype(LD)
    for _ in range(3):
        x = x + np.linalg.solve(A, residual(x).astype(np.float64)).astype(LD)
    assert float(np.linalg.norm(residual(x))) <= 0.5 * EPS * float(np.linalg.norm(b))
    want = np.repeat(x.astype(np.float64)[:, None], nx, axis=1)
    err, tol = float(np.linalg.norm(got[0] - want)), (C(nx) + 1) * EPS * majorants(w, dt, app.inv_2dx)[0]
    print(f"RATIO y_independent[nx={nx}]: error/bound {err / tol:.4f}")
    assert err <= tol, (err, tol)
    assert float(np.linalg.norm(want - w[0])) > 1e3 * tol      # (the step moves the state by far more than the bound)


def _host_class():
    from pymgrit_amd import Burgers2D

    class HostBurgers2D(Burgers2D):     # overriding step sends the hierarchy to the plugin path
        def step(self, u_start, t_start, t_stop):
            return super().step(u_start, t_start, t_stop)
    return HostBurgers2D


# name: (nx, nu, t_stop, nts)
SOLVES = {"nx12_nu0.05": (12, 0.05, 0.25, (17, 9, 5)), "nx16_reference_time_grid": (16, 0.01, 0.5, (129, 65, 33))}


@pytest.mark.parametrize("name", sorted(SOLVES))
def test_plugin_path_solve_matches_the_solve_over_the_reference_step(name):
    """Mgrit over the host step against Mgrit over reference_phi from the initial guess (L = 1; the second case is the time grid of the
    reference's example): the residual histories by the project's rule (tests/cases.py),
    |conv - reference| <= 1e-10 reference + 64 EPS norm(u). Both sides reach 1e-10 (in 4 and 8 iterations with the default options)
    within max_iter"""
    from pymgrit_amd import Mgrit
    nx, nu, t_stop, nts = SOLVES[name]
    logging.disable(logging.WARNING)
    try:
        ours = Mgrit([make(nx, cls=_host_class(), nu=nu, L=1.0, t_stop=t_stop, nt=nt) for nt in nts], tol=1e-10, max_iter=15, logging_lvl=30)
        ref = Mgrit([make(nx, cls=ReferenceBurgers2D, nu=nu, L=1.0, t_stop=t_stop, nt=nt) for nt in nts], tol=1e-10, max_iter=15, logging_lvl=30)
        assert type(ours.backend).__name__ == type(ref.backend).__name__ == "PluginBackend"
        conv, rconv = np.asarray(ours.solve()["conv"]), np.asarray(ref.solve()["conv"])
    finally:
        logging.disable(logging.NOTSET)
    norm_u = cases.spacetime_norm([v.get_values() for v in ours.u[0]])
    print(f"{name}: {len(rconv)} iterations, conv {rconv}")
    assert len(conv) == len(rconv) < 15 and rconv[-1] < 1e-10, (conv, rconv)
    dev = np.abs(conv - rconv)
    print(f"RATIO solve[{name}] conv: largest deviation {np.max(dev) / (EPS * norm_u):.2f} units of eps*norm(u) (allowed {cases.BLK_K})")
    assert np.all(dev <= 1e-10 * rconv + cases.BLK_K * EPS * norm_u), (conv, rconv)


def test_right_hand_side_of_the_reference_is_the_formula():
    """the long-double b_c at one point, written out: axis 0 is x, u multiplies the x difference"""
    nx, L, dt = 5, 5 / 16, 1e-3
    w = np.random.default_rng(3).uniform(-1.0, 1.0, size=(2, nx, nx))
    b = right_hand_side(w, dt, nx, L)
    i, j = 4, 0      # both wraps
    for c in range(2):
        ax = (LD(w[c][0][j]) - LD(w[c][3][j])) / (LD(2) * LD(L) / LD(nx))
        ay = (LD(w[c][i][1]) - LD(w[c][i][4])) / (LD(2) * LD(L) / LD(nx))
        assert b[c][i][j] == LD(w[c][i][j]) - LD(dt) * (LD(w[0][i][j]) * ax + LD(w[1][i][j]) * ay)


def test_vector_interface():
    from pymgrit_amd import Vector, VectorBurgers2D
    nx = 5
    rng = np.random.default_rng(0)
    a, b = VectorBurgers2D(nx), VectorBurgers2D(nx)
    va, vb = rng.normal(size=(2, nx, nx)), rng.normal(size=(2, nx, nx))
    a.set_values(va.copy()), b.set_values(vb.copy())
    assert isinstance(a, Vector) and a.get_values().shape == (2, nx, nx)
    assert np.array_equal((a + b).get_values(), va + vb) and np.array_equal((a - b).get_values(), va - vb)
    assert np.array_equal((a * 2.5).get_values(), va * 2.5)
    assert a.norm() == np.linalg.norm(va.ravel())       # the 2-norm over all 2 nx^2 values
    c = a.clone()
    c.get_values()[0, 0, 0] += 1.0
    assert np.array_equal(a.get_values(), va)            # a clone owns its values
    z = a.clone_zero()
    assert isinstance(z, VectorBurgers2D) and z.get_values().shape == (2, nx, nx) and not z.get_values().any()
    r = a.clone_rand()
    assert r.get_values().shape == (2, nx, nx) and 0.0 <= r.get_values().min() and r.get_values().max() < 1.0
    z.unpack(np.asarray(a.pack()).copy())
    assert np.array_equal(z.get_values(), va)
    assert np.array_equal(np.asarray(a.pack()).ravel()[:nx * nx], va[0].ravel())      # a device row is [u plane | v plane]


def test_initial_guess_is_the_formula():
    app = make(12, L=2.0)
    w = np.asarray(app.vector_t_start.get_values())
    assert w.shape == (2, 12, 12)
    for i in range(12):
        for j in range(12):
            x, y = i * app.dx, j * app.dx
            assert w[0, i, j] == np.sin(2 * np.pi * x / 2.0) and w[1, i, j] == 0.5 * np.sin(2 * np.pi * (x + y) / 2.0), (i, j)
    assert np.ptp(w[0], axis=0).min() > 1.0 and np.ptp(w[1], axis=0).min() > 0.5 and np.ptp(w[1], axis=1).min() > 0.5


def test_constructor_defaults_and_refusals():
    from pymgrit_amd import Burgers2D
    app = Burgers2D(t_start=0, t_stop=0.5, nt=3)
    assert (app.nx, app.nu, app.L, app.method) == (32, 1e-2, 1.0, "IMEX")
    assert app.dx == 1.0 / 32 and app.inv_2dx == 1.0 / (2.0 * app.dx)
    with pytest.raises(Exception, match="Unknown method"):
        make(8, method="nope")
    for bad in (3, 0, -4, 8.5):
        with pytest.raises(Exception, match="nx"):
            make(bad, L=1.0)
    for bad in (dict(nu=0.0), dict(nu=-1.0), dict(nu=float("nan")), dict(nu=float("inf")), dict(L=0.0), dict(L=-1.0), dict(L=float("inf"))):
        with pytest.raises(Exception, match="nu and L"):
            make(8, **bad)
    assert make(4).nx == 4 and make(8.0).nx == 8


def test_device_description():
    app = make(20, nu=0.05)
    assert app.device_stepper() == {"kind": "burgers2d", "n": 800, "nx": 20, "inv_dx2": 1.0 / app.dx ** 2, "inv_2dx": 1.0 / (2.0 * app.dx),
                                    "nu": 0.05}


def test_package_exports():
    import pymgrit_amd
    from pymgrit_amd.core import hip_lib
    for name in ("Burgers2D", "VectorBurgers2D"):
        assert name in pymgrit_amd.__all__ and hasattr(pymgrit_amd, name)
    assert hip_lib.STEPPER_BURGERS2D == 8 and "mgrit_hip_level_burgers2d" in hip_lib.EXPORTS
    from pymgrit_amd.burgers.burgers import Burgers2D
    assert pymgrit_amd.Burgers2D is Burgers2D
