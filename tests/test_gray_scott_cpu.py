"""GrayScott on the host (no GPU): the IMEX step against an independent high-precision solve that uses no transform
(tests/gray_scott_reference.py: sparse LU start, iterative refinement in long double), plugin-path solves over the host step against
the same solves over the reference step, the host-only steppers EXPL and IMPL, the state vector, the initial guess, the refusals and
the device description.

Tolerances of an IMEX step, none of them measured on the code under test (test_allen_cahn_cpu.py derives them):
  * ours: a product with an orthogonal n x n matrix is off by at most n eps (1 - n eps)^-1 times the vector's 2-norm, the spectral scale
    is <= 1, so four products give  norm_F(error) <= (4 nx + 8) eps norm_F(b_c)  per species (the 8: pointwise right-hand side, scale);
  * reference_phi: EPS norm_F(b_c), the rounding of its long-double solution to float64.
Together ((4 nx + 8) + 1) EPS norm_F(b_c) per species, b_c evaluated by this file's own float64 formula.
"""
import logging

import numpy as np
import pytest

import cases
from gray_scott_reference import LD, ReferenceGrayScott, reference_phi

EPS = cases.EPS
PAR = dict(du=1.0, dv=0.01, a=0.09, b=0.086, L=2.0)


def make(nx, method="IMEX", cls=None, **kw):
    from pymgrit_amd import GrayScott
    kw.setdefault("t_start", 0), kw.setdefault("t_stop", 1), kw.setdefault("nt", 2)
    return (cls or GrayScott)(nx=nx, method=method, **kw)


def apply_step(app, w, dt):
    from pymgrit_amd import VectorGrayScott2D
    vec = VectorGrayScott2D(app.nx)
    vec.set_values(np.array(w, dtype=np.float64).reshape(2, app.nx, app.nx))
    return np.asarray(app.step(vec, 0.0, dt).get_values())


def b_norms(w, dt, a, b):
    """norm_F(b_u), norm_F(b_v) of the right-hand sides of the two implicit solves"""
    u, v = w[0], w[1]
    return float(np.linalg.norm(u + dt * (a * (1 - u) - u * v * v))), float(np.linalg.norm(v + dt * (u * v * v - b * v)))


def phi_bounds(nx, w, dt, a, b):
    return [((4 * nx + 8) + 1) * EPS * n for n in b_norms(w, dt, a, b)]


def random_state(rng, nx):
    """u in [0, 1], v in [0, 0.5]: the range the system lives in"""
    return np.stack((rng.uniform(0.0, 1.0, size=(nx, nx)), rng.uniform(0.0, 0.5, size=(nx, nx))))


REF_NX = [4, 20, 33, 66, 97, 129]      # the smallest grid, K steps (32) and tiles (64) of the device product + 1 / + 2
REF_R = [0.1, 10.0, 40.0]              # r = dt du / dx^2


@pytest.mark.parametrize("nx", REF_NX)
def test_host_imex_step_matches_the_high_precision_solve(nx):
    """_step_imex (Hartley table, lam_k, one D table per species) against reference_phi, which shares none of it: a wrong eigenvalue,
    swapped tables or planes, or a wrong reaction term shows here"""
    app = make(nx)
    rng = np.random.default_rng(1000 * nx)
    worst = 0.0
    for r in REF_R:
        dt = r * app.dx ** 2 / app.du
        inputs = [("initial guess", np.asarray(app.initial_guess().get_values()))]
        inputs += [(f"random {k}", random_state(rng, nx)) for k in range(2)]
        for what, w in inputs:
            got, ref = apply_step(app, w, dt), reference_phi(w, dt, nx, **PAR)
            assert got.shape == ref.shape == (2, nx, nx)
            for c, tol in enumerate(phi_bounds(nx, w, dt, app.a, app.b)):
                err = float(np.linalg.norm(got[c] - ref[c]))
                worst = max(worst, err / tol)
                print(f"RATIO host_imex[nx={nx},r={r}] {what} species {'uv'[c]}: error/bound {err / tol:.4f}")
                assert err <= tol, (nx, r, what, c, err, tol)
    print(f"RATIO host_imex[nx={nx}]: worst error/bound {worst:.4f}")


SENS = {"a": 0, "b": 1, "du": 0, "dv": 1}      # the parameter and the species whose solve it enters


@pytest.mark.parametrize("name", sorted(SENS))
def test_the_bound_sees_a_relative_change_of_1e_10_in_a_parameter(name):
    """What the comparison above can see: the host step with ONE parameter changed by 1e-10 relative misses the reference of the
    unchanged parameters by more than the bound, in the species the parameter enters. (With the change set to 0 all four cases fail,
    as they must: checked once by hand when the test was written.)"""
    nx, dt, rel = 20, 0.125, 1e-10
    w = np.random.default_rng(7).uniform(0.0, 1.0, size=(2, nx, nx))
    app = make(nx, **{**PAR, name: PAR[name] * (1.0 + rel)})
    got, ref = apply_step(app, w, dt), reference_phi(w, dt, nx, **PAR)
    c = SENS[name]
    err, tol = float(np.linalg.norm(got[c] - ref[c])), phi_bounds(nx, w, dt, PAR["a"], PAR["b"])[c]
    print(f"RATIO sensitivity[{name}]: error/bound {err / tol:.1f}")
    assert err > tol, (name, err, tol)


def _host_class():
    from pymgrit_amd import GrayScott

    class HostGrayScott(GrayScott):     # overriding step sends the hierarchy to the plugin path
        def step(self, u_start, t_start, t_stop):
            return super().step(u_start, t_start, t_stop)
    return HostGrayScott


SOLVES = {"nx20_3lvl": (20, (33, 17, 9)), "nx33_2lvl": (33, (129, 33))}


@pytest.mark.parametrize("name", sorted(SOLVES))
def test_plugin_path_solve_matches_the_solve_over_the_reference_step(name):
    """Mgrit over the host step against Mgrit over reference_phi on [0, 4] (r = dt du / dx^2 = 50 and 34 on the coarsest levels): the
    residual histories by the project's rule (tests/cases.py), |conv - reference| <= 1e-10 reference + 64 EPS norm(u). Both sides
    reach 1e-9 (in 6 and 7 iterations with the default options) within max_iter"""
    from pymgrit_amd import Mgrit
    nx, nts = SOLVES[name]
    logging.disable(logging.WARNING)
    try:
        ours = Mgrit([make(nx, cls=_host_class(), t_stop=4, nt=nt) for nt in nts], tol=1e-9, max_iter=12, logging_lvl=30)
        ref = Mgrit([make(nx, cls=ReferenceGrayScott, t_stop=4, nt=nt) for nt in nts], tol=1e-9, max_iter=12, logging_lvl=30)
        assert type(ours.backend).__name__ == type(ref.backend).__name__ == "PluginBackend"
        conv, rconv = np.asarray(ours.solve()["conv"]), np.asarray(ref.solve()["conv"])
    finally:
        logging.disable(logging.NOTSET)
    norm_u = cases.spacetime_norm([v.get_values() for v in ours.u[0]])
    print(f"{name}: {len(rconv)} iterations, conv {rconv}")
    assert len(conv) == len(rconv) < 12 and rconv[-1] < 1e-9
    dev = np.abs(conv - rconv)
    print(f"RATIO solve[{name}] conv: largest deviation {np.max(dev) / (EPS * norm_u):.2f} units of eps*norm(u) (allowed {cases.BLK_K})")
    assert np.all(dev <= 1e-10 * rconv + cases.BLK_K * EPS * norm_u), (conv, rconv)


def _lap_ld(p, dx):
    return (np.roll(p, 1, 0) + np.roll(p, -1, 0) + np.roll(p, 1, 1) + np.roll(p, -1, 1) - LD(4) * p) / LD(dx) ** 2


def _rate_ld(w, app):
    """the system's right-hand side (reference gray_scott_2d_petsc.py:106-109) in long double"""
    u, v = w[0].astype(LD), w[1].astype(LD)
    return np.stack((LD(app.du) * _lap_ld(u, app.dx) - u * v ** 2 + LD(app.a) * (1 - u),
                     LD(app.dv) * _lap_ld(v, app.dx) + u * v ** 2 - LD(app.b) * v))


@pytest.mark.parametrize("nx", [4, 20, 33])
def test_explicit_step_matches_the_formula(nx):
    """forward Euler against w + dt rate(w) in long double. A dozen float64 operations per value, each off by at most EPS times the
    size of its operands: 16 EPS (max|w| + dt (8 d / dx^2 + max|w|^2 + |a| + |b|) max(|w|, 1)) per value"""
    app = make(nx, method="EXPL")
    rng = np.random.default_rng(nx)
    for dt in (1e-3, 0.1 * app.dx ** 2):
        for w in (np.asarray(app.initial_guess().get_values()), random_state(rng, nx)):
            got = apply_step(app, w, dt)
            ref = w.astype(LD) + LD(dt) * _rate_ld(w, app)
            m = float(np.abs(w).max())
            tol = 16 * EPS * (m + dt * (8 * max(app.du, app.dv) / app.dx ** 2 + m * m + abs(app.a) + abs(app.b)) * max(m, 1.0))
            assert float(np.abs(got - ref).max()) <= tol, (nx, dt, float(np.abs(got - ref).max()), tol)


@pytest.mark.parametrize("nx", [8, 20])
def test_implicit_step_solves_the_reference_residual(nx):
    """IMPL: the reference's formFunction (:218-240) minus the old state, evaluated here in long double, is below newton_tol at the
    returned state"""
    app = make(nx, method="IMPL")
    rng = np.random.default_rng(nx)
    for dt in (0.01, 0.5):
        for w in (np.asarray(app.initial_guess().get_values()), random_state(rng, nx)):
            x = apply_step(app, w, dt)
            res = x.astype(LD) - LD(dt) * _rate_ld(x, app) - w.astype(LD)
            print(f"IMPL nx={nx} dt={dt}: residual {float(np.abs(res).max()):.3e}")
            assert float(np.abs(res).max()) < app.newton_tol


def test_implicit_and_imex_steps_agree_to_second_order():
    """both are first-order steps of the same system that differ in where the reaction term is evaluated: their difference is
    C dt^2 + O(dt^3) once dt du / dx^2 << 1 (here 0.04 .. 0.01), so halving dt divides it by 4 (within a quarter: the O(dt^3) part at these
    dt), and it is far above newton_tol"""
    nx = 20
    impl, imex = make(nx, method="IMPL", newton_tol=1e-13), make(nx, method="IMEX")
    w = np.asarray(imex.initial_guess().get_values())
    diff = [float(np.linalg.norm(apply_step(impl, w, dt) - apply_step(imex, w, dt))) for dt in (4e-4, 2e-4, 1e-4)]
    print(f"IMPL - IMEX at dt = 4e-4, 2e-4, 1e-4: {diff}")
    assert diff[2] > 1e-9
    for coarse, fine in zip(diff[:-1], diff[1:]):
        assert 3.0 <= coarse / fine <= 5.0, diff


def test_vector_interface():
    from pymgrit_amd import Vector, VectorGrayScott2D
    nx = 5
    rng = np.random.default_rng(0)
    a, b = VectorGrayScott2D(nx), VectorGrayScott2D(nx)
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
    assert isinstance(z, VectorGrayScott2D) and z.get_values().shape == (2, nx, nx) and not z.get_values().any()
    r = a.clone_rand()
    assert r.get_values().shape == (2, nx, nx) and 0.0 <= r.get_values().min() and r.get_values().max() < 1.0
    assert np.array_equal(np.asarray(a.pack()), va)
    z.unpack(np.asarray(a.pack()).copy())
    assert np.array_equal(z.get_values(), va)
    assert np.array_equal(np.asarray(a.pack()).ravel()[:nx * nx], va[0].ravel())      # a device row is [u plane | v plane]


@pytest.mark.parametrize("nx", [16, 33])
def test_initial_guess_is_the_reference_formula(nx):
    """reference :311-325, point by point as it is written there"""
    app = make(nx)
    w = np.asarray(app.vector_t_start.get_values())
    assert w.shape == (2, nx, nx)
    inside = 0
    for i in range(nx):
        for j in range(nx):
            x, y, v = i * app.dx, j * app.dx, 0.0
            if 1.0 <= x <= 1.5 and 1.0 <= y <= 1.5:
                v = (np.sin(4 * np.pi * x) ** 2) * (np.sin(4 * np.pi * y) ** 2) / 4
                inside += 1
            assert w[1, i, j] == v and w[0, i, j] == 1 - 2 * v, (i, j)
    assert inside >= 4 and w[1].max() > 0.2


def test_constructor_refusals():
    from pymgrit_amd import GrayScott
    with pytest.raises(Exception, match=r"Unknown method\. Choose IMPL \(implicit\) or IMEX \(implicit-explicit\)"):
        make(8, method="CN")
    for bad in (dict(du=0.0), dict(du=-1.0), dict(dv=0.0), dict(dv=float("nan")), dict(a=float("inf")), dict(b=float("nan"))):
        with pytest.raises(Exception, match="du|dv|a=|b="):
            make(8, **bad)
    app = GrayScott(t_start=0, t_stop=1, nt=3)      # the defaults of the issue's signature
    assert (app.nx, app.du, app.dv, app.a, app.b, app.L, app.method) == (64, 1.0, 0.01, 0.09, 0.086, 2.0, "IMEX")
    assert (app.newton_tol, app.newton_maxiter) == (1e-10, 100) and app.dx == 2.0 / 64
    make(8, a=-3.0, b=0.0)                          # any finite a, b


def test_device_description():
    app = make(20, **PAR)
    d = app.device_stepper()
    assert d == {"kind": "grayscott2d", "n": 800, "nx": 20, "inv_dx2": 1.0 / app.dx ** 2, "du": 1.0, "dv": 0.01, "a": 0.09, "b": 0.086}
    assert make(20, method="EXPL").device_stepper() is None and make(20, method="IMPL").device_stepper() is None


def test_package_exports():
    import pymgrit_amd
    assert "GrayScott" in pymgrit_amd.__all__ and "VectorGrayScott2D" in pymgrit_amd.__all__
    from pymgrit_amd.gray_scott.gray_scott import GrayScott
    assert pymgrit_amd.GrayScott is GrayScott
