"""Heat2D on CPU against a second implementation of Phi: the oracle's fast-diagonalisation restatement and the product's host ``step``
against the transform-free long-double solve of tests/heat2d_reference.py, one step on standard-normal states with random rims.

test_heat2d_cpu.py holds those two to the reference project's fixtures at 9x12 and 20x17 on a smooth input; the GPU suite holds the
device bit for bit to the oracle. Neither shows that the bits are right above the structural edges of the algorithm (the 64-wide tile,
half sizes 64 / 65 of the folded transforms, P = 2 HP = 128 / 256 / 384, mj >= 2) or for the high modes: that is what this file is for.

Shapes: 3x3 (mi = mj = 1), 4x3 (mj < 2), 20x17 (the fixture shape, now rough), 66x67 (m = 64 / 65), 129x130 (half sizes 64), 131x132
(half sizes 65), 5x200 / 200x5 (strongly rectangular), 259x258 (HP = 192).
Two coefficients per shape:
  mild:  a such that 4 theta dt (fx + fy) = 8, i.e. theta dt lambda <= 8 for every mode: every mode keeps at least 1 / 9 of its weight,
         so a wrong table entry or eigenvalue of ANY mode shows in the result;
  stiff: the suite's own cases.H2D_A = 3.5 (dt lambda_max of order 1e4 at 66x67: only the low modes survive the step).
Forward Euler (three shapes): a such that 4 dt (fx + fy) = 0.9 (stable).

Tolerance, derived in heat2d_reference.phi_bound, nothing measured on the code under test:
  theta > 0:  norm_F(error) <= ((2 mi + 2 mj + 8) + 1) EPS norm_F(babs),        theta = 0:  (8 + 1) EPS norm_F(babs).

Sensitivity (mild coefficient): the oracle on a level spec whose fx (fy, theta) is multiplied by 1 + 1e-10 must EXCEED the bound --
the check sees a relative error of 1e-10 in one coefficient at every shape. With PERTURBATION = 0 those tests fail.
"""
import functools

import numpy as np
import pytest

import cases
from heat2d_reference import ReferenceHeat2D, babs_norm, coefficient, make_app, phi_bound, reference_phi

SHAPES = [(3, 3), (4, 3), (20, 17), (66, 67), (129, 130), (131, 132), (5, 200), (200, 5), (259, 258)]
FE_SHAPES = [(4, 3), (20, 17), (66, 67)]
CONFIGS = [("none", False), ("none", True), ("separable", False), ("separable", True), ("general", True)]      # (forcing, boundary values)
T, I_STOP = np.linspace(0, 1, 33), 4
PERTURBATION = 1e-10


def _ids(shapes):
    return [f"{nx}x{ny}" for nx, ny in shapes]


@functools.lru_cache(maxsize=None)
def _case(nx, ny, method, which, forcing, with_bc):
    """(app, input state, reference Phi, allowed Frobenius error): computed once, shared, never changed"""
    a = coefficient(nx, ny, method, float(T[I_STOP] - T[I_STOP - 1]), which)
    app = make_app(nx, ny, T, method, a, forcing, with_bc)
    u = np.random.default_rng(1000 * nx + ny).standard_normal((nx, ny))
    ref = reference_phi(app, u, T[I_STOP - 1], T[I_STOP])
    allowed = phi_bound(app, babs_norm(app, u, T[I_STOP - 1], T[I_STOP]))
    for arr in (u, ref):
        arr.setflags(write=False)
    return app, u, ref, allowed


def _oracle_phi(oracle, spec, u):
    return oracle.OracleProblem([spec], max_iter=1).phi(0, I_STOP, u.ravel()).reshape(u.shape)


def _host_phi(app, u):
    vec = app.vector_template.clone_zero()
    vec.set_values(u.copy())
    return np.asarray(app.step(vec, T[I_STOP - 1], T[I_STOP]).get_values())


def _check(oracle, nx, ny, method, which):
    worst = 0.0
    for forcing, with_bc in CONFIGS:
        app, u, ref, allowed = _case(nx, ny, method, which, forcing, with_bc)
        if with_bc:
            assert np.any(app.boundary_values())
        for name, got in (("oracle", _oracle_phi(oracle, cases.h2d_level_spec(app), u)), ("host", _host_phi(app, u))):
            err = float(np.linalg.norm(got - ref))
            worst = max(worst, err / allowed)
            assert got.shape == ref.shape and err <= allowed, (name, nx, ny, method, which, forcing, with_bc, err, allowed)
    print(f"RATIO cpu[{nx}x{ny},{method},{which}]: worst error/allowed {worst:.4f}")


@pytest.mark.parametrize("which", ["mild", "stiff"])
@pytest.mark.parametrize("method", ["BE", "CN"])
@pytest.mark.parametrize("nx,ny", SHAPES, ids=_ids(SHAPES))
def test_oracle_and_host_step_match_the_long_double_solve(oracle, nx, ny, method, which):
    _check(oracle, nx, ny, method, which)


@pytest.mark.parametrize("nx,ny", FE_SHAPES, ids=_ids(FE_SHAPES))
def test_forward_euler_matches_the_long_double_formula(oracle, nx, ny):
    _check(oracle, nx, ny, "FE", "mild")
    app, u, ref, _ = _case(nx, ny, "FE", "mild", "separable", True)
    rim = np.ones((nx, ny), dtype=bool)
    rim[1:-1, 1:-1] = False
    assert np.array_equal(ref[rim], (app.boundary_values() + u)[rim])       # boundary values + old rim


def test_the_reference_runs_on_the_plugin_path():
    """ReferenceHeat2D describes no device stepper and its step is the long-double solve (what the GPU comparison relies on)"""
    app = make_app(6, 5, T, "CN", 0.1, "separable", True, cls=ReferenceHeat2D)
    plain = make_app(6, 5, T, "CN", 0.1, "separable", True)
    assert isinstance(app, ReferenceHeat2D) and app.device_stepper() is None and plain.device_stepper() is not None
    u = np.random.default_rng(3).standard_normal((6, 5))
    vec = app.vector_template.clone_zero()
    vec.set_values(u.copy())
    assert np.array_equal(app.step(vec, T[2], T[3]).get_values(), reference_phi(plain, u, T[2], T[3]))


def _perturbed_error(oracle, nx, ny, method, key):
    app, u, ref, allowed = _case(nx, ny, method, "mild", "separable", True)
    spec = dict(cases.h2d_level_spec(app))
    spec[key] = spec[key] * (1.0 + PERTURBATION)
    err = float(np.linalg.norm(_oracle_phi(oracle, spec, u) - ref))
    print(f"RATIO sensitivity[{nx}x{ny},{method},{key}]: error/allowed {err / allowed:.1f}")
    return err, allowed


@pytest.mark.parametrize("nx,ny", SHAPES, ids=_ids(SHAPES))
def test_a_relative_error_of_1e_10_in_fx_is_seen(oracle, nx, ny):
    err, allowed = _perturbed_error(oracle, nx, ny, "BE", "fx")
    assert err > allowed, (err, allowed)


@pytest.mark.parametrize("key,method", [("fy", "BE"), ("theta", "CN")])
@pytest.mark.parametrize("nx,ny", [(20, 17), (66, 67)], ids=_ids([(20, 17), (66, 67)]))
def test_a_relative_error_of_1e_10_in_fy_or_theta_is_seen(oracle, nx, ny, key, method):
    err, allowed = _perturbed_error(oracle, nx, ny, method, key)
    assert err > allowed, (err, allowed)
