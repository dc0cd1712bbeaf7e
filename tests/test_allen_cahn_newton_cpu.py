"""AllenCahn IMPL / CN with linear_solver='pcg' on the host (no GPU): the numpy statement of the Newton-PCG step
against steps and residual histories recorded from the reference (tests/golden/allen_cahn_newton.*, written by
tests/golden/make_golden_allen_cahn_newton.py, and the Newton records of tests/golden/allen_cahn.*), the refusals, the device
description and the iteration caps.

Tolerance of a step (test_allen_cahn_cpu.test_newton_step_matches_the_reference derives it): both sides stop Newton at
norm_inf(g) < newton_tol and J >= (1 - fac / eps^2) I, so the two results differ by at most 2 newton_tol nx / (1 - fac / eps^2) in the
2-norm. Histories: check_history unchanged, the last state to 1e-9 relative.
"""
import logging

import numpy as np
import pytest

import cases
from allen_cahn_fixtures import ARR as ARR_OLD, EPS, META as META_OLD, apply_step, check_history

META = cases.load_json("allen_cahn_newton.json")
ARR = np.load(cases.GOLDEN + "/allen_cahn_newton.npz")

STEPS = {**{k: (v, ARR) for k, v in META["steps"].items()}, **{k: (v, ARR_OLD) for k, v in META_OLD["newton_steps"].items()}}
SOLVES = {**{k: (v, ARR) for k, v in META["solve"].items()}, "impl_2lvl_V": (META_OLD["solve"]["impl_2lvl_V"], ARR_OLD)}


def _app(rec, **kw):
    from pymgrit_amd import AllenCahn
    kw.setdefault("linear_solver", "pcg")
    return AllenCahn(nx=rec["nx"], nu=rec["nu"], eps=rec["eps"], method=rec["method"], t_start=0, t_stop=rec["dt"], nt=2, **kw)


def _input(app, rec, arr):
    return arr[f"rand_nx{rec['nx']}"] if rec.get("src") == "rand" else np.asarray(app.initial_guess().get_values())


@pytest.mark.parametrize("name", sorted(STEPS))
def test_pcg_step_matches_the_reference(name):
    rec, arr = STEPS[name]
    app = _app(rec)
    got = apply_step(app, _input(app, rec, arr), rec["dt"])
    fac = rec["dt"] * app.theta
    tol = 2 * app.newton_tol * rec["nx"] / (1.0 - fac / rec["eps"] ** 2)
    err = float(np.linalg.norm(got - arr["out_" + name]))
    print(f"{name}: err {err:.3e} allowed {tol:.3e}")
    assert got.shape == (rec["nx"], rec["nx"]) and err <= tol, (name, err, tol)


def test_the_fixtures_meet_the_rule():
    for rec, _ in STEPS.values():
        assert rec["dt"] * (0.5 if rec["method"] == "CN" else 1.0) / rec["eps"] ** 2 < 1.0 and rec["nu"] % 2 == 0
    for rec, _ in SOLVES.values():
        dt = META["t_stop"] / (min(rec["nts"]) - 1)
        assert dt * (0.5 if rec["method"] == "CN" else 1.0) / 0.04 ** 2 < 1.0
    assert set(META["solve"]) == {"cn_2lvl_V", "cn_3lvl_F", "impl_3lvl_V_nested"} and len(META["steps"]) == 12


@pytest.mark.parametrize("name", sorted(SOLVES))
def test_pcg_plugin_path_solves_match_the_reference_histories(name, caplog):
    from pymgrit_amd import AllenCahn, Mgrit

    class HostAllenCahn(AllenCahn):
        def step(self, u_start, t_start, t_stop):
            return super().step(u_start, t_start, t_stop)

    rec, arr = SOLVES[name]
    prob = [HostAllenCahn(nx=rec["nx"], method=rec["method"], linear_solver="pcg", t_start=0, t_stop=META["t_stop"], nt=nt)
            for nt in rec["nts"]]
    with caplog.at_level(logging.WARNING):
        mg = Mgrit(prob, logging_lvl=30, **rec["opts"])
    assert type(mg.backend).__name__ == "PluginBackend"
    conv = mg.solve()["conv"]
    u = np.array([np.asarray(v.get_values()) for v in mg.u[0]])
    check_history(name, conv, cases.spacetime_norm(u), ref=rec["conv"])
    last = arr["last_" + name]
    assert np.abs(u[-1] - last).max() <= 1e-9 * np.abs(last).max()


def test_refusals():
    from pymgrit_amd import AllenCahn
    with pytest.raises(Exception, match="even nu"):
        AllenCahn(nx=8, nu=3, method="IMPL", linear_solver="pcg", t_start=0, t_stop=1e-4, nt=3)
    with pytest.raises(Exception, match=r"dt < 0\.0016"):
        AllenCahn(nx=8, method="IMPL", linear_solver="pcg", t_start=0, t_stop=1, nt=3)
    with pytest.raises(Exception, match=r"dt < 0\.0032"):
        AllenCahn(nx=8, method="CN", linear_solver="pcg", t_start=0, t_stop=1, nt=3)
    with pytest.raises(Exception, match="IMEX"):
        AllenCahn(nx=8, method="IMEX", linear_solver="pcg", t_start=0, t_stop=1e-4, nt=3)
    with pytest.raises(Exception, match="Unknown linear_solver"):
        AllenCahn(nx=8, method="IMPL", linear_solver="gmres", t_start=0, t_stop=1e-4, nt=3)
    # the direct solver keeps every grid and every nu
    assert AllenCahn(nx=8, nu=3, method="IMPL", t_start=0, t_stop=1, nt=3).linear_solver == "direct"
    # CN on a grid that IMPL refuses: fac = dt / 2
    assert AllenCahn(nx=8, method="CN", linear_solver="pcg", t_start=0, t_stop=0.004, nt=3).theta == 0.5


def test_description():
    from pymgrit_amd import AllenCahn
    imex = AllenCahn(nx=16, nu=4, method="IMEX", t_start=0, t_stop=1e-3, nt=3).device_stepper()
    for method, theta in (("IMPL", 1.0), ("CN", 0.5)):
        d = AllenCahn(nx=16, nu=4, method=method, linear_solver="pcg", newton_tol=1e-11, newton_maxiter=7, lin_tol=1e-9, lin_maxiter=50,
                      t_start=0, t_stop=1e-3, nt=3).device_stepper()
        assert {k: d[k] for k in imex} == imex
        assert d["theta"] == theta and d["newton_tol"] == 1e-11 and d["newton_maxiter"] == 7 and d["lin_tol"] == 1e-9 and d["lin_maxiter"] == 50
        assert AllenCahn(nx=16, method=method, linear_solver="direct", t_start=0, t_stop=1e-3, nt=3).device_stepper() is None
        assert AllenCahn(nx=16, method=method, t_start=0, t_stop=1e-3, nt=3).device_stepper() is None


def test_newton_maxiter_1_is_one_newton_update():
    """x1 = u - J(u)^-1 g(u), J and g built here from the sparse matrix: the CG solve at lin_tol = 1e-12 leaves
    norm(delta error) <= cond(J) lin_tol norm(delta), cond(J) <= (1 + 8 fac nx^2 + fac nu / eps^2) / (1 - fac / eps^2)"""
    import scipy.sparse as sp
    from scipy.sparse.linalg import spsolve
    from pymgrit_amd import AllenCahn
    nx, dt = 20, 1e-3
    app = AllenCahn(nx=nx, method="IMPL", linear_solver="pcg", newton_maxiter=1, t_start=0, t_stop=dt, nt=2)
    u = np.asarray(app.initial_guess().get_values())
    got = apply_step(app, u, dt)
    flat, inv = u.ravel(), 1.0 / app.eps ** 2
    g = flat - dt * (app.space_disc.dot(flat) + inv * flat * (1 - flat ** 2)) - flat
    jac = sp.eye(nx * nx) - dt * (app.space_disc + inv * sp.diags(1.0 - 3.0 * flat ** 2))
    delta = spsolve(sp.csc_matrix(jac), g)
    want = (flat - delta).reshape(nx, nx)
    cond = (1 + 8 * dt * nx ** 2 + dt * 2 * inv) / (1 - dt * inv)
    tol = 4 * cond * (app.lin_tol + nx * nx * EPS) * float(np.linalg.norm(delta))
    err = float(np.linalg.norm(got - want))
    print(f"one Newton update: err {err:.3e} allowed {tol:.3e}")
    assert err <= tol and np.linalg.norm(delta) > 1e-3          # (one update, and not zero updates)
    two = apply_step(AllenCahn(nx=nx, method="IMPL", linear_solver="pcg", newton_maxiter=2, t_start=0, t_stop=dt, nt=2), u, dt)
    assert np.linalg.norm(two - got) > 1e3 * tol


def test_lin_maxiter_1_still_converges():
    """inexact Newton: one CG iteration per Newton iteration is a preconditioned gradient step, which contracts; the result meets
    the Newton stopping test within newton_maxiter = 100, so it lies within the step tolerance of the full solve"""
    from pymgrit_amd import AllenCahn
    nx, dt = 20, 1e-3
    kw = dict(nx=nx, method="IMPL", linear_solver="pcg", t_start=0, t_stop=dt, nt=2)
    app = AllenCahn(lin_maxiter=1, **kw)
    u = np.asarray(app.initial_guess().get_values())
    got, full = apply_step(app, u, dt), apply_step(AllenCahn(**kw), u, dt)
    flat = got.ravel()
    g = flat - dt * (app.space_disc.dot(flat) + flat * (1 - flat ** 2) / app.eps ** 2) - u.ravel()
    assert np.abs(g).max() < app.newton_tol + 64 * EPS
    assert np.linalg.norm(got - full) <= 2 * app.newton_tol * nx / (1 - dt / app.eps ** 2)
