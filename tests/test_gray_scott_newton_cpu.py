"""CPU tests of GrayScott(method='IMPL', linear_solver='bicgstab'): the host statement of the Newton-BiCGStab step (``_step_bicgstab``,
the specification the gsn_* kernels share) against the independent long-double Phi of
tests/gray_scott_newton_reference.py and against the direct step ``_step_impl``; the constructor's refusals, the description for the
HIP engine, the iteration caps.

Inputs are rough and in the box u in [0, 1], v in [0, 0.5] with dt <= 0.25: dt mu(1.05, 0.55) = 0.25 * 1.97 < 0.5, the regime where the
step has one solution (gray_scott_newton_reference.py derives mu and the inequality used here).

The tolerance tau between two states that both claim to solve F = 0 for the same input, the exit criterion max|F(x)| < newton_tol + E_g
asserted beside it and the operation count behind C_G are derived in tests/gray_scott_newton_reference.py beside the functions that
evaluate them, shared with the GPU tests.
"""
import logging

import numpy as np
import pytest

import cases
from gray_scott_newton_reference import (C_G_HOST, LD, PARS, ReferenceGrayScottNewton, exit_criterion, history_allowance, jacobian, margin, par_of,
                                         reference_phi, residual, tau, tau_phi_a_priori)

EPS = cases.EPS
DT = 0.25


def make(nx, cls=None, **kw):
    from pymgrit_amd import GrayScott
    kw.setdefault("t_start", 0); kw.setdefault("t_stop", 1); kw.setdefault("nt", 5)
    kw.setdefault("method", "IMPL"); kw.setdefault("linear_solver", "bicgstab")
    return (cls or GrayScott)(nx=nx, **kw)


def random_state(rng, nx):
    return np.stack((rng.uniform(0.0, 1.0, size=(nx, nx)), rng.uniform(0.0, 0.5, size=(nx, nx))))


@pytest.mark.parametrize("par", sorted(PARS))
@pytest.mark.parametrize("nx", [4, 20, 33])
def test_bicgstab_step_matches_the_reference_and_the_direct_step(nx, par):
    rng = np.random.default_rng(10 * nx + len(par))
    app = make(nx, **PARS[par])
    worst = 0.0
    for dt in (DT, 0.03):
        w = random_state(rng, nx)
        counts = {}
        x = app._step_bicgstab(w, dt, counts)
        g, allowed_g = exit_criterion(app, w, dt, x, C_G_HOST)
        assert counts["newton_iterations"] < app.newton_maxiter and g < allowed_g, (g, allowed_g, counts)
        for name, y in (("reference", reference_phi(w, dt, nx, par_of(app))), ("direct", app._step_impl(w, dt))):
            err, allowed = float(np.linalg.norm(x - y)), tau(app, w, dt, x, y)
            worst = max(worst, err / allowed)
            assert err <= allowed, (name, dt, err, allowed)
        assert 1 <= counts["newton_iterations"] <= 4 and counts["cg_iterations"] <= 16, counts
    print(f"RATIO host_bicgstab[nx={nx},{par}]: worst error/allowed {worst:.4f}")


def _host_class():
    from pymgrit_amd import GrayScott

    class HostGrayScott(GrayScott):     # overriding step sends the hierarchy to the plugin path
        def step(self, u_start, t_start, t_stop):
            return super().step(u_start, t_start, t_stop)
    return HostGrayScott


@pytest.mark.parametrize("nts", [(17, 9, 5), (33, 9)])
def test_plugin_path_solve_matches_the_solve_over_the_reference_step(nts):
    from pymgrit_amd import Mgrit
    nx, tols = 12, dict(newton_tol=1e-12)
    logging.disable(logging.WARNING)
    try:
        ours = Mgrit([make(nx, cls=_host_class(), nt=nt, **tols) for nt in nts], tol=1e-9, max_iter=12, logging_lvl=30)
        ref = Mgrit([make(nx, cls=ReferenceGrayScottNewton, linear_solver="direct", nt=nt) for nt in nts], tol=1e-9, max_iter=12, logging_lvl=30)
        assert type(ours.backend).__name__ == type(ref.backend).__name__ == "PluginBackend"
        conv, rconv = np.asarray(ours.solve()["conv"]), np.asarray(ref.solve()["conv"])
    finally:
        logging.disable(logging.NOTSET)
    norm_u = cases.spacetime_norm([v.get_values() for v in ours.u[0]])
    assert len(conv) == len(rconv) < 12 and rconv[-1] < 1e-9, (conv, rconv)
    dt = max(float(np.max(np.diff(t))) for t in ref.t)
    allowed = history_allowance(ref, rconv, norm_u, tau_phi_a_priori(ours.problem[0], dt, ref.problem, C_G_HOST))
    dev = np.abs(conv - rconv)
    print(f"RATIO solve[nts={nts}] conv ({len(conv)} iterations): worst deviation/allowed {np.max(dev / allowed):.4f}")
    assert np.all(dev <= allowed), (conv, rconv, allowed)


def test_constructor_refusals_and_defaults():
    from pymgrit_amd import GrayScott
    with pytest.raises(Exception, match="Unknown linear_solver"):
        make(8, linear_solver="pcg")
    for method in ("IMEX", "EXPL"):
        with pytest.raises(Exception, match="linear_solver='bicgstab' is the inner solver of method='IMPL'"):
            make(8, method=method)
    app = GrayScott(t_start=0, t_stop=1, nt=3)
    assert (app.linear_solver, app.lin_tol, app.lin_maxiter) == ("direct", 1e-10, 100)
    # the new arguments are keyword-only: a tenth positional argument is still the first of Application's
    with pytest.raises(TypeError):
        GrayScott(8, 1.0, 0.01, 0.09, 0.086, 2.0, "IMPL", 1e-10, 100, "bicgstab", t_start=0, t_stop=1, nt=3)


def test_device_description():
    app = make(20, newton_tol=1e-9, newton_maxiter=7, lin_tol=1e-8, lin_maxiter=9, **PARS["du=100dv"])
    imex = make(20, method="IMEX", linear_solver="direct", **PARS["du=100dv"]).device_stepper()
    assert app.device_stepper() == {**imex, "theta": 1.0, "newton_tol": 1e-9, "newton_maxiter": 7, "lin_tol": 1e-8, "lin_maxiter": 9}
    assert imex["kind"] == "grayscott2d" and "theta" not in imex
    # the defaults, 'direct' and 'EXPL' have no device form
    assert make(20, linear_solver="direct").device_stepper() is None
    assert make(20, method="EXPL", linear_solver="direct").device_stepper() is None


def test_a_direct_hierarchy_stays_on_the_plugin_path():
    from pymgrit_amd import Mgrit
    mg = Mgrit([make(8, linear_solver="direct", t_stop=0.01, nt=nt) for nt in (9, 3)], logging_lvl=30, max_iter=1)
    assert type(mg.backend).__name__ == "PluginBackend"


def _dense_preconditioner(app, dt):
    """P = blockdiag((1 + dt a) I - dt du L, (1 + dt b) I - dt dv L) as a dense long-double matrix from the stencil"""
    nx, n = app.nx, app.nx ** 2
    lap = np.zeros((n, n), dtype=LD)
    for i in range(nx):
        for j in range(nx):
            p = i * nx + j
            lap[p, p] -= 4
            for q in (((i + 1) % nx) * nx + j, ((i - 1) % nx) * nx + j, i * nx + (j + 1) % nx, i * nx + (j - 1) % nx):
                lap[p, q] += 1
    lap *= (LD(nx) / LD(app.L)) ** 2
    P = np.zeros((2 * n, 2 * n), dtype=LD)
    P[:n, :n] = (1 + LD(dt) * LD(app.a)) * np.eye(n, dtype=LD) - LD(dt) * LD(app.du) * lap
    P[n:, n:] = (1 + LD(dt) * LD(app.b)) * np.eye(n, dtype=LD) - LD(dt) * LD(app.dv) * lap
    return P


def test_newton_maxiter_1_is_one_correction():
    """one Newton correction with the inner solve run to lin_tol: x = w - delta, norm_2(g - J delta) <= lin_tol norm_2(g) for the
    recurrence residual, so delta is within lin_tol norm_2(g) / (1 - dt mu) of J^-1 g (norm_2(J^-1) <= 1 / (1 - dt mu) on the box), plus
    the rounding of lin_maxiter products with J, 4 EPS norm(J) norm_2(delta) each as test_hip_allen_cahn_newton.py counts them"""
    nx = 12
    app, full = make(nx, newton_maxiter=1), make(nx)
    w = random_state(np.random.default_rng(1), nx)
    counts = {}
    x = app._step_bicgstab(w, DT, counts)
    assert counts["newton_iterations"] == 1 and 1 <= counts["cg_iterations"] <= 8
    g = np.asarray(residual(w, w, DT, nx, par_of(app)), dtype=np.float64)
    J = jacobian(w, DT, nx, par_of(app))
    delta = np.linalg.solve(J.toarray(), g.ravel()).reshape(2, nx, nx)
    m = margin(app, DT, w)
    norm_j = 1.0 + DT * (8.0 * app.du / app.dx ** 2 + abs(app.a) + abs(app.b) + 3.0)
    allowed = (app.lin_tol * np.linalg.norm(g) + counts["cg_iterations"] * 4 * EPS * norm_j * np.linalg.norm(delta)) / m + 8 * EPS * np.linalg.norm(w)
    err = float(np.linalg.norm(x - (w - delta)))
    print(f"RATIO newton_maxiter_1: error/allowed {err / allowed:.4f}")
    assert err <= allowed, (err, allowed)
    assert np.linalg.norm(x - full._step_bicgstab(w, DT)) > 1e3 * allowed      # (and it is not the converged step)


def test_lin_maxiter_1_is_one_inner_iteration():
    """newton_maxiter = lin_maxiter = 1: delta = alpha y + omega z of the first BiCGStab iteration, formed here in long double with a
    dense P and the reference's J (nx = 4: 32 unknowns). The float64 step rounds each of its two preconditioner applications (four
    products of length nx: (4 nx + 8) EPS as for the IMEX step), its two products with J and its four inner products of 2 nx^2 terms
    ((2 nx^2 + 2) EPS each, their terms of one sign or nearly so for t . t and g . g; alpha and omega enter delta linearly):
    allowed = (2 (4 nx + 8) + 4 (2 nx^2 + 2) + 16) EPS cond norm_2(delta), cond = norm(J) norm(P^-1) <= norm(J)"""
    nx = 4
    app = make(nx, newton_maxiter=1, lin_maxiter=1)
    w = random_state(np.random.default_rng(2), nx)
    counts = {}
    x = app._step_bicgstab(w, DT, counts)
    assert counts == {"newton_iterations": 1, "cg_iterations": 1}
    g = residual(w, w, DT, nx, par_of(app)).ravel()
    J, Pinv = jacobian(w, DT, nx, par_of(app)).toarray().astype(LD), np.linalg.inv(_dense_preconditioner(app, DT).astype(np.float64)).astype(LD)
    y = Pinv @ g
    v = J @ y
    alpha = (g @ g) / (g @ v)
    s = g - alpha * v
    z = Pinv @ s
    t = J @ z
    omega = (t @ s) / (t @ t)
    delta = np.asarray(alpha * y + omega * z, dtype=np.float64).reshape(2, nx, nx)
    norm_j = 1.0 + DT * (8.0 * app.du / app.dx ** 2 + abs(app.a) + abs(app.b) + 3.0)
    allowed = (2 * (4 * nx + 8) + 4 * (2 * nx * nx + 2) + 16) * EPS * norm_j * float(np.linalg.norm(delta))
    err = float(np.linalg.norm(x - (w - delta)))
    print(f"RATIO lin_maxiter_1: error/allowed {err / allowed:.4f}")
    assert err <= allowed and np.linalg.norm(delta) > 1e-3, (err, allowed)
