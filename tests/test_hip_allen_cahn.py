"""GPU tests of the Allen-Cahn IMEX stepper (csrc/mgrit_hip_allencahn.inc): every sweep of the device path against the SAME hierarchy on
the plugin path (the host ``step``), single steps against the reference fixtures (tests/golden/allen_cahn.*), solves against the
reference's residual histories. The oracle has no Allen-Cahn variant, so nothing here is bit for bit against another implementation:
the host step of this file is the same formula as the device's. The second implementation the device path is held against is the
transform-free long-double solve of tests/allen_cahn_reference.py, in tests/test_hip_allen_cahn_reference.py (size edges, other
exponents, several step sizes per level, sweeps of more than one batch). The bounds are derived (allen_cahn_fixtures.py states them):

  per Phi, one evaluation:                 norm_F(error) <= (4 nx + 8) eps norm_F(b)
  two independent evaluations (host, device):   twice that                                                          = TOL
  the sweep's own arithmetic (a handful of additions / multiplications per value, done on both sides):  8 eps * the largest
    Frobenius norm among the rows involved                                                                          = SLACK
  chained steps (forward_solve): e_k <= Lip_k e_(k-1) + TOL_k + SLACK,  Lip_k = max(|1 + c|, |1 + c (1 - (nu + 1) R^nu)|), c = dt / eps^2,
    R = the largest |value| of the step's input (the implicit solve itself is a contraction).
norm_F(b) is bounded from the input rows by norm_F(|u| + c |u (1 - u^nu)|) with the level's largest c.
"""
import logging
import types

import numpy as np
import pytest

import cases
from allen_cahn_fixtures import ARR, EPS, META, check_history, ours_bound, reference_bound, step_input
from periodic2d_kinds import KINDS
from periodic2d_sweeps import (ALL_SWEEPS, bounds_of, chain, check_every_sweep_twice, compare as _compare, host_class, host_state as _host_state, pair,
                               random_states, row_norm as _row_norm, run_sweeps, set_states as _set_states, uniform as _uniform)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

# sweeps: nt = 17 / 9 / 5 on [0, T_SWEEP], coarsening factor 2 -- every Phi of a relaxation acts on a stored state
T_SWEEP = KINDS["allencahn"].t_sweep(None)
BOUNDS = bounds_of("allencahn", "host")     # TOL of the module docstring: 2 (4 nx + 8) EPS bnorm with the level's largest c


def _pair(nx, nts, t_stop, nu=2, **opts):
    return pair("allencahn", nx, _uniform(nts, t_stop), par=dict(nu=nu), **opts)


SIZES = [9, 20, 63, 64, 66, 130, 200]


@pytest.mark.parametrize("nx", SIZES)
def test_every_sweep_matches_the_plugin_path(nx):
    assert torch.cuda.is_available()
    for w in (1.0, 1.3):
        dev, host = _pair(nx, (17, 9, 5), T_SWEEP, weight_c=w)
        run_sweeps(dev, host, BOUNDS, w, 100 * nx + 1, ALL_SWEEPS)


@pytest.mark.parametrize("nx", [20, 63, 130])
def test_a_sweep_run_twice_gives_the_same_bits(nx):
    """a race in the fused prologue / epilogues would show here, where a tolerance would hide it"""
    assert torch.cuda.is_available()
    dev, host = _pair(nx, (17, 9, 5), T_SWEEP, weight_c=1.3)
    check_every_sweep_twice(dev, random_states("allencahn", host, nx), residual=True)


@pytest.mark.parametrize("name", sorted(META["steps"]))
def test_single_device_phi_matches_the_reference(name):
    from pymgrit_amd import AllenCahn, Mgrit
    assert torch.cuda.is_available()
    rec = META["steps"][name]
    nx, dt = rec["nx"], rec["dt"]
    prob = [AllenCahn(nx=nx, nu=rec["nu"], eps=rec["eps"], method="IMEX", t_interval=t)
            for t in (dt * np.arange(5.0), dt * np.arange(0.0, 5.0, 2.0))]
    mg = Mgrit(prob, nested_iteration=False, logging_lvl=30)
    assert type(mg.backend).__name__ == "HipBackend"
    u, ref = step_input(prob[0], rec), ARR["out_" + name]
    rows = np.zeros((5, nx * nx))
    rows[0] = rows[2] = u.ravel()
    mg.backend.set_natural("u", 0, rows)
    mg.f_relax(0)
    got = mg.backend.natural("u", 0)
    step = float(mg.t[0][1] - mg.t[0][0])
    tol = reference_bound(rec, ref) + ours_bound(prob[0], u, step)
    for i in (1, 3):
        step_i = float(mg.t[0][i] - mg.t[0][i - 1])
        # (k dt - (k - 1) dt is dt to a relative 2 eps: d Phi / d dt is bounded by (|L b| + |u (1 - u^nu)| / eps^2), far below the bound)
        assert abs(step_i - dt) <= 4 * EPS * dt
        err = float(np.abs(got[i].reshape(nx, nx) - ref).max())
        print(f"{name} row {i}: err {err:.3e} allowed {tol:.3e}")
        assert err <= tol, (name, i, err, tol)


@pytest.mark.parametrize("name", sorted(k for k, v in META["solve"].items() if v["method"] == "IMEX"))
def test_solves_match_the_reference_and_the_plugin_path(name):
    assert torch.cuda.is_available()
    rec = META["solve"][name]
    dev, host = _pair(rec["nx"], rec["nts"], META["t_stop"], **rec["opts"])
    conv, hconv = dev.solve()["conv"], host.solve()["conv"]
    u = dev.backend.natural("u", 0)
    norm_u = cases.spacetime_norm(u)
    check_history(name, conv, norm_u)
    assert len(conv) == len(hconv)
    dev_host = np.abs(np.asarray(conv) - np.asarray(hconv))
    print(f"{name}: device against plugin path, largest deviation {np.max(dev_host) / (EPS * norm_u):.2f} units of eps*norm(u)")
    assert np.all(dev_host <= 1e-10 * np.asarray(hconv) + cases.BLK_K * EPS * norm_u), (conv, hconv)
    last = ARR["last_" + name].ravel()
    assert np.abs(u[-1] - last).max() <= 1e-9 * np.abs(last).max()
    assert np.abs(np.asarray(dev.u[0][len(u) - 1].get_values()).ravel() - last).max() <= 1e-9 * np.abs(last).max()


def test_long_coarsest_level_is_solved_step_by_step(monkeypatch):
    """64 coarsest steps: the time-parallel block solve (linear Phi only) must not be chosen, whatever coarse_solve says"""
    from pymgrit_amd.core.options import options
    assert torch.cuda.is_available()
    nx, nts, t_stop = 16, (257, 65), 0.0064      # coarse dt = 1e-4: c = 0.0625
    for setting in ("auto", "sequential"):
        try:
            options.coarse_solve = setting
            dev, host = _pair(nx, nts, t_stop)
        finally:
            options.reset("coarse_solve")
        assert dev.backend.block_r[1] == 0 and dev.backend.block_solve_form(1) == 0
    st = random_states("allencahn", host, 7, zero_g=True)     # g = 0: plain time stepping, the states stay within [-1, 1]
    _set_states(dev, host, st)
    dev.forward_solve(1); host.forward_solve(1)
    uh = _host_state(host, "u", 1)
    e = chain(BOUNDS, host, host.problem[1], host.t[1], uh, 8 * EPS * 3 * _row_norm(uh))
    _compare(dev, host, 1, e, "forward_solve, 64 steps")
    dev2, host2 = _pair(nx, nts, t_stop, max_iter=2, tol=0.0)
    conv, hconv = dev2.solve()["conv"], host2.solve()["conv"]
    norm_u = cases.spacetime_norm(dev2.backend.natural("u", 0))
    assert len(conv) == len(hconv) and np.all(np.abs(conv - hconv) <= 1e-10 * hconv + cases.BLK_K * EPS * norm_u), (conv, hconv)


def test_output_fcn_and_cf_iter():
    from pymgrit_amd import AllenCahn, Mgrit
    assert torch.cuda.is_available()
    seen = []
    prob = [AllenCahn(nx=20, method="IMEX", t_start=0, t_stop=META["t_stop"], nt=nt) for nt in (33, 9)]
    mg = Mgrit(prob, logging_lvl=30, cf_iter=2, max_iter=3, tol=0.0, output_fcn=lambda s: seen.append(float(s.u[0][-1].norm())))
    hprob = [host_class(AllenCahn)(nx=20, method="IMEX", t_start=0, t_stop=META["t_stop"], nt=nt) for nt in (33, 9)]
    hseen = []
    hmg = Mgrit(hprob, logging_lvl=30, cf_iter=2, max_iter=3, tol=0.0, output_fcn=lambda s: hseen.append(float(s.u[0][-1].norm())))
    conv, hconv = mg.solve()["conv"], hmg.solve()["conv"]
    norm_u = cases.spacetime_norm(mg.backend.natural("u", 0))
    assert len(conv) == len(hconv) and np.all(np.abs(conv - hconv) <= 1e-10 * hconv + cases.BLK_K * EPS * norm_u), (conv, hconv)
    assert len(seen) == len(hseen) >= 1 and np.allclose(seen, hseen, rtol=1e-10, atol=0)


def test_newton_methods_run_on_the_plugin_path(caplog):
    from pymgrit_amd import AllenCahn, Mgrit
    prob = [AllenCahn(nx=16, method="IMPL", t_start=0, t_stop=0.002, nt=nt) for nt in (17, 5)]
    mg = Mgrit(prob, logging_lvl=30, max_iter=1)
    assert type(mg.backend).__name__ == "PluginBackend"
    assert len(mg.solve()["conv"]) >= 1
    # a hierarchy that mixes a device-capable level with a host-only one warns and runs on the plugin path, like other host hierarchies
    mixed = [AllenCahn(nx=16, method="IMEX", t_start=0, t_stop=0.002, nt=9), AllenCahn(nx=16, method="IMPL", t_start=0, t_stop=0.002, nt=3)]
    with caplog.at_level(logging.WARNING):
        mg = Mgrit(mixed, logging_lvl=30, max_iter=1)
    assert type(mg.backend).__name__ == "PluginBackend"
    assert any("no device description" in r.getMessage() for r in caplog.records)


def test_what_is_not_covered_is_refused():
    from pymgrit_amd import AllenCahn, AtMgrit, Mgrit
    from pymgrit_amd.core.backend_hip import HipBackend
    from pymgrit_amd.core.hip_lib import MgritHipError

    def prob():
        return [AllenCahn(nx=12, method="IMEX", t_start=0, t_stop=0.002, nt=nt) for nt in (9, 3)]
    with pytest.raises(MgritHipError, match="AT-MGRIT is not supported"):
        AtMgrit(k=2, problem=prob(), logging_lvl=30)
    with pytest.raises(MgritHipError, match="global convergence criteria only"):
        Mgrit(prob(), conv_crit=2, logging_lvl=30)
    stub = types.SimpleNamespace(desc=[p.device_stepper() for p in prob()])
    with pytest.raises(MgritHipError, match="one time rank only"):
        HipBackend._check_periodic(stub, types.SimpleNamespace(comm_time_size=2, global_conv_crit=True), "allencahn2d")
    with pytest.raises(Exception, match="outside"):
        Mgrit([AllenCahn(nx=3, method="IMEX", t_start=0, t_stop=0.002, nt=nt) for nt in (9, 3)], logging_lvl=30)
