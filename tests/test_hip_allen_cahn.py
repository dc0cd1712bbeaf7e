"""GPU tests of the Allen-Cahn IMEX stepper (csrc/mgrit_hip_allencahn.inc): every sweep of the device path against the SAME hierarchy on
the plugin path (the host ``step``), single steps against the reference fixtures (tests/golden/allen_cahn.*), solves against the
reference's residual histories. The oracle has no Allen-Cahn variant, so nothing here is bit for bit against another implementation:
the host step of this file is the same formula as the device's. The second implementation the device path is held against is the
transform-free long-double solve of tests/allen_cahn_reference.py, in tests/test_hip_allen_cahn_reference.py (size edges, other
exponents, several step sizes per level, sweeps of more than one batch). The bounds are derived (test_allen_cahn_cpu.py states them):

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
from periodic2d_sweeps import compare as _compare, host_state as _host_state, lists as _lists, row_norm as _row_norm, set_states as _set_states
from test_allen_cahn_cpu import ARR, EPS, META, check_history, ours_bound, reference_bound, step_input

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

T_SWEEP = 0.002     # sweeps: nt = 17 / 9 / 5 on [0, T_SWEEP], coarsening factor 2 -- every Phi of a relaxation acts on a stored state


def _host_class():
    from pymgrit_amd import AllenCahn

    class HostAllenCahn(AllenCahn):     # overriding step sends the hierarchy to the plugin path
        def step(self, u_start, t_start, t_stop):
            return super().step(u_start, t_start, t_stop)
    return HostAllenCahn


def _pair(nx, nts, t_stop, nu=2, **opts):
    from pymgrit_amd import AllenCahn, Mgrit
    opts.setdefault("nested_iteration", False)
    dev = Mgrit([AllenCahn(nx=nx, nu=nu, method="IMEX", t_start=0, t_stop=t_stop, nt=nt) for nt in nts], logging_lvl=30, **opts)
    host = Mgrit([_host_class()(nx=nx, nu=nu, method="IMEX", t_start=0, t_stop=t_stop, nt=nt) for nt in nts], logging_lvl=30, **opts)
    assert type(dev.backend).__name__ == "HipBackend" and type(host.backend).__name__ == "PluginBackend"
    return dev, host


def _random_states(host, seed, zero_g=False):
    rng = np.random.default_rng(seed)
    out = {}
    for lvl in range(host.lvl_max):
        for name, lst in _lists(host, lvl):
            n = host.problem[lvl].nx ** 2
            out[(name, lvl)] = np.zeros((len(lst), n)) if (zero_g and name == "g") else rng.uniform(-1.0, 1.0, size=(len(lst), n))
    return out


def _b_norm(app, rows, c):
    rows = np.abs(np.atleast_2d(rows))
    return float(np.max(np.linalg.norm(rows + c * np.abs(rows * (1.0 - rows ** app.nu)), axis=1)))


def _tol(host, lvl, rows):
    """TOL of the level for inputs among rows"""
    app = host.problem[lvl]
    c = float(np.max(np.diff(host.t[lvl]))) / app.eps ** 2
    return 2 * (4 * app.nx + 8) * EPS * _b_norm(app, rows, c)


SIZES = [9, 20, 63, 64, 66, 130, 200]


@pytest.mark.parametrize("nx", SIZES)
def test_every_sweep_matches_the_plugin_path(nx):
    assert torch.cuda.is_available()
    nts = (17, 9, 5)
    for w in (1.0, 1.3):
        dev, host = _pair(nx, nts, T_SWEEP, weight_c=w)
        top = dev.lvl_max - 1
        seed = 100 * nx

        def fresh():
            nonlocal seed
            seed += 1
            st = _random_states(host, seed)
            _set_states(dev, host, st)
            return st

        for lvl in range(top):
            st = fresh()
            slack = 8 * EPS * 3 * _row_norm(*st.values())
            dev.f_relax(lvl); host.f_relax(lvl)
            _compare(dev, host, lvl, _tol(host, lvl, st[("u", lvl)]) + slack, "f_relax")
            st = fresh()
            dev.c_relax(lvl); host.c_relax(lvl)
            _compare(dev, host, lvl, max(1.0, w) * _tol(host, lvl, st[("u", lvl)]) + slack * (abs(w) + abs(1 - w)), f"c_relax w={w}")
            st = fresh()
            dev.fas_residual(lvl); host.fas_residual(lvl)
            # g of the coarse level: one Phi of the fine level, one of the coarse level on restricted (= copied) rows of the fine u
            _compare(dev, host, lvl + 1, _tol(host, lvl, st[("u", lvl)]) + _tol(host, lvl + 1, st[("u", lvl)]) + slack, "fas_residual")
        # forward solve on the coarsest level: the chained bound
        st = fresh()
        dev.forward_solve(top); host.forward_solve(top)
        app, t = host.problem[top], host.t[top]
        uh = _host_state(host, "u", top)
        e = 0.0
        for k in range(1, len(t)):
            c = (t[k] - t[k - 1]) / app.eps ** 2
            R = float(np.abs(uh[k - 1]).max())
            lip = max(abs(1 + c), abs(1 + c * (1 - (app.nu + 1) * R ** app.nu)))
            e = lip * e + 2 * (4 * nx + 8) * EPS * _b_norm(app, uh[k - 1], c) + 8 * EPS * 3 * _row_norm(uh, st[("g", top)])
        _compare(dev, host, top, e, "forward_solve")
        for lvl in range(top - 1, -1, -1):
            st = fresh()
            dev.error_correction(lvl); host.error_correction(lvl)
            _compare(dev, host, lvl, 8 * EPS * 3 * _row_norm(*st.values()), "error_correction")
        st = fresh()
        got, ref = np.asarray(dev.compute_residual()), np.asarray(host.compute_residual())
        allowed = _tol(host, 0, st[("u", 0)]) + 8 * EPS * 3 * _row_norm(st[("u", 0)]) + (nx * nx + 2) * EPS * ref
        print(f"residual norms: worst deviation {np.abs(got - ref).max():.3e}, allowed {allowed.min():.3e}")
        assert got.shape == ref.shape and np.all(np.abs(got - ref) <= allowed), np.abs(got - ref).max()


@pytest.mark.parametrize("nx", [20, 63, 130])
def test_a_sweep_run_twice_gives_the_same_bits(nx):
    """a race in the fused prologue / epilogues would show here, where a tolerance would hide it"""
    assert torch.cuda.is_available()
    dev, host = _pair(nx, (17, 9, 5), T_SWEEP, weight_c=1.3)
    st = _random_states(host, nx)
    top = dev.lvl_max - 1
    sweeps = [("f_relax", lambda l=l: dev.f_relax(l)) for l in range(top)] + [("c_relax", lambda l=l: dev.c_relax(l)) for l in range(top)] + \
             [("fas_residual", lambda l=l: dev.fas_residual(l)) for l in range(top)] + [("forward_solve", lambda: dev.forward_solve(top))]
    for name, run in sweeps:
        out = []
        for rep in range(2):
            for (which, lvl), val in st.items():
                dev.backend.set_natural(which, lvl, val)
            run()
            out.append({key: dev.backend.natural(*key) for key in st})
        for key in st:
            assert np.array_equal(out[0][key], out[1][key]), (name, key)
    res = []
    for rep in range(2):
        for (which, lvl), val in st.items():
            dev.backend.set_natural(which, lvl, val)
        res.append(np.asarray(dev.compute_residual()))
    assert np.array_equal(res[0], res[1])


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
    st = _random_states(host, 7, zero_g=True)     # g = 0: plain time stepping, the states stay within [-1, 1]
    _set_states(dev, host, st)
    dev.forward_solve(1); host.forward_solve(1)
    app, t, uh = host.problem[1], host.t[1], _host_state(host, "u", 1)
    e = 0.0
    for k in range(1, len(t)):
        c = (t[k] - t[k - 1]) / app.eps ** 2
        R = float(np.abs(uh[k - 1]).max())
        lip = max(abs(1 + c), abs(1 + c * (1 - (app.nu + 1) * R ** app.nu)))
        e = lip * e + 2 * (4 * nx + 8) * EPS * _b_norm(app, uh[k - 1], c) + 8 * EPS * 3 * _row_norm(uh)
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
    hprob = [_host_class()(nx=20, method="IMEX", t_start=0, t_stop=META["t_stop"], nt=nt) for nt in (33, 9)]
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
