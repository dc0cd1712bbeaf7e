"""GPU: corrected level-0 C-points the way up does not store because nobody reads them before they are overwritten
(include/mgrit_hip.h, mgrit_hip_lagged). A lagging mgrit_hip_ec_relax_res(store_all_f = 2) leaves P = Phi(F''_last) in row cend-1 and
row cend in turn and the uncorrected C-point in the other one; mgrit_hip_cf_fas(pre_relaxed = 1) reads P where it is, and every
other way into level 0 -- or into u of level 1 -- finds the rows put in place first. Everything is compared bit for bit with the same
sequence run with the switch off (MGRIT_HIP_LAG=0), and against the oracle. Hierarchy: Heat1D, 3 levels, m = 4, nt = 257 (64 level-0
intervals) at one state size per kernel instance, in chunks of 3, 4 and 16 intervals (chunk starts, a chunk cut, a short last
chunk), and nt = 1025 (a coarsest level of four blocks)."""
import ctypes as C

import numpy as np
import pytest

import heat1d_cycles as hc
from heat1d_cycles import DOWN, UP, coarse_state, lagged, need_gpu, problem, same, coarse_cycle as cycle, lag_build as build

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

# (nx, forcing, nt, chunk)
SHAPES = [(nx, forcing, 257, 4) for nx in hc.SIZES for forcing in (False, True)] + \
         [(4097, True, 257, 3), (16382, True, 257, 16), (1022, True, 1025, 16)]
GUARD_SHAPE = (4097, True, 257, 4)


def after(mg, name, col=2):
    return [rec[col] for rec in mg.backend.lib.log if rec[0] == name]


_OFF = {}     # shape -> what six cycles with the switch off leave, level 0 looked at behind every one (computed once, never modified)


def off_run(shape):
    """mode 0: per cycle [residual, coarse slabs..., natural u of level 0]. (The look changes no bit of a later cycle: with the
    switch off that is what tests/test_hip_deferred_rows.py holds the engine to.)"""
    if shape not in _OFF:
        mg = build(*shape, 0)
        out = []
        for it in range(6):
            out.append(cycle(mg, it) + [mg.backend.natural("u", 0)])
        assert set(after(mg, DOWN) + after(mg, UP)) == {-1}, "pending with the switch off"
        _OFF[shape] = (out, np.array(mg.conv[1:7]))
    return _OFF[shape]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"nx{s[0]}_{'forcing' if s[1] else 'plain'}_nt{s[2]}_chunk{s[3]}")
def test_six_cycles_bit_identical_and_lagged(shape, oracle):
    need_gpu()
    off, conv_off = off_run(shape)
    # one solver, six cycles nobody looks at level 0 in between: lagged(1), lagged(0), lagged(1), ... behind the way ups
    mg = build(*shape, 2)
    for it in range(6):
        same(cycle(mg, it), off[it][:-1], (shape, "cycle", it))
        assert lagged(mg) >= 0
    same([mg.backend.natural("u", 0)], off[5][-1:], (shape, "level 0 behind cycle 6"))
    assert lagged(mg) == -1
    # that it happened: every way up leaves its list pending, every way down drops it (and defers from the second cycle on)
    down, up = after(mg, DOWN), after(mg, UP)
    assert len(up) == 6 and all(d >= 0 for d in up) and len(set(up)) == 1, up
    assert down == [-1] * 6, down
    assert after(mg, DOWN, 1) == [0, 1, 1, 1, 1, 1] and after(mg, UP, 1) == [2] * 6
    assert all(d >= 0 for d in after(mg, DOWN, 3)[1:])
    assert np.array_equal(np.array(mg.conv[1:7]), conv_off)
    # level 0 behind cycles 1..6, each on a fresh solver: the rows put in place from lagged(1) (odd) and from lagged(0) (even)
    for n in range(1, 7):
        mg_n = build(*shape, 2)
        for it in range(n):
            cycle(mg_n, it)
        assert lagged(mg_n) >= 0
        same([mg_n.backend.natural("u", 0)], off[n - 1][-1:], (shape, "level 0 behind cycle", n))
    # ... and against the oracle: the same cycles, the residual history to rounding of the norm, level 0 bit for bit
    hc.against_oracle(oracle, mg, off[5][-1], hc.heat_specs(*shape[:3]), 6)


def test_mode_0_never_lags():
    need_gpu()
    off_run(GUARD_SHAPE)      # (asserts it)


def test_store_all_f_never_lags(monkeypatch):
    need_gpu()
    monkeypatch.setenv("PYMGRIT_AMD_STORE_ALL_F", "1")
    mg = build(1022, True, 257, 4, 2)
    for it in range(3):
        cycle(mg, it)
    log = mg.backend.lib.log
    assert after(mg, UP, 1) == [1, 1, 1] and {x[2] for x in log} == {-1}, log


def test_loopback_ranks_never_lag():
    need_gpu()
    from pymgrit_amd.core.comm import run_loopback_ranks

    def rank(comm):
        mg = build(1022, True, 257, 4, 2, comm=comm, max_iter=3)
        assert mg.backend.device_links
        mg.solve()
        mg.backend.sync()
        return mg.backend.lib.log
    world, logs = run_loopback_ranks(2, rank)
    world.close()
    for log in logs:
        assert any(x[0] == DOWN for x in log) and {x[2] for x in log} == {-1}, log


@pytest.mark.parametrize("blocks", [1, 3])
def test_planned_cycles(blocks):
    """a planned cycle runs launch by launch twice (a block's way up lags, the next pass of another block has the rows put in place),
    then as a captured graph, into which nothing lags and nothing is settled"""
    need_gpu()
    shape = GUARD_SHAPE
    with hc.planned_graph():
        runs = []
        for lag in (0, 2):
            mg = build(*shape, lag, **({} if blocks == 1 else dict(plan_blocks=blocks)))
            runs.append((mg, [cycle(mg, it) for it in range(5)] + [[mg.backend.natural("u", 0)]]))
    (mg_off, off), (mg_on, on) = runs
    for it, (a, b) in enumerate(zip(on, off)):
        same(a, b, (blocks, "cycle", it))
    same(off[-1], off_run(shape)[0][4][-1:], (blocks, "planned against program order"))
    assert {x[2] for x in mg_off.backend.lib.log} == {-1}
    log = mg_on.backend.lib.log
    captured = [x for x in log if x[4]]
    assert any(x[0] == UP for x in captured), log
    assert {x[2] for x in captured} == {-1}, captured
    assert any(x[0] == UP and x[2] >= 0 for x in log if not x[4]), log
    assert lagged(mg_on) == -1


def timed_then_replayed(lag, timed):
    """a one-block planned cycle: launch by launch twice, captured, replayed; then `timed` cycles with the sweeps timed, which run
    launch by launch on the same plan (and may lag), then replays again -- a replay goes past the engine"""
    mg = build(*GUARD_SHAPE, lag, max_iter=12)
    be = mg.backend
    out = [cycle(mg, it) for it in range(5)]
    assert any(x[4] for x in be.lib.log), "no cycle was captured"
    calls = len(be.lib.log)
    out.append(cycle(mg, 5))
    assert len(be.lib.log) == calls, "the sixth cycle was not a replay"
    if timed == "first iteration":     # the plan of a solve's first iteration: launch by launch, from plain rows (lagged(1))
        timed = 1
        out.append(cycle(mg, 0))
    else:
        be.set_timing(True)
        out += [cycle(mg, it) for it in range(6, 6 + timed)]
        be.set_timing(False)
        be.timing_drain()
    assert len(be.lib.log) == calls + 2 * timed and (lagged(mg) >= 0) == (lag > 0), (lag, after(mg, UP))
    calls = len(be.lib.log)
    out += [cycle(mg, it) for it in range(6 + timed, 8 + timed)]
    assert len(be.lib.log) == calls and lagged(mg) == -1, "replays, in front of which the rows were put in place"
    return out + [[be.natural("u", 0)]]


@pytest.mark.parametrize("lag,timed", [(2, 1), (2, 2), (1, 3), (1, 4), (2, "first iteration")])
def test_replay_behind_cycles_that_lagged(lag, timed):
    """mode 2 lags in the first launch-by-launch cycle behind the graph (lagged(0): the way up is the partner of a deferring way
    down), mode 1 in the third; one cycle more leaves the other parity. Behind lagged(1) the graph itself reads the right rows, but
    the record would stay pending through the replays and the next look would rebuild row cend from rows the graph has rewritten"""
    need_gpu()
    with hc.planned_graph():
        off, on = timed_then_replayed(0, timed), timed_then_replayed(lag, timed)
    for k, (a, b) in enumerate(zip(on, off)):
        same(a, b, (lag, timed, k))


def test_two_solves_on_one_solver():
    """mode 2, planned cycles: the second solve() runs the first iteration's plan launch by launch, which lags, and then replays the
    graph of the later iterations"""
    need_gpu()
    with hc.planned_graph():
        got = []
        for lag in (0, 2):
            mg = build(*GUARD_SHAPE, lag, max_iter=6)
            out = []
            for _ in range(2):
                res = mg.solve()
                out += [np.array(res["conv"]), mg.backend.natural("u", 0)] + coarse_state(mg)
                assert lagged(mg) == -1
            if lag:
                assert any(x[4] for x in mg.backend.lib.log) and any(x[0] == UP and x[2] >= 0 for x in mg.backend.lib.log)
            got.append(out)
    same(got[1], got[0], "two solves")


# ---- the waiting rule of mode 1 ---------------------------------------------------------------------------------------------
def test_waiting_rule():
    need_gpu()
    shape = GUARD_SHAPE
    got = []
    for lag in (0, 1):
        mg = build(*shape, lag, max_iter=20)
        out = [cycle(mg, it) for it in range(5)]
        if lag:      # cycle 0 is nobody's partner, cycles 1 and 2 are counted, cycle 3 lags
            up = after(mg, UP)
            assert up[:3] == [-1] * 3 and up[3] >= 0 and up[4] >= 0, up
        out.append([mg.backend.natural("u", 0)])      # a miss: wait 2 -> 4
        assert lagged(mg) == -1
        out += [cycle(mg, it) for it in range(5, 11)]
        if lag:      # the cycle behind the look starts from plain rows (no partner), then four partner way ups wait, the fifth lags
            up = after(mg, UP)
            assert up[5:10] == [-1] * 5 and up[10] >= 0, up
        out.append([mg.backend.natural("u", 0)])
        got.append(out)
    for k, (a, b) in enumerate(zip(got[1], got[0])):
        same(a, b, ("waiting rule", k))


# ---- the guard: with a record pending, every other way into level 0 (or u of level 1) sees the rows in place --------------------
def pending(mg, parity):
    """one cycle leaves lagged(1), two leave lagged(0)"""
    n = 1 if parity == 1 else 2
    for it in range(n):
        cycle(mg, it)
    return n


def finish(mg, n, extra=()):
    """two whole cycles behind whatever the guard test did, then everything there is to see"""
    out = list(extra)
    for it in range(n, n + 2):
        out += cycle(mg, it)
    return out + [mg.backend.natural("u", 0)]


def guard(action):
    return lambda mg, n: finish(mg, n, action(mg))


def g_vector_write(mg, n):
    vec = mg.u[1][3]          # (a coarse row: any vector of the right size)
    mg.u[0][8] = vec
    mg.u[0][11] = vec
    return finish(mg, n)


def g_relax_level_1(mg, n):
    """writes u of level 1, which the record needs as the way up found it"""
    mg.backend.relax(1, mg._f_runs(1), 'F')
    assert lagged(mg) == -1
    return finish(mg, n, [mg.backend.natural("u", 1)])


def g_settle(lvl):
    def run(mg, n):
        hc.settle(lvl)(mg)
        assert lagged(mg) == -1
        return finish(mg, n, hc.raw_U((0,))(mg))
    return run


def g_second_way_up(mg, n):
    mg._up(0, mg._level_intervals(0))
    mg.convergence_criterion(iteration=n + 1)
    return finish(mg, n, [np.asarray(mg.compute_residual())])


GUARDS = {"natural": guard(hc.natural("u", 0)), "U": guard(hc.U((0,))), "raw_U": guard(hc.raw_U((0,))),
          "payload": guard(hc.payload(0, (4, 8, 255, 256))), "vector_read": guard(hc.vector_read("u", 0, (4, 7, 8, 256))),
          "vector_write": g_vector_write, "set_natural": guard(hc.set_natural_level0), "relax_F": guard(hc.relax_level0('F')),
          "relax_C": guard(hc.relax_level0('C')), "relax_FC": guard(hc.relax_level0('FC')), "residual": guard(hc.residual_norms_fresh),
          "correction_by_hand": guard(hc.correction_by_hand(0)), "relax_level_1": g_relax_level_1, "settle_0": g_settle(0),
          "settle_1": g_settle(1), "second_way_up": g_second_way_up}


@pytest.mark.parametrize("parity", [1, 0])
@pytest.mark.parametrize("name", sorted(GUARDS))
def test_guard(name, parity):
    need_gpu()
    got = []
    for lag in (0, 2):
        mg = build(*GUARD_SHAPE, lag)
        n = pending(mg, parity)
        assert (lagged(mg) >= 0) == (lag == 2), (name, lag)
        got.append(GUARDS[name](mg, n))
        assert lagged(mg) == -1
    same(got[1], got[0], (name, parity))


# ---- other cycle forms --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["F_cycle", "cf_iter2", "four_levels", "defer_off", "mirror"])
def test_other_cycle_forms(name):
    need_gpu()
    kw = {"F_cycle": dict(cycle_type='F'), "cf_iter2": dict(cf_iter=2), "four_levels": dict(levels=4), "defer_off": dict(env={"MGRIT_HIP_DEFER": "0"}),
          "mirror": {}}[name]
    shape = (4097, True, 1025 if name == "four_levels" else 257, 4)
    runs = []
    for lag in (0, 2):
        mg = build(*shape, lag, **kw)
        out = []
        if name == "mirror":      # every corrected C-point also goes to a slab of the caller's: the same rows whether the pass lags or not
            pts = [int(i) for i in mg.index_local_c[0]]
            mg.backend.mirror_cpoints(0, pts)
        for it in range(4):
            out.append(cycle(mg, it))
            if name == "mirror":
                out[-1].append(mg.backend._snap[0].cpu().numpy())
        up, down = after(mg, UP), after(mg, DOWN)
        if lag == 0 or name == "cf_iter2":      # (cf_iter = 2: a plain C-relaxation reads the level next, so the way up stores mode 0)
            assert set(up + down) == {-1}, (name, lag, up, down)
        else:
            assert all(d >= 0 for d in up) and set(down) == {-1}, (name, lag, up, down)
        if name == "defer_off":      # the way down finds the rows put in place and stores row cend: every way up reads it there
            assert set(after(mg, DOWN, 3)) == {-1}
        out.append([mg.backend.natural("u", 0)])
        assert lagged(mg) == -1
        runs.append(out)
    for it, (a, b) in enumerate(zip(runs[1], runs[0])):
        same(a, b, (name, it))


def test_switch_and_argument_checks():
    need_gpu()
    mg = build(1022, True, 257, 4, 0)
    lib, h = mg.backend.lib, mg.backend.h
    null = C.c_void_p(None)
    assert lib.mgrit_hip_lagged(null, 0) == -2 and lib.mgrit_hip_lagged(h, -1) == -2 and lib.mgrit_hip_lagged(h, 99) == -2
    assert lib.mgrit_hip_lagged(h, 0) == -1 and lib.mgrit_hip_lagged(h, 1) == -1
    assert lib.mgrit_hip_set_lag(null, 1) != 0 and lib.mgrit_hip_set_lag(h, 3) != 0 and lib.mgrit_hip_set_lag(h, -1) != 0
    assert lib.mgrit_hip_lag_settle(null, 0) != 0 and lib.mgrit_hip_lag_settle(h, -1) != 0 and lib.mgrit_hip_lag_settle(h, 99) != 0
    assert lib.mgrit_hip_lag_settle(h, 0) == 0 and lib.mgrit_hip_lag_settle(h, 1) == 0
    # the setter: off (the environment), eager for the second cycle, off again for the third
    cycle(mg, 0)
    assert lagged(mg) == -1
    assert lib.mgrit_hip_set_lag(h, 2) == 0
    cycle(mg, 1)
    assert lagged(mg) >= 0
    # a record that is pending stays pending when the switch goes off; its partner drops it
    assert lib.mgrit_hip_set_lag(h, 0) == 0 and lagged(mg) >= 0
    cycle(mg, 2)
    assert lagged(mg) == -1 and after(mg, DOWN) == [-1] * 3 and after(mg, DOWN, 3)[2] >= 0
    # the lag-only settle touches no other record: pending rows of the way down stay pending
    assert lib.mgrit_hip_set_lag(h, 2) == 0
    cycle(mg, 3)
    assert lagged(mg) >= 0 and lib.mgrit_hip_lag_settle(h, 0) == 0 and lagged(mg) == -1
    mg0 = build(1022, True, 257, 4, 0)
    for it in range(4):
        cycle(mg0, it)
    same([mg.backend._U[0].cpu().numpy()], [mg0.backend._U[0].cpu().numpy()], "raw rows behind the lag-only settle")


def test_environment_variable(monkeypatch):
    """MGRIT_HIP_LAG as a child process finds it when its engine is made: 2 lags in the second cycle. Unset, the engine waits (this
    process: nothing lags in the second cycle, and the setter's refusals have left the mode alone)"""
    need_gpu()
    from pymgrit_amd import Mgrit
    monkeypatch.delenv("MGRIT_HIP_LAG", raising=False)
    mg = Mgrit(problem(1022, True, 257), logging_lvl=30, max_iter=2, tol=0.0)
    for it in range(2):
        cycle(mg, it)
    assert mg.backend.lib.mgrit_hip_lagged(mg.backend.h, 0) == -1
    got = hc.child_cycles({"MGRIT_HIP_LAG": "2"}, 2, cycle="coarse_cycle")
    assert got["lagged"] >= 0, got
