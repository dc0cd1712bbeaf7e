"""GPU: the way up of levels 1 and 0 in one pass (include/mgrit_hip.h, mgrit_hip_up2_pending). Where the level-0 way up lags,
mgrit_hip_ec_relax of level 1 launches nothing and the level-0 pass computes u of level 1 where it needs it (up2_kernel); u of level 1
is brought up -- by the deferred pass, run late -- only for whoever asks. Everything is compared bit for bit with the same sequence
run with the switch off (MGRIT_HIP_UP2=0) in the same process, and against the oracle's level 0 and residual history. The solver
is the lag tests' (heat1d_cycles.lag_build) with MGRIT_HIP_UP2 beside MGRIT_HIP_LAG; pending_trace.py scripts the same guards. Hierarchy:
Heat1D, 3 levels, m = 4, at one state size per kernel instance, with and without forcing, level-0 chunks of 4 and 16 intervals
(a chunk must start on a C-point of level 1's own coarsening to pair: chunks of 3, and m = (4, 3), do not)."""
import ctypes as C

import numpy as np
import pytest

import cases
import heat1d_cycles as hc
from heat1d_cycles import (blind_cycle, coarse_state, half_cycle, lagged, need_gpu, same, coarse_cycle as cycle, up2_finish as finish,
                           up2_pending as pending, UP2_GUARDS as GUARDS)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

# (nx, forcing, nt, chunk): one wave per state / 512 threads / 1024 threads, each with and without forcing; chunks of 16; a coarsest
# level that steps sequentially (nt = 257)
SHAPES = [(nx, forcing, 1025, chunk) for chunk in (4, 16) for nx in hc.SIZES for forcing in (False, True)] + [(4097, True, 257, 4)]
GUARD_SHAPE = (4097, True, 257, 4)


def build(nx, forcing, nt, chunk, up2, lag=2, env=(), **kw):
    return hc.lag_build(nx, forcing, nt, chunk, lag, env=dict(env, MGRIT_HIP_UP2=str(up2)), **kw)


_OFF = {}     # shape -> what six cycles with the switch off leave (computed once, never modified)


def off_run(shape):
    """MGRIT_HIP_UP2=0, lag mode 2: per cycle [residual, coarse slabs..., natural u of level 0]"""
    if shape not in _OFF:
        mg = build(*shape, 0)
        out = []
        for it in range(6):
            out.append(cycle(mg, it) + [mg.backend.natural("u", 0)])
            assert pending(mg) == 0
        _OFF[shape] = (out, np.array(mg.conv[1:7]))
    return _OFF[shape]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"nx{s[0]}_{'forcing' if s[1] else 'plain'}_nt{s[2]}_chunk{s[3]}")
def test_six_cycles_bit_identical_and_fused(shape, oracle):
    need_gpu()
    off, conv_off = off_run(shape)
    # one solver, six cycles; the look at the coarse slabs behind every cycle brings level 1 up from the record
    mg = build(*shape, 1)
    for it in range(6):
        res = blind_cycle(mg, it)
        # the first cycle's way down is nobody's partner and defers nothing: two passes; from the second on, one
        assert pending(mg) == (0 if it == 0 else 2), (shape, it)
        assert lagged(mg) >= 0
        same(res + coarse_state(mg), off[it][:-1], (shape, "cycle", it))
        assert pending(mg) == 0 and lagged(mg) >= 0      # (level 1 is brought up; the lagged rows of level 0 stay as they are)
    same([mg.backend.natural("u", 0)], off[5][-1:], (shape, "level 0 behind cycle 6"))
    assert np.array_equal(np.array(mg.conv[1:7]), conv_off)
    # six cycles nobody looks into: every way down drops the record unread; level 0 behind cycles 1..6, each on a fresh solver
    for n in range(1, 7):
        mg_n = build(*shape, 1)
        for it in range(n):
            same(blind_cycle(mg_n, it), off[it][:1], (shape, "blind cycle", it))
        assert pending(mg_n) == (0 if n == 1 else 2) and lagged(mg_n) >= 0
        same([mg_n.backend.natural("u", 0)], off[n - 1][-1:], (shape, "level 0 behind cycle", n))
        assert pending(mg_n) == 0
        if n == 6:
            same(coarse_state(mg_n), off[5][1:-1], (shape, "coarse levels behind six blind cycles"))
    # ... and against the oracle: the residual history to rounding of the norm, level 0 bit for bit
    hc.against_oracle(oracle, mg, off[5][-1], hc.heat_specs(*shape[:3]), 6)


def test_cpoint_followed_by_cpoint():
    """a level-1 run list with a C-point that another C-point follows (m = (4, 1) is no hierarchy: the time grid of level 2 keeps two
    neighbours of level 1): nt = 1025, level 2 = every fourth point of level 1 plus point 5"""
    need_gpu()
    from pymgrit_amd import Heat1D
    got = []
    for up2 in (0, 1):
        kw = dict(x_start=0, x_end=1, nx=1022, a=1, init_cond=cases.init_cond, rhs_separable=[(cases.rhs_space, cases.rhs_time)])
        t0 = np.linspace(0, 2, 1025)
        t1 = t0[::4]
        idx2 = np.unique(np.concatenate((np.arange(0, 257, 4), [5])))
        prob = [Heat1D(t_start=0, t_stop=2, nt=1025, **kw), Heat1D(t_interval=t1, **kw), Heat1D(t_interval=t1[idx2], **kw)]
        mg = hc.build(prob, env={"MGRIT_HIP_LAG": "2", "MGRIT_HIP_UP2": str(up2)}, chunk=4, max_iter=6, tol=0.0)
        be = mg.backend
        out, seen = [], []
        for it in range(4):
            out += blind_cycle(mg, it)
            seen.append(be.lib.mgrit_hip_up2_pending(be.h))
            out += coarse_state(mg)
        out.append(be.natural("u", 0))
        assert seen == ([0, 2, 2, 2] if up2 else [0] * 4), seen
        got.append(out)
    same(got[1], got[0], "C-point followed by a C-point")


@pytest.mark.parametrize("name", ["chunks_of_3", "m_4_3"])
def test_does_not_pair(name):
    need_gpu()
    got = []
    for up2 in (0, 1):
        if name == "chunks_of_3":
            mg = build(4097, True, 257, 3, up2)
        else:
            from pymgrit_amd import Heat1D
            kw = dict(x_start=0, x_end=1, nx=1022, a=1, init_cond=cases.init_cond, t_start=0, t_stop=2)
            mg = hc.build([Heat1D(nt=nt, **kw) for nt in (769, 193, 65)], env={"MGRIT_HIP_LAG": "2", "MGRIT_HIP_UP2": str(up2)}, chunk=4,
                          max_iter=6, tol=0.0)
        out = []
        for it in range(3):
            out += blind_cycle(mg, it)
            assert mg.backend.lib.mgrit_hip_up2_pending(mg.backend.h) == 0 and mg.backend.lib.mgrit_hip_lagged(mg.backend.h, 0) >= 0
            out += coarse_state(mg)
        got.append(out + [mg.backend.natural("u", 0)])
    same(got[1], got[0], name)


def test_never_pending_mode_0_lag_0_store_all_f(monkeypatch):
    need_gpu()
    for kw in (dict(up2=0), dict(up2=1, lag=0)):
        mg = build(1022, True, 257, 4, **kw)
        for it in range(3):
            blind_cycle(mg, it)
            assert pending(mg) == 0
    monkeypatch.setenv("PYMGRIT_AMD_STORE_ALL_F", "1")
    mg = build(1022, True, 257, 4, 1)
    for it in range(3):
        blind_cycle(mg, it)
        assert pending(mg) == 0 and lagged(mg) == -1


def test_loopback_ranks_never_pending():
    need_gpu()
    from pymgrit_amd.core.comm import run_loopback_ranks

    def rank(comm):
        mg = build(1022, True, 257, 4, 1, comm=comm, max_iter=3)
        assert mg.backend.device_links
        seen = []
        for it in range(3):
            blind_cycle(mg, it)
            seen.append(pending(mg))
        mg.backend.sync()
        return seen
    world, seen = run_loopback_ranks(2, rank)
    world.close()
    assert seen == [[0, 0, 0], [0, 0, 0]], seen


@pytest.mark.parametrize("blocks", [1, 3])
def test_planned_cycles_never_pending_inside_a_capture(blocks):
    need_gpu()
    with hc.planned_graph():
        runs = []
        for up2 in (0, 1):
            mg = build(*GUARD_SHAPE, up2, **({} if blocks == 1 else dict(plan_blocks=blocks)))
            out, seen = [], []
            for it in range(5):
                out += blind_cycle(mg, it)
                seen.append((pending(mg), any(x[4] for x in mg.backend.lib.log)))
                out += coarse_state(mg)
            runs.append((out + [mg.backend.natural("u", 0)], seen, mg))
    same(runs[1][0], runs[0][0], (blocks, "planned"))
    assert any(c for _, c in runs[1][1]), "no cycle was captured"
    assert all(p == 0 for p, c in runs[1][1] if c), runs[1][1]      # captured and replayed cycles leave nothing pending
    assert all(p == 0 for p, _ in runs[0][1])


# ---- the guard: with a record pending, every way to a row it needs finds the rows of the two passes -------------------------------
@pytest.mark.parametrize("state", ["done1", "done0", "noted"])
@pytest.mark.parametrize("name", sorted(GUARDS))
def test_guard(name, state):
    need_gpu()
    got = []
    for up2 in (0, 1):
        mg = build(*GUARD_SHAPE, up2)
        n = {"done1": 3, "done0": 2, "noted": 2}[state]
        for it in range(n):
            blind_cycle(mg, it)
        rest = None
        if state == "noted":
            rest = half_cycle(mg, n)
            n += 1
        assert pending(mg) == (0 if not up2 else 1 if state == "noted" else 2), (name, state, up2)
        out = GUARDS[name](mg)
        out = [np.asarray(x) for x in out] if isinstance(out, list) else []
        # (a second way up of level 1 in the middle of the cycle is noted again: the level-0 way up that follows still lags)
        assert pending(mg) == (1 if (name, state, up2) == ("second_way_up_1", "noted", 1) else 0), (name, state)
        if rest is not None:      # the level-0 way up of the interrupted cycle, in two passes now
            mg.backend.ec_relax_res(*rest)
            mg.backend.residual_ready(mg._c_points(0))
            mg.convergence_criterion(iteration=n)
            out.append(np.asarray(mg.compute_residual()))
        got.append(out + finish(mg, n))
        assert pending(mg) == 0
    same(got[1], got[0], (name, state))


def test_second_way_up_of_level_0():
    """a level-0 way up behind the one-pass way up: not the partner of anything, it finds every row put in place"""
    need_gpu()
    got = []
    for up2 in (0, 1):
        mg = build(*GUARD_SHAPE, up2)
        for it in range(2):
            blind_cycle(mg, it)
        assert pending(mg) == 2 * up2
        mg._up(0, mg._level_intervals(0))
        assert pending(mg) == 0
        mg.convergence_criterion(iteration=3)
        got.append([np.asarray(mg.compute_residual())] + finish(mg, 2))
    same(got[1], got[0], "second way up")


def test_waiting_rule_of_the_level_1_record():
    """lag mode 1, a look at u of level 1 behind every cycle: the list lags from the fourth cycle on and keeps lagging (the look does
    not touch level 0), and every look that had to bring level 1 up behind a one-pass way up doubles the number of following ways
    up of level 1 that are not deferred: 2, 4, 8"""
    need_gpu()
    got = []
    for up2 in (0, 1):
        mg = build(*GUARD_SHAPE, up2, lag=1, max_iter=30)
        out, seen = [], []
        for it in range(14):
            out += blind_cycle(mg, it)
            seen.append(pending(mg))
            assert (lagged(mg) >= 0) == (it >= 3), (up2, it)
            if it >= 3:
                out.append(mg.backend.natural("u", 1))
                assert pending(mg) == 0 and lagged(mg) >= 0
        assert seen == ([0, 0, 0, 2, 0, 0, 2, 0, 0, 0, 0, 2, 0, 0] if up2 else [0] * 14), (up2, seen)
        got.append(out + coarse_state(mg) + [mg.backend.natural("u", 0)])
    same(got[1], got[0], "waiting rule of the level-1 record")


# ---- other solver shapes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["F_cycle", "cf_iter2", "four_levels", "mirror"])
def test_other_cycle_forms(name):
    need_gpu()
    kw = {"F_cycle": dict(cycle_type='F'), "cf_iter2": dict(cf_iter=2), "four_levels": dict(levels=4), "mirror": {}}[name]
    shape = (4097, True, 1025 if name == "four_levels" else 257, 4)
    runs = []
    for up2 in (0, 1):
        mg = build(*shape, up2, **kw)
        out, seen = [], []
        if name == "mirror":
            mg.backend.mirror_cpoints(0, [int(i) for i in mg.index_local_c[0]])
        for it in range(4):
            out += blind_cycle(mg, it)
            seen.append(pending(mg))
            if name == "mirror":
                out.append(mg.backend._snap[0].cpu().numpy())
            if it % 2:
                out += coarse_state(mg)
        if name in ("cf_iter2", "mirror"):      # (a plain C-relaxation reads level 0 next: the way up does not lag, nothing is deferred;
            assert seen == [0] * 4, seen        # an engine with a C-point mirror keeps the two passes: a mirrored row carries its padding)
        elif name == "F_cycle":     # (the first visit's way up of level 1 is noted and the second visit brings it up before any one-pass
            assert seen == [0] * 4, seen      # launch; the second visit's own way up is a whole-level pass, which is never deferred)
        else:
            assert seen == ([0, 2, 2, 2] if up2 else [0] * 4), (name, seen)
        out += coarse_state(mg) + [mg.backend.natural("u", 0)]
        assert pending(mg) == 0
        runs.append(out)
    same(runs[1], runs[0], name)


def test_two_solves_and_replay_behind_deferring_cycles():
    """planned cycles: launch by launch twice (the second defers), captured, replayed -- a replay goes past the engine, so the record is
    settled in front of it --; a second solve() runs its first iteration launch by launch again"""
    need_gpu()
    with hc.planned_graph():
        got = []
        for up2 in (0, 1):
            mg = build(*GUARD_SHAPE, up2, max_iter=6)
            out = []
            for _ in range(2):
                res = mg.solve()
                out += [np.array(res["conv"]), mg.backend.natural("u", 0)] + coarse_state(mg)
                assert pending(mg) == 0
            got.append(out)
    same(got[1], got[0], "two solves")


def test_interface():
    need_gpu()
    from pymgrit_amd.core import hip_lib
    mg = build(1022, True, 257, 4, 0)
    lib, h = mg.backend.lib, mg.backend.h
    null = C.c_void_p(None)
    assert lib.mgrit_hip_up2_pending(null) == -2 and lib.mgrit_hip_up2_pending(h) == 0
    assert lib.mgrit_hip_up2_settle(null) != 0 and lib.mgrit_hip_up2_settle(h) == 0
    assert lib.mgrit_hip_set_up2(null, 1) != 0 and lib.mgrit_hip_set_up2(h, 2) != 0 and lib.mgrit_hip_set_up2(h, -1) != 0
    blind_cycle(mg, 0)
    blind_cycle(mg, 1)
    assert pending(mg) == 0          # off (the environment, and the refusals have left it alone)
    hip_lib.set_up2(h, 1)
    blind_cycle(mg, 2)
    assert hip_lib.up2_pending(h) == 2
    hip_lib.set_up2(h, 0)            # a record that is pending stays pending; the next way down drops it
    assert pending(mg) == 2
    blind_cycle(mg, 3)
    assert pending(mg) == 0 and lagged(mg) >= 0
    hip_lib.set_up2(h, 1)
    blind_cycle(mg, 4)
    assert pending(mg) == 2
    hip_lib.up2_settle(h)            # brings level 1 up and nothing else
    assert pending(mg) == 0 and lagged(mg) >= 0
    blind_cycle(mg, 5)
    assert pending(mg) == 2
    hip_lib.lag_settle(h, 0)         # the lag settle brings level 1 up first, then puts the lagged rows in place
    assert pending(mg) == 0 and lagged(mg) == -1
    mg0 = build(1022, True, 257, 4, 0)
    for it in range(6):
        blind_cycle(mg0, it)
    same([mg.backend._U[k].cpu().numpy() for k in (0, 1)], [mg0.backend._U[k].cpu().numpy() for k in (0, 1)], "raw rows behind the settle")


@pytest.mark.parametrize("value,expected", [("0", 0), ("1", 2), (None, 2)])
def test_environment_variable(value, expected):
    need_gpu()
    got = hc.child_cycles({"MGRIT_HIP_LAG": "2", "MGRIT_HIP_UP2": value}, 2, nt=1025, chunk=4)
    assert got["up2_pending"] == expected, got
