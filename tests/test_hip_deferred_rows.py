"""GPU: rows the level-0 way down does not store because their bits sit in the row in front of them (include/mgrit_hip.h,
mgrit_hip_deferred). mgrit_hip_cf_fas(pre_relaxed = 1) leaves the closing C-point of every interval unwritten, the way up
(mgrit_hip_ec_relax_res, store_all_f = 2) reads it from the last F-point's row, and every other entry point of the level puts the
rows in place first. Everything is compared bit for bit with the same sequence run with the switch off (MGRIT_HIP_DEFER=0), and
against the oracle. Hierarchy: Heat1D, 3 levels, m = 4, nt = 257 (64 level-0 intervals: chunk starts and a chunk cut, 16 coarsest
steps) at one state size per kernel instance, and nt = 1025 (a coarsest level of four blocks)."""
import contextlib
import ctypes as C

import pytest

import heat1d_cycles as hc
from heat1d_cycles import need_gpu, same, raw_cycle as cycle

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SHAPES = [(nx, forcing, 257) for nx in hc.SIZES for forcing in (False, True)] + [(1022, True, 1025)]
WATCHED = ("mgrit_hip_cf_fas", "mgrit_hip_ec_relax_res")


def note(lib, h, name, args):
    """behind every whole-level pass of level 0: (export, its last integer argument, mgrit_hip_deferred(level 0) after the call, was
    the stream capturing)"""
    if args[1] == 0:
        return name, int(args[3]), lib.mgrit_hip_deferred(h, 0), hc.capturing()


def build(nx, forcing, nt, defer, comm=None, **kw):
    """a solver whose engine was created with the switch on (the variable absent) or off, its library handle probed"""
    return hc.build(hc.problem(nx, forcing, nt), env={"MGRIT_HIP_DEFER": None if defer else "0"}, comm=comm,
                    probe=lambda lib, h: hc.Probe(lib, h, WATCHED, note), **dict(dict(max_iter=5, tol=0.0), **kw))


def deferred_after(mg, name):
    return [d for n, _, d, _ in mg.backend.lib.log if n == name]


_OFF = {}     # shape -> what five cycles with the switch off leave (computed once, never modified)


def five_cycles(shape, defer):
    mg = build(*shape, defer)
    out = [cycle(mg, it) for it in range(5)]
    out.append([mg.backend.natural("u", 0)])
    return mg, out


def off_run(shape):
    if shape not in _OFF:
        mg, out = five_cycles(shape, False)
        assert set(deferred_after(mg, WATCHED[0]) + deferred_after(mg, WATCHED[1])) == {-1}, "pending with the switch off"
        assert [pre for n, pre, _, _ in mg.backend.lib.log if n == WATCHED[0]] == [0, 1, 1, 1, 1]
        _OFF[shape] = out
    return _OFF[shape]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"nx{s[0]}_{'forcing' if s[1] else 'plain'}_nt{s[2]}")
def test_five_cycles_bit_identical_and_deferred(shape, oracle):
    need_gpu()
    mg, got = five_cycles(shape, True)
    for it, (a, b) in enumerate(zip(got, off_run(shape))):
        same(a, b, (shape, "cycle", it))
    # that it happened: the first cycle's C-points are not pre-relaxed (pre = 0), every later way down leaves its list pending,
    # every way up clears it
    down, up = deferred_after(mg, WATCHED[0]), deferred_after(mg, WATCHED[1])
    assert len(down) == 5 and down[0] == -1 and all(d >= 0 for d in down[1:]) and len(set(down[1:])) == 1, down
    assert up == [-1] * 5, up
    assert [mode for n, mode, _, _ in mg.backend.lib.log if n == WATCHED[1]] == [2] * 5
    # ... and against the oracle: the same cycles, the residual history to rounding of the norm, level 0 bit for bit
    hc.against_oracle(oracle, mg, got[-1][0], hc.heat_specs(*shape), 5)


def test_store_all_f_never_defers(monkeypatch):
    need_gpu()
    monkeypatch.setenv("PYMGRIT_AMD_STORE_ALL_F", "1")
    mg = build(1022, True, 257, True)
    for it in range(3):
        cycle(mg, it)
    log = mg.backend.lib.log
    assert [x[1] for x in log if x[0] == WATCHED[0]] == [0, 0, 0] and {x[2] for x in log} == {-1}, log


def test_loopback_ranks_never_defer():
    need_gpu()
    from pymgrit_amd.core.comm import run_loopback_ranks

    def rank(comm):
        mg = build(1022, True, 257, True, comm=comm, max_iter=3)
        assert mg.backend.device_links
        mg.solve()
        mg.backend.sync()
        return mg.backend.lib.log
    world, logs = run_loopback_ranks(2, rank)
    world.close()
    for log in logs:
        assert any(n == WATCHED[0] for n, _, _, _ in log) and {d for _, _, d, _ in log} == {-1}, log


@pytest.mark.parametrize("blocks", [1, 3])
def test_planned_cycles(blocks):
    """a planned cycle runs launch by launch twice (a block's way down defers, the next block's settles it), then as a captured
    graph, into which nothing is deferred and nothing settled"""
    need_gpu()
    shape = (4097, True, 257)
    with hc.planned_graph():
        runs = []
        for defer in (False, True):
            # (one block: planned and captured on request alone, options.plan_graph; a plan_blocks=1 request means program order)
            mg = build(*shape, defer, **({} if blocks == 1 else dict(plan_blocks=blocks)))
            runs.append((mg, [cycle(mg, it) for it in range(5)] + [[mg.backend.natural("u", 0)]]))
    (mg_off, off), (mg_on, on) = runs
    for it, (a, b) in enumerate(zip(on, off)):
        same(a, b, (blocks, "cycle", it))
    same(off[-1], off_run(shape)[-1], (blocks, "planned against program order"))
    assert {d for _, _, d, _ in mg_off.backend.lib.log} == {-1}
    log = mg_on.backend.lib.log
    captured = [x for x in log if x[3]]
    assert any(n == WATCHED[0] and pre == 1 for n, pre, _, _ in captured), log
    assert {d for _, _, d, _ in captured} == {-1}, captured
    assert any(n == WATCHED[0] and d >= 0 for n, _, d, c in log if not c), log
    assert mg_on.backend.lib.mgrit_hip_deferred(mg_on.backend.h, 0) == -1


# ---- the guard: with a list pending, every other way into level 0 sees the rows in place --------------------------------------
def pending(mg):
    """two cycles, then the way down of a third: level 0 waits for its way up"""
    for it in range(2):
        cycle(mg, it)
    mg.backend.begin_cycle()
    mg._down_level(0, mg._level_intervals(0))


def finish(mg, extra=()):
    """a whole cycle behind whatever the guard test did, then everything there is to see"""
    out = list(extra) + cycle(mg, 2)
    return out + [mg.backend.natural("u", 0)]


def guard(action):
    return lambda mg: finish(mg, action(mg))


def g_ecf_route(mg):
    """the way up of a solver whose stopping criterion is not the residual: correction + F-relaxation without the residual sums"""
    mg.conv_crit = 1
    try:
        mg._up(0, mg._level_intervals(0))
    finally:
        mg.conv_crit = 0
    return finish(mg)


GUARDS = {"relax_F": guard(hc.relax_level0('F')), "relax_C": guard(hc.relax_level0('C')), "relax_FC": guard(hc.relax_level0('FC')),
          "residual": guard(hc.residual_norms), "correction_by_hand": guard(hc.correction_by_hand(0)), "natural": guard(hc.natural("u", 0)),
          "payload": guard(hc.payload(0, (4, 8, 255, 256))), "set_natural": guard(hc.set_natural_level0), "ecf_route": g_ecf_route}


@pytest.mark.parametrize("name", sorted(GUARDS))
def test_guard(name):
    need_gpu()
    got = []
    for defer in (False, True):
        mg = build(4097, True, 257, defer)
        pending(mg)
        held = mg.backend.lib.mgrit_hip_deferred(mg.backend.h, 0)
        assert (held >= 0) == defer, (name, defer, held)
        got.append(GUARDS[name](mg))
        assert mg.backend.lib.mgrit_hip_deferred(mg.backend.h, 0) == -1
    same(got[1], got[0], name)


@pytest.mark.parametrize("name", ["sequential", "F_cycle", "cf_iter2"])
def test_other_cycle_shapes(name):
    need_gpu()
    kw = {"sequential": {}, "F_cycle": dict(cycle_type='F'), "cf_iter2": dict(cf_iter=2)}[name]
    with hc.sequential_coarse() if name == "sequential" else contextlib.nullcontext():
        runs = []
        for defer in (False, True):
            mg = build(4097, True, 257, defer, **kw)
            runs.append([cycle(mg, it) for it in range(4)] + [[mg.backend.natural("u", 0)]])
            assert mg.backend.lib.mgrit_hip_deferred(mg.backend.h, 0) == -1
            down = deferred_after(mg, WATCHED[0])
            if name == "cf_iter2":      # a plain C-relaxation stands in front of the pass: never pre-relaxed
                assert set(down) == {-1}
            else:
                assert any(d >= 0 for d in down) == defer, (name, defer, down)
    for it, (a, b) in enumerate(zip(runs[1], runs[0])):
        same(a, b, (name, it))


def test_switch_and_argument_checks():
    need_gpu()
    mg = build(1022, True, 257, True)
    lib, h = mg.backend.lib, mg.backend.h
    null = C.c_void_p(None)
    assert lib.mgrit_hip_deferred(null, 0) == -2 and lib.mgrit_hip_deferred(h, -1) == -2 and lib.mgrit_hip_deferred(h, 99) == -2
    assert lib.mgrit_hip_deferred(h, 0) == -1 and lib.mgrit_hip_deferred(h, 1) == -1
    assert lib.mgrit_hip_set_defer(null, 1) != 0 and lib.mgrit_hip_set_defer(h, 2) != 0 and lib.mgrit_hip_set_defer(h, -1) != 0
    # the setter: off before the way down of the third cycle, on again for the fourth
    assert lib.mgrit_hip_set_defer(h, 0) == 0
    pending(mg)
    assert lib.mgrit_hip_deferred(h, 0) == -1
    mg._up(0, mg._level_intervals(0))
    assert lib.mgrit_hip_set_defer(h, 1) == 0
    mg.backend.begin_cycle()
    mg._down_level(0, mg._level_intervals(0))
    assert lib.mgrit_hip_deferred(h, 0) >= 0
    # a list that is pending stays pending when the switch goes off; its partner clears it
    assert lib.mgrit_hip_set_defer(h, 0) == 0 and lib.mgrit_hip_deferred(h, 0) >= 0
    mg._up(0, mg._level_intervals(0))
    assert lib.mgrit_hip_deferred(h, 0) == -1
