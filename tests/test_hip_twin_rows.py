"""GPU: rows of u of a coarse level that are not stored because the same bits go to the row of v in the same slot
(include/mgrit_hip.h, mgrit_hip_twin). Two producers: (B) mgrit_hip_cf_fas leaves out u^1 at the level-1 C-points, whose next reader
-- the F-C-relaxation of level 1 -- starts from v^1 and rewrites them; (A) the chunked FAS pass with its F-relaxation leaves out u of
the coarsest level, whose time-parallel solve in its six-launch form reads the level's current values from v. Every other entry
point finds the rows put in place, and a record that was ever settled that way is not deferred again. Everything is compared bit
for bit with the same sequence run with the switch off (MGRIT_HIP_TWIN=0), and against the oracle. Hierarchy: Heat1D, 3 levels,
m = 4, nt = 1025 (a coarsest level of 64 steps, the smallest that takes the time-parallel solve) at the state sizes of the 512- and
1024-thread instances and of the one-wave instance (whose coarsest level is solved in ONE launch: (A) never defers there), and
nt = 4097 (level-1 chunks of more than one item with a short last chunk)."""
import ctypes as C
import os

import numpy as np
import pytest

import heat1d_cycles as hc
from heat1d_cycles import need_gpu, problem, same, twin_cycle as cycle, twin_finish as finish, twin_pending as pending
from pymgrit_amd.core import hip_lib

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SHAPES = [(nx, forcing, 1025) for nx in (4097, 16382) for forcing in (False, True)] + [(1022, True, 1025), (4097, True, 4097)]
WATCHED = ("mgrit_hip_cf_fas", "mgrit_hip_relax", "mgrit_hip_fas_fused_opts", "mgrit_hip_block_solve")
RELAX_FC, RELAX_CHAIN = hip_lib.RELAX_FC, hip_lib.RELAX_CHAIN


def probe(lib, h, n_levels=3):
    """the library handle with a note behind every producer and partner: (export, level, its last integer argument, mgrit_hip_twin
    of every level > 0 after the call, was the stream capturing)"""
    def note(lib, h, name, args):
        return name, int(args[1]), int(args[3]) if len(args) > 3 else int(args[2]), hc.twins(lib, h, n_levels), hc.capturing()
    return hc.Probe(lib, h, WATCHED, note, n_levels)


def build(nx, forcing, nt, mask, comm=None, levels=3, **kw):
    """a solver whose engine was created with MGRIT_HIP_TWIN = mask, its library handle probed"""
    return hc.build(problem(nx, forcing, nt, levels), env={"MGRIT_HIP_TWIN": str(mask)}, comm=comm,
                    probe=lambda lib, h: probe(lib, h, levels), **dict(dict(max_iter=5, tol=0.0), **kw))


def after(mg, name, lvl, coarse, arg=None):
    """mgrit_hip_twin(coarse) behind every call of the export on level lvl (with the last integer argument arg)"""
    log = mg if isinstance(mg, list) else mg.backend.lib.log
    return [t[coarse - 1] for n, l, a, t, _ in log if n == name and l == lvl and (arg is None or a == arg)]


def five_cycles(shape, mask):
    mg = build(*shape, mask)
    out = [cycle(mg, it) for it in range(5)]
    out.append([mg.backend.natural("u", 0)])
    return mg, out


_OFF = {}     # shape -> what five cycles with the switch off leave (computed once, never modified; the slabs stay on the device)


def off_run(shape):
    if shape not in _OFF:
        mg, out = five_cycles(shape, 0)
        assert never(mg), "pending with the switch off"
        _OFF[shape] = out
    return _OFF[shape]


@pytest.mark.parametrize("mask", [3, 1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"nx{s[0]}_{'forcing' if s[1] else 'plain'}_nt{s[2]}")
def test_five_cycles_bit_identical_and_deferred(shape, mask):
    need_gpu()
    mg, got = five_cycles(shape, mask)
    for it, (a, b) in enumerate(zip(got, off_run(shape))):
        same(a, b, (shape, mask, "cycle", it))
    # that it happened: (B) behind EVERY way down of level 0 (a miss would have stopped it), cleared by the F-C-relaxation of level 1
    down, fc = after(mg, WATCHED[0], 0, 1), after(mg, WATCHED[1], 1, 1, RELAX_FC)
    assert len(down) == 5 and len(fc) == 5 and set(fc) == {-1}, (down, fc)
    assert all(d >= 0 for d in down) if mask & 1 else set(down) == {-1}, down
    # (A) behind every FAS pass onto the coarsest level, cleared by its solve -- never on the one-wave shape (one-launch solve)
    fas, solve = after(mg, WATCHED[2], 1, 2), after(mg, WATCHED[1], 2, 2, RELAX_CHAIN)
    assert len(fas) == 5 and len(solve) >= 5 and set(solve) == {-1}, (fas, solve)
    assert all(d >= 0 for d in fas) if (mask & 2 and shape[0] > 1024) else set(fas) == {-1}, fas
    assert mg.backend.block_solve_form(2) == (2 if shape[0] <= 1024 else 1)


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[3], SHAPES[4]], ids=lambda s: f"nx{s[0]}_{'forcing' if s[1] else 'plain'}_nt{s[2]}")
def test_against_the_oracle(shape, oracle):
    need_gpu()
    mg, got = five_cycles(shape, 3)
    hc.against_oracle(oracle, mg, got[-1][0], hc.heat_specs(*shape), 5)


def never(mg):
    return {x for _, _, _, t, _ in mg.backend.lib.log for x in t} == {-1}


def test_loopback_ranks_never_defer():
    need_gpu()
    from pymgrit_amd.core.comm import run_loopback_ranks

    def rank(comm):
        mg = build(1022, True, 257, 3, comm=comm, max_iter=3)
        assert mg.backend.device_links
        mg.solve()
        mg.backend.sync()
        return mg.backend.lib.log
    world, logs = run_loopback_ranks(2, rank)
    world.close()
    for log in logs:
        assert any(n == WATCHED[0] for n, _, _, _, _ in log) and {x for _, _, _, t, _ in log for x in t} == {-1}, log


def test_captured_planned_cycle_never_defers():
    need_gpu()
    shape = (4097, True, 1025)
    with hc.planned_graph():
        runs = []
        for mask in (0, 3):
            mg = build(*shape, mask)
            runs.append((mg, [cycle(mg, it) for it in range(5)] + [[mg.backend.natural("u", 0)]]))
    (mg_off, off), (mg_on, on) = runs
    for it, (a, b) in enumerate(zip(on, off)):
        same(a, b, ("planned", it))
    same(off[-1], off_run(shape)[-1], "planned against program order")
    assert never(mg_off)
    captured = [x for x in mg_on.backend.lib.log if x[4]]
    assert any(n == WATCHED[0] for n, _, _, _, _ in captured) and any(n == WATCHED[2] for n, _, _, _, _ in captured), captured
    assert {x for _, _, _, t, _ in captured for x in t} == {-1}, captured


def test_item_by_item_fas_pass_and_sequential_solve_never_defer_the_coarsest_level():
    need_gpu()
    shape = (4097, True, 1025)
    ref = off_run(shape)
    mg = build(*shape, 3)
    mg.backend.set_fas_chunk(-1)       # fas_fused1_kernel, as MGRIT_HIP_FFAS=0 in the engine's environment asks for
    got = [cycle(mg, it) for it in range(5)] + [[mg.backend.natural("u", 0)]]
    for it, (a, b) in enumerate(zip(got, ref)):
        same(a, b, ("item by item", it))
    assert set(after(mg, WATCHED[2], 1, 2)) == {-1} and all(d >= 0 for d in after(mg, WATCHED[0], 0, 1))
    with hc.sequential_coarse():
        runs = []
        for mask in (0, 3):
            mg = build(*shape, mask)
            runs.append((mg, [cycle(mg, it) for it in range(3)]))
    for it, (a, b) in enumerate(zip(runs[1][1], runs[0][1])):
        same(a, b, ("sequential", it))
    mg = runs[1][0]
    assert len(after(mg, WATCHED[2], 1, 2)) == 3 and set(after(mg, WATCHED[2], 1, 2)) == {-1}
    assert all(d >= 0 for d in after(mg, WATCHED[0], 0, 1))


# ---- the guard: with a record pending, every other way to the rows sees them in place -------------------------------------------
def g_natural(mg, lvl):
    return finish(mg, [mg.backend.natural("u", lvl)])


def g_level_above(mg, lvl):
    """an entry point of the level above reads the pending level too: the residual of level 0, an F-relaxation of level 1"""
    if lvl == 1:
        return finish(mg, hc.residual_norms(mg))
    hc.relax(1, 'F')(mg)
    return finish(mg)


def g_correction_by_hand(mg, lvl):
    mg.error_correction(lvl=lvl - 1)
    return finish(mg)


def g_second_producer(mg, lvl):
    if lvl == 1:
        mg.backend.cf_fas(0, mg._level_intervals(0))
    else:
        lists = mg._route(1, True)[1]
        mg.backend.fas_fused(1, lists[1], with_f_relax=True, skip_coarse_u=lists[3])
    return finish(mg)


# HipBackend's readers and writers of coarse slabs that go past the engine (torch on the slab): each puts the rows in place first
def g_U(mg, lvl):
    return finish(mg, [mg.backend.U[lvl].clone()])


def g_payload(mg, lvl):
    return finish(mg, [mg.backend.payload(lvl, 4).clone(), mg.backend.payload(lvl, 7).clone()])


def g_set_natural(which):
    def run(mg, lvl):
        values = mg.backend.natural("v", lvl) * 0.5 + 0.25     # (natural("v") settles nothing: the record is still pending here)
        mg.backend.set_natural(which, lvl, values)
        return finish(mg, hc.raw_slabs(mg))
    return run


def g_vector_read(mg, lvl):
    return finish(mg, [np.asarray(mg.u[lvl][4].pack()).copy(), np.asarray(mg.u[lvl][7].pack()).copy()])


def g_vector_write(which):
    def run(mg, lvl):
        vec = mg.v[lvl][5]          # (a read of v settles nothing)
        (mg.u if which == "u" else mg.v)[lvl][4] = vec
        return finish(mg, hc.raw_slabs(mg))
    return run


GUARDS = {"natural": g_natural, "relax_F": hc.twin_relax('F'), "relax_C": hc.twin_relax('C'), "relax_FC": hc.twin_relax('FC'),
          "relax_CHAIN": hc.twin_relax('CHAIN'),
          "residual": g_level_above, "correction_by_hand": g_correction_by_hand, "block_solve_by_phases": hc.twin_block_solve_by_phases,
          "second_producer": g_second_producer, "U": g_U, "payload": g_payload, "set_natural_u": g_set_natural("u"),
          "set_natural_v": g_set_natural("v"), "vector_read": g_vector_read, "vector_write_u": g_vector_write("u"),
          "vector_write_v": g_vector_write("v")}


# (the step-by-step chain by hand belongs to the coarsest level)
@pytest.mark.parametrize("name,lvl", [(name, lvl) for name in sorted(GUARDS) for lvl in (1, 2) if (name, lvl) != ("relax_CHAIN", 1)])
def test_guard(name, lvl):
    need_gpu()
    got = []
    for mask in (0, 3):
        mg = build(4097, True, 1025, mask)
        pending(mg, lvl)
        assert (mg.backend.lib.twins()[lvl - 1] >= 0) == (mask == 3), (name, lvl, mask)
        n_log = len(mg.backend.lib.log)
        got.append(GUARDS[name](mg, lvl))
        if mask == 3:
            # after the miss the list no longer defers: the way down of the cycle that finish() has run
            late = [t[lvl - 1] for n, l, _, t, _ in mg.backend.lib.log[n_log:] if (n, l) == ((WATCHED[0], 0) if lvl == 1 else (WATCHED[2], 1))]
            assert late and set(late[-1:]) == {-1}, (name, lvl, late)
    same(got[1], got[0], (name, lvl))


@pytest.mark.parametrize("name", ["F_cycle", "cf_iter2", "four_levels"])
def test_other_cycle_shapes(name):
    need_gpu()
    kw = {"F_cycle": dict(cycle_type='F'), "cf_iter2": dict(cf_iter=2), "four_levels": dict(levels=4)}[name]
    nt = 4097 if name == "four_levels" else 1025
    runs = []
    for mask in (0, 3):
        mg = build(4097, True, nt, mask, **kw)
        runs.append((mg, [cycle(mg, it) for it in range(4)] + [[mg.backend.natural("u", 0)]]))
    for it, (a, b) in enumerate(zip(runs[1][1], runs[0][1])):
        same(a, b, (name, it))
    assert never(runs[0][0])
    mg = runs[1][0]
    top = mg.lvl_max - 1
    assert any(d >= 0 for d in after(mg, WATCHED[0], 0, 1))
    # (cf_iter = 2: level 1 goes down sweep by sweep -- its F-relaxation is the miss of (B), and no chunked FAS pass runs for (A))
    assert any(d >= 0 for d in after(mg, WATCHED[2], top - 1, top)) == (name != "cf_iter2")
    if name == "four_levels":       # (B) on the pair 0 -> 1, (A) on the pair 2 -> 3, nothing ever on level 2
        assert all(d >= 0 for d in after(mg, WATCHED[0], 0, 1)) and all(d >= 0 for d in after(mg, WATCHED[2], 2, 3))
        assert {t[1] for _, _, _, t, _ in mg.backend.lib.log} == {-1}


def test_switch_and_argument_checks():
    need_gpu()
    mg = build(4097, True, 1025, 3)
    lib, h = mg.backend.lib, mg.backend.h
    null = C.c_void_p(None)
    for fn in (lib.mgrit_hip_twin,):
        assert fn(null, 0) == -2 and fn(h, -1) == -2 and fn(h, 99) == -2 and fn(h, 0) == -1 and fn(h, 1) == -1
    assert lib.mgrit_hip_set_twin(null, 1) != 0 and lib.mgrit_hip_set_twin(h, 4) != 0 and lib.mgrit_hip_set_twin(h, -1) != 0
    assert lib.mgrit_hip_settle(null, 0) != 0 and lib.mgrit_hip_settle(h, 99) != 0 and lib.mgrit_hip_settle(h, 1) == 0
    # the setter: off before the way down of the third cycle ...
    assert lib.mgrit_hip_set_twin(h, 0) == 0
    pending(mg, 2)
    assert lib.twins() == (-1, -1)
    mg.iteration(lvl=2, cycle_type='V', iteration=2, first_f=True)
    # ... (A) alone, then both, for the next ways down; a record that is pending stays pending when the switch goes off, its
    # partner clears it
    assert lib.mgrit_hip_set_twin(h, 2) == 0
    mg._down_level(0, mg._level_intervals(0))
    assert lib.twins() == (-1, -1)
    lists = mg._route(1, True)[1]
    mg._down_coarse(1, lists)
    assert lib.twins()[0] == -1 and lib.twins()[1] >= 0
    assert lib.mgrit_hip_set_twin(h, 0) == 0 and lib.twins()[1] >= 0
    mg.iteration(lvl=2, cycle_type='V', iteration=2, first_f=True)
    assert lib.twins() == (-1, -1)
    assert lib.mgrit_hip_set_twin(h, 3) == 0
    mg._down_level(0, mg._level_intervals(0))
    assert lib.twins()[0] >= 0
    # mgrit_hip_settle puts the rows in place, and counts as a miss
    assert lib.mgrit_hip_settle(h, 1) == 0 and lib.twins() == (-1, -1)
    mg._down_level(0, mg._level_intervals(0))
    assert lib.twins() == (-1, -1)
    # the environment variable: anything but one digit 0..3, or none, leaves the default, which is (A) alone
    for text, want in (("1", (True, False)), ("3", (True, True)), ("0", (False, False)), ("7", (False, True)), ("x", (False, True)),
                       (None, (False, True))):
        m2 = hc.build(problem(4097, True, 1025), env={"MGRIT_HIP_TWIN": text}, probe=probe, max_iter=1, tol=0.0)
        cycle(m2, 0)
        assert (all(d >= 0 for d in after(m2, WATCHED[0], 0, 1)), all(d >= 0 for d in after(m2, WATCHED[2], 1, 2))) == want, text


def test_ffas_switched_off_in_the_environment_never_defers_the_coarsest_level():
    """MGRIT_HIP_FFAS is read once per process, so the engine that sees MGRIT_HIP_FFAS=0 lives in a child: two cycles there, the
    probe's notes come back on its standard output"""
    need_gpu()
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MGRIT_HIP_FFAS="0", PYTHONPATH=os.pathsep.join([root] + os.environ.get("PYTHONPATH", "").split(os.pathsep)).rstrip(os.pathsep))
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    log = json.loads(r.stdout.strip().splitlines()[-1])
    fas, down = after(log, WATCHED[2], 1, 2), after(log, WATCHED[0], 0, 1)
    assert len(fas) == 2 and set(fas) == {-1}, fas
    assert len(down) == 2 and all(d >= 0 for d in down), down


if __name__ == "__main__":      # the child of the test above
    import json
    child = build(4097, True, 1025, 3)
    for k in range(2):
        cycle(child, k)
    print(json.dumps(child.backend.lib.log))
