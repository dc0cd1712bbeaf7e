"""The harness the GPU tests of the Heat1D V-cycle's unstored rows share (test_hip_deferred_rows.py, test_hip_twin_rows.py,
test_hip_lagged_cpoints.py, test_hip_up2.py, test_hip_cfas_form.py, and the scripts of pending_trace.py): the hierarchy, a solver whose
engine is created under given environment variables with its library handle probed, one cycle and the looks behind it, the
comparisons, and the guard actions that are the same call sequence for more than one record. A plain helper like cases.py: no tests,
no fixtures. A new record's tests start here: a `watched` tuple and a `note` for the Probe, a `cycle` composed of the looks, a
`finish`, and a GUARDS table over the actions below.

A look settles records (natural() and payload() put rows in place, a raw slab does not), so WHICH look runs WHERE is behaviour:
every module composes its own `cycle` from the named parts and none of them looks at more than it says."""
import contextlib
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import cases

SIZES = (1022, 4097, 16382)       # one wave per state / 512 threads / 1024 threads


# ---- shapes and problems -------------------------------------------------------------------------------------------------------
def level_nts(nt, levels=3):
    return [(nt - 1) // 4 ** k + 1 for k in range(levels)]


def problem(nx, forcing, nt, levels=3):
    from pymgrit_amd import Heat1D
    kw = dict(rhs_separable=[(cases.rhs_space, cases.rhs_time)]) if forcing else {}
    return [Heat1D(x_start=0, x_end=1, nx=nx, a=1, init_cond=cases.init_cond, t_start=0, t_stop=2, nt=k, **kw) for k in level_nts(nt, levels)]


def heat_specs(nx, forcing, nt, levels=3):
    """the oracle's description of problem(nx, forcing, nt, levels)"""
    return [cases.heat_level_spec(nx, cases.lin(2, k), forcing=forcing) for k in level_nts(nt, levels)]


# ---- a solver with its library handle probed -----------------------------------------------------------------------------------
_ENV_LOCK = threading.Lock()
_ENV_HELD = {}      # variable -> [its value before the first holder, holders]


@contextlib.contextmanager
def engine_env(env):
    """the variables of env set (a value of None: unset) while an engine is created, the previous state back on every way out.
    Loopback ranks create their engines on threads of one process, at the same time and with the same variables: the state that
    comes back is the one the FIRST holder found, when the last one leaves (each rank saving and restoring for itself leaves the
    variable set for the rest of the process whenever the second rank saves what the first has set)"""
    env = dict(env)
    with _ENV_LOCK:
        for k, v in env.items():
            _ENV_HELD.setdefault(k, [os.environ.get(k), 0])[1] += 1
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    try:
        yield
    finally:
        with _ENV_LOCK:
            for k in env:
                _ENV_HELD[k][1] -= 1
                if _ENV_HELD[k][1] == 0:
                    before = _ENV_HELD.pop(k)[0]
                    os.environ.pop(k, None)
                    if before is not None:
                        os.environ[k] = before


def capturing():
    import torch
    return bool(torch.cuda.is_current_stream_capturing())


def twins(lib, h, n_levels):
    return tuple(lib.mgrit_hip_twin(h, lvl) for lvl in range(1, n_levels))


class Probe:
    """the backend's library handle with a note behind every call of a watched export: note(lib, h, export, args), taken after the
    call, goes to `log` unless it is None. Every other attribute is the library's own."""

    def __init__(self, lib, h, watched, note, n_levels=None):
        self.__dict__.update(_lib=lib, _h=h, _watched=watched, _note=note, _n=n_levels, log=[])

    def twins(self):
        return twins(self._lib, self._h, self._n)

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in self._watched:
            return fn

        def call(*args):
            rc = fn(*args)
            rec = self._note(self._lib, self._h, name, args)
            if rec is not None:
                self.log.append(rec)
            return rc
        return call


def build(levels, *, env=(), chunk=None, comm=None, probe=None, **mgrit_kw):
    """a solver of the hierarchy `levels` whose engine was created with the variables of env (engine_env), whose level-0 passes walk
    chunks of `chunk` intervals if one is given (the library's rule gives levels this small chunks of one), its library handle
    wrapped by probe(lib, h)"""
    from pymgrit_amd import Mgrit
    with engine_env(env):
        mg = Mgrit(levels, logging_lvl=30, comm_time=comm, **mgrit_kw)
    be = mg.backend
    assert type(be).__name__ == "HipBackend"
    if chunk is not None:
        ids, length = be._intervals_id, chunk

        def intervals_id(lvl, intervals, chunk=None):
            return ids(lvl, intervals, chunk=length if lvl == 0 and chunk is None else chunk)
        be._intervals_id = intervals_id
    if probe is not None:
        be.lib = probe(be.lib, be.h)
    return mg


DOWN, UP = "mgrit_hip_cf_fas", "mgrit_hip_ec_relax_res"      # the whole-level passes


def lag_note(lib, h, name, args):
    """behind every whole-level pass of level 0: (export, its last integer argument, mgrit_hip_lagged(level 0) and
    mgrit_hip_deferred(level 0) after the call, was the stream capturing)"""
    if args[1] == 0:
        return name, int(args[3]), lib.mgrit_hip_lagged(h, 0), lib.mgrit_hip_deferred(h, 0), capturing()


def lag_build(nx, forcing, nt, chunk, lag, env=(), comm=None, levels=3, probe=None, **kw):
    """a solver whose engine was created with MGRIT_HIP_LAG = lag (and whatever else env names), whose level-0 passes walk chunks of
    `chunk` intervals, its library handle probed (lag_note unless the caller brings a probe): the lag, up and trace tests' solver"""
    return build(problem(nx, forcing, nt, levels), env=dict(env, MGRIT_HIP_LAG=str(lag)), chunk=chunk, comm=comm,
                 probe=probe or (lambda lib, h: Probe(lib, h, (DOWN, UP), lag_note)), **dict(dict(max_iter=6, tol=0.0), **kw))


@contextlib.contextmanager
def option(name, value):
    from pymgrit_amd.core.options import options
    setattr(options, name, value)
    try:
        yield
    finally:
        options.reset(name)      # back to environment / default (an assignment would pin the value for later tests)


def planned_graph():
    return option("plan_graph", "require")


def sequential_coarse():
    return option("coarse_solve", "sequential")


def need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU visible")


# ---- one cycle, and the looks behind it ----------------------------------------------------------------------------------------
def run_cycle(mg, it):
    """one cycle with its residual check"""
    mg.iteration(lvl=0, cycle_type=mg.cycle_type, iteration=it, first_f=True)
    mg.convergence_criterion(iteration=it + 1)


def residual(mg):
    """the residual sums (the way up's own, fetched): settles nothing"""
    return [np.asarray(mg.compute_residual())]


def raw_level0(mg):
    """the level-0 slab as it lies: nothing is put in place for the look"""
    return [mg.backend._U[0].cpu().numpy()]


def raw_slabs(mg):
    """copies of the raw slabs of u, v, g of every level, on the device: nothing is put in place for the look"""
    be = mg.backend
    return [s[lvl].clone() for lvl in range(mg.lvl_max) for s in (be._U, be.V, be.G) if s[lvl] is not None]


def coarse_state(mg):
    """u, v, g of the coarse levels, their rows put in place"""
    return [mg.backend.natural(which, lvl) for lvl in range(1, mg.lvl_max) for which in "uvg"]


def blind_cycle(mg, it):
    """one cycle and no look at any slab: what it leaves pending stays pending"""
    run_cycle(mg, it)
    return residual(mg)


def coarse_cycle(mg, it):
    """one cycle WITHOUT a look at level 0, which would have the rows put in place"""
    return blind_cycle(mg, it) + coarse_state(mg)


def raw_cycle(mg, it):
    """one cycle WITHOUT anything of level 0 put in place for the look"""
    run_cycle(mg, it)
    return raw_level0(mg) + residual(mg) + coarse_state(mg)


def lagged(mg):
    return mg.backend.lib.mgrit_hip_lagged(mg.backend.h, 0)


def up2_pending(mg):
    return mg.backend.lib.mgrit_hip_up2_pending(mg.backend.h)


# ---- comparisons ---------------------------------------------------------------------------------------------------------------
def same(a, b, what):
    """bit for bit: equal lengths at every nesting level, torch.equal for tensors, np.array_equal for arrays"""
    import torch
    if isinstance(a, (list, tuple)):
        assert isinstance(b, (list, tuple)) and len(a) == len(b), what
        for k, (x, y) in enumerate(zip(a, b)):
            same(x, y, (what, k))
    elif torch.is_tensor(a):
        assert torch.is_tensor(b) and torch.equal(a, b), what
    else:
        assert not isinstance(b, (list, tuple)) and np.array_equal(a, b), what


def against_oracle(oracle, mg, level0_u, specs, n, **kw):
    """the same n cycles by the oracle: the residual history to rounding of the norm, level 0 bit for bit"""
    op = oracle.OracleProblem(specs, variant=1, max_iter=n, tol=0.0, **kw)
    ref = op.solve()
    conv = mg.conv[1:n + 1]
    assert np.max(np.abs(conv - ref) / ref) <= 1e-10, (conv, ref)
    assert np.array_equal(level0_u, op.state("u", 0))


# ---- guard actions: action(mg) -> list of looks. A module wraps each with its own finish ------------------------------------------
def relax_level0(mode):
    def action(mg):
        runs = mg._c_runs(0) if mode == 'C' else mg._f_runs(0)
        if mode == 'FC':       # not a sweep of level 0: refused, behind the guard
            from pymgrit_amd.core.hip_lib import MgritHipError
            with pytest.raises(MgritHipError):
                mg.backend.relax(0, runs, mode)
        else:
            mg.backend.relax(0, runs, mode)
        return []
    return action


def relax(lvl, mode):
    """a sweep of a coarse level over the cycle's own list"""
    return lambda mg: mg.backend.relax(lvl, mg._c_runs(lvl) if mode == 'C' else mg._f_runs(lvl), mode) or []


def natural(which, lvl):
    return lambda mg: [mg.backend.natural(which, lvl)]


def payload(lvl, points):
    return lambda mg: [mg.backend.payload(lvl, int(i)).cpu().numpy() for i in points]


def set_natural_level0(mg):
    x, _ = cases.heat_grid(mg.problem[0].nx + 2)
    mg.backend.set_natural("u", 0, np.stack([cases.heat_input(x, k) for k in range(len(mg.problem[0].t))]))
    return []


def scale_natural(which, lvl):
    return lambda mg: mg.backend.set_natural(which, lvl, 0.5 * mg.backend.natural(which, lvl)) or []


def correction_by_hand(lvl):
    def action(mg):
        mg.error_correction(lvl=lvl)
        mg.f_relax(lvl=lvl)
        return []
    return action


def residual_norms(mg):
    """the sums the way up has left, where it has left some"""
    return [np.asarray(mg.backend.residual_norms(mg._c_points(0)))]


def residual_norms_fresh(mg):
    mg.backend._invalidate()      # (not the sums the way up has left: the residual kernel's own)
    return residual_norms(mg)


def U(levels):
    return lambda mg: [mg.backend.U[k].cpu().numpy() for k in levels]


def raw_U(levels):
    return lambda mg: [mg.backend._U[k].cpu().numpy() for k in levels]


def vector_read(which, lvl, points):
    return lambda mg: [np.asarray(getattr(mg, which)[lvl][i].get_values()) for i in points]


def vector_copy(which, lvl, dst, src):
    def action(mg):
        slab = getattr(mg, which)[lvl]
        slab[dst] = slab[src]
        return []
    return action


def settle(lvl):
    def action(mg):
        from pymgrit_amd.core import hip_lib
        hip_lib.settle(mg.backend.h, lvl)
        return []
    return action


# ---- the twin record (test_hip_twin_rows.py, pending_trace.py) -------------------------------------------------------------------
def twin_cycle(mg, it):
    """one cycle; what it leaves: the residual sums and every raw slab"""
    run_cycle(mg, it)
    assert set(mg.backend.lib.twins()) == {-1}, "a record is pending behind a whole cycle"
    return residual(mg) + raw_slabs(mg)


def twin_pending(mg, lvl):
    """two cycles, then the way down of a third as far as the pass that fills level lvl: the level waits for its partner"""
    for it in range(2):
        twin_cycle(mg, it)
    mg.backend.begin_cycle()
    mg._down_level(0, mg._level_intervals(0))
    if lvl == 2:
        route, lists = mg._route(1, True)
        assert route == 'coarse'
        mg._down_coarse(1, lists)


def twin_finish(mg, extra=()):
    """a whole cycle behind whatever the guard test did, then everything there is to see"""
    return list(extra) + twin_cycle(mg, 2) + [mg.backend.natural("u", 0)]


COARSEST_RUNS = {'F': [(1, 3), (5, 3)], 'C': [(4, 1), (8, 1)], 'FC': [(1, 4), (5, 4)], 'CHAIN': [(1, 10)]}


def twin_relax(mode):
    def run(mg, lvl):
        if lvl == 2:   # the coarsest level has no cycle lists of its own: two intervals' worth by hand, in the mode
            mg.backend.relax(lvl, COARSEST_RUNS[mode], mode)     # asked for; CHAIN: a part of the forward solve, step by step
        elif mode == 'FC':   # another run list: every second interval of the level
            fc_runs = mg._route(1, True)[1][0]
            mg.backend.relax(1, [(int(s), int(n)) for s, n in list(fc_runs)[::2]], 'FC')
        else:
            relax(1, mode)(mg)
        return twin_finish(mg)
    return run


def twin_block_solve_by_phases(mg, lvl):
    if lvl == 1:
        before = mg.backend.lib.twins()
        mg.backend.block_solve(2, 7)      # (reaches level 2 only: the record of level 1 stays, its partner is still to come)
        assert mg.backend.lib.twins() == before
        relax(1, 'F')(mg)
    else:
        mg.backend.block_solve(2, 1)
        mg.backend.block_solve(2, 6)
    return twin_finish(mg)


# ---- the up record (test_hip_up2.py, pending_trace.py) -----------------------------------------------------------------------------
def half_cycle(mg, it):
    """a V-cycle up to and including the way up of level 1 (Mgrit.iteration(lvl=0) with the level-0 way up left out), then what is
    left of it"""
    real = mg.backend.ec_relax_res
    skipped = []
    mg.backend.ec_relax_res = lambda lvl, intervals, base=0: skipped.append((lvl, intervals, base)) if lvl == 0 else real(lvl, intervals, base)
    try:
        mg.iteration(lvl=0, cycle_type=mg.cycle_type, iteration=it, first_f=True)
    finally:
        mg.backend.ec_relax_res = real
    assert len(skipped) == 1
    return skipped[0]


def up2_finish(mg, n):
    """two blind cycles behind whatever the guard test did, then everything there is to see"""
    out = []
    for it in range(n, n + 2):
        out += blind_cycle(mg, it)
    return out + coarse_state(mg) + [mg.backend.natural("u", 0)]


UP2_GUARDS = {
    "natural_u0": natural("u", 0), "natural_u1": natural("u", 1), "natural_g1": natural("g", 1), "natural_u2": natural("u", 2),
    "U": U((0, 1)), "raw_U": raw_U((0, 1, 2)),
    "payload_0": payload(0, (4, 8, 256)), "payload_1": payload(1, (3, 4, 5, 64)),
    "vector_read_1": vector_read("u", 1, (3, 4, 5, 64)), "vector_read_g1": vector_read("g", 1, (3, 4, 5)),
    "set_natural_0": set_natural_level0,
    "relax_F_0": relax_level0('F'), "relax_C_0": relax_level0('C'), "relax_F_1": relax(1, 'F'), "relax_C_1": relax(1, 'C'),
    "relax_FC_1": lambda mg: mg.backend.relax(1, [(int(s), int(n) + 1) for s, n in mg._f_runs(1)], 'FC'),
    "relax_F_2": lambda mg: mg.backend.relax(2, [(1, 3)], 'F'),
    "settle_0": settle(0), "settle_1": settle(1), "settle_2": settle(2),
    "correction_by_hand_0": correction_by_hand(0), "correction_by_hand_1": correction_by_hand(1),
    "second_way_up_1": lambda mg: mg._ec_f_relax(1),
    "write_g1": vector_copy("g", 1, 5, 6), "write_u2": vector_copy("u", 2, 3, 2),
    "set_natural_g1": scale_natural("g", 1), "set_natural_u2": scale_natural("u", 2),
}


# ---- the child process of the environment-variable tests ---------------------------------------------------------------------------
_CHILD = """
import json
import sys
sys.path.insert(0, {tests!r})
import heat1d_cycles as hc
mg = hc.build(hc.problem(1022, True, {nt}), chunk={chunk!r}, max_iter={n}, tol=0.0)
for it in range({n}):
    hc.{cycle}(mg, it)
print("RECORDS", json.dumps(dict(lagged=hc.lagged(mg), up2_pending=hc.up2_pending(mg))))
"""


def child_cycles(env, n, nt=257, chunk=None, cycle="blind_cycle"):
    """n cycles (hc.<cycle>) of problem(1022, True, nt) in a fresh process whose engine finds the variables of env (None: unset)
    when it is made -- some are read once per process; what is pending behind them: {"lagged": ..., "up2_pending": ...}"""
    tests = os.path.dirname(os.path.abspath(__file__))
    env = {k: v for k, v in dict(os.environ, **env).items() if v is not None}
    env["PYTHONPATH"] = os.pathsep.join([os.path.dirname(tests), tests] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    code = _CHILD.format(tests=tests, nt=nt, chunk=chunk, n=n, cycle=cycle)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout.split("RECORDS")[1])
