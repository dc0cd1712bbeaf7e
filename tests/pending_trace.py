"""The scripted call sequences of the record of the unstored-row bookkeeping (pymgrit_amd/csrc/pending_rows.h),
shared by tests/golden/make_golden_pending_trace.py, which records tests/golden/pending_trace.json, and
tests/test_hip_pending_trace.py, which replays every script and compares with equality. Needs a GPU.

A script is a sequence of backend calls the record tests already walk (test_hip_deferred_rows.py, test_hip_twin_rows.py,
test_hip_lagged_cpoints.py, test_hip_up2.py); scripts and tests take the solver, the cycles, the guard tables and the finishes from
heat1d_cycles.py, and no test module is imported here. Behind EVERY library call of the backend, and behind every step of the script, the
state of the four records is noted: mgrit_hip_deferred(l) and mgrit_hip_twin(l) of every level, mgrit_hip_lagged(0) and
mgrit_hip_up2_pending. At the end mgrit_hip_settle runs on every level and the raw u, v and g slabs of every level are digested
(SHA-256). What is kept per script: the number of calls, the digest of the whole trace, the calls at which the state changed
(readable when the test fails), and the slab digests folded into one (pack, at the end of this file, lays the file out). These are host decisions, so the shapes are small: Heat1D, 3 levels, m = 4,
nt = 1025, level-0 chunks of 4, forcing on, at the smallest and the largest state size of heat1d_cycles.SIZES (one wave per
state, 1024 threads; the one-wave coarsest level is solved in one launch and never leaves u of it out), and one four-level script."""
import hashlib
import json
import os

import numpy as np

import cases
import heat1d_cycles as hc

GOLDEN_FILE = os.path.join(cases.GOLDEN, "pending_trace.json")
NT, CHUNK = 1025, 4
SIZES = (hc.SIZES[0], hc.SIZES[-1])
GETTERS = ("mgrit_hip_deferred", "mgrit_hip_twin", "mgrit_hip_lagged", "mgrit_hip_up2_pending")


class Traced:
    """every export but the four getters"""

    def __contains__(self, name):
        return name.startswith("mgrit_hip_") and name not in GETTERS


class Tracer(hc.Probe):
    """the record tests' probe, watching every call: the state of the four records behind it goes to `trace` (and nothing to `log`)"""

    def __init__(self, lib, h, n_levels):
        super().__init__(lib, h, Traced(), lambda lib, h, name, args: self.note(name), n_levels)
        self.trace = []

    def state(self):
        lib, h = self._lib, self._h
        return "held %s twin %s lag %d up %d" % (",".join(str(lib.mgrit_hip_deferred(h, l)) for l in range(self._n)),
                                                  ",".join(str(lib.mgrit_hip_twin(h, l)) for l in range(self._n)),
                                                  lib.mgrit_hip_lagged(h, 0), lib.mgrit_hip_up2_pending(h))

    def note(self, label):
        self.trace.append((label, self.state()))


def build(nx, lag=2, up2=1, twin=None, levels=3, **kw):
    env = {"MGRIT_HIP_UP2": str(up2)}
    if twin is not None:
        env["MGRIT_HIP_TWIN"] = str(twin)
    return hc.lag_build(nx, True, NT, CHUNK, lag, env=env, levels=levels, probe=lambda lib, h: Tracer(lib, h, levels), **kw)


def step(mg, label, fn):
    out = fn()
    mg.backend.lib.note("step " + label)
    return out


def blind(mg, first, n):
    for it in range(first, first + n):
        step(mg, f"cycle {it}", lambda: hc.blind_cycle(mg, it))


# ---- the scripts: name -> function of the state size that returns the solver it has driven --------------------------------------
def s_six_blind_cycles(nx):
    mg = build(nx)
    blind(mg, 0, 6)
    return mg


def s_guard(name, state):
    def run(nx):
        mg = build(nx)
        n = {"done1": 3, "done0": 2, "noted": 2}[state]
        blind(mg, 0, n)
        rest = None
        if state == "noted":
            rest = step(mg, "half cycle", lambda: hc.half_cycle(mg, n))
            n += 1
        step(mg, "guard " + name, lambda: hc.UP2_GUARDS[name](mg))
        if rest is not None:
            step(mg, "way up of level 0", lambda: mg.backend.ec_relax_res(*rest))
            mg.backend.residual_ready(mg._c_points(0))
            mg.convergence_criterion(iteration=n)
            mg.compute_residual()
        step(mg, "finish", lambda: hc.up2_finish(mg, n))
        return mg
    return run


def s_second_way_up_of_level_0(nx):
    mg = build(nx)
    blind(mg, 0, 2)
    step(mg, "second way up", lambda: mg._up(0, mg._level_intervals(0)))
    mg.convergence_criterion(iteration=3)
    mg.compute_residual()
    step(mg, "finish", lambda: hc.up2_finish(mg, 2))
    return mg


def s_waiting_rule_lag(nx):
    """lag mode 1: a look at level 0 behind a lagging way up is a miss; the wait goes 2 -> 4 -> 8"""
    mg = build(nx, lag=1, max_iter=40)
    it = 0
    for n in (5, 6, 10):
        blind(mg, it, n)
        it += n
        step(mg, "look at level 0", lambda: mg.backend.natural("u", 0))
    blind(mg, it, 2)
    return mg


def s_waiting_rule_up(nx):
    """lag mode 1, a look at u of level 1 behind every cycle from the fourth on: the wait of the level-1 record goes 1 -> 2 -> 4 -> 8"""
    mg = build(nx, lag=1, max_iter=40)
    for it in range(14):
        blind(mg, it, 1)
        if it >= 3:
            step(mg, "look at level 1", lambda: mg.backend.natural("u", 1))
    return mg


APART, NOT_APART = [(0, 0)], [(4, 1), (8, 2)]      # (fine point, coarse slot): the first point of the level / two closing C-points


def s_pairs_lag(call, pairs):
    """a pair list on level 0 with a lag record (and the level-1 record) pending"""
    def run(nx):
        mg = build(nx)
        blind(mg, 0, 2)
        step(mg, call, lambda: getattr(mg.backend, call)(0, pairs))
        step(mg, "finish", lambda: hc.up2_finish(mg, 2))
        return mg
    return run


def s_pairs_twin(pairs):
    """mgrit_hip_copy_pairs_u_to_v on level 0 with the twin record of level 1 pending"""
    def run(nx):
        mg = build(nx, twin=3)
        step(mg, "pending", lambda: hc.twin_pending(mg, 1))
        step(mg, "copy", lambda: mg.backend.copy_pairs_u_to_v(0, pairs))
        step(mg, "finish", lambda: hc.twin_finish(mg))
        return mg
    return run


def s_twin(lvl, partner):
    """the twin record of level lvl met by its partner (the F-C-relaxation of the cycle's own list / the coarsest level's solve) or by
    somebody else (an F-C-relaxation of every second interval / the solve phase by phase)"""
    def run(nx):
        mg = build(nx, twin=3)
        step(mg, "pending", lambda: hc.twin_pending(mg, lvl))
        if partner:
            step(mg, "partner", lambda: mg.iteration(lvl=lvl, cycle_type='V', iteration=2, first_f=True))
        else:
            step(mg, "non-partner", lambda: (hc.twin_relax('FC') if lvl == 1 else hc.twin_block_solve_by_phases)(mg, lvl))
        step(mg, "cycle", lambda: hc.twin_cycle(mg, 3))
        return mg
    return run


def s_stream_switch(nx):
    import torch
    mg = build(nx)
    be = mg.backend
    blind(mg, 0, 2)
    home, other = be._cur_stream, torch.cuda.Stream()
    step(mg, "to another stream", lambda: be._use_stream(other))
    torch.cuda.synchronize()
    step(mg, "back", lambda: be._use_stream(home))
    torch.cuda.synchronize()
    blind(mg, 2, 2)
    return mg


def s_modes(lag, up2, twin):
    def run(nx):
        mg = build(nx, lag=lag, up2=up2, twin=twin)
        blind(mg, 0, 4)
        step(mg, "look at the coarse levels", lambda: hc.coarse_state(mg))
        blind(mg, 4, 1)
        return mg
    return run


def s_four_levels(nx):
    mg = build(nx, twin=3, levels=4)
    for it in range(4):
        blind(mg, it, 1)
        if it % 2:
            step(mg, "look at the coarse levels", lambda: hc.coarse_state(mg))
    return mg


def _make_scripts():
    out = {"six_blind_cycles": s_six_blind_cycles, "second_way_up_of_level_0": s_second_way_up_of_level_0,
           "waiting_rule_lag": s_waiting_rule_lag, "waiting_rule_up": s_waiting_rule_up, "stream_switch_lag_pending": s_stream_switch}
    for name in sorted(hc.UP2_GUARDS):
        for state in ("done1", "done0", "noted"):
            out[f"guard_{name}_{state}"] = s_guard(name, state)
    for call in ("copy_pairs_u_to_v", "restrict_u"):
        out[f"{call}_lag_apart"], out[f"{call}_lag_not_apart"] = s_pairs_lag(call, APART), s_pairs_lag(call, NOT_APART)
    out["copy_pairs_twin_apart"], out["copy_pairs_twin_not_apart"] = s_pairs_twin(APART), s_pairs_twin(NOT_APART)
    for lvl in (1, 2):
        out[f"twin_{lvl}_partner"], out[f"twin_{lvl}_non_partner"] = s_twin(lvl, True), s_twin(lvl, False)
    for lag in (0, 1, 2):
        for up2 in (0, 1):
            for twin in range(4):
                out[f"modes_lag{lag}_up{up2}_twin{twin}"] = s_modes(lag, up2, twin)
    return out


SCRIPTS = _make_scripts()
CASES = [(name, nx) for name in sorted(SCRIPTS) for nx in SIZES] + [("four_levels", SIZES[0])]


def case_id(case):
    return f"{case[0]}/nx{case[1]}"


def run_case(case):
    """{"calls": notes taken, "trace": digest of all of them, "changes": [[index, label, state]] where the state moved, "slabs": digests}"""
    name, nx = case
    mg = (s_four_levels if name == "four_levels" else SCRIPTS[name])(nx)
    be = mg.backend
    for lvl in range(mg.lvl_max):
        be.lib.mgrit_hip_settle(be.h, lvl)
    be.sync()
    trace = be.lib.trace
    changes = [[k, label, state] for k, (label, state) in enumerate(trace) if k == 0 or state != trace[k - 1][1]]
    slabs = {}
    for lvl in range(mg.lvl_max):
        for which, slab in (("u", be._U), ("v", be.V), ("g", be.G)):
            if slab[lvl] is not None:
                slabs[f"{which}{lvl}"] = hashlib.sha256(np.ascontiguousarray(slab[lvl].cpu().numpy()).tobytes()).hexdigest()
    return {"calls": len(trace), "trace": hashlib.sha256(json.dumps(trace).encode()).hexdigest(), "changes": changes, "slabs": slabs}


# ---- the golden file: small enough to read. Labels and states are kept once in two tables and a change is three integers; the slab
# digests of a case are folded into one (run_case still hands out each, and the test prints them when the folded one differs) -------
def slabs_digest(slabs):
    return hashlib.sha256(json.dumps(sorted(slabs.items())).encode()).hexdigest()


def pack(hipcc, results):
    """the golden record of {case id: run_case result}"""
    labels = sorted({c[1] for r in results.values() for c in r["changes"]})
    states = sorted({c[2] for r in results.values() for c in r["changes"]})
    li, si = {x: k for k, x in enumerate(labels)}, {x: k for k, x in enumerate(states)}
    cases = {cid: {"calls": r["calls"], "trace": r["trace"], "slabs": slabs_digest(r["slabs"]),
                   "changes": [x for k, label, state in r["changes"] for x in (k, li[label], si[state])]} for cid, r in results.items()}
    return {"hipcc": hipcc, "labels": labels, "states": states, "cases": cases}


def unpack(golden, cid):
    """a case of the golden record in run_case's form, its slab digests folded"""
    rec, flat = golden["cases"][cid], golden["cases"][cid]["changes"]
    changes = [[flat[k], golden["labels"][flat[k + 1]], golden["states"][flat[k + 2]]] for k in range(0, len(flat), 3)]
    return {"calls": rec["calls"], "trace": rec["trace"], "changes": changes, "slabs": rec["slabs"]}


def dump(golden, path):
    """one line per table and per case"""
    short = dict(separators=(",", ":"))
    with open(path, "w") as f:
        f.write('{"hipcc":%s,\n"labels":%s,\n"states":%s,\n"cases":{\n' % tuple(json.dumps(golden[k], **short) for k in ("hipcc", "labels", "states")))
        f.write(",\n".join("%s:%s" % (json.dumps(cid), json.dumps(golden["cases"][cid], sort_keys=True, **short)) for cid in sorted(golden["cases"])))
        f.write("\n}}\n")
