"""Every way down and up a level that ``Mgrit.iteration()`` can take, pinned call by call: the driver runs over a stand-in
backend that answers the capability questions of one case and records every other call (name, arguments, order), on one rank
and on several (threads over tests/mock_comm.py). What it records is compared with tests/golden/cycle_routes.json: per case
and rank the (name, level) sequence in clear text and a SHA-256 of the full argument trace. The file is written by

    python tests/test_cycle_routes.py --write

and is NOT rewritten when the host driver is restructured: a refactoring of core/mgrit.py / core/rank_schedules.py passes
against the file as recorded before it. No GPU: the hierarchy is Heat1D with ``device_stepper`` masked."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    _here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(_here), _here]

from mock_comm import run_ranks

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cycle_routes.json")


def _uniform(n0, n1, n2):
    return [np.linspace(0, 1, n) for n in (n0, n1, n2)]


def _gapless():
    """three levels, non-uniform coarsening: fine points 8 and 9 are both C-points, so one interval has no F-point"""
    fine = np.linspace(0, 1, 33)
    mid = fine[[0, 4, 8, 9, 12, 16, 20, 24, 28, 32]]
    return [fine, mid, mid[[0, 2, 4, 6, 9]]]


GRIDS = {"65": lambda: _uniform(65, 17, 5), "129": lambda: _uniform(129, 33, 9), "gapless": _gapless}

_ALL = staticmethod(lambda lvl: True)
CAPS = {
    "none": {},
    "fas_ec": {"can_fuse_fas": _ALL, "can_fuse_ec": _ALL},
    "level": {"can_fuse_level": staticmethod(lambda lvl: lvl == 0), "can_fuse_coarse_down": staticmethod(lambda lvl: lvl > 0),
              "can_fuse_fas": _ALL, "can_fuse_ec": _ALL},
    "gen": {"can_gen_level": _ALL, "can_fuse_ec": _ALL},
}
CAPS["level_up"] = dict(CAPS["level"], can_fuse_level_up=_ALL)


def _canon(x):
    """arguments as JSON-able values; index lists (IndexList / IndexArray / lists of tuples) flattened to lists of ints"""
    if x is None or isinstance(x, (bool, str)):
        return x
    if isinstance(x, (int, np.integer)):
        return int(x)
    if isinstance(x, (float, np.floating)):
        return float(x)
    if isinstance(x, dict):
        return {str(k): _canon(v) for k, v in sorted(x.items())}
    if isinstance(x, np.ndarray):
        return x.tolist()
    return [_canon(v) for v in x]       # list, tuple, IndexList, IndexArray


class Recorder:
    """the stand-in backend: answers the can_* questions it was given (the others do not exist), every other call is recorded
    and returns None; the rows of an exchange point arrive as backend.exchange / exchange_staged (device_links)"""
    device_links = True
    block_r = {}
    block_sharded = {}

    def __init__(self, caps, cycle_pre=False, mirror_on=False):
        self.__dict__.update(caps={k: v.__func__ for k, v in caps.items()}, calls=[], _cycle_pre=cycle_pre, _mirror_on=mirror_on,
                             _follows=False)

    @property
    def f_relax_follows(self):
        return self._follows

    @f_relax_follows.setter
    def f_relax_follows(self, value):
        self.__dict__["_follows"] = value
        self.calls.append(("set_f_relax_follows", [bool(value)], {}))

    def __getattr__(self, name):
        if name.startswith("can_"):
            if name in self.caps:
                return self.caps[name]
            raise AttributeError(name)
        if name.startswith("__"):
            raise AttributeError(name)

        def call(*args, **kwargs):
            self.calls.append((name, _canon(args), _canon(kwargs)))
            return False if name == "plan_allowed" else None     # (program order: iteration() itself runs in every cycle)
        return call


def _subclass(kind):
    from pymgrit_amd import Mgrit
    if kind == "c_relax":
        class OwnCRelax(Mgrit):
            def c_relax(self, lvl):
                super().c_relax(lvl)
        return OwnCRelax
    if kind == "compute_residual":
        class OwnResidual(Mgrit):
            def compute_residual(self):
                return super().compute_residual()
        return OwnResidual
    return Mgrit


# name -> (grid, caps, ranks, aligned, Mgrit arguments, extras, markers that must appear, markers that must not)
# Every case runs the first cycle (iteration 0, opened by the level-0 F-relaxation) and a later one on the same object.
# extras: 'pre' (_cycle_pre), 'nested' (nested_iteration() first), 'sub:<method>' (a subclass overriding that method and
# nothing else), 'no_pass_on_level_0' (the grid leaves level 0 without a whole-level list)
CASES = {
    "plain_65":                 ("65", "none", 1, False, {}, (), ["fas_rhs"], ["cf_fas", "gen_down", "relax_FC"]),
    "plain_129_fused_sweeps_F": ("129", "fas_ec", 1, False, {"cycle_type": "F", "cf_iter": 2}, (), ["fas_fused", "ec_relax"],
                                 ["cf_fas", "gen_down", "relax_FC", "fas_rhs"]),
    "plain_65_conv1_cf0":       ("65", "fas_ec", 1, False, {"conv_crit": 1, "cf_iter": 0}, (), ["fas_fused"], ["cf_fas"]),
    "level_65":                 ("65", "level", 1, False, {}, (), ["cf_fas", "relax_FC", "fas_fused_f", "ec_relax_res"],
                                 ["ec_relax_res_up", "gen_down"]),
    "level_129_F_conv1":        ("129", "level", 1, False, {"cycle_type": "F", "conv_crit": 1}, (), ["cf_fas", "relax_FC", "fas_fused_f"],
                                 ["ec_relax_res"]),
    "level_65_weight":          ("65", "level", 1, False, {"weight_c": 1.3}, (), ["fas_fused"], ["cf_fas", "relax_FC", "fas_fused_f"]),
    "level_129_cf2":            ("129", "level", 1, False, {"cf_iter": 2}, (), ["cf_fas", "set_f_relax_follows"], ["relax_FC"]),
    "level_up_65":              ("65", "level_up", 1, False, {}, (), ["cf_fas", "relax_FC", "fas_fused_f", "ec_relax_res_up"], []),
    "level_up_129_F_cf0":       ("129", "level_up", 1, False, {"cycle_type": "F", "cf_iter": 0}, (), ["fas_fused_f", "ec_relax_res_up"],
                                 ["cf_fas", "relax_FC"]),
    "level_up_65_cf12":         ("65", "level_up", 1, False, {"cf_iter": [1, 2]}, (), ["cf_fas", "ec_relax_res_up"], ["relax_FC"]),
    "level_up_129_nested_F":    ("129", "level_up", 1, False, {"cycle_type": "F"}, ("nested",), ["cf_fas", "relax_FC", "interpolate"], []),
    "gen_65":                   ("65", "gen", 1, False, {}, (), ["gen_down", "gen_up"], ["cf_fas", "relax_FC"]),
    "gen_129_F_conv1_cf2":      ("129", "gen", 1, False, {"cycle_type": "F", "conv_crit": 1, "cf_iter": 2}, (),
                                 ["gen_down", "gen_up", "set_f_relax_follows"], []),
    "gen_65_cf0_nested":        ("65", "gen", 1, False, {"cf_iter": 0}, ("nested",), ["ec_relax"], ["gen_down"]),
    "gapless_level_up":         ("gapless", "level_up", 1, False, {}, ("no_pass_on_level_0",), ["fas_fused"], ["cf_fas"]),
    "gapless_gen":              ("gapless", "gen", 1, False, {}, ("no_pass_on_level_0",), ["fas_rhs"], []),
    "ranks2_plain":             ("65", "none", 2, False, {}, (), ["fas_rhs", "exchange"], ["cf_fas"]),
    "ranks3_plain_F_cf2":       ("129", "fas_ec", 3, False, {"cycle_type": "F", "cf_iter": 2, "conv_crit": 1}, (), ["fas_fused", "exchange"],
                                 ["cf_fas"]),
    "ranks2_shard":             ("65", "level", 2, False, {}, (), ["cf_fas", "relax_FC", "fas_fused_f", "ec_relax_res_to"], []),
    "ranks3_shard_cf211":       ("129", "level_up", 3, False, {"cf_iter": [2, 1, 1]}, (), ["cf_fas", "relax_FC", "ec_relax_res_to",
                                                                                           "set_f_relax_follows"], []),
    "ranks3_shard_F_conv1":     ("129", "level", 3, False, {"cycle_type": "F", "conv_crit": 1}, (), ["cf_fas", "relax_FC"],
                                 ["ec_relax_res_to"]),
    "ranks3_gen_unaligned":     ("65", "gen", 3, False, {}, (), ["ec_relax", "exchange"], ["gen_down"]),
    "aligned2_level_up":        ("65", "level_up", 2, True, {}, (), ["cf_fas", "relax_FC", "fas_fused_f", "exchange_staged",
                                                                    "ec_relax_res_up"], []),
    "aligned4_level_up_pre":    ("129", "level_up", 4, True, {}, ("pre",), ["cf_fas", "relax_FC", "exchange_staged"], []),
    "aligned4_level_F_nested":  ("129", "level", 4, True, {"cycle_type": "F"}, ("nested",), ["cf_fas", "relax_FC", "exchange_staged"], []),
    "aligned2_level_cf0":       ("65", "level_up", 2, True, {"cf_iter": 0}, (), ["fas_fused_f", "exchange"], ["cf_fas"]),
    "aligned2_gen":             ("65", "gen", 2, True, {}, (), ["gen_down", "gen_up", "exchange_staged"], []),
    "aligned4_gen_F_cf2":       ("129", "gen", 4, True, {"cycle_type": "F", "cf_iter": 2}, (), ["gen_down", "exchange_staged"], []),
    "own_c_relax":              ("65", "level_up", 1, False, {}, ("sub:c_relax",), ["fas_fused"],
                                 ["cf_fas", "relax_FC", "fas_fused_f", "ec_relax_res"]),
    "own_c_relax_gen":          ("65", "gen", 1, False, {}, ("sub:c_relax",), ["fas_rhs"], ["gen_down"]),
    # compute_residual is named by the whole-level and the general lists only (the residual sums are part of those passes):
    # level 0 goes sweep by sweep, the coarse-level passes and a rank's share of level 0 stay
    "own_residual":             ("65", "level_up", 1, False, {}, ("sub:compute_residual",), ["relax_FC", "fas_fused_f"],
                                 ["cf_fas", "ec_relax_res"]),
    "own_residual_gen":         ("65", "gen", 1, False, {}, ("sub:compute_residual",), ["fas_rhs"], ["gen_down"]),
    "own_residual_ranks2":      ("65", "level", 2, False, {}, ("sub:compute_residual",), ["cf_fas", "relax_FC", "ec_relax_res_to"], []),
}


def _marks(calls):
    """the calls that tell the routes apart"""
    got = set()
    for name, args, kwargs in calls:
        got.add(name)
        if name == "relax" and args[2] == "FC":
            got.add("relax_FC")
        if name == "fas_fused" and kwargs.get("with_f_relax"):
            got.add("fas_fused_f")
        if name == "ec_relax_res" and args[0] > 0:
            got.add("ec_relax_res_up")
    return got


def _accessors(mg):
    """every pass list of every level, asked twice: the second answer must be the very objects of the first (the backend
    hangs device handles on them, residual_ready compares by identity)"""
    out = {}
    for lvl in range(mg.lvl_max - 1):
        for label, ask in (("level", lambda: mg._level_intervals(lvl)), ("level_up", lambda: mg._level_intervals(lvl, up=True)),
                           ("gen", lambda: mg._gen_intervals(lvl)), ("coarse_down", lambda: mg._coarse_down(lvl)),
                           ("coarse_down_rank", lambda: mg._coarse_down_rank(lvl)), ("rank", lambda: mg._rank_intervals(lvl)),
                           ("rank_up", lambda: mg._rank_intervals_up(lvl))):
            first, second = ask(), ask()
            assert (first is None) == (second is None), (label, lvl)
            if first is not None:
                whole = label in ("level", "level_up", "gen")
                members = [(first, second)] if whole else list(zip(tuple(first), tuple(second)))
                for a, b in members:
                    if isinstance(a, (bool, int)):
                        assert a == b, (label, lvl)
                    else:
                        assert a is b, (label, lvl)
                        if len(a):
                            a.handle = 1    # (a plain list would refuse)
                first = first if whole else tuple(first)
            out[f"{label}:{lvl}"] = _canon(first)
    return out


def _run_rank(case, comm):
    from pymgrit_amd import Heat1D
    grid, caps, ranks, aligned, kwargs, extras, _, _ = CASES[case]
    prob = [Heat1D(x_start=0, x_end=1, nx=9, a=1, t_interval=t) for t in GRIDS[grid]()]
    for p in prob:
        p.device_stepper = lambda: None          # host path: no GPU here
    sub = [e[4:] for e in extras if e.startswith("sub:")]
    mg = _subclass(sub[0] if sub else None)(prob, logging_lvl=40, max_iter=1, nested_iteration=False, comm_time=comm, **kwargs)
    rec = Recorder(CAPS[caps], cycle_pre="pre" in extras)
    mg.backend = rec
    if ranks > 1:
        detected = mg._detect_aligned()
        assert detected or not aligned, case      # (an aligned case sits on a grid whose shares really end on C-points)
        mg._aligned = aligned
        mg.__dict__.pop("_index_lists", None)
    del rec.calls[:]
    if "nested" in extras:
        mg.nested_iteration()
    mg.iteration(0, mg.cycle_type, 0, True)
    mg.iteration(0, mg.cycle_type, 1, False)
    mg.compute_residual()
    calls = list(rec.calls)
    lists = _accessors(mg)
    if "no_pass_on_level_0" in extras:       # an interval without F-point: neither whole-level list exists
        assert lists["level:0"] is None and lists["level_up:0"] is None and lists["gen:0"] is None
    return {"calls": calls, "lists": lists}


def _run_case(case):
    ranks = CASES[case][2]
    if ranks == 1:
        return [_run_rank(case, None)]
    return run_ranks(ranks, lambda comm: _run_rank(case, comm), timeout=60)


def _digest(rank_result):
    blob = json.dumps(rank_result, sort_keys=True, separators=(",", ":"))
    seq = " ".join(f"{name}:{args[0] if args and isinstance(args[0], int) and not isinstance(args[0], bool) else '-'}"
                   for name, args, _ in rank_result["calls"])
    return {"sequence": seq, "sha256": hashlib.sha256(blob.encode()).hexdigest()}


def _golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


def test_the_fixture_holds_exactly_the_cases_of_this_module():
    assert sorted(_golden()["cases"]) == sorted(CASES)


@pytest.mark.parametrize("case", sorted(CASES))
def test_cycle_route(case):
    want = _golden()["cases"].get(case)
    assert want is not None, f"{case} is not in {GOLDEN}"
    got = _run_case(case)
    seen = set().union(*(_marks(r["calls"]) for r in got))
    _, _, _, _, _, _, present, absent = CASES[case]
    assert not [m for m in present if m not in seen], (case, "route not reached", sorted(seen))
    assert not [m for m in absent if m in seen], (case, "unexpected route", sorted(seen))
    assert len(want) == len(got)
    for rank, (w, r) in enumerate(zip(want, got)):
        g = _digest(r)
        assert g["sequence"].split() == w["sequence"].split(), (case, rank)
        assert g["sha256"] == w["sha256"], (case, rank, "same calls in the same order, other arguments or other pass lists")


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: python tests/test_cycle_routes.py --write")
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    head = subprocess.run(["git", "-C", root, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip()
    doc = {"recorded_at": head or None, "cases": {case: [_digest(r) for r in _run_case(case)] for case in sorted(CASES)}}
    with open(GOLDEN, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(f"wrote {len(doc['cases'])} cases to {GOLDEN}")
