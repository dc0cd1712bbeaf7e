"""GPU: what ``HipBackend`` asks of the library and of its streams, pinned call by call. ``hip_lib.load`` is replaced by a proxy
around the real library that forwards every call and records those that core/backend_hip.py makes (export name, ``c_int``
arguments, ``c_double`` arguments by ``float.hex()``, ``c_void_p`` arguments as null / non-null, host arrays whose length follows
from the call's own integers by the SHA-256 of their bytes, the stream of ``mgrit_hip_set_stream`` by ordinal of first appearance;
typed output pointers are left out); ``torch.cuda.Event.record``, ``torch.cuda.Stream.wait_event`` and
``torch.cuda.Event.synchronize`` are wrapped for the duration of a case and record (operation, stream ordinal, event ordinal) into
the same list. The list is per thread: loopback ranks are threads, a trace is a rank's. What is recorded is compared with
tests/golden/backend_calls.json: per case and rank the name sequence in clear text (runs of one name as ``name*k``) and a SHA-256
of the full trace. The file is written by

    python tests/test_hip_backend_calls.py --write

and is NOT rewritten when core/backend_hip.py is restructured: a refactoring passes against the file as recorded before it.
``mgrit_hip_destroy`` runs whenever the collector finds an old engine, so it is noted as reached and kept out of the traces."""
import contextlib
import ctypes as C
import gc
import hashlib
import json
import os
import re
import sys
import threading

import numpy as np
import pytest

if __name__ == "__main__":
    _here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(_here), _here]

import cases
import dist_worker

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "backend_calls.json")
BACKEND_SOURCE = os.path.join(dist_worker.ROOT, "pymgrit_amd", "core", "backend_hip.py")
NOT_REACHED = {"mgrit_hip_links_close"}      # only after a neighbour's timeout, which nobody provokes

_TL = threading.local()       # .rec: the Recording of the case this thread (= rank) is running, or absent
_DESTROYED = set()


def _cols(n_at, *positions):
    return {p: (lambda a, n_at=n_at: 4 * a[n_at]) for p in positions}


# export -> {argument position: bytes of the host array there, from the call's integer arguments}
HOST_ARRAYS = {
    "mgrit_hip_runs_create": _cols(2, 3, 4),
    "mgrit_hip_pairs_create": _cols(2, 3, 4),
    "mgrit_hip_triples_create": _cols(2, 3, 4, 5),
    "mgrit_hip_ec_runs_create": _cols(2, 3, 4, 5),
    "mgrit_hip_intervals_create": _cols(2, 3, 4, 5, 6, 7, 10),
    # (h, lvl, n_pts, t_local, n, ld, fac, K, s, tau)
    "mgrit_hip_level_heat1d": {3: lambda a: 8 * a[2], 8: lambda a: 8 * a[7] * a[4], 9: lambda a: 8 * a[7] * a[2]},
    # (h, lvl, n_pts, t_local, n, ld, fac, dtau, order, K, s, tau, tau2)
    "mgrit_hip_level_heat1d_2pts": {3: lambda a: 8 * a[2], 10: lambda a: 8 * a[9] * a[4], 11: lambda a: 8 * a[9] * a[2],
                                    12: lambda a: 8 * a[9] * a[2]},
    "mgrit_hip_level_advection1d": {3: lambda a: 8 * a[2]},
    # (h, lvl, n_pts, t_local, nx, ny, ld, fx, fy, theta, bc, K, S, tau)
    "mgrit_hip_level_heat2d": {3: lambda a: 8 * a[2], 10: lambda a: 8 * a[4] * a[5], 12: lambda a: 8 * a[11] * (a[4] - 2) * (a[5] - 2),
                               13: lambda a: 8 * a[11] * a[2]},
    "mgrit_hip_level_allencahn2d": {3: lambda a: 8 * a[2]},
    # (kind, n, fac, n_points, global t, out)
    "mgrit_hip_block_solve_rank": {4: lambda a: 8 * a[3]},
}


def _plain(a):
    """a ctypes argument as a Python number (pointers: the address, null = 0)"""
    if a is None:
        return 0
    a = getattr(a, "value", a)
    return 0 if a is None else a


class Recording:
    def __init__(self):
        self.calls, self.streams, self.events = [], {}, {}

    def stream(self, address):
        return self.streams.setdefault(int(address or 0), len(self.streams))

    def event(self, ev):
        # (the event itself is kept: an address that the allocator hands out again must not take the ordinal of a dead event)
        return self.events.setdefault(id(ev), (len(self.events), ev))[0]

    def lib_call(self, name, args):
        from pymgrit_amd.core import hip_lib
        argtypes = hip_lib.EXPORTS[name][1]
        a = [_plain(x) if t in (C.c_int, C.c_double, C.c_void_p) else None for t, x in zip(argtypes, args)]
        out = []
        for i, t in enumerate(argtypes):
            if t is C.c_int:
                out.append(int(a[i]))
            elif t is C.c_double:
                out.append(float(a[i]).hex())
            elif t is C.c_void_p:
                if name == "mgrit_hip_set_stream" and i == 1:
                    out.append(f"stream{self.stream(a[i])}")
                elif not a[i]:
                    out.append("null")
                elif i in HOST_ARRAYS.get(name, {}):
                    out.append(hashlib.sha256(C.string_at(a[i], int(HOST_ARRAYS[name][i](a)))).hexdigest())
                else:
                    out.append("ptr")
        self.calls.append([name[len("mgrit_hip_"):], out])

    def stream_op(self, op, stream, ev):
        self.calls.append([op, [None if stream is None else f"stream{self.stream(stream.cuda_stream)}", f"event{self.event(ev)}"]])


class LibProxy:
    """forwards every export to the real library; calls made by core/backend_hip.py on a recording thread are noted first"""

    def __init__(self, lib):
        self.__dict__["_lib"] = lib

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*args):
            if sys._getframe(1).f_code.co_filename.endswith("backend_hip.py"):
                if name == "mgrit_hip_destroy":
                    _DESTROYED.add(name)
                else:
                    rec = getattr(_TL, "rec", None)
                    if rec is not None:
                        rec.lib_call(name, args)
            return fn(*args)
        self.__dict__[name] = call
        return call


@contextlib.contextmanager
def recording_installed():
    """hip_lib.load answers with the proxy, the three stream operations record; everything is put back at the end"""
    from pymgrit_amd.core import hip_lib
    load, record, wait_event, synchronize = hip_lib.load, torch.cuda.Event.record, torch.cuda.Stream.wait_event, torch.cuda.Event.synchronize
    proxy = LibProxy(load())

    def rec_record(self, stream=None):
        rec = getattr(_TL, "rec", None)
        if rec is not None:
            rec.stream_op("record", stream if stream is not None else torch.cuda.current_stream(), self)
        return record(self, stream)

    def rec_wait_event(self, event):
        rec = getattr(_TL, "rec", None)
        if rec is not None:
            rec.stream_op("wait_event", self, event)
        return wait_event(self, event)

    def rec_synchronize(self):
        rec = getattr(_TL, "rec", None)
        if rec is not None:
            rec.stream_op("synchronize", None, self)
        return synchronize(self)
    hip_lib.load = lambda: proxy
    torch.cuda.Event.record, torch.cuda.Stream.wait_event, torch.cuda.Event.synchronize = rec_record, rec_wait_event, rec_synchronize
    try:
        yield
    finally:
        hip_lib.load = load
        torch.cuda.Event.record, torch.cuda.Stream.wait_event, torch.cuda.Event.synchronize = record, wait_event, synchronize


@contextlib.contextmanager
def environment(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


# ---- the hierarchies -----------------------------------------------------------------------------------------------------------
def _from_worker(name):
    return lambda: dist_worker.build_problem(name, "hip")


def _allen_cahn():
    """the small solve of tests/test_hip_allen_cahn.py (test_output_fcn_and_cf_iter)"""
    from pymgrit_amd import AllenCahn
    from allen_cahn_fixtures import META
    return ([AllenCahn(nx=20, method="IMEX", t_start=0, t_stop=META["t_stop"], nt=nt) for nt in (33, 9)], None,
            dict(cf_iter=2, max_iter=3, tol=0.0))


def _general_forcing():
    """forcing_rows on Heat1D levels (tests/test_hip_forcing.py)"""
    return cases.general_forcing_problem(65, [cases.lin(2, 65), cases.lin(2, 17), cases.lin(2, 5)]), None, dict(max_iter=3, tol=0.0)


def _general_forcing_heat2d():
    """forcing_rows on Heat2D levels"""
    return [cases.h2d_general_app(12, 10, t) for t in cases.h2d_grids([33, 9])], None, dict(max_iter=3, tol=0.0, nested_iteration=False)


def _user_transfer():
    """a user's GridTransfer between Heat1D levels (tests/test_hip_user_transfer.py): restriction and interpolation on the host"""
    from pymgrit_amd import GridTransfer, GridTransferCopy, GridTransferHeat
    from pymgrit_amd.heat.heat_1d import VectorHeat1D

    class UserFullWeighting(GridTransfer):
        def restriction(self, u):
            f = u.get_values()
            n_c = (len(f) - 1) // 2
            out = VectorHeat1D(n_c)
            out.set_values(f[0:2 * n_c:2] * 1 / 4 + f[1:2 * n_c:2] * 1 / 2 + f[2:2 * n_c + 1:2] * 1 / 4)
            return out

        def interpolation(self, u):
            c = u.get_values()
            vals = np.zeros(2 * len(c) + 1)
            vals[1::2] += c
            vals[2::2] += 1 / 2 * c
            vals[0:len(vals) - 1:2] += 1 / 2 * c
            out = VectorHeat1D(len(vals))
            out.set_values(vals)
            return out

    class OwnCopy(GridTransferCopy):
        def restriction(self, u):
            return super().restriction(u)
    prob, tr, opts = dist_worker.build_problem("heat_spatial_coarsening", "hip")
    return prob, [UserFullWeighting() if isinstance(t, GridTransferHeat) else OwnCopy() for t in tr], opts


# ---- what a case does with its solver -------------------------------------------------------------------------------------------
def _solve(mg):
    mg.solve()


def _solve_then_hooks(mg):
    """a solve, then the measurement hooks and the questions about routes that the tools and bench.py ask"""
    mg.solve()
    be = mg.backend
    be.set_timing(True)
    be.timing_drain()
    be.relax(0, mg._f_runs(0), 'F')
    be.last_kernel_ms()         # (of the timed launch just made: a drain forgets it)
    mg.iteration(lvl=0, cycle_type='V', iteration=0, first_f=True)
    be.timing_drain()
    be.chain_clock()
    be.set_timing(False)
    triples = mg._coarse_down(1)[1]
    be.fas_chunks(1, triples)
    be.set_fas_chunk(-1)
    be.fas_chunks(1, triples)
    be.set_fas_chunk(0)
    be.block_solve_form(mg.lvl_max - 1)
    be.sync()


def _by_hand(mg):
    """the sequence of test_c_point_storage_rebuilds_every_f_point (tests/test_hip_level_fusion.py)"""
    for it in range(4):
        mg.iteration(lvl=0, cycle_type='V', iteration=it, first_f=True)
        mg.convergence_criterion(iteration=it + 1)
    mg.u[0][2].get_values()
    mg.backend.natural("u", 0)
    mg.iteration(lvl=0, cycle_type='V', iteration=4, first_f=True)
    mg.convergence_criterion(iteration=5)
    mg.c_relax(0)
    mg.f_relax(0)
    mg.iteration(lvl=0, cycle_type='V', iteration=5, first_f=True)
    mg.backend.U[0]
    mg.backend.set_natural("u", 0, mg.backend.natural("u", 0))
    mg.iteration(lvl=0, cycle_type='V', iteration=6, first_f=True)


def _case(make, ranks=1, env=None, run=_solve, **kw):
    if isinstance(make, str):
        make = _from_worker(make)
    return dict(make=make, ranks=ranks, env=env or {}, run=run, kw=kw)


CASES = {
    "heat_nx33_V_nested": _case("heat_nx33_V_nested"),
    "heat_nx33_V_nested_blocks1": _case("heat_nx33_V_nested", plan_blocks=1),
    "heat_nx33_V_nested_hooks": _case("heat_nx33_V_nested", run=_solve_then_hooks),
    "heat_nx33_F_nonested": _case("heat_nx33_F_nonested"),
    "heat_nx33_V_jump": _case("heat_nx33_V_jump"),
    "heat_nx33_V_cf2": _case("heat_nx33_V_cf2"),
    "heat_nx33_V_weight13": _case("heat_nx33_V_weight13"),
    "heat_nx257_nt257_blocks2": _case("heat_nx257_nt257", plan_blocks=2),
    "heat_nx257_nt257_blocks2_graph": _case("heat_nx257_nt257", env={"PYMGRIT_AMD_PLAN_GRAPH": "1"}, plan_blocks=2),
    "heat_nx257_nt257_store_all_f": _case("heat_nx257_nt257", env={"PYMGRIT_AMD_STORE_ALL_F": "1"}),
    "heat_nx257_nt257_no_pre_relax": _case("heat_nx257_nt257", env={"PYMGRIT_AMD_NO_PRE_RELAX": "1"}),
    "heat_nx257_nt257_by_hand": _case("heat_nx257_nt257", run=_by_hand),
    "heat_nx257_nt257_by_hand_blocks2": _case("heat_nx257_nt257", run=_by_hand, plan_blocks=2),
    "heat_spatial_coarsening": _case("heat_spatial_coarsening"),
    "advection_3lvl_F": _case("advection_3lvl_F"),
    "heat_nx2050_wide": _case("heat_nx2050_wide"),
    "heat_nx2050_wide_blocks2": _case("heat_nx2050_wide", plan_blocks=2),      # (chain parts that resume the part before them)
    "heat_nx3100_wide_2lvl": _case("heat_nx3100_wide_2lvl"),
    "bdf2_example_small": _case("bdf:bdf2_example_small"),
    "h2d_be_3lvl_F_bc": _case("h2d:be_3lvl_F_bc"),
    "h2d_be_3lvl_F_bc_masked": _case("h2d:be_3lvl_F_bc", env={"PYMGRIT_AMD_PLAN_BLOCKS_HEAT2D": "3"}),
    "h2d_general_forcing": _case(_general_forcing_heat2d),
    "allen_cahn_small": _case(_allen_cahn),
    "heat_general_forcing": _case(_general_forcing),
    "heat_user_transfer": _case(_user_transfer),
    "ranks2_heat_nx33_V_nested": _case("heat_nx33_V_nested", ranks=2),
    "ranks3_heat_nx33_V_nested": _case("heat_nx33_V_nested", ranks=3),
    "ranks4_heat_nx257_nt257": _case("heat_nx257_nt257", ranks=4),
    "ranks4_heat_nx33_procs_without_points": _case("heat_nx33_procs_without_points", ranks=4),
    "ranks4_heat_blk_r127_2lvl": _case("heat_blk_r127_2lvl", ranks=4),
    "ranks3_heat_nx33_V_nested_depth1": _case("heat_nx33_V_nested", ranks=3, pipeline_depth=1),
    "ranks2_at_heat_nx33_k3": _case("at:heat_nx33_k3", ranks=2),
}


def _run_rank(case, comm):
    from pymgrit_amd import AtMgrit, Mgrit
    spec = CASES[case]
    _TL.rec = rec = Recording()
    try:
        prob, tr, opts = spec["make"]()
        opts = dict(opts, **spec["kw"])
        make = Mgrit
        if "_at_k" in opts:
            k = opts.pop("_at_k")
            make = lambda *a, **kw: AtMgrit(k, 0, *a, **kw)   # noqa: E731
        mg = make(prob, transfer=tr, logging_lvl=30, comm_time=comm, **opts)
        assert type(mg.backend).__name__ == "HipBackend"
        assert comm is None or mg.backend.device_links
        spec["run"](mg)
        mg.backend.sync()
    finally:
        _TL.rec = None
    return rec.calls


_TRACES = {}     # case -> [per-rank calls]: recorded once per process, shared by the case's test and the coverage test


def _run_case(case):
    if case not in _TRACES:
        from pymgrit_amd.core.comm import run_loopback_ranks
        spec = CASES[case]
        with environment(spec["env"]), recording_installed():
            if spec["ranks"] == 1:
                got = [_run_rank(case, None)]
            else:
                world, got = run_loopback_ranks(spec["ranks"], lambda comm: _run_rank(case, comm))
                world.close()
        _TRACES[case] = got
    return _TRACES[case]


def _sequence(calls):
    out = []
    for name, _ in calls:
        if out and out[-1][0] == name:
            out[-1][1] += 1
        else:
            out.append([name, 1])
    return " ".join(name if k == 1 else f"{name}*{k}" for name, k in out)


def _digest(calls):
    blob = json.dumps(calls, separators=(",", ":"))
    return {"sequence": _sequence(calls), "sha256": hashlib.sha256(blob.encode()).hexdigest()}


def _golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


def _names_in_source():
    with open(BACKEND_SOURCE) as fh:
        return set(re.findall(r"self\.lib\.(mgrit_hip_\w+)", fh.read()))


def _missing(seen):
    gc.collect()        # the engines of the cases so far: their destructors are the backend's only mgrit_hip_destroy
    return sorted(_names_in_source() - seen - _DESTROYED - NOT_REACHED)


def test_the_fixture_holds_exactly_the_cases_of_this_module():
    assert sorted(_golden()["cases"]) == sorted(CASES)


@pytest.mark.parametrize("case", sorted(CASES))
def test_backend_calls(case):
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU visible")
    want = _golden()["cases"].get(case)
    assert want is not None, f"{case} is not in {GOLDEN}"
    got = _run_case(case)
    assert len(want) == len(got)
    for rank, (w, calls) in enumerate(zip(want, got)):
        g = _digest(calls)
        assert g["sequence"].split() == w["sequence"].split(), (case, rank)
        assert g["sha256"] == w["sha256"], (case, rank, "same calls in the same order, other arguments")


def test_every_export_the_backend_names_is_reached():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU visible")
    seen = set()
    for case in sorted(CASES):
        for calls in _run_case(case):
            seen.update("mgrit_hip_" + name for name, _ in calls)
    assert not _missing(seen), _missing(seen)


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: python tests/test_hip_backend_calls.py --write")
    import subprocess
    head = subprocess.run(["git", "-C", dist_worker.ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip()
    doc = {"recorded_at": head or None, "cases": {}}
    for case in sorted(CASES):
        doc["cases"][case] = [_digest(calls) for calls in _run_case(case)]
        print(f"{case}: {[len(calls) for calls in _run_case(case)]} calls", flush=True)
    left = _missing({"mgrit_hip_" + name for case in CASES for calls in _run_case(case) for name, _ in calls})
    if left:
        sys.exit(f"exports named by core/backend_hip.py that no case reaches: {left}")
    with open(GOLDEN, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(f"wrote {len(doc['cases'])} cases to {GOLDEN}")
