"""What the multi-process tests and their worker (dist_worker.py) share: ``launch``, which starts one worker process per rank and
collects what they saved, and the cases the worker builds by name. A plain helper like cases.py: no tests, no fixtures."""
import os
import socket
import subprocess
import sys
import tempfile

import numpy as np

import cases

HERE = os.path.dirname(os.path.abspath(__file__))


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


_ONE_RANK = {}     # results of one-rank launches, the baseline several tests compare their sharded runs with


def launch(world, case, mode="plugin", backend="gloo", timeout=600, depth=None, slow_rank=None, no_groups_rank=None,
           per_rank=False):
    # a one-rank run is a pure function of (case, mode, lag, the library's / package's environment switches): computed once per
    # session (every launch is a fresh process: a second or two of start-up each on the GPU box)
    memo = None
    if world == 1 and slow_rank is None and no_groups_rank is None:
        memo = (case, mode, depth, per_rank, tuple(sorted((k, v) for k, v in os.environ.items() if k.startswith(("MGRIT_", "PYMGRIT_")))))
        if memo in _ONE_RANK:
            return _ONE_RANK[memo]
    res = _launch(world, case, mode, backend, timeout, depth, slow_rank, no_groups_rank, per_rank)
    if memo is not None:
        _ONE_RANK[memo] = res
    return res


def _launch(world, case, mode, backend, timeout, depth, slow_rank, no_groups_rank, per_rank):
    out = tempfile.mkdtemp(prefix=f"mgrit_{case}_{world}_")
    port = free_port()
    env = dict(os.environ)
    env.pop("MGRIT_TEST_PIPELINE_DEPTH", None)
    env.pop("MGRIT_TEST_SLOW_RANK", None)
    if depth is not None:
        env["MGRIT_TEST_PIPELINE_DEPTH"] = str(depth)
    if slow_rank is not None:
        env["MGRIT_TEST_SLOW_RANK"] = str(slow_rank)
    env.pop("PYMGRIT_AMD_NO_EXTRA_GROUPS", None)
    if no_groups_rank is not None:
        env["PYMGRIT_AMD_NO_EXTRA_GROUPS"] = "1"
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "dist_worker.py"), str(r), str(world), str(port), case,
                               mode, out, backend], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env)
             for r in range(world)]
    logs = []
    try:
        for p in procs:
            o, _ = p.communicate(timeout=timeout)
            logs.append(o.decode(errors="replace"))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    bad = [r for r, p in enumerate(procs) if p.returncode != 0]
    if bad:
        # a rank that only saw its peer disappear is an echo of the real failure: show the root cause first
        root = [r for r in bad if "Connection closed by peer" not in logs[r]] or bad
        raise AssertionError(f"ranks {bad} failed; rank {root[0]}:\n{logs[root[0]][-3000:]}")
    res = [np.load(os.path.join(out, f"rank{r}.npz")) for r in range(world)]
    if per_rank:     # local criteria: every rank has its own residual history
        return [(r["conv"], r["u"]) for r in res]
    conv = res[0]["conv"]
    for r in res[1:]:
        assert np.array_equal(r["conv"], conv), "every rank must hold the same residual history"
    t = np.concatenate([r["t"] for r in res])
    u = np.concatenate([r["u"] for r in res if r["u"].size], axis=0)
    assert np.all(np.diff(t) > 0), "owned blocks must tile the time grid in rank order"
    return conv, u


AT_CASES = {   # AT-MGRIT (tests/test_at_mgrit.py): name -> (nx, nts, k, options)
    "heat_nx33_k1": (33, [65, 17, 5], 1, dict(tol=1e-9, max_iter=8)),
    "heat_nx33_k2": (33, [65, 17, 5], 2, dict(tol=1e-9, max_iter=8)),
    "heat_nx33_k3": (33, [65, 17, 5], 3, dict(tol=1e-9, max_iter=8)),
    "heat_nx33_k5": (33, [65, 17, 5], 5, dict(tol=1e-9, max_iter=8)),
    "heat_nx33_k3_nonested_F": (33, [129, 33, 9], 3, dict(tol=1e-9, max_iter=8, nested_iteration=False, cycle_type='F')),
    "heat_nx33_2lvl_k4_w13": (33, [65, 17], 4, dict(tol=1e-9, max_iter=8, weight_c=1.3)),
    "heat_nx33_k2_jump": (33, [65, 17, 5], 2, dict(tol=1e-9, max_iter=8, conv_crit=1)),
}


def at_heat(nx, nts, host_only, x_end=1.0):
    from pymgrit_amd import Heat1D
    prob = [Heat1D(x_start=0, x_end=x_end, nx=nx, a=1, init_cond=cases.init_cond,
                   rhs_separable=[(cases.rhs_space, cases.rhs_time)], t_start=0, t_stop=2, nt=nt) for nt in nts]
    if host_only:
        for p in prob:
            p.device_stepper = lambda: None
    return prob


def local_conv_ranks_problem(name):
    """local stopping criteria on several ranks (tests/test_local_conv.py): (builder of the problem, Mgrit options)"""
    from pymgrit_amd import Dahlquist, Heat1D, simple_setup_problem
    if name.startswith("dahlquist"):
        return (lambda: simple_setup_problem(Dahlquist(t_start=0, t_stop=5, nt=101), level=3, coarsening=2)), dict(tol=1e-10, conv_crit=2)
    table = {
        "heat_crit2_V": ([65, 17, 5], dict(tol=1e-7, max_iter=12, conv_crit=2)),
        "heat_crit3_V": ([65, 17, 5], dict(tol=1e-7, max_iter=12, conv_crit=3)),
        "heat_crit2_F_nonested": ([65, 17, 5], dict(tol=1e-7, max_iter=12, conv_crit=2, cycle_type='F', nested_iteration=False)),
        "heat_crit2_maxiter": ([65, 17, 5], dict(tol=1e-14, max_iter=3, conv_crit=2)),
        "heat_crit2_2lvl_cf2": ([65, 9], dict(tol=1e-7, max_iter=12, conv_crit=2, cf_iter=2)),
    }
    nts, opts = table[name]

    def make():
        prob = [Heat1D(x_start=0, x_end=1, nx=33, a=1, init_cond=cases.init_cond, rhs_separable=[(cases.rhs_space, cases.rhs_time)],
                       t_start=0, t_stop=2, nt=nt) for nt in nts]
        for p in prob:
            p.device_stepper = lambda: None
        return prob
    return make, opts
