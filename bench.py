#!/usr/bin/env python3
"""bench.py -- MGRIT V-cycle throughput of the MI355X engine on BASELINE.json's headline workload.

Workload (config.workload): BASELINE configs[2] = heat_1d nx=16384 (16382 DOF), nt=65537, 3-level m=4, FCF-relaxation,
V-cycle. It fits one MI355X (16.6 GB of slabs), so it is also the N=1 workload; with N>1 the SAME problem is sharded
over the ranks by time blocks (strong scaling) and ghost time points travel over RCCL point-to-point.

One "step" = one steady-state MGRIT V-cycle on level 0 (C-relax, F-relax, FAS residual, recursion, error correction,
F-relax) + the residual-norm convergence check -- exactly what Mgrit.solve() does per iteration after the first.
value = time-point-DOF updates per second = (Phi applications of the cycle, SURVEY 3.5 work model) x DOFs / wall time,
inputs resident in HBM.

A plain run sets up, warms up, times the steps, writes --dump-outputs and prints the headline line; nothing else. Everything
else is measured only with --full, after the headline numbers: "sweeps" lists every sweep of the cycle with its device time
(HIP events around every entry point on the engine's stream, three extra cycles in program order) and SURVEY 8d's algorithmic
bytes; "roofline" is the row with the largest share of the cycle; "cpu_baseline", "iters_to_tol" and
"parity"; "other_configs": BASELINE configs[1], [3], [4] on the same GPU, measured in child processes (full lines: --all-configs).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec


def rhs_space(x):
    return - np.sin(np.pi * x)


def rhs_time(t):
    return np.sin(t) - 1 * np.pi ** 2 * np.cos(t)


def init_cond(x):
    return np.sin(np.pi * x)


def phi_counts(nts, m_list, first_iteration=False):
    """SURVEY 3.5 work model: Phi applications per level for one V-cycle with cf_iter=1 incl. the residual check."""
    L = len(nts)
    counts = []
    for l in range(L):
        N = nts[l] - 1
        if l == L - 1:
            counts.append(N + (nts[l] - 1 if L > 1 else 0))  # forward solve + coarse half of fas_residual(L-2)
            continue
        m = m_list[l]
        F, C = N * (m - 1) // m, N // m
        if l == 0:
            counts.append((3 if first_iteration else 2) * F + 3 * C)
        else:
            counts.append(3 * F + 2 * C + (nts[l] - 1))
    return counts


def cycle_phi_counts(nts, m_list, cycle_type='V'):
    """Phi applications per level of one steady-state cycle (iteration >= 1, cf_iter = 1) + the residual check, obtained by
    walking the recursion of Mgrit.iteration (reference mgrit.py:261-290); equals phi_counts() for V-cycles."""
    L = len(nts)
    N = [n - 1 for n in nts]
    C = [N[l] // m_list[l] if l < L - 1 else N[l] for l in range(L)]
    F = [N[l] - C[l] for l in range(L)]
    counts = [0] * L

    def it(lvl, ctype, first_f):
        if lvl == L - 1:
            counts[lvl] += N[lvl]
            return
        if first_f and lvl > 0:
            counts[lvl] += F[lvl]
        counts[lvl] += C[lvl] + F[lvl]            # C-relax, F-relax
        counts[lvl] += C[lvl]                     # fas_residual: fine Phi per C-point
        counts[lvl + 1] += N[lvl + 1]             #               coarse Phi per coarse point
        it(lvl + 1, ctype, True)
        counts[lvl] += F[lvl]                     # F-relax after the correction
        if lvl != 0 and ctype == 'F':
            it(lvl, 'V', False)
    it(0, cycle_type, True)
    counts[0] += C[0]                             # residual check
    return counts


def cpu_baseline(nx, nt=16385):
    """The parity oracle ("port" of the reference's algorithm: variant 0 = plain Thomas solves) timed on this host on a bounded
    sample of the same workload: nx as given, nt = 16385 (a quarter of the time grid: 4096 F-intervals / C-points per level-0
    sweep, enough independent work for every core), 3-level m=4, steady-state V-cycles incl. the residual check. Single-threaded,
    and with the independent F-intervals / C-points of every sweep spread over OpenMP threads (the parallelism the reference's
    mpi4py path has across ranks; the coarsest-level solve stays serial there as well) for several thread counts up to all
    cores. `value` is the best of them, `cores` the threads that gave it."""
    import cases
    from oracle import oracle as orc
    nts = (nt, (nt - 1) // 4 + 1, (nt - 1) // 16 + 1)
    upd_per_cycle = sum(c * (nx - 2) for c in phi_counts(nts, [4, 4]))

    def run(threads, min_cycles, budget):
        levels = [cases.heat_level_spec(nx, cases.lin(2.0 * (nts[0] - 1) / 65536, n)) for n in nts]
        p = orc.OracleProblem(levels, variant=0, nested_iteration=False, max_iter=1, tol=0.0, norm_spec=False)
        used = p.set_threads(threads)
        p.iteration(0, 'V', 0, True)  # warm-up cycle (first iteration does one more F-relax)
        t0, cycles = time.perf_counter(), 0
        while True:
            p.iteration(0, 'V', 1, True)
            p.residual_norms()
            cycles += 1
            el = time.perf_counter() - t0
            if (cycles >= min_cycles and el > budget) or cycles >= 64:
                break
        return upd_per_cycle * cycles / el, used, cycles, el
    v1, _, c1, e1 = run(1, 1, 0.0)
    # the cores this process may really use: the affinity mask cut down to the cgroup's CPU quota (a one-GPU box of the pool shows
    # 256 logical CPUs and grants 16: threads beyond the quota are throttled, not run -- round 4's `by_threads` fell from 1.3e9 at 32
    # threads to 2.8e8 at 256 for that reason, and its "256 cores" was never the box's share)
    avail = cases.usable_cpus()
    tried = {}
    for threads in sorted({min(avail, t) for t in (4, 8, 16, 32, 64, 128, avail)}):
        if threads > 1:
            tried[threads] = run(threads, 2, 1.5)
    best = max(tried, key=lambda t: tried[t][0]) if tried else 1
    vn, used, cn, en = tried[best] if tried else (v1, 1, c1, e1)
    if v1 > vn:
        vn, used, cn, en = v1, 1, c1, e1
    # calibration of the port against the reference itself: BASELINE.md section 2 holds the unmodified reference's
    # numbers on config 2 (heat_1d nx=1024 nt=4097, 3-level m=4; one Python process on the 8-core build container, no GPU); the port
    # runs the same configuration here, single-threaded, steady-state V-cycles incl. the residual check
    nts2 = (4097, 1025, 257)
    lv2 = [cases.heat_level_spec(1024, cases.lin(2.0, n)) for n in nts2]
    p2 = orc.OracleProblem(lv2, variant=0, nested_iteration=False, max_iter=1, tol=0.0, norm_spec=False)
    p2.iteration(0, 'V', 0, True)
    t2, c2 = time.perf_counter(), 0
    while c2 < 3 or time.perf_counter() - t2 < 1.0:
        p2.iteration(0, 'V', 1, True)
        p2.residual_norms()
        c2 += 1
    e2 = time.perf_counter() - t2
    port2 = sum(c * 1022 for c in phi_counts(nts2, [4, 4])) * c2 / e2
    reference = {"config": "BASELINE configs[1]: heat_1d nx=1024 (1022 DOF) nt=4097, 3-level m=4, V-cycle FCF", "updates_per_s": 2.61e6,
                 "s_per_v_cycle": 4.97, "s_per_residual_check": 0.55, "processes": 1,
                 "provenance": "BASELINE.md section 2: the unmodified reference (PyMGRIT v1.0.6, scipy SuperLU per step) measured in the "
                               "8-core build container during the survey; it cannot travel to the GPU box",
                 "port_same_config_updates_per_s_1core": port2, "port_over_reference": port2 / 2.61e6,
                 "port_sample": f"{c2} V-cycles incl. residual check in {e2:.2f} s on 1 core of this host"}
    return {"value": vn, "unit": "time-point-DOF updates/s", "cores": used, "kind": "port", "value_1core": v1,
            "reference_python": reference,
            # the same calibration as plain scalars (a consumer that keeps only the scalar fields of this object still sees it)
            "reference_python_updates_per_s": reference["updates_per_s"], "reference_python_config": reference["config"],
            "port_over_reference_python": reference["port_over_reference"],
            "host_cores": os.cpu_count(), "host_cores_usable": avail, "by_threads": {str(t): r[0] for t, r in tried.items()},
            "sample": f"port = parity oracle variant 0 (Thomas solves, reference operation order), {used} of the {avail} CPUs this "
                      f"process may use (cgroup quota / affinity; the host shows {os.cpu_count()}): heat_1d nx={nx} nt={nts[0]} 3-level m=4 ({(nts[0] - 1) // 4} F-intervals per level-0 sweep), "
                      f"V-cycles incl. residual check: {c1} cycle(s) in {e1:.1f} s on 1 core, {cn} cycles in {en:.1f} s on "
                      f"{used} OpenMP threads (tried {sorted(tried)}; {avail} usable cores)"}


def iters_to_tol(problem, nx, tol=1e-10):
    """Second half of BASELINE.json's metric ("iters-to-tol vs CPU ref"): Mgrit.solve() to the reference's default tolerance
    on the full workload (GPU; tolerance tightened from the reference default 1e-7, which this workload meets after two cycles), and on the bounded sample of cpu_baseline() on both the GPU and the CPU oracle (same
    arithmetic spec), whose residual histories must agree. Outside every timed region; part of the cpu_baseline leg."""
    import cases
    from oracle import oracle as orc
    from pymgrit_amd import Heat1D, Mgrit
    from pymgrit_amd.core.options import options
    import torch
    runs = []
    for _ in range(2):   # the first constructor of a process also pays for fresh hipMalloc of the slabs (the timed Mgrit above is
        torch.cuda.synchronize()   # still alive); the second finds them in the allocator's cache, as a long-lived service would
        t0 = time.perf_counter()
        mg = Mgrit(problem, cf_iter=1, cycle_type='V', nested_iteration=True, max_iter=30, tol=tol, logging_lvl=30)
        res = mg.solve()
        torch.cuda.synchronize()
        runs.append((1e3 * res["time_setup"], 1e3 * res["time_solve"], 1e3 * (time.perf_counter() - t0)))
        if len(runs) < 2:
            del mg
            import gc
            gc.collect()      # (the solver object holds reference cycles: only now do its slabs go back to the allocator's cache)
    tts = {"note": f"Mgrit(...).solve() of the full workload to {tol:g} on this GPU: setup = constructor incl. tables, slabs and the "
                   f"nested iteration, solve = the iterations incl. every stopping test and the final F-relaxation that puts all "
                   f"F-points in place; second of two runs (slabs from the allocator's cache), the first is setup_ms_cold",
           "setup_ms": runs[1][0], "solve_ms": runs[1][1], "wall_ms": runs[1][2], "setup_ms_cold": runs[0][0],
           "solve_ms_cold": runs[0][1], "iterations": int(len(res["conv"]))}
    conv_full = res["conv"]
    del mg
    nts = (1025, 257, 65)
    grids = [cases.lin(2.0 * (nts[0] - 1) / 65536, nt) for nt in nts]
    small = [Heat1D(x_start=0, x_end=1, nx=nx, a=1, init_cond=init_cond, rhs_separable=[(rhs_space, rhs_time)], t_interval=g)
             for g in grids]
    conv_gpu = Mgrit(small, cf_iter=1, cycle_type='V', nested_iteration=True, max_iter=30, tol=tol, logging_lvl=30).solve()["conv"]
    conv_cpu = orc.OracleProblem([cases.heat_level_spec(nx, g) for g in grids], variant=1, cf_iter=1, nested_iteration=True,
                                 max_iter=30, tol=tol).solve()
    k = min(len(conv_gpu), len(conv_cpu))
    parity = coarse_solve_parity(problem, iters=5, cf_iter=1, cycle_type='V', nested_iteration=True)
    return {"tol": tol, "time_to_solution_ms": tts, "parity": parity,
            "full_workload": {"gpu_iters": int(len(conv_full)), "conv_last": float(conv_full[-1])},
            "sample_nt1025": {"gpu_iters": int(len(conv_gpu)), "cpu_iters": int(len(conv_cpu)),
                              "max_rel_conv_diff": float(np.max(np.abs(conv_gpu[:k] - conv_cpu[:k]) / np.abs(conv_cpu[:k])))}}


def spacetime_norm_gpu(be):
    """2-norm of the level-0 solution over space and time, on the device (padding positions of the rows left out)"""
    U, perm = be.U[0], be.perm[0]
    import torch
    acc = torch.zeros((), dtype=torch.float64, device=U.device)
    for a in range(0, U.shape[0], 4096):
        blk = U[a:a + 4096][:, perm]
        acc += (blk * blk).sum()
    return float(acc.sqrt().item())


def coarse_solve_parity(problem, iters=5, **kw):
    """Which form of forward_solve the coarsest level takes by default, and what that costs in parity. The reference steps through
    the coarsest level point by point (mgrit.py:459-486); the default here is the time-parallel block form wherever the level
    qualifies -- the same solve in another association. Both forms are run on this GPU from the same start for
    `iters` iterations (tol = 0); reported per iteration k: conv of both, the relative deviation, the absolute one, and the absolute
    one in units of eps * ||u|| (2-norm of the solution over space and time: the rounding level of a residual). The bar
    (tests/cases.py BLK_K_FORM; tests/test_oracle_golden.py pins both forms to the reference's histories): 1e-10 * conv + 2 eps ||u||."""
    import gc
    from pymgrit_amd import Mgrit
    from pymgrit_amd.core.options import options
    conv, norm_u, form = {}, None, None
    for which in ("auto", "sequential"):
        try:
            options.coarse_solve = which
            mg = Mgrit(problem, max_iter=iters, tol=0.0, logging_lvl=30, **kw)
        finally:
            options.reset("coarse_solve")
        conv[which] = np.asarray(mg.solve()["conv"], dtype=np.float64)
        if which == "auto":
            norm_u = spacetime_norm_gpu(mg.backend)
            r = getattr(mg.backend, "block_r", {}).get(mg.lvl_max - 1, 0)
            form = f"time-parallel blocks of 16 steps ({r} modes)" if r else "sequential (the level does not qualify)"
        del mg
        gc.collect()
    a, b = conv["auto"], conv["sequential"]
    k = min(len(a), len(b))
    eps = float(np.finfo(np.float64).eps)
    dev = np.abs(a[:k] - b[:k])
    bound = 1e-10 * b[:k] + 2.0 * eps * norm_u
    return {"coarse_solve": form, "conv": a.tolist(), "conv_sequential": b.tolist(),
            "rel_dev_vs_sequential": (dev / b[:k]).tolist(), "abs_dev": dev.tolist(),
            "abs_dev_in_eps_norm_u": (dev / (eps * norm_u)).tolist(), "norm_u_spacetime": norm_u,
            "bound": "1e-10 * conv + 2 * eps * ||u||_spacetime", "within_bound": bool(len(a) == len(b) and np.all(dev <= bound))}


DUMP_ROW_BYTES = 48 * 2 ** 20     # --dump-outputs: level-0 rows of the sample; with the small arrays the dump stays under 64 MB


def dump_outputs(mg, out_dir):
    """--dump-outputs DIR: what the last timed step computed, as a caller of Mgrit.iteration + convergence_criterion reads it, one
    float64 .npy file per array: conv (the stopping value of the step), residual_norms (the per-C-point norms it reduces),
    u_level0_sample (the level-0 solution in natural order at a fixed sample of time points: all of them where they fit, else the
    first, the last and a seeded draw of the others, sorted) and u_level0_sample_index (those time points). The same arguments
    give the same sample, so two builds can be compared array for array. Outside every timed region."""
    os.makedirs(out_dir, exist_ok=True)
    u = mg.u[0]
    n_pts = len(u)
    first = np.asarray(u[0].get_values(), dtype=np.float64).ravel()
    rows = max(1, min(n_pts, DUMP_ROW_BYTES // (8 * first.size)))
    if rows >= n_pts:
        idx = np.arange(n_pts)
    else:
        draw = np.random.default_rng(0).choice(np.arange(1, n_pts - 1), size=rows - 2, replace=False)
        idx = np.sort(np.concatenate(([0, n_pts - 1], draw)))
    sample = np.stack([first if i == 0 else np.asarray(u[int(i)].get_values(), dtype=np.float64).ravel() for i in idx])
    arrays = {"conv": np.array([mg.conv[1]], dtype=np.float64),
              "residual_norms": np.asarray(mg.compute_residual(), dtype=np.float64).ravel(),
              "u_level0_sample": sample, "u_level0_sample_index": idx.astype(np.float64)}
    for name, arr in arrays.items():
        np.save(os.path.join(out_dir, f"{name}.npy"), arr)


FP64_MFMA_PEAK_TFLOPS = 78.6  # AMD MI355X datasheet, FP64 matrix (the on-box guide lists no f64 MFMA row)


def bench_heat2d(args):
    """Secondary workload (not the driver's default): BASELINE configs[3] = heat_2d nx=ny=512, nt=16385, 2-level m=8.
    Reports the V-cycle throughput and the MFMA roofline of the level-0 F-relax sweep (per Phi: four half-size sine
    transforms = 4*512*512*512 flops at 512^2 on v_mfma_f64_16x16x4_f64 -- the even/odd split halves the 8*512^3 of four
    full products --, plus the O(n^2) rhs / epilogue kernels inside the timed launch)."""
    import torch
    from pymgrit_amd import Heat2D, Mgrit
    torch.cuda.set_device(0)
    nx, nt0 = args.nx2d, args.nt2d
    t0 = np.linspace(0, 1, nt0)
    prob = [Heat2D(x_start=0, x_end=1, y_start=0, y_end=1, nx=nx, ny=nx, a=1.0, method="BE",
                   init_cond=lambda x, y: np.sin(np.pi * x) * np.sin(np.pi * y), t_interval=t) for t in (t0, t0[::8])]
    mg = Mgrit(prob, cf_iter=1, nested_iteration=False, max_iter=1, tol=0.0, logging_lvl=30, plan_blocks=args.plan_blocks)
    be = mg.backend
    dof = nx * nx
    counts = phi_counts([nt0, (nt0 - 1) // 8 + 1], [8])

    def cycle(it):
        mg.iteration(lvl=0, cycle_type='V', iteration=it, first_f=True)
        mg.convergence_criterion(iteration=1)
    cycle(0)
    for _ in range(args.warmup):
        cycle(1)
    torch.cuda.synchronize()
    t_start = time.perf_counter()
    for _ in range(args.steps):
        cycle(1)
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t_start
    if args.dump_outputs:
        dump_outputs(mg, args.dump_outputs)
    out = {"metric": "time-point-DOF updates/sec per MGRIT V-cycle", "value": sum(c * dof for c in counts) * args.steps / elapsed,
           "unit": "time-point-DOF updates/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
           "ms_per_step": 1e3 * elapsed / args.steps, "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
           "dtype": "f64", "data": "synthetic",
           "config": {"workload": f"heat_2d nx=ny={nx} nt={nt0} 2-level m=8 FCF V-cycle + residual check (BASELINE configs[3])",
                      "phi_per_cycle_by_level": counts, "dof": dof}}
    if not args.full:
        print(json.dumps(out), flush=True)
        return
    f_runs = mg._f_runs(0)
    n_f = sum(r[1] for r in f_runs)
    be.set_timing(True)
    ms = []
    for _ in range(3):
        be.relax(0, f_runs, 'F')
        ms.append(be.last_kernel_ms())
    be.set_timing(False)
    f_ms = float(np.mean(ms[1:]))
    HP = (((nx - 2 + 1) // 2 + 63) // 64) * 64      # padded half size of an axis; P = 2 HP slots
    flops_per_phi = 4.0 * (2 * HP) * (2 * HP) * (HP + HP)   # four half-size transforms: 2 MACs x P x P x HP each way per axis
    tflops = n_f * flops_per_phi / (f_ms * 1e-3) / 1e12
    out["roofline"] = {"bound": "mfma", "achieved": tflops, "peak": FP64_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                       "frac": tflops / FP64_MFMA_PEAK_TFLOPS, "traffic": None,
                       "kernel": "level-0 F-relax = per Phi 2 x h2d_fwd_kernel (the first reads the state rows: no rhs launch for the "
                                 "homogeneous step) + 2 x h2d_inv_kernel (f64 MFMA, half-size transforms; the sweep's arithmetic in the last one) + rim",
                       "flops_per_phi": flops_per_phi,
                       "launch_ms": f_ms, "us_per_phi": 1e3 * f_ms / n_f}
    out["sweeps"] = timed_sweeps(mg, be, cycle, cycles=1)
    out["cycle"] = {"sum_of_sweep_ms_in_program_order": sum(r["ms_per_cycle"] for r in out["sweeps"].values())}
    # the roofline row = the launch kind with the largest share of the cycle's device time, priced with the Phi it applies
    N0, N1 = nt0 - 1, (nt0 - 1) // 8
    phi_per_launch = {"relax_f L0": n_f, "relax_c L0": N1, "residual L0": N1, "fas_rhs L0": 2 * N1, "chain L1": N1}
    for key, row in out["sweeps"].items():
        if key in phi_per_launch:
            row["phi_per_launch"] = phi_per_launch[key]
            row["tflops"] = phi_per_launch[key] * flops_per_phi / (row["ms_per_launch"] * 1e-3) / 1e12
            row["mfma_frac"] = row["tflops"] / FP64_MFMA_PEAK_TFLOPS
    dominant = max(out["sweeps"], key=lambda k: out["sweeps"][k]["ms_per_cycle"])
    drow = out["sweeps"][dominant]
    out["roofline_level0_f_relax"] = out["roofline"]
    out["roofline"] = {"bound": "mfma", "achieved": drow.get("tflops"), "peak": FP64_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                       "frac": drow.get("mfma_frac"), "traffic": None, "kernel": f"{dominant}: per Phi 2 x h2d_fwd_kernel + 2 x "
                       "h2d_inv_kernel (f64 MFMA, half-size transforms; no rhs launch for the homogeneous step) + rim", "flops_per_phi": flops_per_phi,
                       "mfma_sustained_frac_of_peak": 0.89,   # tools/micro/mfma_f64_peak.hip, LDS operands (profiles/r05_mfma_f64_peak.txt)
                       "launch_ms": drow["ms_per_launch"], "launches_per_cycle": drow["launches_per_cycle"], "ms_per_cycle": drow["ms_per_cycle"],
                       "limited_by": "MFMA issue + operand traffic of the batched half-size transforms" if not dominant.startswith("chain") else
                       "latency: the sequential coarsest-level solve, one state per step (64 output tiles for 256 CUs)"}
    print(json.dumps(out), flush=True)


def bench_advection(args):
    """Secondary workload (not the driver's default): BASELINE configs[4] = advection_1d nx=8193 (8192 periodic DOF),
    nt=32769, F-cycle, 4 levels m=2, spatial coarsening (periodic full weighting / linear interpolation) on the first two
    level pairs and the copy transfer on the last (mirrors examples/example_spatial_coarsening.py:112-123). Reports the
    F-cycle throughput and the HBM roofline of the level-0 F-relax launch (16*n bytes per Phi)."""
    import torch
    from pymgrit_amd import Advection1D, GridTransferAdvection, GridTransferCopy, Mgrit
    torch.cuda.set_device(0)
    nt0 = args.nt_adv
    t0 = np.linspace(0, 2, nt0)
    nx0 = args.nx_adv          # (default 8193; e.g. 8001: periodic grids that are not powers of two, coarsest-level transforms as ordered sums)
    nxs = [nx0, (nx0 - 1) // 2 + 1, (nx0 - 1) // 4 + 1, (nx0 - 1) // 4 + 1]
    prob = [Advection1D(c=1, x_start=-1, x_end=1, nx=nx, t_interval=t0[::2 ** lvl]) for lvl, nx in enumerate(nxs)]
    transfer = [GridTransferAdvection(), GridTransferAdvection(), GridTransferCopy()]
    mg = Mgrit(prob, transfer=transfer, cf_iter=1, cycle_type='F', nested_iteration=False, max_iter=1, tol=0.0, logging_lvl=30,
               plan_blocks=args.plan_blocks)
    be = mg.backend

    def cycle(it):
        mg.iteration(lvl=0, cycle_type='F', iteration=it, first_f=True)
        mg.convergence_criterion(iteration=1)
    cycle(0)
    for _ in range(args.warmup):
        cycle(1)
    torch.cuda.synchronize()
    t_start = time.perf_counter()
    for _ in range(args.steps):
        cycle(1)
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t_start
    if args.dump_outputs:
        dump_outputs(mg, args.dump_outputs)
    out = {"metric": "time-point-DOF updates/sec per MGRIT F-cycle", "value": None, "unit": "time-point-DOF updates/s",
           "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1e3 * elapsed / args.steps,
           "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
           "config": {"workload": f"advection_1d nx={nxs[0]} nt={nt0} 4-level m=2 F-cycle, spatial coarsening on the first two "
                                  f"level pairs + residual check (BASELINE configs[4])", "dof_by_level": [n - 1 for n in nxs]}}
    counts = cycle_phi_counts([len(p.t) for p in prob], [2, 2, 2], 'F')
    out["config"]["phi_per_cycle_by_level"] = counts
    out["value"] = sum(c * d for c, d in zip(counts, out["config"]["dof_by_level"])) * args.steps / elapsed
    if not args.full:
        print(json.dumps(out), flush=True)
        return
    f_runs = mg._f_runs(0)
    n_f = sum(r[1] for r in f_runs)
    be.set_timing(True)
    ms = []
    for _ in range(4):
        be.relax(0, f_runs, 'F')
        ms.append(be.last_kernel_ms())
    be.set_timing(False)
    f_ms = float(np.mean(ms[1:]))
    dof = nxs[0] - 1
    achieved = n_f * 16.0 * dof / (f_ms * 1e-3) / 1e9
    out["roofline"] = {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
                       "traffic": None, "kernel": "relax_kernel<ADVECTION1D,false,ROLE_F> (level-0 F-relax)", "launch_ms": f_ms,
                       "algorithmic_bytes_per_launch": n_f * 16.0 * dof}
    out["sweeps"] = timed_sweeps(mg, be, cycle)
    out["cycle"] = {"sum_of_sweep_ms_in_program_order": sum(r["ms_per_cycle"] for r in out["sweeps"].values())}
    # SURVEY 8d algorithmic bytes per launch of every sweep kind (Phi = 16 n B on level 0, 24 n B on coarser levels; residual
    # 16 n per C-point; fas_residual per C-point (16|24) n_l + 32 n_{l+1}; error_correction per C-point 16 n_l + 16 n_{l+1}),
    # and the roofline row = the launch kind with the largest share of the cycle's device time
    dofs, Ns = out["config"]["dof_by_level"], [len(p.t) - 1 for p in prob]
    for key, row in out["sweeps"].items():
        kind, lv = key.split()[0], int(key.split()[1][1:])
        n, N = dofs[lv], Ns[lv]
        F, C = (N - N // 2, N // 2) if lv < len(prob) - 1 else (0, N)
        phi = 16.0 if lv == 0 else 24.0
        nc = dofs[lv + 1] if lv + 1 < len(dofs) else n
        alg = {"relax_f": F * phi * n, "relax_c": C * phi * n, "chain": N * 24.0 * n, "residual": C * 16.0 * n,
               "fas_rhs": C * (phi * n + 32.0 * nc), "fas_fused": C * (phi * n + 32.0 * nc), "ec_relax": C * 32.0 * n + F * phi * n,
               "error_correction": C * (16.0 * n + 16.0 * nc), "restrict": C * (8.0 * n + 8.0 * nc), "copy": None,
               # the whole-level passes are priced by the rows ONE pass over the level has to move, not by the
               # sum of the reference's sweeps they replace (that sum exceeds what any fused pass moves and would read as more
               # than the peak). Way down, per coarse interval: the C-point row read [+ g rows of the interval], the relaxed
               # C-point written, u, v, g of the coarse level written, then fas_coarse: v and g read, g written. Way up: the fine
               # C-point and the two coarse rows read [+ g], the m rows of the interval written
               "gen_down": C * ((16.0 + (16.0 if lv else 0.0)) * n + 48.0 * nc),
               "gen_up": C * ((8.0 + (16.0 if lv else 0.0)) * n + 16.0 * nc + 16.0 * n)}.get(kind)
        if kind == "copy":
            alg = (Ns[lv + 1] + 1 if lv + 1 < len(Ns) else N) * 16.0 * nc
        row["algorithmic_bytes_per_launch"] = alg
        row["algorithmic_GBps"] = alg / (row["ms_per_launch"] * 1e-3) / 1e9 if alg else None
    # physical HBM bytes of the kernels that run, from the committed PMC passes of this workload (tools/profile_round.sh ->
    # profiles/<tag>_traffic_advection.json, keys kernel@workgroup size: 512 threads = level 0, 256 = level 1, 128 = levels 2, 3)
    K, src, stale = pmc_traffic(16384, 65537, 1, name="traffic_advection") if nt0 == 32769 else ({}, None, False)
    if stale:
        out["cycle"]["physical_bytes_source"] = src
    if K:
        per = lambda name: K.get(name, {}).get("hbm_bytes_per_launch")
        cyc = K.get("gen_down_kernel<2, 0, false>@512", {}).get("launches_fetch_pass")     # once per cycle
        if cyc:
            extra = ("relax_kernel<2, 0, false, 0>@512",)      # the four stand-alone level-0 F-relaxations of the figure above
            total = sum(v["hbm_bytes_per_launch"] * v["launches_fetch_pass"] for k, v in K.items() if k not in extra and "rocclr" not in k) / cyc
            out["cycle"].update({"physical_bytes": total, "physical_GBps": total / (out["ms_per_step"] * 1e-3) / 1e9,
                                 "physical_frac": total / (out["ms_per_step"] * 1e-3) / 1e9 / HBM_PEAK_GBS,
                                 "physical_bytes_source": src})
        wg = [512, 256, 128, 128]
        for key, row in out["sweeps"].items():
            kind, lv = key.split()[0], int(key.split()[1][1:])
            g = "true" if lv > 0 else "false"
            names = {"gen_down": [f"gen_down_kernel<2, 0, {g}>@{wg[lv]}"] + ([f"fas_coarse_kernel<2, 0>@{wg[lv + 1]}"] if lv + 1 < 4 else []),
                     "gen_up": [f"gen_up_kernel<2, 0, {g}, {'true' if lv == 0 else 'false'}>@{wg[lv]}"],
                     "relax_f": [f"relax_kernel<2, 0, {g}, 0>@{wg[lv]}"],
                     # the time-parallel coarsest-level solve: local pass, two FFT launches, scan, finish
                     "chain": ["blk_local_kernel<2, 0>@128", "adv_fft_rows_kernel@1024", "adv_fft_rows_kernel@1024", "adv_scan_kernel@256",
                               "blk_finish_kernel<2, 0>@128"]}.get(kind, [])
            got = [per(nm) for nm in names]
            if got and all(b is not None for b in got):
                # (fas_coarse_kernel@128 serves the level pairs 1 -> 2 and 2 -> 3 alike: its per-launch average is exact for neither)
                row["kernels"] = names
                row["physical_bytes_per_launch"] = sum(got)
                row["physical_GBps"] = sum(got) / (row["ms_per_launch"] * 1e-3) / 1e9
                row["physical_frac"] = row["physical_GBps"] / HBM_PEAK_GBS
    dominant = max(out["sweeps"], key=lambda k: out["sweeps"][k]["ms_per_cycle"])
    drow = out["sweeps"][dominant]
    out["roofline_level0_f_relax"] = out["roofline"]
    out["roofline"] = {"bound": "hbm", "achieved": drow["algorithmic_GBps"], "peak": HBM_PEAK_GBS, "unit": "GB/s",
                       "frac": drow["algorithmic_GBps"] / HBM_PEAK_GBS if drow["algorithmic_GBps"] else None,
                       "traffic": drow.get("physical_bytes_per_launch"),
                       "kernel": f"{dominant} ({'blk_local_kernel / adv_fft_rows_kernel / adv_scan_kernel / blk_finish_kernel' if dominant.startswith('chain') else 'gen_down_kernel / gen_up_kernel<2, 0, ...> and fas_coarse_kernel<2, 0>'})",
                       "launch_ms": drow["ms_per_launch"], "launches_per_cycle": drow["launches_per_cycle"], "ms_per_cycle": drow["ms_per_cycle"],
                       "algorithmic_bytes_per_launch": drow["algorithmic_bytes_per_launch"],
                       "limited_by": "launch latency of the five small kernels of the time-parallel coarsest-level solve" if dominant.startswith("chain") else "HBM bandwidth"}
    print(json.dumps(out), flush=True)


KERNEL_OF = {"relax_f": "relax_kernel<1, 1, {g}, 0>", "relax_c": "relax_kernel<1, 1, {g}, 1>", "fas_fused": "fas_fused1_kernel<4, false>",
             "ec_relax": "ecf_kernel<1, 1, {g}>", "residual": "residual_kernel<1, 1>", "chain": "chain2_kernel<1, true>",
             "cf_fas": "cfas_kernel<2>", "ec_relax_res": "ecfr_kernel<4, false, true>", "relax_fc": "relax_kernel<1, 1, true, 3>",
             "f_fas": "fas_fused1_kernel<4, true>"}
LIMITED_BY = {"chain": "latency: the coarsest-level solve is sequential, one cross-workgroup exchange per step (measured floor "
                       "0.98 us/step = one store -> L2 -> load round trip); bytes are not what bounds it",
              "chain_blocks": "the time-parallel forward solve (DESIGN.md 3.8): two batched passes over all blocks of 16 steps (HBM "
                              "bandwidth where the level is large: config 3) around a modal recurrence over the blocks; on small "
                              "levels (config 2: one launch, blk_one_kernel) the latency of 2 x 16 Phi of a single wave",
              "default": "HBM bandwidth (one 1024-thread workgroup per CU streaming rows; 6.29 TB/s copy ceiling of the guide)"}


def sweep_bytes(nts, m_list, dof):
    """SURVEY 8d algorithmic bytes per steady-state V-cycle + residual check, by (sweep, level): Phi = 16*n B on level 0, 24*n
    on coarser levels; fas_residual per C-point (16|24)*n + 24*n + 8*n; error_correction per C-point 32*n; residual 16*n."""
    L = len(nts)
    out = {}
    for lvl in range(L - 1):
        N, m = nts[lvl] - 1, m_list[lvl]
        F, C = N * (m - 1) // m, N // m
        phi = 16.0 if lvl == 0 else 24.0
        out[f"relax_c L{lvl}"] = C * phi * dof
        out[f"relax_f L{lvl}"] = (1 if lvl == 0 else 2) * F * phi * dof
        out[f"fas_fused L{lvl}"] = C * (phi + 32.0) * dof
        out[f"ec_relax L{lvl}"] = (C * 32.0 + F * phi) * dof
        # whole-level passes (level 0): the sweeps they replace, with those sweeps' algorithmic bytes
        out[f"cf_fas L{lvl}"] = out[f"relax_c L{lvl}"] + F * phi * dof + out[f"fas_fused L{lvl}"]
        # coarser levels' way down in two passes: F-relaxation + C-relaxation, F-relaxation + FAS sweep
        out[f"relax_fc L{lvl}"] = F * phi * dof + out[f"relax_c L{lvl}"]
        out[f"f_fas L{lvl}"] = F * phi * dof + out[f"fas_fused L{lvl}"]
        out[f"ec_relax_res L{lvl}"] = out[f"ec_relax L{lvl}"] + C * 16.0 * dof
    out["residual L0"] = ((nts[0] - 1) // m_list[0]) * 16.0 * dof
    out[f"chain L{L - 1}"] = (nts[-1] - 1) * 24.0 * dof
    return out


def timed_sweeps(mg, be, cycle, cycles=2):
    """per (sweep, level): launches and device milliseconds per cycle in program order (HIP events around every entry point,
    mgrit_hip_set_timing); no byte model -- the secondary workloads' tables"""
    keep = mg._plan_request
    mg._plan_request = 1
    try:
        cycle(1)
        be.sync()
        be.set_timing(True)
        be.timing_drain()
        for _ in range(cycles):
            cycle(1)
        recs = be.timing_drain(max_records=65536)
        be.set_timing(False)
    finally:
        mg._plan_request = keep
    agg = {}
    for kind, lvl, ms in recs:
        a = agg.setdefault(f"{kind} L{lvl}", [0, 0.0])
        a[0] += 1
        a[1] += ms
    return {key: {"launches_per_cycle": n / cycles, "ms_per_launch": tot / n, "ms_per_cycle": tot / cycles}
            for key, (n, tot) in sorted(agg.items(), key=lambda kv: -kv[1][1])}


def build_stamp():
    """what the kernels were built from: sha256 over csrc/*.hip, csrc/*.inc and include/*.h (sorted by name), and of the library
    itself. profiles/<tag>_traffic.json carries the stamp of the build its counters were collected on (tools/summarize_profiles.py,
    run on the GPU box by tools/profile_round.sh)."""
    import glob
    import hashlib
    h = hashlib.sha256()
    for f in sorted(glob.glob(os.path.join(ROOT, "pymgrit_amd", "csrc", "*.hip")) + glob.glob(os.path.join(ROOT, "pymgrit_amd", "csrc", "*.inc")) +
                    glob.glob(os.path.join(ROOT, "include", "*.h"))):
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    lib = os.path.join(ROOT, "pymgrit_amd", "lib", "libmgrit_hip.so")
    return {"source_sha256": h.hexdigest(), "lib_sha256": hashlib.sha256(open(lib, "rb").read()).hexdigest() if os.path.exists(lib) else None}


def pmc_traffic(nx, nt0, world, name="traffic"):
    """per-kernel HBM bytes per launch from the committed rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this workload
    (tools/profile_round.sh -> profiles/<tag>_<name>.json; program order, full-width launches): (kernels, source, stale). The file
    must carry the stamp of THIS build (build_stamp): counters collected on other kernels price nothing -- ({}, reason, True)."""
    if not (world == 1 and nx == 16384 and nt0 == 65537):
        return {}, None, False
    import glob
    import re
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", f"r[0-9][0-9]_{name}.json")), reverse=True)     # newest round first
    want = build_stamp()["source_sha256"]
    stale = None
    for tfile in files:
        tag = re.match(r"(r\d\d)_", os.path.basename(tfile)).group(1)
        rec = json.load(open(tfile))
        have = (rec.get("build") or {}).get("source_sha256")
        if have != want:
            stale = stale or (f"profiles/{tag}_{name}.json was collected on another build (sources {str(have)[:12]} there, {want[:12]} here): "
                              f"not used")
            continue
        return rec["kernels"], (f"profiles/{tag}_{name}.json (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, separate passes, KiB units, read "
                                f"side doubled per the guide's gfx950 note; collected on this build, sources {want[:12]}; not "
                                f"collected in this run)"), False
    if stale:
        return {}, stale, True
    return {}, None, False


def sweep_table(mg, be, nts, m_list, dof, cycle, cycles=3):
    from pymgrit_amd.core import hip_lib
    keep = mg._plan_request
    mg._plan_request = 1          # program order: one full-width launch per sweep and level
    try:
        cycle(1)
        be.sync()
        be.set_timing(True)
        be.timing_drain()
        for _ in range(cycles):
            cycle(1)
        recs = be.timing_drain()
        be.set_timing(False)
    finally:
        mg._plan_request = keep
    agg = {}
    for kind, lvl, ms in recs:
        a = agg.setdefault(f"{kind} L{lvl}", [0, 0.0])
        a[0] += 1
        a[1] += ms
    alg = sweep_bytes(nts, m_list, dof)
    table = {}
    for key, (n, tot) in sorted(agg.items(), key=lambda kv: -kv[1][1]):
        kind = key.split()[0]
        sym = KERNEL_OF.get(kind, kind).format(g="true" if not key.endswith("L0") else "false")
        why = kind
        if kind == "chain" and getattr(be, "block_r", {}).get(len(nts) - 1):
            sym = "blk_local_kernel + blk_scan_kernel + blk_finish_kernel"     # the time-parallel forward solve
            why = "chain_blocks"
            if getattr(be, "block_solve_form", lambda lvl: 1)(len(nts) - 1) == 2:
                sym = "blk_one_kernel"       # small levels: the whole solve in one launch
        elif kind == "chain" and dof <= 1024:
            sym = "chain_kernel<1, 1, true, true>"    # one group of values: the single-workgroup chain, no exchange
        if dof <= 1024 and kind in ("cf_fas", "ec_relax_res", "relax_fc", "f_fas", "fas_fused") or (dof <= 1024 and kind == "ec_relax" and not key.endswith("L0")):
            sym = sym[:-1] + ", 64>"                  # levels of one group of values: the instances compiled for one wave per workgroup
        table[key] = {"kernel_symbol": sym, "launches_per_cycle": n / cycles, "ms_per_launch": tot / n, "ms_per_cycle": tot / cycles,
                      "algorithmic_bytes_per_cycle": alg.get(key, 0.0),
                      "limited_by": LIMITED_BY.get(why, LIMITED_BY["default"])}
    return table


OTHER_CONFIGS = (["--nx", "1024", "--nt", "4097", "--steps", "200", "--warmup", "20", "--no-cpu-baseline"],
                 ["--workload", "heat2d", "--steps", "3", "--warmup", "1"],
                 ["--workload", "advection", "--steps", "10", "--warmup", "3"])


def other_configs(timeout=150):
    """BASELINE configs[1], [3], [4] on this GPU, one child process each (--full: the roofline row is among its figures):
    workload, ms per cycle, updates/s, the roofline row"""
    import subprocess
    rows = []
    for extra in OTHER_CONFIGS:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__)] + extra + ["--full"], capture_output=True, text=True,
                               timeout=timeout)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
            b = json.loads(line)
            rf = b.get("roofline", {})
            rows.append({"workload": b["config"]["workload"], "ms_per_step": b["ms_per_step"], "value": b["value"], "unit": b["unit"],
                         "steps": b["steps"], "warmup": b["warmup"],
                         "roofline": {k: rf.get(k) for k in ("bound", "achieved", "peak", "unit", "frac", "kernel", "launch_ms",
                                                             "launches_per_cycle", "ms_per_cycle", "limited_by")}})
        except Exception as exc:   # noqa: BLE001 - secondary numbers: report, never fail the headline
            rows.append({"workload": " ".join(extra), "error": repr(exc)[:300]})
    return rows


def bench_emulated(args):
    """`--emulate-rank r/P` (r a rank number or `all`): the time-sharded run of BASELINE configs[2] on P ranks, rehearsed on ONE GPU.
    All P ranks are built in this process (threads sharing the GPU and its stream, pymgrit_amd.core.comm.LoopbackWorld); every
    exchange point is the stream operation of the engine it is on an RCCL link (mgrit_hip_exchange), with a mailbox in device
    memory in the place of ncclSend / ncclRecv. After warm-up cycles of ALL ranks together (true ghost rows), rank r replays its
    cycle alone against what its neighbours sent last (frozen mailboxes: receives complete at once, sends go nowhere): device
    time per cycle of that shard and the host time to enqueue it -- what a rank of the real job costs when it never waits for
    a neighbour. A step = one V-cycle + its residual values kept for the (lagged) stopping test + the C-point snapshot of
    the pipelined solve loop (Mgrit._pl_advance), i.e. everything a rank does per iteration but the collectives.
    `all`: also the P ranks together on the one GPU (lockstep, true data): the whole job's work per cycle on one device."""
    import threading
    import torch
    from pymgrit_amd import Heat1D, Mgrit
    from pymgrit_amd.core.options import options
    from pymgrit_amd.core.comm import LoopbackWorld
    torch.cuda.set_device(0)
    which, P = args.emulate_rank.split("/")
    P = int(P)
    ranks = list(range(P)) if which == "all" else [int(which)]
    adv = args.workload == "advection"     # BASELINE configs[4] instead of configs[2]: advection_1d, 4 levels m = 2, F-cycle
    if adv:
        from pymgrit_amd import Advection1D, GridTransferAdvection, GridTransferCopy
        nt0, nxs = args.nt_adv, [8193, 4097, 2049, 2049]
        t0 = np.linspace(0, 2, nt0)
        grids = [t0[::2 ** k] for k in range(4)]
        nts, ctype = [len(g) for g in grids], 'F'
        dofs = [n - 1 for n in nxs]
        counts = cycle_phi_counts(nts, [2, 2, 2], 'F')
    else:
        nx, nt0 = args.nx, args.nt
        nts, ctype = [nt0, (nt0 - 1) // 4 + 1, (nt0 - 1) // 16 + 1], 'V'
        t0 = np.linspace(0, 2.0 * (nt0 - 1) / 65536, nt0)
        grids = [t0, t0[::4], t0[::16]]
        dofs = [nx - 2] * 3
        counts = phi_counts(nts, [4, 4])
    dof = dofs[0]
    world = LoopbackWorld(P)
    gate = threading.Barrier(P)
    out, err = {}, []

    def one_cycle(mg, it, pl):
        mg.backend.mirror_cpoints(it % 6, pl)
        mg.iteration(lvl=0, cycle_type=ctype, iteration=it, first_f=True)
        handle = mg.backend.residual_begin(mg._c_points(0))
        mg.backend.snapshot_cpoints(it % 6, pl)
        return handle

    def work(q):
        try:
            comm = world.comm(q)
            if adv:
                problem = [Advection1D(c=1, x_start=-1, x_end=1, nx=n, t_interval=g) for n, g in zip(nxs, grids)]
                transfer = [GridTransferAdvection(), GridTransferAdvection(), GridTransferCopy()]
            else:
                problem = [Heat1D(x_start=0, x_end=1, nx=nx, a=1, init_cond=init_cond, rhs_separable=[(rhs_space, rhs_time)],
                                  t_interval=g) for g in grids]
                transfer = None
            mg = Mgrit(problem, transfer=transfer, cf_iter=1, cycle_type=ctype, nested_iteration=False, max_iter=1000, tol=0.0,
                       logging_lvl=30, comm_time=comm, plan_blocks=args.plan_blocks)
            be = mg.backend
            pl = [int(i) for i in mg.index_local_c[0]]
            handles = [one_cycle(mg, 0, pl)]
            for k in range(args.warmup + 3):          # all ranks together: true ghost rows, plans recorded and captured
                handles.append(one_cycle(mg, 1 + k, pl))
            for h in handles:
                be.residual_end(h)
            be.sync()
            gate.wait()
            lock = {}
            if which == "all":     # the whole job on the one device: every rank's cycle, in lockstep
                gate.wait()
                t_a = time.perf_counter()
                hs = [one_cycle(mg, 10 + k, pl) for k in range(args.steps)]
                for h in hs:
                    be.residual_end(h)
                be.sync()
                gate.wait()
                lock["all_ranks_ms_per_cycle"] = 1e3 * (time.perf_counter() - t_a) / args.steps
            out[q] = (mg, be, pl, comm, lock)
            gate.wait()
        except BaseException as exc:   # noqa: BLE001
            err.append(exc)
            gate.abort()
    threads = [threading.Thread(target=work, args=(q,), daemon=True) for q in range(P)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    if err:
        raise err[0]
    world.frozen = True
    rows = []
    for r in ranks:
        mg, be, pl, comm, lock = out[r]
        for k in range(3):
            be.residual_end(one_cycle(mg, 100 + k, pl))
        be.sync()
        sent0 = comm.stats["messages"]
        torch.cuda.synchronize()
        t_a = time.perf_counter()
        hs = [one_cycle(mg, 200 + k, pl) for k in range(args.steps)]
        t_host = time.perf_counter() - t_a
        for h in hs:
            be.residual_end(h)
        be.sync()
        el = time.perf_counter() - t_a
        share = [c // P for c in counts]
        row = {"rank": r, "ms_per_cycle": 1e3 * el / args.steps, "host_enqueue_ms_per_cycle": 1e3 * t_host / args.steps,
               "messages_sent_per_cycle": (comm.stats["messages"] - sent0) / args.steps, "aligned": bool(getattr(mg, "_aligned", False)),
               "plan_blocks": mg.plan_blocks(),
               "cycle_graph": any(p is not None and getattr(p, "_hip", {}).get("graph") is not None for p in mg._plans.values()),
               "local_points_by_level": [len(t) for t in mg.t]}
        if os.environ.get("BENCH_EMULATE_PLAN"):
            plan = [pp for k, pp in mg._plans.items() if pp is not None and not k[1]][-1]
            for n in plan.order:
                print(f"{n.start*1e3:7.3f}-{n.finish*1e3:7.3f} {n.stream:5s} #{n.idx:3d} {n.name:14s} L{n.lvl} b{n.chunk}  preds "
                      f"{sorted(plan.nodes[q].idx for q in n.preds)}", file=sys.stderr)
        if args.emulate_sweeps:
            def cyc(it):
                be.residual_end(one_cycle(mg, 300, pl))
            row["sweeps"] = timed_sweeps(mg, be, cyc)
        row.update(lock)
        rows.append(row)
    worst = max(rows, key=lambda x: x["ms_per_cycle"])
    updates = float(sum(c * d for c, d in zip(counts, dofs)))
    res = {"metric": "time-point-DOF updates/sec per MGRIT V-cycle (EMULATED rank of a sharded run, one GPU)",
           "value": updates / P / (worst["ms_per_cycle"] * 1e-3), "unit": "time-point-DOF updates/s (this rank's share)",
           "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "ms_per_step": worst["ms_per_cycle"], "higher_is_better": True,
           "dtype": "f64", "data": "synthetic", "vs_baseline": None,
           "config": {"workload": (f"advection_1d nx=8193 nt={nt0} 4-level m=2 F-cycle with spatial coarsening" if adv else
                                   f"heat_1d nx={nx} nt={nt0} 3-level m=4 FCF V-cycle") +
                                  f" + residual values + C-point snapshot: rank(s) {which} of {P} emulated on one GPU (loopback "
                                  f"exchange)", "emulated_ranks": P,
                      "phi_per_cycle_by_level_whole_job": counts, "dof": dof},
           "ranks": rows}
    for x in rows:
        x["general_passes_on_levels"] = [lvl for lvl in range(out[x["rank"]][0].lvl_max - 1)
                                         if out[x["rank"]][0]._level_intervals(lvl) is None and out[x["rank"]][0]._gen_intervals(lvl) is not None]
    if which == "all":
        res["all_ranks_on_one_gpu_ms_per_cycle"] = max(x.get("all_ranks_ms_per_cycle", 0.0) for x in rows)
        res["exchange"] = {"messages_per_cycle": sum(x["messages_sent_per_cycle"] for x in rows),
                           "note": "point-to-point ghost rows of all ranks per V-cycle (SURVEY 2b: 24-27 at P=4)"}
    print(json.dumps(res), flush=True)


def bench_emulated_solve(args):
    """`--emulate-solve P`: the whole of Mgrit(...).solve() -- constructor, nested iteration, every cycle with its exchange points and
    op-5 hand-overs, the stopping test's all-gather, the final F-relaxation -- of BASELINE configs[2] on P ranks to 1e-10, rehearsed
    on ONE GPU: the P ranks are threads of this process (LoopbackWorld: true ghost rows, device mailboxes in the place of ncclSend /
    ncclRecv). What it shows: the sharded path runs end to end at full size on P ranks and reproduces the one-rank residual history
    bit for bit; how many iterations; what the host of a rank spends. What it cannot show is a parallel time -- the ranks share the
    one device, `wall_ms_all_ranks_on_one_gpu` is the SUM of their work. `critical_path_model` puts the measured pieces together:
    a rank's setup, `iterations` cycles of the slowest rank as measured alone (--emulate-rank), the P - 1 hops of a forward solve's
    hand-over chain (recurrence over a rank's blocks + its corrected last point + one message, measured per hop here), said to be
    a model."""
    import torch
    from pymgrit_amd import Heat1D, Mgrit
    from pymgrit_amd.core.comm import run_loopback_ranks
    torch.cuda.set_device(0)
    P = int(args.emulate_solve)
    nx, nt0 = args.nx, args.nt
    t0 = np.linspace(0, 2.0 * (nt0 - 1) / 65536, nt0)
    grids = [t0, t0[::4], t0[::16]]

    def build(comm):
        problem = [Heat1D(x_start=0, x_end=1, nx=nx, a=1, init_cond=init_cond, rhs_separable=[(rhs_space, rhs_time)], t_interval=g)
                   for g in grids]
        return Mgrit(problem, cf_iter=1, cycle_type='V', nested_iteration=True, max_iter=30, tol=1e-10, logging_lvl=30, comm_time=comm)

    def target(comm):
        torch.cuda.synchronize()
        comm.barrier()
        w0 = time.perf_counter()
        mg = build(comm)
        w1 = time.perf_counter()
        res = mg.solve()
        torch.cuda.synchronize()
        w2 = time.perf_counter()
        be = mg.backend
        out = {"rank": comm.rank, "conv": [float(v) for v in res["conv"]], "setup_ms": 1e3 * (w1 - w0), "solve_ms": 1e3 * (w2 - w1),
               "aligned": bool(getattr(mg, "_aligned", False)), "block_solve_sharded": bool(getattr(be, "block_sharded", {}).get(2)),
               "breakdown": getattr(mg, "solve_breakdown", None), "messages": int((mg.exchange_stats or {}).get("messages", 0)),
               "local_points_by_level": [len(t) for t in mg.t]}
        if out["block_solve_sharded"] and comm.rank == comm.size // 2:     # one hop of the hand-over chain: phase 2 of the block solve
            be.set_timing(True); be.timing_drain()       # (recurrence over the rank's blocks + its corrected last point; the state is
            for _k in range(10):                         # thrown away afterwards)
                be.block_solve(2, 2)
            recs = be.timing_drain(); be.set_timing(False)
            out["hop_block_phase2_us"] = 1e3 * float(np.mean([m for k, lv, m in recs if k == "chain"] or [0.0]))
        return out

    def run(size):      # twice: the second world finds its slabs in the allocator's cache (as bench.iters_to_tol's second run)
        rows = None
        for _ in range(2):
            import gc
            world, rows = run_loopback_ranks(size, target, timeout=900)
            world.close()
            gc.collect()
        return rows
    rows = run(P)
    one = run(1)[0] if P > 1 else None
    conv = rows[0]["conv"]
    same_all = all(r["conv"] == conv for r in rows)
    res = {"metric": "Mgrit.solve() end to end on P emulated ranks of ONE GPU (rehearsal, not a parallel time)", "emulated_ranks": P,
           "config": {"workload": f"heat_1d nx={nx} nt={nt0} 3-level m=4 FCF V-cycle, nested iteration, tol 1e-10"},
           "iterations": len(conv), "conv": conv, "every_rank_reports_the_same_history": bool(same_all),
           "equals_one_rank_history_bit_for_bit": (one is not None and one["conv"] == conv) if P > 1 else None,
           "wall_ms_all_ranks_on_one_gpu": {"setup": max(r["setup_ms"] for r in rows), "solve": max(r["solve_ms"] for r in rows)},
           "one_rank_ms": ({"setup": one["setup_ms"], "solve": one["solve_ms"]} if one else None),
           "ranks": [{k: v for k, v in r.items() if k != "conv"} for r in rows]}
    print(json.dumps(res), flush=True)


def sharded_emulation(ms_one_gpu, timeout=150):
    """the time-sharded run rehearsed on this ONE GPU (bench.py --emulate-rank r/P, child processes): device time per cycle of
    the middle rank of 2, 4 and 8 when it never waits for a neighbour, its host enqueue time, and what that bounds the
    N-GPU cycle by. Not a multi-GPU measurement: RCCL latency and the wait for the neighbour's hand-over are not in it."""
    import subprocess
    rows = []
    for P in (2, 4, 8):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--emulate-rank", f"{P // 2}/{P}", "--steps", "20", "--warmup", "3"],
                               capture_output=True, text=True, timeout=timeout)
            b = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
            k = b["ranks"][0]
            rows.append({"ranks": P, "rank": k["rank"], "ms_per_cycle": k["ms_per_cycle"], "host_enqueue_ms_per_cycle": k["host_enqueue_ms_per_cycle"],
                         "messages_sent_per_cycle": k["messages_sent_per_cycle"], "plan_blocks": k["plan_blocks"], "cycle_graph": k["cycle_graph"],
                         "aligned": k["aligned"], "one_gpu_ms_over_rank_ms": ms_one_gpu / k["ms_per_cycle"]})
        except Exception as exc:   # noqa: BLE001 - secondary numbers: report, never fail the headline
            rows.append({"ranks": P, "error": repr(exc)[:300]})
    # ... and Mgrit.solve() end to end on eight emulated ranks (bench.py --emulate-solve 8): iterations, the one-rank history bit for bit
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--emulate-solve", "8"], capture_output=True, text=True, timeout=timeout)
        b = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        rows.append({"solve_rehearsal_ranks": 8, "iterations": b["iterations"], "equals_one_rank_history_bit_for_bit": b["equals_one_rank_history_bit_for_bit"],
                     "every_rank_reports_the_same_history": b["every_rank_reports_the_same_history"],
                     "all_ranks_aligned_with_sharded_block_solve": all(x["aligned"] and x["block_solve_sharded"] for x in b["ranks"]),
                     "hop_block_phase2_us": next((x["hop_block_phase2_us"] for x in b["ranks"] if "hop_block_phase2_us" in x), None),
                     "wall_ms_all_ranks_on_one_gpu": b["wall_ms_all_ranks_on_one_gpu"],
                     "note": "threads of one process sharing the GPU: a rehearsal of the sharded path at full size, not a parallel time"})
    except Exception as exc:   # noqa: BLE001
        rows.append({"solve_rehearsal_ranks": 8, "error": repr(exc)[:300]})
    return rows


def cycle_figures(mg, be, nts, nx, nt0, dof, cycle, world, backend, ms_step):
    """--full, heat1d: the per-sweep table of the cycle with its bytes, the roofline row (the sweep with the largest share of
    the cycle) and the level-0 FCF figure. Every rank takes part (the FCF figure is the maximum over the ranks)."""
    import torch
    import torch.distributed as dist

    # --- per-sweep device times: HIP events around EVERY sweep entry point (mgrit_hip_set_timing), measured live on the
    # engine's stream over three more cycles in PROGRAM order (one full-width launch per sweep and level, nothing beside it:
    # these are the kernel times a rocprofv3 --kernel-trace --stats run of `bench.py --plan-blocks 1` shows per kernel)
    table = sweep_table(mg, be, nts, [4, 4], dof, cycle)
    local_share = 1.0 / world      # the table holds THIS rank's launches: its share of the job's bytes
    pmc, pmc_src, pmc_stale = pmc_traffic(nx, nt0, world)

    def pmc_bytes(sym):
        """HBM bytes per launch of a table row's kernel(s) from the PMC file; a row of several kernels (the time-parallel solve): their sum"""
        if not pmc:
            return None
        parts = [p.strip() for p in sym.split(" + ")]
        tot, hit = 0.0, 0
        for part in parts:
            for name, rec in pmc.items():
                if name == part or (len(parts) > 1 and name.startswith(part)):
                    tot += rec["hbm_bytes_per_launch"]
                    hit += 1
        return tot if hit >= len(parts) else None

    for row in table.values():
        # algorithmic = SURVEY 8d's bytes of the SWEEPS a launch stands for (a whole-level pass stands for two or three of them
        # and keeps the state in registers between them, so it moves far fewer bytes than that); physical = what the HBM
        # counters saw. Only physical bytes are priced against the HBM roofline.
        row["algorithmic_bytes_per_cycle"] *= local_share
        per_launch = pmc_bytes(row["kernel_symbol"])
        phys = per_launch * row["launches_per_cycle"] if per_launch else None
        row["physical_bytes_per_cycle"] = phys
        row["physical_GBps"] = phys / (row["ms_per_cycle"] * 1e-3) / 1e9 if (phys and row["ms_per_cycle"]) else None
        row["physical_frac"] = row["physical_GBps"] / HBM_PEAK_GBS if row["physical_GBps"] else None
        row["fused_vs_unfused_bytes"] = row["algorithmic_bytes_per_cycle"] / phys if phys else None
        row["algorithmic_GBps"] = row["algorithmic_bytes_per_cycle"] / (row["ms_per_cycle"] * 1e-3) / 1e9 if row["ms_per_cycle"] else None
    # the north_star's sweep-only figure: level-0 F-relax + C-relax + F-relax as launches of their own (inside a cycle they
    # may be part of a whole-level pass)
    be.set_timing(True)
    be.timing_drain()
    for _ in range(4):
        be.relax(0, mg._f_runs(0), 'F')
    for _ in range(4):
        be.relax(0, mg._c_runs(0), 'C')
    recs = be.timing_drain()
    be.set_timing(False)
    f_ms = float(np.mean([ms for k, _, ms in recs if k == "relax_f"][1:]))
    c_ms = float(np.mean([ms for k, _, ms in recs if k == "relax_c"][1:]))
    fcf_ms = 2 * f_ms + c_ms
    if world > 1:
        red = torch.tensor([fcf_ms], dtype=torch.float64, device="cuda" if backend == "nccl" else "cpu")
        dist.all_reduce(red, op=dist.ReduceOp.MAX)
        fcf_ms = float(red.item())
    N0 = nts[0] - 1
    fcf_bytes = (2 * (N0 * 3 // 4) + N0 // 4) * 16.0 * dof          # whole job: (2 F_0 + C_0) x 16 B x DOF  
    fcf_gbs = fcf_bytes / (fcf_ms * 1e-3) / 1e9
    dominant = max(table, key=lambda k: table[k]["ms_per_cycle"])
    dom = table[dominant]
    cycle_bytes = sum(r["algorithmic_bytes_per_cycle"] for r in table.values()) / local_share
    traffic = pmc_bytes(dom["kernel_symbol"])
    traffic_src = pmc_src
    phys_cycle = sum(r["physical_bytes_per_cycle"] or 0.0 for r in table.values()) if pmc else None
    # The roofline entry: the kernel with the largest share of the cycle's device time. For a whole-level pass the ALGORITHMIC bytes
    # are the rows the pass itself has to move (it stands for three sweeps of the reference's cycle but keeps the state
    # in registers between them -- the sweeps' own 8d bytes are listed beside it as `unfused_algorithmic_bytes_per_launch`)
    dom_unfused = dom["algorithmic_bytes_per_cycle"] / max(dom["launches_per_cycle"], 1)
    kind = dominant.split()[0]
    n_int = ((nts[0] - 1) // 4) * local_share
    row_b = 8.0 * dof
    if kind == "cf_fas":       # per interval: 1 row read (the pre-relaxed C-point); written: the C-point, g^{l+1}, u^{l+1} at the coarse
                               # level's C-points (1 in 4), v^{l+1} where a chunk of the way up starts (1 in 4)
        dom_alg = n_int * 3.5 * row_b
    elif kind == "ec_relax_res":   # per interval: u^{l+1} and the fine C-point read (+ v^{l+1} at chunk starts); the C-point and the last F-point written
        dom_alg = n_int * 4.25 * row_b
    else:
        dom_alg = dom_unfused
    dom_gbs = dom_alg / (dom["ms_per_launch"] * 1e-3) / 1e9
    return {
        # the kernel that takes the largest share of the cycle's device time (this rank), priced against the HBM roofline with
        # SURVEY 8d's algorithmic bytes; `limited_by` says what really bounds it
        "roofline": {"bound": "hbm", "achieved": dom_gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                     "frac": dom_gbs / HBM_PEAK_GBS, "traffic": traffic, "traffic_source": traffic_src, "stale": bool(pmc_stale),
                     "unfused_algorithmic_bytes_per_launch": dom_unfused,
                     "kernel": f"{dom['kernel_symbol']} ({dominant})", "launch_ms": dom["ms_per_launch"],
                     "launches_per_cycle": dom["launches_per_cycle"], "ms_per_cycle": dom["ms_per_cycle"],
                     "algorithmic_bytes_per_launch": dom_alg, "limited_by": dom["limited_by"]},
        "sweeps": table,
        "cycle": {"algorithmic_bytes": cycle_bytes, "physical_bytes": phys_cycle,
                  "physical_GBps": phys_cycle / (ms_step * 1e-3) / 1e9 if phys_cycle else None,
                  "physical_frac": phys_cycle / (ms_step * 1e-3) / 1e9 / (HBM_PEAK_GBS * world) if phys_cycle else None,
                  "fused_vs_unfused_bytes": cycle_bytes / phys_cycle if phys_cycle else None,
                  "physical_bytes_source": pmc_src,
                  "sum_of_sweep_ms_in_program_order": sum(r["ms_per_cycle"] for r in table.values()),
                  "note": "whole V-cycle + residual check. algorithmic = SURVEY 8d bytes of every sweep of the reference's cycle; "
                          "physical = HBM bytes of the kernels that run (PMC); physical_frac = physical bytes / wall time of a "
                          "step / 8 TB/s. In a planned cycle the chain runs beside the sweeps, so a step is shorter than the "
                          "sum of its sweeps"},
        "fcf_relax_level0": {"ms": fcf_ms, "algorithmic_GBps": fcf_gbs,
                             "frac_of_hbm_peak": fcf_gbs / (HBM_PEAK_GBS * world),
                             "updates_per_s": (2 * (N0 * 3 // 4) + N0 // 4) * dof / (fcf_ms * 1e-3),
                             "c_relax_ms": c_ms, "f_relax_ms": f_ms,
                             "note": "kernel time of the level-0 F-relax + C-relax + F-relax launches (max over ranks), "
                                     "whole-job bytes; the sweep-only figure of the north_star (bar: 0.60)"},
    }


def self_launch(n):
    """`python bench.py --gpus N` with no launcher environment: run the same command line under torch.distributed.run
    (one rank per GPU, rendezvous on 127.0.0.1 at a free port) as a CHILD process and pass its output and exit code on."""
    import socket
    import subprocess
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    proc = subprocess.run(cmd, env=env)
    if proc.returncode != 0:
        raise SystemExit(proc.returncode if proc.returncode > 0 else 1)
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--nx", type=int, default=16384)
    ap.add_argument("--nt", type=int, default=65537)
    ap.add_argument("--full", action="store_true",
                    help="after the headline numbers, measure everything else as well: per-sweep device times, roofline, the "
                         "level-0 FCF figure; heat1d on one GPU also the CPU baseline, iterations and time to tolerance, parity, "
                         "the other configurations and the sharded-rank emulation (child processes); several ranks also the "
                         "steps with a stopping test after every cycle. Off: the headline line alone")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: leave out the CPU baseline, iterations to "
                    "tolerance, parity, the other configurations and the sharded-rank emulation")
    ap.add_argument("--no-ramp", action="store_true", help="skip the one-second clock ramp (profiling runs: it would "
                    "fill the kernel summary with its own F-relax launches)")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend for N>1 (nccl = RCCL; gloo only to "
                    "smoke-test the N>1 path with several ranks on ONE GPU)")
    ap.add_argument("--nt-adv", dest="nt_adv", type=int, default=32769)
    ap.add_argument("--nx-adv", dest="nx_adv", type=int, default=8193, help="--workload advection: level-0 grid points (nx - 1 periodic "
                    "values, a multiple of 4; default BASELINE configs[4])")
    ap.add_argument("--at-k", dest="at_k", type=int, default=0,
                    help="AT-MGRIT with local coarse grids of k points instead of MGRIT (not the headline algorithm)")
    ap.add_argument("--pipeline-depth", dest="pipeline_depth", type=int, default=None,
                    help="N>1: how many iterations the stopping value may lag (default: the solver's default, 4; 0 = check "
                         "after every cycle like the reference's loop)")
    ap.add_argument("--plan-blocks", dest="plan_blocks", type=int, default=None,
                    help="blocks of time points of the planned cycle (core/cycle_plan.py); default: the backend's choice, "
                         "1 = program order")
    ap.add_argument("--all-configs", dest="all_configs", action="store_true",
                    help="after the headline line (BASELINE configs[2]) print one more JSON line per other GPU configuration: "
                         "configs[1] heat_1d 1024 x 4097, configs[3] heat_2d 512^2, configs[4] advection_1d (each in a child "
                         "process of its own, with --full if this run has it)")
    ap.add_argument("--workload", default="heat1d", choices=["heat1d", "heat2d", "advection"],
                    help="heat1d = BASELINE configs[2] (default, the driver's run); heat2d = configs[3] on one GPU")
    ap.add_argument("--emulate-rank", dest="emulate_rank", default=None,
                    help="r/P or all/P: rank r of a P-rank sharded run emulated on this ONE GPU (loopback exchange): ms per "
                         "cycle of that shard and host enqueue ms per cycle")
    ap.add_argument("--emulate-sweeps", dest="emulate_sweeps", action="store_true", help="with --emulate-rank: per-sweep device times")
    ap.add_argument("--emulate-solve", dest="emulate_solve", type=int, default=0,
                    help="P: Mgrit.solve() of the workload end to end on P emulated ranks of the one GPU (threads, loopback exchange), "
                         "its residual history against the one-rank run")
    ap.add_argument("--nx2d", type=int, default=512)
    ap.add_argument("--nt2d", type=int, default=16385)
    ap.add_argument("--dump-outputs", dest="dump_outputs", default=None, metavar="DIR",
                    help="after the timed steps, write what the last of them computed to DIR/<name>.npy (float64, under 64 MB; "
                         "one GPU, one process)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.dump_outputs and (args.gpus > 1 or args.emulate_rank or args.emulate_solve or "WORLD_SIZE" in os.environ
                              and int(os.environ["WORLD_SIZE"]) > 1):
        ap.error("--dump-outputs: one GPU, one process only")
    if args.emulate_rank:
        return bench_emulated(args)
    if args.emulate_solve:
        return bench_emulated_solve(args)
    if args.workload == "heat2d":
        return bench_heat2d(args)
    if args.workload == "advection":
        return bench_advection(args)

    # ---- N > 1 without a launcher around us: start the ranks ourselves, BEFORE anything touches the GPU. The children are
    # separate processes of `python -m torch.distributed.run` (never an exec of this one); rank 0's JSON line is relayed and
    # any child failure is this process's exit code.
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return self_launch(args.gpus)
    if "WORLD_SIZE" in os.environ and int(os.environ["WORLD_SIZE"]) != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={os.environ['WORLD_SIZE']} ranks")

    import torch
    import torch.distributed as dist
    from pymgrit_amd import Heat1D, Mgrit
    from pymgrit_amd.core.options import options

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the HIP path has no CPU fallback")
    local_rank = local_rank % torch.cuda.device_count()
    torch.cuda.set_device(local_rank)
    if world > 1:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(args.backend)

    nx, nt0 = args.nx, args.nt
    nts = [nt0, (nt0 - 1) // 4 + 1, (nt0 - 1) // 16 + 1]
    t0 = np.linspace(0, 2.0 * (nt0 - 1) / 65536, nt0)
    grids = [t0, t0[::4], t0[::16]]
    problem = [Heat1D(x_start=0, x_end=1, nx=nx, a=1, init_cond=init_cond, rhs_separable=[(rhs_space, rhs_time)],
                      t_interval=g) for g in grids]
    if args.at_k:   # AT-MGRIT variant of the same hierarchy (core/at_mgrit.py): truncated coarsest-level solves of distance k
        from pymgrit_amd import AtMgrit
        mg = AtMgrit(args.at_k, 0, problem, cf_iter=1, cycle_type='V', nested_iteration=False,
                     max_iter=2 + args.warmup + args.steps, tol=0.0, logging_lvl=30)
    else:
        mg = Mgrit(problem, cf_iter=1, cycle_type='V', nested_iteration=False, max_iter=2 + args.warmup + args.steps, tol=0.0,
                   logging_lvl=30, pipeline_depth=args.pipeline_depth, plan_blocks=args.plan_blocks)
    be = mg.backend
    # several ranks on RCCL links: every link of the job answers BEFORE anything is timed -- per-link latency into the line, a link
    # that does not answer ends every rank with the same message naming the pair (exit code 1)
    link_us = None
    if world > 1 and getattr(be, "device_links", False) and hasattr(mg.comm_time, "ping_links"):
        ping_buf = torch.zeros(8, dtype=torch.float64, device="cuda")
        try:
            link_us = mg.comm_time.ping_links(be, ping_buf.data_ptr())
        except RuntimeError as exc:
            raise SystemExit(f"bench.py --gpus {world}: {exc}")
    dof = nx - 2
    counts = phi_counts(nts, [4, 4])
    if args.at_k:   # coarsest level: point p is recomputed by min(p, k-1) steps instead of one step of the sequential solve
        counts[-1] = counts[-1] - (nts[-1] - 1) + sum(min(p, args.at_k - 1) for p in range(1, nts[-1]))
    updates_per_cycle = float(sum(c * dof for c in counts))

    def cycle(it):
        mg.iteration(lvl=0, cycle_type='V', iteration=it, first_f=True)
        mg.convergence_criterion(iteration=1)

    def fence():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    # a GPU that has just been handed to the process is still ramping its clocks (first run on a fresh box: 20.6 ms per cycle,
    # every later run 19.0-19.2): keep it busy for a second with level-0 F-relax launches -- idempotent on a relaxed state, no
    # exchange, so every rank can do it on its own clock -- before the W warm-up steps
    fence()
    t_ramp = time.perf_counter()
    while not args.no_ramp and time.perf_counter() - t_ramp < 1.0:
        for _ in range(20):
            be.relax(0, mg._f_runs(0), 'F')
        be.sync()
    pipelined = mg.pipeline_depth() > 0   # several ranks: the solver's own pipelined loop (Mgrit._solve_pipelined)
    comm_stats = getattr(mg.comm_time, "stats", None)      # per-process counters: only the timed steps' share is reported
    stats0 = None
    if pipelined:
        # the same steps through the solver's pipelined loop: every step still is one cycle + its stopping value; the values
        # are gathered asynchronously and ALL of them are resolved inside the timed region (_pl_finish)
        mg._pl_advance(1 + args.warmup, stop_on_tol=False)
        mg._pl_finish(stop_on_tol=False)
        fence()
        stats0 = dict(comm_stats) if comm_stats is not None else None
        t_start = time.perf_counter()
        mg._pl_advance(args.steps, stop_on_tol=False)
        mg._pl_finish(stop_on_tol=False)
        fence()
    else:
        cycle(0)  # iteration 0 (does the extra leading F-relax), then steady-state warm-up
        for _ in range(args.warmup):
            cycle(1)
        fence()
        stats0 = dict(comm_stats) if comm_stats is not None else None
        t_start = time.perf_counter()
        for _ in range(args.steps):
            cycle(1)
        # C-point storage (backend_hip.materialise): the cycles store, of every level-0 interval's F-points, only the last one;
        # Mgrit.solve() ends with the one F-relaxation that puts the others in place, so the timed steps end with it too
        getattr(be, "materialise", lambda: None)()
        fence()
    elapsed = time.perf_counter() - t_start
    if args.dump_outputs:
        dump_outputs(mg, args.dump_outputs)
    stats_timed = {k: comm_stats[k] - stats0[k] for k in comm_stats} if comm_stats is not None and stats0 is not None else None
    # several ranks: the same steps once more through the reference's own loop (mgrit.py:621-646: the stopping value examined after
    # every cycle, a blocking gather) -- what a solve costs when nothing may lag; outside `value`, --full only
    ms_checked = None
    if pipelined and args.full:
        cycle(1)
        fence()
        t_c = time.perf_counter()
        for _ in range(args.steps):
            cycle(1)
        getattr(be, "materialise", lambda: None)()
        fence()
        ms_checked = 1e3 * (time.perf_counter() - t_c) / args.steps
    chain_clock = be.chain_clock() if hasattr(be, "chain_clock") else (0.0, 0.0)   # last chain launch of the timed region
    if world > 1:
        tmax = torch.tensor([elapsed], dtype=torch.float64, device="cuda" if args.backend == "nccl" else "cpu")
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        elapsed = float(tmax.item())

    ms_step = 1e3 * elapsed / args.steps
    # Phi applications the ENGINE performs per cycle (the work model behind `value` counts the sweeps of the reference's cycle,
    # SURVEY 3.5): with pre-relaxed C-points the level-0 C-relaxation's Phi is the residual check's of the cycle before;
    # the time-parallel coarsest-level solve applies two Phi per step (less block 0's second pass and one per block)
    applied = list(counts)
    if not args.at_k and mg.cf_iter[0] == 1 and not options.no_pre_relax and mg._level_intervals(0) is not None:
        applied[0] -= (nts[0] - 1) // 4
    if getattr(be, "block_r", {}).get(len(nts) - 1):
        n_c = nts[-1] - 1
        applied[-1] += n_c - 16 - (n_c // 16 - 1)
    applied_updates = float(sum(c * dof for c in applied))

    out = {
        "metric": "time-point-DOF updates/sec per MGRIT V-cycle", "value": updates_per_cycle * args.steps / elapsed,
        # the same with the Phi applications the engine really executes (config.phi_applied_by_level)
        "value_applied": applied_updates * args.steps / elapsed,
        "unit": "time-point-DOF updates/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": ms_step, "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
        "dtype": "f64", "data": "synthetic",
        "config": {"workload": ("AT-MGRIT k=%d: " % args.at_k if args.at_k else "") +
                               f"heat_1d nx={nx} nt={nt0} 3-level m=4 FCF V-cycle + residual check "
                               f"(BASELINE configs[{2 if (nx, nt0) == (16384, 65537) else 1 if (nx, nt0) == (1024, 4097) else '-'}]; "
                               f"time points sharded over {world} GPU(s))",
                   "phi_per_cycle_by_level": counts, "phi_applied_by_level": applied, "dof": dof, "pipeline_depth": mg.pipeline_depth(),
                   "plan_blocks": mg.plan_blocks(), "chain_shader_mhz": chain_clock[0], "chain_us_per_step": chain_clock[1],
                   "cycle_graph": any(p is not None and getattr(p, "_hip", {}).get("graph") is not None for p in mg._plans.values())},
    }
    if args.full:
        out.update(cycle_figures(mg, be, nts, nx, nt0, dof, cycle, world, args.backend, ms_step))
    if world > 1:
        comm = mg.comm_time
        st = stats_timed
        if st is not None:
            per = torch.tensor([float(st["messages"]), float(st["bytes"]), float(st["device_messages"])], dtype=torch.float64,
                               device="cuda" if args.backend == "nccl" else "cpu")
            dist.all_reduce(per, op=dist.ReduceOp.SUM)
            cycles_run = args.steps      # the counters' difference over the timed steps alone
            out["exchange"] = {"backend": args.backend,
                               "path": ("mgrit_hip_exchange on RCCL links (ncclSend / ncclRecv under the C ABI)" if getattr(be, "device_links", False)
                                        else "torch.distributed send / recv" + (f" (links failed: {be.link_error})" if getattr(be, "link_error", None) else "")),
                               "messages_total": int(per[0].item()), "bytes_total": int(per[1].item()),
                               "device_resident_messages": int(per[2].item()),
                               "messages_per_cycle": per[0].item() / cycles_run, "bytes_per_cycle": per[1].item() / cycles_run,
                               "link_latency_us": link_us, "ms_per_step_check_every_cycle": ms_checked,
                               "ms_per_step_pipelined": ms_step if pipelined else None,
                               "note": "point-to-point ghost rows of all ranks (ops 0-5, 7 of reference mgrit.py:693-713); "
                                       "SURVEY 2b counts 24-27 per V-cycle at P=4"}
        out["nccl_ranks"] = dist.get_world_size() if args.backend == "nccl" else 0
    if rank == 0:
        if world == 1 and args.full and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(nx)
            out["iters_to_tol"] = iters_to_tol(problem, nx)
            out["time_to_solution_ms"] = out["iters_to_tol"].pop("time_to_solution_ms", None)
            out["parity"] = out["iters_to_tol"].pop("parity", None)
            if (nx, nt0) == (16384, 65537) and not args.all_configs and not args.at_k:
                # the other GPU configurations of BASELINE.json, each measured in a child process of its own AFTER everything
                # above, folded into this ONE line (the full lines: --all-configs); a failure there never touches the headline
                out["other_configs"] = other_configs()
                out["sharded_rank_emulation"] = sharded_emulation(ms_step)
                iters = out["iters_to_tol"]["full_workload"]["gpu_iters"]
                for row in out["sharded_rank_emulation"]:
                    if "ms_per_cycle" in row:   # the solve's iterations on that rank when it never waits for a neighbour: a lower
                        row["cycles_to_tol"] = iters       # bound of the sharded time to solution (one GPU: iterations x ms_per_step)
                        row["iterations_ms_if_never_waiting"] = iters * row["ms_per_cycle"]
                r8 = next((r for r in out["sharded_rank_emulation"] if r.get("ranks") == 8 and "ms_per_cycle" in r), None)
                reh = next((r for r in out["sharded_rank_emulation"] if r.get("solve_rehearsal_ranks") == 8 and "iterations" in r), None)
                if r8 and reh and out.get("time_to_solution_ms"):
                    hop = (reh.get("hop_block_phase2_us") or 0.0) + 10.0      # + one message of 131 KB + 2 KB, ASSUMED 10 us (no link was measured)
                    tts = out["time_to_solution_ms"]
                    reh["critical_path_model_ms"] = {
                        "setup_host_of_a_rank": tts["setup_ms"],      # host-bound (tables, lists): does not shrink with the rank count
                        "iterations": reh["iterations"] * r8["ms_per_cycle"],
                        "handover_chain_fill": 7 * hop * 1e-3,        # the last rank's first forward solve waits for seven hops; later ones overlap (lagged stopping test)
                        "final_f_relaxation": out["sweeps"].get("ec_relax_res L0", {}).get("ms_per_cycle", 0.0) / 8.0,
                        "one_gpu_wall_ms": tts["wall_ms"],
                        "note": "a MODEL from pieces measured on one GPU (rank cycle replayed alone, hop = block-solve phase 2 + an assumed "
                                "10 us message): sum = setup + iterations + fill + final; no multi-GPU hardware has run it"}
                    m = reh["critical_path_model_ms"]
                    m["sum"] = m["setup_host_of_a_rank"] + m["iterations"] + m["handover_chain_fill"] + m["final_f_relaxation"]
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    if args.all_configs and world == 1:
        import subprocess
        del mg, be, problem
        torch.cuda.empty_cache()
        me = os.path.abspath(__file__)
        for extra in OTHER_CONFIGS:
            r = subprocess.run([sys.executable, me] + extra + (["--full"] if args.full else []), capture_output=True, text=True)
            lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
            print(lines[-1] if lines and r.returncode == 0 else json.dumps({"config": {"workload": " ".join(extra)}, "error": r.stderr[-400:]}),
                  flush=True)


if __name__ == "__main__":
    main()
