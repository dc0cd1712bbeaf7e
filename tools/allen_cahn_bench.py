#!/usr/bin/env python3
"""AllenCahn(nx=512, method='IMEX'), nt = 4097, three levels, m = 4: device time of the level-0 F-relaxation and of one V-cycle, in
microseconds per Phi and as a fraction of the FP64 matrix peak (78.6 TF/s), with the project's Heat2D at 512 x 512 on the same time
grid measured in the same run beside it. Operations per Phi, counted from the shapes: Allen-Cahn four products with the full
nx x nx Hartley table, 4 * 2 nx^3; Heat2D four half-size (folded) sine transforms on the (nx-2)^2 interior, 4 * (nx-2)^3.

The same two legs for AllenCahn(method='IMPL', linear_solver='pcg') -- the batched Newton-PCG step -- on the same grids
(steps 0.01 / 4096, / 1024, / 256: fac / eps^2 = 1.5e-3, 6.1e-3, 2.4e-2, inside the solver's rule): microseconds per Phi and the Newton
and CG iterations per Phi from HipBackend.newton_stats; beside them the seconds per Phi of the host 'direct' step (sparse LU per Newton
iteration) on a sample of 4 states at the same nx, on the CPU, in the same process.

Each leg runs once, as a child process under its own time limit; the first failure ends the run. One JSON line per leg.
Usage:  python tools/allen_cahn_bench.py [nx [nt]]"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK = 78.6e12
LEGS = (("allencahn_f_relax", 300), ("heat2d_f_relax", 300), ("allencahn_v_cycle", 300), ("heat2d_v_cycle", 300),
        ("allencahn_pcg_f_relax", 600), ("allencahn_pcg_v_cycle", 600))


def leg(name, nx, nt):
    sys.path.insert(0, ROOT)
    import numpy as np
    from pymgrit_amd import AllenCahn, Heat2D, Mgrit
    t0 = np.linspace(0, 0.01, nt)
    grids = (t0, t0[::4], t0[::16])
    pcg = name.startswith("allencahn_pcg")
    if pcg:
        prob = [AllenCahn(nx=nx, method="IMPL", linear_solver="pcg", t_interval=g) for g in grids]
        flop = 8.0 * nx ** 3      # per application of the preconditioner
    elif name.startswith("allencahn"):
        prob = [AllenCahn(nx=nx, method="IMEX", t_interval=g) for g in grids]
        flop = 8.0 * nx ** 3
    else:
        prob = [Heat2D(x_start=0, x_end=1, y_start=0, y_end=1, nx=nx, ny=nx, a=1.0, method="BE", t_interval=g) for g in grids]
        flop = 4.0 * (nx - 2) ** 3
    mg = Mgrit(prob, cf_iter=1, nested_iteration=False, max_iter=3, tol=0.0, logging_lvl=30)
    be = mg.backend
    assert type(be).__name__ == "HipBackend"
    out = {"leg": name, "nx": nx, "nt": nt, "flop_per_phi": flop}

    def newton_counts():
        st = [be.newton_stats(lvl) for lvl in range(len(grids))]
        phi = max(1, sum(s["phi"] for s in st))
        return dict(newton_phi=phi, newton_per_phi=sum(s["newton_iterations"] for s in st) / phi,
                    cg_per_phi=sum(s["cg_iterations"] for s in st) / phi, at_newton_maxiter=sum(s["at_newton_maxiter"] for s in st))
    if name.endswith("f_relax"):
        runs = mg._f_runs(0)
        n_phi = sum(r[1] for r in runs)
        if pcg:      # states that are worth a Newton iteration: one V-cycle from the initial guess
            mg.iteration(lvl=0, cycle_type='V', iteration=0, first_f=True)
        for _ in range(1 if pcg else 2):
            be.relax(0, runs, 'F')
        be.sync()
        if pcg:
            # (host-driven loop: the sweep is timed on the host clock around a synchronisation, its kernels and host reads together)
            import time
            newton_counts()      # (every level: the warm-up cycle has stepped the coarse levels too)
            ms = []
            for _ in range(3):
                a = time.perf_counter()
                be.relax(0, runs, 'F')
                be.sync()
                ms.append(1e3 * (time.perf_counter() - a))
            best, mean = float(np.min(ms)), float(np.mean(ms))
            out.update(phi_per_sweep=n_phi, sweep_ms_mean=mean, sweep_ms_min=best, us_per_phi=1e3 * mean / n_phi, **newton_counts())
            # the host 'direct' step on 4 states of this level: seconds per Phi on the CPU
            direct = AllenCahn(nx=nx, method="IMPL", t_interval=grids[0])
            rows = be.natural("u", 0)[[0, 1, len(grids[0]) // 2, len(grids[0]) - 1]]
            a = time.perf_counter()
            for row in rows:
                direct._step_newton(row.reshape(nx, nx), float(grids[0][1] - grids[0][0]))
            out.update(host_direct_s_per_phi=(time.perf_counter() - a) / len(rows))
        else:
            be.set_timing(True); be.timing_drain()
            for _ in range(8):
                be.relax(0, runs, 'F')
            ms = [m for k, _, m in be.timing_drain() if k == "relax_f"]
            best, mean = float(np.min(ms)), float(np.mean(ms))
            out.update(phi_per_sweep=n_phi, sweep_ms_mean=mean, sweep_ms_min=best, us_per_phi=1e3 * mean / n_phi,
                       fraction_of_fp64_matrix_peak=n_phi * flop / (mean * 1e-3) / PEAK)
    else:
        import time
        import torch
        # Phi applications of one V-cycle with FCF relaxation (cf_iter = 1), counted from the level sizes: per level below the coarsest
        # F + C + F relaxation and the two halves of the FAS right-hand side, the coarsest solve, the F-relaxations on the way up
        mg.iteration(lvl=0, cycle_type='V', iteration=0, first_f=True)
        mg.convergence_criterion(iteration=0)
        torch.cuda.synchronize()
        times = []
        if pcg:
            newton_counts()
        for it in range(1, 3 if pcg else 4):
            a = time.perf_counter()
            mg.iteration(lvl=0, cycle_type='V', iteration=it, first_f=True)
            torch.cuda.synchronize()
            times.append(1e3 * (time.perf_counter() - a))
        out.update(cycle_ms=times, cycle_ms_mean=float(np.mean(times)))
        if pcg:
            counts = newton_counts()
            out.update(us_per_phi=1e3 * float(np.sum(times)) / counts["newton_phi"], **counts)
    print(json.dumps(out), flush=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--leg":
        leg(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))
        return
    nx = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    nt = int(sys.argv[2]) if len(sys.argv) > 2 else 4097
    for name, limit in LEGS:
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", name, str(nx), str(nt)], timeout=limit).returncode
        if rc != 0:
            sys.exit(f"leg {name} failed with exit status {rc}: stopping")


if __name__ == "__main__":
    main()
