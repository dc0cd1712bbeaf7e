#!/usr/bin/env python3
"""AllenCahn(nx=512, method='IMEX'), nt = 4097, three levels, m = 4: device time of the level-0 F-relaxation and of one V-cycle, in
microseconds per Phi and as a fraction of the FP64 matrix peak (78.6 TF/s), with the project's Heat2D at 512 x 512 on the same time
grid measured in the same run beside it. Operations per Phi, counted from the shapes: Allen-Cahn four products with the full
nx x nx Hartley table, 4 * 2 nx^3; Heat2D four half-size (folded) sine transforms on the (nx-2)^2 interior, 4 * (nx-2)^3.

Each leg runs once, as a child process under its own time limit; the first failure ends the run. One JSON line per leg.
Usage:  python tools/allen_cahn_bench.py [nx [nt]]"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK = 78.6e12
LEGS = (("allencahn_f_relax", 300), ("heat2d_f_relax", 300), ("allencahn_v_cycle", 300), ("heat2d_v_cycle", 300))


def leg(name, nx, nt):
    sys.path.insert(0, ROOT)
    import numpy as np
    from pymgrit_amd import AllenCahn, Heat2D, Mgrit
    t0 = np.linspace(0, 0.01, nt)
    grids = (t0, t0[::4], t0[::16])
    if name.startswith("allencahn"):
        prob = [AllenCahn(nx=nx, method="IMEX", t_interval=g) for g in grids]
        flop = 8.0 * nx ** 3
    else:
        prob = [Heat2D(x_start=0, x_end=1, y_start=0, y_end=1, nx=nx, ny=nx, a=1.0, method="BE", t_interval=g) for g in grids]
        flop = 4.0 * (nx - 2) ** 3
    mg = Mgrit(prob, cf_iter=1, nested_iteration=False, max_iter=3, tol=0.0, logging_lvl=30)
    be = mg.backend
    assert type(be).__name__ == "HipBackend"
    out = {"leg": name, "nx": nx, "nt": nt, "flop_per_phi": flop}
    if name.endswith("f_relax"):
        runs = mg._f_runs(0)
        n_phi = sum(r[1] for r in runs)
        for _ in range(2):
            be.relax(0, runs, 'F')
        be.sync()
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
        for it in range(1, 4):
            a = time.perf_counter()
            mg.iteration(lvl=0, cycle_type='V', iteration=it, first_f=True)
            torch.cuda.synchronize()
            times.append(1e3 * (time.perf_counter() - a))
        out.update(cycle_ms=times, cycle_ms_mean=float(np.mean(times)))
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
