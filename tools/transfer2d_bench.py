#!/usr/bin/env python3
"""The 2-D library transfers on the device against the same arithmetic through the caller's path, and the two kernels alone.

Hierarchies: Heat2D 513 x 513 -> 257 x 257 (backward Euler), AllenCahn 512 x 512 -> 256 x 256 (IMEX) and, rows of two planes,
GrayScott (IMEX) and Burgers2D 512 x 512 -> 256 x 256; two levels, nt = 257, m = 4, steps equal bit for bit (the caller's path takes one
step size per level). Legs, each a child process under its own time limit:

  *_cycle_library   one V-cycle with GridTransferHeat2D / GridTransferAllenCahn / GridTransferGrayScott / GridTransferBurgers (kernels
                    restrict2d_rows_kernel / interp2d_rows_kernel)
  *_cycle_caller    the same with a subclass that overrides both methods by super() calls: the Python methods row by row on the host
                    between the kernels (MGRIT_HIP_TRANSFER_CALLER)
  *_kernels         mgrit_hip_restrict_u and mgrit_hip_interpolate over the level's 64 C-points alone, device events; bytes moved =
                    8 * planes * (n_fine + n_coarse) per pair (every value of the source row read once, every value of the
                    destination written once; planes = 2 for grayscott_* and burgers_*), as a fraction of the 8 TB/s HBM peak

The first failure ends the run. One JSON line per leg.  Usage:  python tools/transfer2d_bench.py [nt [leg ...]]  (no leg named: all)"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK = 8.0e12
LEGS = tuple((f"{app}_{what}", 420) for app in ("heat2d", "allencahn", "grayscott", "burgers") for what in ("kernels", "cycle_library", "cycle_caller"))


def leg(name, nt):
    sys.path.insert(0, ROOT)
    import time
    import numpy as np
    import torch
    from pymgrit_amd import (AllenCahn, Burgers2D, GrayScott, GridTransferAllenCahn, GridTransferBurgers, GridTransferGrayScott,
                             GridTransferHeat2D, Heat2D, Mgrit)
    app = name.split("_")[0]
    heat = app == "heat2d"
    base = {"heat2d": GridTransferHeat2D, "allencahn": GridTransferAllenCahn, "grayscott": GridTransferGrayScott,
            "burgers": GridTransferBurgers}[app]
    planes = 2 if app in ("grayscott", "burgers") else 1

    class ViaPython(base):
        def restriction(self, u):
            return super().restriction(u)

        def interpolation(self, u):
            return super().interpolation(u)
    t0 = np.arange(nt) * (2.0 ** -16 if not heat else 2.0 ** -10)      # exact steps: one bit pattern of dt per level
    grids = (t0, t0[::4])
    if heat:
        sizes = (513, 257)
        prob = [Heat2D(x_start=0, x_end=1, y_start=0, y_end=1, nx=n, ny=n, a=1.0, method="BE", t_interval=g) for n, g in zip(sizes, grids)]
    else:
        sizes = (512, 256)
        make = {"allencahn": lambda **kw: AllenCahn(method="IMEX", **kw), "grayscott": lambda **kw: GrayScott(method="IMEX", **kw),
                "burgers": Burgers2D}[app]
        prob = [make(nx=n, t_interval=g) for n, g in zip(sizes, grids)]
    tr = ViaPython() if name.endswith("caller") else base()
    mg = Mgrit(prob, transfer=[tr], cf_iter=1, nested_iteration=False, max_iter=3, tol=0.0, logging_lvl=30)
    be = mg.backend
    assert type(be).__name__ == "HipBackend" and be._device_transfer(0) == (not name.endswith("caller"))
    out = {"leg": name, "nt": nt, "fine": sizes[0], "coarse": sizes[1], "planes": planes}
    if name.endswith("kernels"):
        pairs = [(4 * j, j) for j in range(1, len(grids[1]))]
        moved = 8.0 * planes * (sizes[0] ** 2 + sizes[1] ** 2) * len(pairs)
        for sweep, kind in ((be.restrict_u, "restrict"), (be.interpolate, "interpolate")):
            for _ in range(2):
                sweep(0, pairs)
            be.sync()
            be.set_timing(True); be.timing_drain()
            for _ in range(8):
                sweep(0, pairs)
            ms = [m for k, _, m in be.timing_drain() if k == kind]
            be.set_timing(False)
            mean = float(np.mean(ms))
            out[kind] = dict(pairs=len(pairs), bytes=moved, ms_mean=mean, ms_min=float(np.min(ms)), tb_per_s=moved / (mean * 1e-3) / 1e12,
                             fraction_of_hbm_peak=moved / (mean * 1e-3) / HBM_PEAK)
    else:
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
        leg(sys.argv[2], int(sys.argv[3]))
        return
    nt = int(sys.argv[1]) if len(sys.argv) > 1 else 257
    unknown = set(sys.argv[2:]) - {name for name, _ in LEGS}
    if unknown:
        sys.exit(f"unknown legs {sorted(unknown)}: one of {[name for name, _ in LEGS]}")
    for name, limit in LEGS:
        if sys.argv[2:] and name not in sys.argv[2:]:
            continue
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", name, str(nt)], timeout=limit).returncode
        if rc != 0:
            sys.exit(f"leg {name} failed with exit status {rc}: stopping")


if __name__ == "__main__":
    main()
