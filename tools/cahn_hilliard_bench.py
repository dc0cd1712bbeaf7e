#!/usr/bin/env python3
"""CahnHilliard beside AllenCahn(method='IMEX') at nx = 256, 512, 1024: device time of the level-0 F-relaxation in microseconds per Phi,
both applications on the same time grid in the same process, their sweeps alternating over several rounds. Three levels, m = 4, on a
dyadic grid (steps 2^-20, exact: one bit pattern of dt, so a sweep's batches are as large as the grid allows for both applications).

The expectation to check is the product count: a Cahn-Hilliard Phi is six P x P item-products with the full Hartley table (the first
over two items per state, the combine product's two K loops, two products back), an Allen-Cahn Phi four -- a ratio of 1.5 where the
matrix cores are the limit. Operations per Phi, counted from the shapes: 6 * 2 nx^3 against 4 * 2 nx^3.

One child process per nx under its own time limit; the first failure ends the run. One JSON line per nx.
Usage:  python tools/cahn_hilliard_bench.py [nx ...]"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK = 78.6e12
NT = {256: 2049, 512: 1025, 1024: 257}      # level-0 points: the state slabs of three levels stay below 8 GB
ROUNDS, SWEEPS = 5, 4


def hierarchy(kind, nx, nt):
    import numpy as np
    from pymgrit_amd import AllenCahn, CahnHilliard, Mgrit
    t0 = 2.0 ** -20 * np.arange(float(nt))
    grids = (t0, t0[::4], t0[::16])
    if kind == "cahnhilliard":
        prob = [CahnHilliard(nx=nx, t_interval=g) for g in grids]
    else:
        prob = [AllenCahn(nx=nx, method="IMEX", t_interval=g) for g in grids]
    mg = Mgrit(prob, cf_iter=1, nested_iteration=False, max_iter=3, tol=0.0, logging_lvl=30)
    assert type(mg.backend).__name__ == "HipBackend"
    return mg


def sweep_ms(mg, runs):
    be = mg.backend
    be.timing_drain()
    for _ in range(SWEEPS):
        be.relax(0, runs, 'F')
    return [m for k, _, m in be.timing_drain() if k == "relax_f"]


def leg(nx):
    sys.path.insert(0, ROOT)
    import numpy as np
    nt = NT.get(nx, 257)
    made = {kind: hierarchy(kind, nx, nt) for kind in ("cahnhilliard", "allencahn")}
    runs = {kind: mg._f_runs(0) for kind, mg in made.items()}
    n_phi = sum(r[1] for r in runs["allencahn"])
    assert n_phi == sum(r[1] for r in runs["cahnhilliard"])
    for kind, mg in made.items():      # warm-up: tables, work slabs, batch plans
        for _ in range(2):
            mg.backend.relax(0, runs[kind], 'F')
        mg.backend.sync()
        mg.backend.set_timing(True)
    means = {kind: [] for kind in made}
    for _ in range(ROUNDS):
        for kind, mg in made.items():
            means[kind].append(1e3 * float(np.mean(sweep_ms(mg, runs[kind]))) / n_phi)
    ch, ac = np.asarray(means["cahnhilliard"]), np.asarray(means["allencahn"])
    print(json.dumps({"nx": nx, "nt": nt, "phi_per_sweep": n_phi, "rounds": ROUNDS, "sweeps_per_round": SWEEPS,
                      "cahnhilliard_us_per_phi": float(ch.mean()), "cahnhilliard_spread": float(ch.max() - ch.min()),
                      "allencahn_us_per_phi": float(ac.mean()), "allencahn_spread": float(ac.max() - ac.min()),
                      "ratio": float(ch.mean() / ac.mean()), "ratio_min": float((ch / ac).min()), "ratio_max": float((ch / ac).max()),
                      "cahnhilliard_fraction_of_fp64_matrix_peak": 12.0 * nx ** 3 / (ch.mean() * 1e-6) / PEAK,
                      "allencahn_fraction_of_fp64_matrix_peak": 8.0 * nx ** 3 / (ac.mean() * 1e-6) / PEAK}), flush=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--leg":
        leg(int(sys.argv[2]))
        return
    sizes = [int(a) for a in sys.argv[1:]] or [256, 512, 1024]
    for nx in sizes:
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", str(nx)], timeout=300).returncode
        if rc != 0:
            sys.exit(f"nx = {nx} failed with exit status {rc}: stopping")


if __name__ == "__main__":
    main()
