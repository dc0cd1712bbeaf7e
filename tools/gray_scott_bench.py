#!/usr/bin/env python3
"""GrayScott(nx=512, method='IMEX') beside AllenCahn(nx=512, method='IMEX') on the same time grid (nt = 4097, three levels, m = 4): device
time of the level-0 F-relaxation in microseconds per Phi, both in ONE process on one card, the two alternating round by round so that
a drift of the card's clock or a neighbour's work meets both alike. Operations per Phi, counted from the shapes: Allen-Cahn four
products with the full nx x nx Hartley table, 4 * 2 nx^3; Gray-Scott the same four products for each of its two species, twice that.
The expectation is a ratio of 2; the spread of the rounds says how far from 2 a single figure may lie by chance.

Per round and application: two warm-up sweeps, then 8 sweeps timed by the engine's own device events (HipBackend.set_timing). One JSON
line per round and application, and a last line with the means, the spread (max - min over the rounds' means) and the ratio.
Usage:  python tools/gray_scott_bench.py [nx [nt [rounds]]]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK = 78.6e12
SWEEPS = 8


def hierarchy(kind, nx, nt):
    import numpy as np
    from pymgrit_amd import AllenCahn, GrayScott, Mgrit
    if kind == "grayscott":
        # steps of r = dt du / dx^2 = 0.8 on the fine level (the time grid plays no part in the sweep's cost)
        t0 = np.linspace(0, (nt - 1) * 0.8 * (2.0 / nx) ** 2, nt)
        prob = [GrayScott(nx=nx, method="IMEX", t_interval=g) for g in (t0, t0[::4], t0[::16])]
        flop = 16.0 * nx ** 3
    else:
        t0 = np.linspace(0, 0.01, nt)
        prob = [AllenCahn(nx=nx, method="IMEX", t_interval=g) for g in (t0, t0[::4], t0[::16])]
        flop = 8.0 * nx ** 3
    mg = Mgrit(prob, cf_iter=1, nested_iteration=False, max_iter=3, tol=0.0, logging_lvl=30)
    assert type(mg.backend).__name__ == "HipBackend"
    return mg, flop


def timed_sweeps(mg):
    """ms of each of SWEEPS level-0 F-relaxations after two untimed ones"""
    be, runs = mg.backend, mg._f_runs(0)
    be.set_timing(False)
    for _ in range(2):
        be.relax(0, runs, 'F')
    be.sync()
    be.set_timing(True)
    be.timing_drain()
    for _ in range(SWEEPS):
        be.relax(0, runs, 'F')
    ms = [m for k, _, m in be.timing_drain() if k == "relax_f"]
    assert len(ms) == SWEEPS, ms
    return ms, sum(r[1] for r in runs)


def main():
    sys.path.insert(0, ROOT)
    import numpy as np
    nx = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    nt = int(sys.argv[2]) if len(sys.argv) > 2 else 4097
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    made = {kind: hierarchy(kind, nx, nt) for kind in ("grayscott", "allencahn")}
    means = {kind: [] for kind in made}
    for rnd in range(rounds):
        for kind, (mg, flop) in made.items():
            ms, n_phi = timed_sweeps(mg)
            mean = float(np.mean(ms))
            means[kind].append(1e3 * mean / n_phi)
            print(json.dumps({"round": rnd, "app": kind, "nx": nx, "nt": nt, "phi_per_sweep": n_phi, "sweep_ms_mean": mean,
                              "sweep_ms_min": float(np.min(ms)), "us_per_phi": means[kind][-1], "flop_per_phi": flop,
                              "fraction_of_fp64_matrix_peak": n_phi * flop / (mean * 1e-3) / PEAK}), flush=True)
    gs, ac = np.asarray(means["grayscott"]), np.asarray(means["allencahn"])
    print(json.dumps({"summary": "us per Phi, level-0 F-relaxation", "nx": nx, "nt": nt, "rounds": rounds,
                      "grayscott_us_per_phi": float(gs.mean()), "grayscott_spread": float(gs.max() - gs.min()),
                      "allencahn_us_per_phi": float(ac.mean()), "allencahn_spread": float(ac.max() - ac.min()),
                      "ratio": float(gs.mean() / ac.mean()), "ratio_min": float((gs / ac).min()), "ratio_max": float((gs / ac).max())}),
          flush=True)


if __name__ == "__main__":
    main()
