#!/usr/bin/env python3
"""GinzburgLandau2D beside GrayScott(method='IMEX') at nx = 128, 256, 512 on the same time grid (nt = 1025, three levels, m = 4): device
time of the level-0 F-relaxation in milliseconds per Phi, both in ONE process on one card, the two alternating round by round so that a
drift of the card's clock or a neighbour's work meets both alike. Gray-Scott IMEX is the closest sibling: its Phi is four two-plane
Hartley products over two work slab items per state (16 nx^3 operations), the second of which scales each item with its own table.
Ginzburg-Landau does the same four products on the same items; its second is p2d_cross_kernel, ONE workgroup per tile
and state that runs the K loop of both items, reads both tables and writes both items: half as many workgroups in that launch, each
with twice the work and two accumulators. The ratio Ginzburg-Landau / Gray-Scott is what that exchange costs.

Per round and application: two warm-up sweeps, then 8 sweeps timed by the engine's own device events (HipBackend.set_timing). One JSON
line per size, round and application, and a line per size with the means, the spread (max - min over the rounds' means) and the ratio.
Usage:  python tools/ginzburg_landau_bench.py [nt [rounds [nx ...]]]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK = 78.6e12       # FP64 matrix operations per second
SWEEPS = 8


def hierarchy(kind, nx, nt):
    import numpy as np
    from pymgrit_amd import GinzburgLandau2D, GrayScott, Mgrit
    # one time grid for both: steps of 0.8 dx^2 of the grid with L = 2, as tools/gray_scott_bench.py; the grid plays no part in a
    # sweep's cost
    t0 = np.linspace(0, (nt - 1) * 0.8 * (2.0 / nx) ** 2, nt)
    if kind == "ginzburglandau":
        prob = [GinzburgLandau2D(nx=nx, L=2.0, t_interval=g) for g in (t0, t0[::4], t0[::16])]
    else:
        prob = [GrayScott(nx=nx, method="IMEX", t_interval=g) for g in (t0, t0[::4], t0[::16])]
    mg = Mgrit(prob, cf_iter=1, nested_iteration=False, max_iter=3, tol=0.0, logging_lvl=30)
    assert type(mg.backend).__name__ == "HipBackend"
    return mg, 16.0 * nx ** 3


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
    nt = int(sys.argv[1]) if len(sys.argv) > 1 else 1025
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    sizes = [int(a) for a in sys.argv[3:]] or [128, 256, 512]
    for nx in sizes:
        made = {kind: hierarchy(kind, nx, nt) for kind in ("ginzburglandau", "grayscott")}
        means = {kind: [] for kind in made}
        for rnd in range(rounds):
            for kind, (mg, flop) in made.items():
                ms, n_phi = timed_sweeps(mg)
                mean = float(np.mean(ms))
                means[kind].append(mean / n_phi)
                print(json.dumps({"round": rnd, "app": kind, "nx": nx, "nt": nt, "phi_per_sweep": n_phi, "sweep_ms_mean": mean,
                                  "sweep_ms_min": float(np.min(ms)), "ms_per_phi": means[kind][-1], "flop_per_phi": flop,
                                  "fraction_of_fp64_matrix_peak": n_phi * flop / (mean * 1e-3) / PEAK}), flush=True)
        gl, gs = np.asarray(means["ginzburglandau"]), np.asarray(means["grayscott"])
        flop = made["grayscott"][1]
        print(json.dumps({"summary": "ms per Phi, level-0 F-relaxation", "nx": nx, "nt": nt, "rounds": rounds,
                          "ginzburglandau_ms_per_phi": float(gl.mean()), "ginzburglandau_spread": float(gl.max() - gl.min()),
                          "ginzburglandau_fraction_of_fp64_matrix_peak": float(flop / (gl.mean() * 1e-3) / PEAK),
                          "grayscott_ms_per_phi": float(gs.mean()), "grayscott_spread": float(gs.max() - gs.min()),
                          "grayscott_fraction_of_fp64_matrix_peak": float(flop / (gs.mean() * 1e-3) / PEAK),
                          "ratio": float(gl.mean() / gs.mean()), "ratio_min": float((gl / gs).min()), "ratio_max": float((gl / gs).max())}),
              flush=True)
        del made      # the slabs of this size go back before the next size allocates


if __name__ == "__main__":
    main()
