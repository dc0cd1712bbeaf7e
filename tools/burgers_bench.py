#!/usr/bin/env python3
"""Burgers2D(nx=512) beside GrayScott(nx=512, method='IMEX') on the same time grid (nt = 4097, three levels, m = 4): device time of the
level-0 F-relaxation in microseconds per Phi, both in ONE process on one card, the two alternating round by round so that a drift of
the card's clock or a neighbour's work meets both alike. Gray-Scott IMEX is the yardstick: its Phi is four two-plane Hartley products
and nothing else (16 nx^3 operations), the first of which forms the right-hand side while it stages its operand from the state row.
Burgers runs four products over the same items behind one more launch, the stencil pass bg_rhs_kernel, which reads
the two planes of a state once and writes two P x P work slab items: (2 nx^2 + 2 P^2) * 8 bytes per Phi; its first product is then a
plain one that reads those items back. So the ratio Burgers / Gray-Scott minus 1 is the cost of (stencil pass + plain product) over
(staging product), not the pass alone -- it can be negative, and on an MI355X it is ("Burgers IMEX").

Per round and application: two warm-up sweeps, then 8 sweeps timed by the engine's own device events (HipBackend.set_timing). One JSON
line per round and application, and a last line with the means, the spread (max - min over the rounds' means) and the ratio. The
pass's own duration comes from a kernel trace of this tool (`bash tools/quick_prof.sh burgers tools/burgers_bench.py 512 4097 1`):
the total time of bg_rhs_kernel over the states its launches carried (rounds * 2 * (2 + 8) sweeps * phi_per_sweep, half of them
Burgers'), against stencil_bytes_per_phi.
Usage:  python tools/burgers_bench.py [nx [nt [rounds]]]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK = 78.6e12       # FP64 matrix operations per second
HBM_PEAK = 8.0e12    # bytes per second
SWEEPS = 8


def hierarchy(kind, nx, nt):
    import numpy as np
    from pymgrit_amd import Burgers2D, GrayScott, Mgrit
    # one time grid for both: steps of 0.8 dx^2 of the Gray-Scott grid (L = 2, du = 1), as tools/gray_scott_bench.py; the grid plays no
    # part in a sweep's cost. On Burgers' grid (L = 1, nu = 0.01) that is dt nu / dx^2 = 0.032 and dt / dx = 0.0063 per unit of |u|
    t0 = np.linspace(0, (nt - 1) * 0.8 * (2.0 / nx) ** 2, nt)
    if kind == "burgers":
        prob = [Burgers2D(nx=nx, t_interval=g) for g in (t0, t0[::4], t0[::16])]
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
    nx = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    nt = int(sys.argv[2]) if len(sys.argv) > 2 else 4097
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    P = ((nx + 63) // 64) * 64
    stencil_bytes = (2 * nx * nx + 2 * P * P) * 8
    made = {kind: hierarchy(kind, nx, nt) for kind in ("burgers", "grayscott")}
    means = {kind: [] for kind in made}
    for rnd in range(rounds):
        for kind, (mg, flop) in made.items():
            ms, n_phi = timed_sweeps(mg)
            mean = float(np.mean(ms))
            means[kind].append(1e3 * mean / n_phi)
            print(json.dumps({"round": rnd, "app": kind, "nx": nx, "nt": nt, "phi_per_sweep": n_phi, "sweep_ms_mean": mean,
                              "sweep_ms_min": float(np.min(ms)), "us_per_phi": means[kind][-1], "flop_per_phi": flop,
                              "fraction_of_fp64_matrix_peak": n_phi * flop / (mean * 1e-3) / PEAK}), flush=True)
    bg, gs = np.asarray(means["burgers"]), np.asarray(means["grayscott"])
    print(json.dumps({"summary": "us per Phi, level-0 F-relaxation", "nx": nx, "nt": nt, "rounds": rounds,
                      "burgers_us_per_phi": float(bg.mean()), "burgers_spread": float(bg.max() - bg.min()),
                      "grayscott_us_per_phi": float(gs.mean()), "grayscott_spread": float(gs.max() - gs.min()),
                      "ratio": float(bg.mean() / gs.mean()), "ratio_min": float((bg / gs).min()), "ratio_max": float((bg / gs).max()),
                      "ratio_minus_1": float(bg.mean() / gs.mean() - 1.0), "burgers_minus_grayscott_us_per_phi": float(bg.mean() - gs.mean()),
                      "stencil_bytes_per_phi": stencil_bytes, "stencil_us_per_phi_at_hbm_peak": 1e6 * stencil_bytes / HBM_PEAK}), flush=True)


if __name__ == "__main__":
    main()
