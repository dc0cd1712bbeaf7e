#!/usr/bin/env python3
"""NavierStokes2D(nx=512) beside AllenCahn(nx=512, method='IMEX') on the same time grid (nt = 4097, three levels, m = 4): device time of
the level-0 F-relaxation in microseconds per Phi, both in ONE process on one card, the two alternating round by round so that a drift
of the card's clock or a neighbour's work meets both alike. Allen-Cahn IMEX is the yardstick: its Phi is four one-plane Hartley
products and nothing else (8 nx^3 operations), the first of which forms the right-hand side while it stages its operand from the
state row. Navier-Stokes runs eight such products -- four for the stream function, four for the diffusion solve -- around one more
launch, the stencil pass ns_rhs_kernel, which reads the psi item (nx^2 of its P^2 values), the state's plane and
writes one P x P work slab item: (2 nx^2 + P^2) * 8 bytes per Phi without a forcing. The prediction is 2 x Allen-Cahn + the pass's own
time; what is beyond it is the gaps of nine launches instead of four (the summary line's "beyond_prediction").

Per round and application: two warm-up sweeps, then 8 sweeps timed by the engine's own device events (HipBackend.set_timing). One JSON
line per round and application, and a last line with the means, the spread (max - min over the rounds' means) and the ratio. The
pass's own duration comes from a kernel trace of this tool (`bash tools/quick_prof.sh navier_stokes tools/navier_stokes_bench.py 512
4097 1`): the total time of ns_rhs_kernel over the states its launches carried (rounds * (2 + 8) sweeps * phi_per_sweep), against
stencil_bytes_per_phi; given as the fourth argument (microseconds per Phi) it enters the summary line.
Usage:  python tools/navier_stokes_bench.py [nx [nt [rounds [stencil_us_per_phi]]]]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK = 78.6e12       # FP64 matrix operations per second
HBM_PEAK = 8.0e12    # bytes per second
SWEEPS = 8


def hierarchy(kind, nx, nt):
    import numpy as np
    from pymgrit_amd import AllenCahn, Mgrit, NavierStokes2D
    # one time grid for both: steps of 0.8 dx^2 of the unit square, as tools/allen_cahn_bench.py; the grid plays no part in a sweep's
    # cost. On the Navier-Stokes grid (L = 2 pi, nu = 0.01) that is dt nu / dx^2 = 0.0002 and a CFL number far below 1
    t0 = np.linspace(0, (nt - 1) * 0.8 * (1.0 / nx) ** 2, nt)
    if kind == "navierstokes":
        prob = [NavierStokes2D(nx=nx, t_interval=g) for g in (t0, t0[::4], t0[::16])]
        flop = 16.0 * nx ** 3
    else:
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
    stencil_us = float(sys.argv[4]) if len(sys.argv) > 4 else None
    P = ((nx + 63) // 64) * 64
    stencil_bytes = (2 * nx * nx + P * P) * 8
    made = {kind: hierarchy(kind, nx, nt) for kind in ("navierstokes", "allencahn")}
    means = {kind: [] for kind in made}
    for rnd in range(rounds):
        for kind, (mg, flop) in made.items():
            ms, n_phi = timed_sweeps(mg)
            mean = float(np.mean(ms))
            means[kind].append(1e3 * mean / n_phi)
            print(json.dumps({"round": rnd, "app": kind, "nx": nx, "nt": nt, "phi_per_sweep": n_phi, "sweep_ms_mean": mean,
                              "sweep_ms_min": float(np.min(ms)), "us_per_phi": means[kind][-1], "flop_per_phi": flop,
                              "fraction_of_fp64_matrix_peak": n_phi * flop / (mean * 1e-3) / PEAK}), flush=True)
    ns, ac = np.asarray(means["navierstokes"]), np.asarray(means["allencahn"])
    out = {"summary": "us per Phi, level-0 F-relaxation", "nx": nx, "nt": nt, "rounds": rounds,
           "navierstokes_us_per_phi": float(ns.mean()), "navierstokes_spread": float(ns.max() - ns.min()),
           "allencahn_us_per_phi": float(ac.mean()), "allencahn_spread": float(ac.max() - ac.min()),
           "ratio": float(ns.mean() / ac.mean()), "ratio_min": float((ns / ac).min()), "ratio_max": float((ns / ac).max()),
           "navierstokes_minus_twice_allencahn_us_per_phi": float(ns.mean() - 2.0 * ac.mean()),
           "stencil_bytes_per_phi": stencil_bytes, "stencil_us_per_phi_at_hbm_peak": 1e6 * stencil_bytes / HBM_PEAK}
    if stencil_us is not None:
        beyond = float(ns.mean() - 2.0 * ac.mean() - stencil_us)
        out.update({"stencil_us_per_phi": stencil_us, "stencil_fraction_of_hbm_peak": 1e6 * stencil_bytes / HBM_PEAK / stencil_us,
                    "beyond_prediction_us_per_phi": beyond, "beyond_prediction_fraction_of_total": beyond / float(ns.mean())})
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
