#!/usr/bin/env python3
"""GrayScott(nx=512, method='IMEX') beside AllenCahn(nx=512, method='IMEX') on the same time grid (nt = 4097, three levels, m = 4): device
time of the level-0 F-relaxation in microseconds per Phi, both in ONE process on one card, the two alternating round by round so that
a drift of the card's clock or a neighbour's work meets both alike. Operations per Phi, counted from the shapes: Allen-Cahn four
products with the full nx x nx Hartley table, 4 * 2 nx^3; Gray-Scott the same four products for each of its two species, twice that.
The expectation is a ratio of 2; the spread of the rounds says how far from 2 a single figure may lie by chance.

Per round and application: two warm-up sweeps, then 8 sweeps timed by the engine's own device events (HipBackend.set_timing). One JSON
line per round and application, and a last line with the means, the spread (max - min over the rounds' means) and the ratio.

Legs ``grayscott_bicgstab_f_relax`` and ``grayscott_bicgstab_v_cycle``: GrayScott(nx=512, method='IMPL', linear_solver='bicgstab') -- the
batched Newton-BiCGStab step -- on the same grids, each leg a process of its own: milliseconds per sweep / cycle and
microseconds per Phi on the host clock around a synchronisation (the loop is host-driven: its kernels and host reads together), Newton and
BiCGStab iterations per Phi from ``newton_stats``. A third leg, ``grayscott_bicgstab_host_direct``, needs no GPU: for scale, the host
'direct' step (a sparse LU per Newton iteration) on two states of the same level -- the initial guess and the step from it -- in seconds
per Phi.
Usage:  python tools/gray_scott_bench.py [nx [nt [rounds]]]
        python tools/gray_scott_bench.py --bicgstab [nx [nt [dt]]]      (dt: the fine step, in place of the IMEX legs' 0.8 dx^2 / du)"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK = 78.6e12
SWEEPS = 8


BICGSTAB_LEGS = (("grayscott_bicgstab_f_relax", 900), ("grayscott_bicgstab_v_cycle", 900), ("grayscott_bicgstab_host_direct", 900))


def hierarchy(kind, nx, nt, dt=None):
    import numpy as np
    from pymgrit_amd import AllenCahn, GrayScott, Mgrit
    if kind.startswith("grayscott"):
        # steps of r = dt du / dx^2 = 0.8 on the fine level (the time grid plays no part in the IMEX sweep's cost)
        t0 = np.linspace(0, (nt - 1) * (0.8 * (2.0 / nx) ** 2 if dt is None else dt), nt)
        step = dict(method="IMPL", linear_solver="bicgstab") if kind == "grayscott_bicgstab" else dict(method="IMEX")
        prob = [GrayScott(nx=nx, t_interval=g, **step) for g in (t0, t0[::4], t0[::16])]
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


def bicgstab_leg(name, nx, nt, dt0=None):
    import time
    import numpy as np
    from pymgrit_amd import GrayScott
    if name.endswith("host_direct"):
        dt = 0.8 * (2.0 / nx) ** 2 if dt0 is None else dt0
        direct = GrayScott(nx=nx, method="IMPL", t_start=0, t_stop=2 * dt, nt=3)
        w, secs = direct.initial_guess().get_values(), []
        for _ in range(2):
            a = time.perf_counter()
            w = direct._step_impl(w, dt)
            secs.append(time.perf_counter() - a)
        print(json.dumps({"leg": name, "nx": nx, "dt": dt, "host_direct_s": secs, "host_direct_s_per_phi": float(np.mean(secs))}), flush=True)
        return
    mg, flop = hierarchy("grayscott_bicgstab", nx, nt, dt0)
    be = mg.backend
    out = {"leg": name, "nx": nx, "nt": nt, "dt": float(mg.t[0][1] - mg.t[0][0]), "flop_per_preconditioner": flop}

    def newton_counts():
        st = [be.newton_stats(lvl) for lvl in range(mg.lvl_max)]
        phi = max(1, sum(s["phi"] for s in st))
        return dict(newton_phi=phi, newton_per_phi=sum(s["newton_iterations"] for s in st) / phi,
                    bicgstab_per_phi=sum(s["cg_iterations"] for s in st) / phi, at_newton_maxiter=sum(s["at_newton_maxiter"] for s in st))
    # states that are worth a Newton iteration: one V-cycle from the initial guess
    mg.iteration(lvl=0, cycle_type='V', iteration=0, first_f=True)
    mg.convergence_criterion(iteration=0)
    be.sync()
    if name.endswith("f_relax"):
        runs = mg._f_runs(0)
        n_phi = sum(r[1] for r in runs)
        be.relax(0, runs, 'F')
        be.sync()
        newton_counts()      # (every level: the warm-up cycle has stepped the coarse levels too)
        ms = []
        for _ in range(3):
            a = time.perf_counter()
            be.relax(0, runs, 'F')
            be.sync()
            ms.append(1e3 * (time.perf_counter() - a))
        mean = float(np.mean(ms))
        out.update(phi_per_sweep=n_phi, sweep_ms_mean=mean, sweep_ms_min=float(np.min(ms)), us_per_phi=1e3 * mean / n_phi, **newton_counts())
    else:
        newton_counts()
        times = []
        for it in range(1, 3):
            a = time.perf_counter()
            mg.iteration(lvl=0, cycle_type='V', iteration=it, first_f=True)
            be.sync()
            times.append(1e3 * (time.perf_counter() - a))
        counts = newton_counts()
        out.update(cycle_ms=times, cycle_ms_mean=float(np.mean(times)), us_per_phi=1e3 * float(np.sum(times)) / counts["newton_phi"], **counts)
    print(json.dumps(out), flush=True)


def main():
    sys.path.insert(0, ROOT)
    import numpy as np
    if len(sys.argv) > 1 and sys.argv[1] == "--leg":
        bicgstab_leg(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), float(sys.argv[5]) if len(sys.argv) > 5 else None)
        return
    if len(sys.argv) > 1 and sys.argv[1] == "--bicgstab":
        nx = int(sys.argv[2]) if len(sys.argv) > 2 else 512
        nt = int(sys.argv[3]) if len(sys.argv) > 3 else 4097
        for name, limit in BICGSTAB_LEGS:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", name, str(nx), str(nt)] + sys.argv[4:5], timeout=limit).returncode
            if rc != 0:
                sys.exit(f"leg {name} failed with exit status {rc}: stopping")
        return
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
