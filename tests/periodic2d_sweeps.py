"""The sweep harness the GPU tests of the periodic 2-D applications share (Allen-Cahn IMEX and Newton-PCG, Gray-Scott IMEX and
Newton-BiCGStab, Cahn-Hilliard): a device hierarchy ``dev`` against the SAME hierarchy ``ref`` on the plugin path, every sweep on fresh
random states, the error of every row of every list against an allowance. A plain helper like cases.py: no tests, no fixtures.

What differs between the applications comes in as ``bounds``, a small object of the test module (a types.SimpleNamespace) with
  random_states(ref, seed)        states[(name, lvl)] = [n_pts][values of one state] for every list of every level
  phi_term(ref, app, rows, dt)    the allowance of ONE Phi of app with the step dt for inputs among rows (the module's mathematics)
  lip(app, dt, rows)              the Lipschitz factor of that Phi, for chained steps
  values_per_state(app)           nx * nx or 2 * nx * nx: the sum behind a residual norm
  coarse_rows(ref, st, lvl)       the rows the coarse-level Phi of fas_residual(lvl) acts on, read after the sweep
  weight_in_key                   whether the C-relaxation's record key carries the weight ("c_relax w=1.3") or not ("c_relax")
  after(dev)                      optional: checked at the end of run_sweeps

The sweeps' own arithmetic takes SLACK = 8 EPS * 3 * the largest row norm involved; chained steps (forward_solve, the F-points of one
interval) e_k = Lip_k e_(k-1) + the step's per-Phi term + SLACK. Each module's docstring derives its per-Phi term and Lip_k.
"""
import numpy as np

import cases

EPS = cases.EPS
ALL_SWEEPS = ("f_relax", "c_relax", "fas_residual", "forward_solve", "error_correction", "compute_residual")
STORED_STATE_SWEEPS = ("f_relax", "c_relax", "fas_residual", "compute_residual")


def uniform(nts, t_stop):
    return [dict(t_start=0, t_stop=t_stop, nt=nt) for nt in nts]


def intervals(ts):
    return [dict(t_interval=np.asarray(t)) for t in ts]


def distinct_steps(t):
    return len(set(np.diff(np.asarray(t, dtype=np.float64)).view(np.int64).tolist()))


def lists(mg, lvl):
    return [(name, lst[lvl]) for name, lst in (("u", mg.u), ("v", mg.v), ("g", mg.g)) if lst[lvl] is not None]


def set_states(dev, host, states):
    """states[(name, lvl)] = [n_pts][values of one state in row-major order] (nx x nx here, nx x ny for Heat2D; Gray-Scott: two planes)"""
    for (name, lvl), val in states.items():
        dev.backend.set_natural(name, lvl, val)
        lst = dict(lists(host, lvl))[name]
        for i in range(len(lst)):
            lst[i].set_values(val[i].reshape(np.shape(lst[i].get_values())).copy())


def host_state(host, name, lvl):
    return np.array([np.asarray(v.get_values()).ravel() for v in dict(lists(host, lvl))[name]])


def row_norm(*arrays):
    return max(float(np.max(np.linalg.norm(np.atleast_2d(a), axis=1))) for a in arrays)


def compare(dev, host, lvl, allowed, what):
    worst = 0.0
    for name, _ in lists(host, lvl):
        got, ref = dev.backend.natural(name, lvl), host_state(host, name, lvl)
        err = float(np.max(np.linalg.norm(got - ref, axis=1)))
        worst = max(worst, err)
        assert err <= allowed, (what, name, lvl, err, allowed)
    print(f"{what} level {lvl}: worst row error {worst:.3e}, allowed {allowed:.3e}")
    return worst


def ratio(record, what, err, allowed):
    record[what] = max(record.get(what, 0.0), err / allowed if allowed > 0.0 else 0.0)


def report(test, record):
    for what, r in record.items():
        print(f"RATIO {test} {what}: worst error/allowed {r:.4f}")


def tol(bounds, ref, lvl, rows):
    """the per-Phi term of the level for inputs among rows, with the level's largest step"""
    return bounds.phi_term(ref, ref.problem[lvl], rows, float(np.max(np.diff(ref.t[lvl]))))


def chain(bounds, ref, app, t, inputs, slack):
    """e_k = Lip_k e_(k-1) + per-Phi term + SLACK over the steps t[k-1] -> t[k], inputs[k-1] the reference's input of step k"""
    e = 0.0
    for k in range(1, len(t)):
        dt = float(t[k] - t[k - 1])
        e = bounds.lip(app, dt, inputs[k - 1]) * e + bounds.phi_term(ref, app, inputs[k - 1], dt) + slack
    return e


def run_sweeps(dev, ref, bounds, w, seed, sweeps, levels=None, record=None):
    """the named sweeps on fresh random states, each against the reference hierarchy. Transfers: copy, or any the two sides share"""
    record = {} if record is None else record
    top = dev.lvl_max - 1
    levels = list(range(top)) if levels is None else levels
    seeds = iter(range(seed, seed + 1000))

    def fresh():
        st = bounds.random_states(ref, next(seeds))
        set_states(dev, ref, st)
        return st

    for lvl in levels:
        app = ref.problem[lvl]
        if "f_relax" in sweeps:
            st = fresh()
            slack = 8 * EPS * 3 * row_norm(*st.values())
            dev.f_relax(lvl); ref.f_relax(lvl)
            cpts = [int(i) for i in np.asarray(ref.cpts[lvl])]
            if (max(np.diff(cpts)) if len(cpts) > 1 else 1) <= 2:      # every Phi acts on a stored state
                allowed = tol(bounds, ref, lvl, st[("u", lvl)]) + slack
            else:                                                      # F-points of one interval are chained
                after, t, allowed = host_state(ref, "u", lvl), ref.t[lvl], 0.0
                for a, z in zip(cpts[:-1], cpts[1:]):
                    allowed = max(allowed, chain(bounds, ref, app, t[a:z], [st[("u", lvl)][a]] + [after[i] for i in range(a + 1, z - 1)], slack))
            ratio(record, "f_relax", compare(dev, ref, lvl, allowed, "f_relax"), allowed)
        if "c_relax" in sweeps:
            st = fresh()
            slack = 8 * EPS * 3 * row_norm(*st.values())
            dev.c_relax(lvl); ref.c_relax(lvl)
            allowed = max(1.0, w) * tol(bounds, ref, lvl, st[("u", lvl)]) + slack * (abs(w) + abs(1 - w))
            ratio(record, f"c_relax w={w}" if bounds.weight_in_key else "c_relax", compare(dev, ref, lvl, allowed, f"c_relax w={w}"), allowed)
        if "fas_residual" in sweeps:
            st = fresh()
            slack = 8 * EPS * 3 * row_norm(*st.values())
            dev.fas_residual(lvl); ref.fas_residual(lvl)
            # g of the coarse level: one Phi of the fine level, one of the coarse level on the restricted rows of the fine u
            allowed = tol(bounds, ref, lvl, st[("u", lvl)]) + tol(bounds, ref, lvl + 1, bounds.coarse_rows(ref, st, lvl)) + slack
            ratio(record, "fas_residual", compare(dev, ref, lvl + 1, allowed, "fas_residual"), allowed)
    if "forward_solve" in sweeps:
        st = fresh()
        dev.forward_solve(top); ref.forward_solve(top)
        uh = host_state(ref, "u", top)
        allowed = chain(bounds, ref, ref.problem[top], ref.t[top], uh, 8 * EPS * 3 * row_norm(uh, st[("g", top)]))
        ratio(record, "forward_solve", compare(dev, ref, top, allowed, "forward_solve"), allowed)
    if "error_correction" in sweeps:
        for lvl in reversed(levels):
            st = fresh()
            dev.error_correction(lvl); ref.error_correction(lvl)
            allowed = 8 * EPS * 3 * row_norm(*st.values())
            ratio(record, "error_correction", compare(dev, ref, lvl, allowed, "error_correction"), allowed)
    if "compute_residual" in sweeps:
        st = fresh()
        got, want = np.asarray(dev.compute_residual()), np.asarray(ref.compute_residual())
        # the norm of one point: its values' errors, and (n + 2) EPS relative for the sum of a state's n squares and the root
        allowed = (tol(bounds, ref, 0, st[("u", 0)]) + 8 * EPS * 3 * row_norm(st[("u", 0)])
                   + (bounds.values_per_state(ref.problem[0]) + 2) * EPS * want)
        assert got.shape == want.shape and got.size == len(ref.cpts[0]) - 1
        print(f"residual norms: worst deviation {np.abs(got - want).max():.3e}, allowed {allowed.min():.3e}")
        assert np.all(np.abs(got - want) <= allowed), np.abs(got - want).max()
        ratio(record, "compute_residual", float(np.max(np.abs(got - want) / allowed)), 1.0)
    if getattr(bounds, "after", None):
        bounds.after(dev)
    return record
