"""The sweep harness the GPU tests of the periodic 2-D applications share (Allen-Cahn IMEX and Newton-PCG, Gray-Scott IMEX and
Newton-BiCGStab, Cahn-Hilliard): a device hierarchy ``dev`` against the SAME hierarchy ``ref`` on the plugin path, every sweep on fresh
random states, the error of every row of every list against an allowance. A plain helper like cases.py: no tests, no fixtures.

Beside the harness: ``host_class``, ``pair`` and ``random_states``, which build a kind's hierarchies and states from its entry in
periodic2d_kinds.py, and the case bodies the kinds' test files share (``both_weights``, ``check_*``).

What differs between the applications comes in as ``bounds``, a small object (a types.SimpleNamespace; ``bounds_of`` takes a kind's from
the table) with
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
import collections
import ctypes as C

import numpy as np

import cases
from periodic2d_kinds import KINDS, reference_class

EPS = cases.EPS
ALL_SWEEPS = ("f_relax", "c_relax", "fas_residual", "forward_solve", "error_correction", "compute_residual")
STORED_STATE_SWEEPS = ("f_relax", "c_relax", "fas_residual", "compute_residual")


def uniform(nts, t_stop):
    return [dict(t_start=0, t_stop=t_stop, nt=nt) for nt in nts]


def intervals(ts):
    return [dict(t_interval=np.asarray(t)) for t in ts]


def distinct_steps(t):
    return len(set(np.diff(np.asarray(t, dtype=np.float64)).view(np.int64).tolist()))


def dt_groups(t):
    """the sizes of the dt groups (one per bit pattern of the step) among the F-points and among the relaxed C-points of a level
    coarsened by 2, each list sorted"""
    t = np.asarray(t)
    return [sorted(collections.Counter((t[pts] - t[pts - 1]).view(np.int64).tolist()).values())
            for pts in (np.arange(1, len(t), 2), np.arange(2, len(t), 2))]


def lists(mg, lvl):
    return [(name, lst[lvl]) for name, lst in (("u", mg.u), ("v", mg.v), ("g", mg.g)) if lst[lvl] is not None]


def host_class(cls):
    """the subclass whose overridden step sends a hierarchy to the plugin path"""
    class Host(cls):
        def step(self, u_start, t_start, t_stop):
            return super().step(u_start, t_start, t_stop)
    Host.__name__ = Host.__qualname__ = "Host" + cls.__name__
    return Host


def pair(kind, nxs, grids, side="host", par=None, transfer=None, newton=False, dev_par=None, levels=None, **opts):
    """(device Mgrit, plugin Mgrit over the side's class) on the same hierarchy. nxs: one nx, or one per level (the kind's default
    parameters are those of the finest); grids: uniform() or intervals(); par: application parameters other than the kind's; newton:
    the Newton variant (the device side alone takes the kind's ``newton`` parameters and dev_par); levels: further arguments per level"""
    import pymgrit_amd
    entry = KINDS[kind]
    opts.setdefault("nested_iteration", False)
    if transfer is not None:
        opts["transfer"] = transfer
    nxs = [nxs] * len(grids) if np.isscalar(nxs) else list(nxs)
    args = {k: v for k, v in entry.par(nxs[0]).items() if not (newton and k == "method")}
    args.update(par or {})
    dev_only = dict(entry.newton, **(dev_par or {})) if newton else dict(dev_par or {})
    levels = [{}] * len(grids) if levels is None else levels
    cls = getattr(pymgrit_amd, entry.cls)
    other_cls = host_class(cls) if side == "host" else reference_class(kind, newton)
    dev = pymgrit_amd.Mgrit([cls(nx=nx, **args, **dev_only, **lv, **g) for nx, lv, g in zip(nxs, levels, grids)], logging_lvl=30, **opts)
    other = pymgrit_amd.Mgrit([other_cls(nx=nx, **args, **lv, **g) for nx, lv, g in zip(nxs, levels, grids)], logging_lvl=30, **opts)
    assert type(dev.backend).__name__ == "HipBackend" and type(other.backend).__name__ == "PluginBackend"
    for a, b in zip(dev.t, other.t):
        assert np.array_equal(a, b)
    return dev, other


def draw(kind, rng, name, n_pts, nx, newton=False):
    """[n_pts][values of one state] for the list ``name``: one draw per range of the kind, side by side"""
    entry = KINDS[kind]
    spans = entry.ranges(name, newton)
    parts = [rng.uniform(lo, hi, size=(n_pts, entry.planes * nx * nx // len(spans))) for lo, hi in spans]
    return parts[0] if len(parts) == 1 else np.concatenate(parts, axis=1)


def random_states(kind, ref, seed, newton=False, mean=None, zero_g=False):
    """states[(name, lvl)] for every list of every level in the kind's ranges (+ mean; zero_g: the right-hand sides zero, not drawn)"""
    rng = np.random.default_rng(seed)
    out = {}
    for lvl in range(ref.lvl_max):
        for name, lst in lists(ref, lvl):
            nx = ref.problem[lvl].nx
            if zero_g and name == "g":
                out[(name, lvl)] = np.zeros((len(lst), KINDS[kind].planes * nx * nx))
            else:
                out[(name, lvl)] = draw(kind, rng, name, len(lst), nx, newton)
                if mean is not None:
                    out[(name, lvl)] += mean
    return out


def bounds_of(kind, side="host", **state_opts):
    """the kind's bounds for run_sweeps (periodic2d_kinds.py), with its random states"""
    bounds = KINDS[kind].bounds(side)
    bounds.random_states = lambda ref, seed: random_states(kind, ref, seed, **state_opts)
    return bounds


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


# ---- the case bodies the kinds' test files share -----------------------------------------------------------------------------------
def both_weights(pair_for, bounds, seed, seed13, label, sweeps=ALL_SWEEPS, sweeps13=("c_relax",), check=None, run=run_sweeps):
    """the sweeps with weight_c = 1 from seed, then sweeps13 (C-relaxation is the one sweep the weight enters) with 1.3 from seed13, each
    on a pair of its own: pair_for(w) builds it, check(dev) asserts what the case relies on. One record, reported under label"""
    record = {}
    for w, names, first in ((1.0, sweeps, seed), (1.3, sweeps13, seed13)):
        dev, ref = pair_for(w)
        if check is not None:
            check(dev)
        run(dev, ref, bounds, w, first, names, record=record)
    report(label, record)


def check_ragged(dev, grid, unit=None):
    """several step sizes on every level; coarsening 4: the three F-points of one interval do not share one pair of D tables. unit: the
    grid's unit step where its steps are no exact multiples (the bit patterns AND the rounded multiples must differ)"""
    def steps(t):
        return distinct_steps(t) if unit is None else len(set(np.round(np.diff(t) / unit, 6)))
    for t in dev.t:
        assert distinct_steps(t) >= 3 and steps(t) >= 3, np.diff(t)
    if grid == "by4_2lvl":
        assert sum(steps(dev.t[0][a:a + 4]) >= 2 for a in range(0, 16, 4)) >= 2


def check_one_phi(dev, ref, bounds, seed, label):
    """one F-relaxation of level 0 on random states: every row within the per-Phi term + SLACK"""
    st = bounds.random_states(ref, seed)
    set_states(dev, ref, st)
    dev.f_relax(0); ref.f_relax(0)
    allowed = tol(bounds, ref, 0, st[("u", 0)]) + 8 * EPS * 3 * row_norm(*st.values())
    worst = compare(dev, ref, 0, allowed, "f_relax")
    print(f"RATIO {label} f_relax: worst error/allowed {worst / allowed:.4f}")


def check_history(dev, ref, what, iterations=None, last_state=True):
    """both solves: the residual (or jump) histories by the rule of tests/cases.py, the last state to 1e-9 relative (last_state=False:
    printed only). iterations=None: at least two, as many on both sides. Returns (conv, reference conv, the device's level-0 u)"""
    conv, rconv = np.asarray(dev.solve()["conv"]), np.asarray(ref.solve()["conv"])
    u = dev.backend.natural("u", 0)
    norm_u = cases.spacetime_norm(u)
    if iterations is None:
        assert len(conv) == len(rconv) >= 2, (conv, rconv)
        what_conv = f"{what} conv ({len(conv)} iterations)"
    else:
        assert len(conv) == len(rconv) == iterations, (conv, rconv)
        what_conv = f"{what} conv"
    dev_ref = np.abs(conv - rconv)
    print(f"RATIO {what_conv}: largest deviation {np.max(dev_ref) / (EPS * norm_u):.2f} units of eps*norm(u) "
          f"(allowed {cases.BLK_K} beyond 1e-10 relative)")
    assert np.all(dev_ref <= 1e-10 * rconv + cases.BLK_K * EPS * norm_u), (conv, rconv)
    last = host_state(ref, "u", 0)[-1]
    print(f"RATIO {what} last state: relative deviation {np.abs(u[-1] - last).max() / np.abs(last).max():.3e}")
    assert not last_state or np.abs(u[-1] - last).max() <= 1e-9 * np.abs(last).max()
    return conv, rconv, u


def check_jump_criterion(dev, ref, positive):
    """conv_crit = 1, three iterations from the initial guess: the same rule as for the residual histories; the first ``positive``
    jumps of the reference are not zero"""
    conv, rconv = np.asarray(dev.solve()["conv"]), np.asarray(ref.solve()["conv"])
    norm_u = cases.spacetime_norm(dev.backend.natural("u", 0))
    assert len(conv) == len(rconv) == 3 and np.all(rconv[:positive] > 0.0), (conv, rconv)
    print(f"RATIO solve[jump] conv: largest deviation {np.max(np.abs(conv - rconv)) / (EPS * norm_u):.2f} units of eps*norm(u)")
    assert np.all(np.abs(conv - rconv) <= 1e-10 * rconv + cases.BLK_K * EPS * norm_u), (conv, rconv)


def check_every_sweep_twice(dev, st, residual=False):
    """every relaxation, fas_residual and the forward solve run twice from the same states: every list of every level the same bits"""
    top = dev.lvl_max - 1
    sweeps = [("f_relax", lambda l=l: dev.f_relax(l)) for l in range(top)] + [("c_relax", lambda l=l: dev.c_relax(l)) for l in range(top)] + \
             [("fas_residual", lambda l=l: dev.fas_residual(l)) for l in range(top)] + [("forward_solve", lambda: dev.forward_solve(top))]
    for name, run in sweeps:
        out = []
        for rep in range(2):
            for (which, lvl), val in st.items():
                dev.backend.set_natural(which, lvl, val)
            run()
            out.append({key: dev.backend.natural(*key) for key in st})
        for key in st:
            assert np.array_equal(out[0][key], out[1][key]), (name, key)
    if residual:
        res = []
        for rep in range(2):
            for (which, lvl), val in st.items():
                dev.backend.set_natural(which, lvl, val)
            res.append(np.asarray(dev.compute_residual()))
        assert np.array_equal(res[0], res[1])


def check_level_0_twice(dev, ref, st):
    """the relaxations of level 0 run twice from the same states: the whole u slab, pads included, the same bits"""
    import torch
    for sweep in ("f_relax", "c_relax"):
        slabs = []
        for _ in range(2):
            set_states(dev, ref, st)
            getattr(dev, sweep)(0)
            slabs.append(dev.backend.U[0].clone())
        assert torch.equal(slabs[0], slabs[1]), sweep
    assert not torch.equal(slabs[0][1], slabs[0][3])      # (rows of different states differ)


def f_relaxed_rows(dev, ref, st, state, at):
    """``state`` put at the C-points ``at`` of level 0 among the states st: the rows F-relaxation leaves behind them (device tensors)"""
    for i in at:
        st[("u", 0)][i] = state
    set_states(dev, ref, st)
    dev.f_relax(0)
    U = dev.backend.U[0]
    return [U[i + 1].clone() for i in at]


def check_level_entry_point(entry, n_levels, bad_level, t_stop, ok, small, large, short, odd, bad, grid_msg, ld_msg, bad_msg, describe,
                            tail=(), large_says_grid=True, also_invalid=(), then=None):
    """what every mgrit_hip_level_<kind>2d refuses, through raw ctypes -- a null engine, a level out of range, a grid below / above the
    range (``small``, ``large``: EUNSUPPORTED, grid_msg), a row length shorter than a state or no multiple of 16 (``short``, ``odd``:
    EINVAL, ld_msg), each of the ``bad`` parameter tuples (EINVAL, bad_msg), a null or empty time grid -- then ``describe`` = [(level,
    arguments)] accepted, a level described twice refused, and no time-parallel forward solve for a non-linear Phi (r > 0 refused, the
    rule r < 0 leaves it step by step). ``tail``: the arguments behind the parameters; also_invalid: (all arguments, message) refused with EINVAL;
    then(lib, eng, fn, tp, msg): the kind's own"""
    import torch
    from pymgrit_amd.core import hip_lib
    lib = hip_lib.load()
    EINVAL, EUNSUPPORTED = -1, -4
    fn, cfg, msg = getattr(lib, entry), lib.mgrit_hip_block_solve_config, lib.mgrit_hip_last_error
    eng = C.c_void_p()
    assert lib.mgrit_hip_create(C.byref(eng), n_levels, C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    try:
        t9 = np.ascontiguousarray(np.linspace(0.0, t_stop, 9))
        tp, null = C.c_void_p(t9.ctypes.data), C.c_void_p(0)
        assert fn(None, 0, 9, tp, *ok, *tail) < 0 and fn(eng, bad_level, 9, tp, *ok, *tail) < 0 and fn(eng, -1, 9, tp, *ok, *tail) < 0
        assert fn(eng, 0, 9, tp, *small, *tail) == EUNSUPPORTED and grid_msg in msg()
        assert fn(eng, 0, 9, tp, *large, *tail) == EUNSUPPORTED and (not large_says_grid or grid_msg in msg())
        assert fn(eng, 0, 9, tp, *short, *tail) == EINVAL and ld_msg in msg()
        assert fn(eng, 0, 9, tp, *odd, *tail) == EINVAL
        for b in bad:
            assert fn(eng, 0, 9, tp, *b, *tail) == EINVAL and bad_msg in msg(), b
        for args, fragment in also_invalid:
            assert fn(eng, 0, 9, tp, *args) == EINVAL and fragment in msg(), fragment
        assert fn(eng, 0, 9, null, *ok, *tail) == EINVAL
        assert fn(eng, 0, -1, tp, *ok, *tail) == EINVAL
        for lvl, args in describe:
            assert fn(eng, lvl, 9, tp, *args) == 0, (lvl, args)
        assert fn(eng, 0, 9, tp, *ok, *tail) < 0 and b"already" in msg()
        assert cfg(eng, 1, 4, 1, 0, null, null) == EUNSUPPORTED
        assert cfg(eng, 1, -1, 1, 0, null, null) == 0
        if then is not None:
            then(lib, eng, fn, tp, msg)
    finally:
        assert lib.mgrit_hip_destroy(eng) == 0
