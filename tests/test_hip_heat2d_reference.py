"""GPU tests of the Heat2D device path against a second implementation of Phi: every sweep of the device hierarchy against the SAME
hierarchy on the plugin path over ``ReferenceHeat2D`` (tests/heat2d_reference.py), whose step is a transform-free solve of
(I + theta dt L) x = b refined in long double. It shares neither the sine tables nor the fold nor the eigenvalues nor the right-hand
side's code with the device, the oracle or the host step, so a mistake common to those (test_hip_heat2d.py compares the device with the
oracle bit for bit; the oracle restates the device's algorithm) shows here. What the cases are chosen for:

  a. every sweep at the size edges of the tile product: 4x3 (mj < 2), 34x35 (m = 32 / 33), 66x67 (m = 64 / 65: one tile and just past it),
     129x130 / 131x132 (half sizes 64 / 65 of the folded transforms), 5x200 (strongly rectangular), with backward Euler, boundary values
     and separable forcing; Crank-Nicolson at two of them, forward Euler at 20x17, general forcing rows at 66x67;
  b. the homogeneous backward-Euler step (zero forcing, zero boundary values: the first transform reads the state rows, h2d_kloop GRID),
     random rims that must not leak in; 4x3 falls back to the staged path;
  c. several step sizes on one level: batch_make_plans groups a sweep's items by the bit pattern of dt, and the residual norms come
     back permuted by group (``pos``): compute_residual on such a grid pins that permutation;
  d. sweeps of more than H2D_MAX_BATCH = 1024 items (several launches, index arrays offset per plan) on dyadic grids, whose steps are exact;
  e. one Phi at 259x258 and 258x259 (HP = 192, P = 384);
  f. the time-parallel forward solve (77 coarsest steps, through the full sine spectrum) against the reference's step-by-step solve.

The coefficient is "mild" wherever the method is implicit: a such that 4 theta dt (fx + fy) = 8 for the largest step in use, so every mode
keeps at least 1 / 9 of its weight and a wrong entry for ANY mode shows (with the suite's a = 3.5 the step damps the high modes to
nothing and such a check is blind to them; tests/test_heat2d_reference_cpu.py shows both; heat2d_reference.coefficient). Forward Euler: 4 dt (fx + fy) = 0.9.

Tolerances, nothing measured on the device (heat2d_reference.phi_bound states the per-Phi term):
  per Phi:       ((2 mi + 2 mj + 8) + 1) EPS norm_F(babs)  (theta > 0),   (8 + 1) EPS norm_F(babs)  (theta = 0),
                 babs of the step's actual input row and end points, the largest over the steps of the sweep
  + SLACK        8 EPS * 3 * the largest row norm involved, for the sweep's own arithmetic
  c_relax:       scaled by max(1, w) and |w| + |1 - w|;  fas_residual: the sum over the two levels;
  residual norm: + (nx ny + 2) EPS * the norm itself
  chained steps (forward_solve, F-relaxation over 3 F-points):  e_k = Lip e_(k-1) + the step's per-Phi term + SLACK,
                 Lip = 1 for BE and CN (the interior map is a 2-norm contraction, the rim is the boundary values on both sides),
                 Lip = max(1, |1 - dt 4 (fx + fy)|) for FE
  time-parallel form (f): + cases.BLK_K EPS * the spacetime norm of the level, the allowance test_oracle_golden.py gives block against
                 stepped form.
Every comparison covers all rows of a list. Each sweep prints its worst error / allowed ("RATIO" lines).
"""
import numpy as np
import pytest

import cases
from heat2d_reference import EPS, ReferenceHeat2D, babs_norm, coefficient, make_app, phi_bound
from periodic2d_kinds import AC_BATCH_GRIDS as BATCH_GRIDS, AC_BATCH_GROUPS as BATCH_GROUPS, H, KINDS
from periodic2d_sweeps import (ALL_SWEEPS, STORED_STATE_SWEEPS, compare as _compare, distinct_steps as _distinct_steps, dt_groups, host_state as _host_state,
                               lists as _lists, ratio as _ratio, report as _report, row_norm as _row_norm, set_states as _set_states)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

RAGGED_GRIDS = KINDS["allencahn"].ragged(None)      # the ragged grids and the batch grids of the Allen-Cahn reference test
UNIFORM = cases.h2d_grids([17, 9, 5])


def _pair(nx, ny, ts, method="BE", a=None, forcing="separable", with_bc=True, **opts):
    """(device Mgrit, plugin Mgrit over ReferenceHeat2D) on the same hierarchy; a = None: the mild coefficient for the largest step"""
    from pymgrit_amd import Mgrit
    from pymgrit_amd.heat.heat_2d import Heat2D
    opts.setdefault("nested_iteration", False)
    if a is None:
        a = coefficient(nx, ny, method, max(float(np.max(np.diff(t))) for t in ts), "mild")
    dev = Mgrit([make_app(nx, ny, t, method, a, forcing, with_bc) for t in ts], logging_lvl=30, **opts)
    ref = Mgrit([make_app(nx, ny, t, method, a, forcing, with_bc, cls=ReferenceHeat2D) for t in ts], logging_lvl=30, **opts)
    assert type(dev.backend).__name__ == "HipBackend" and type(ref.backend).__name__ == "PluginBackend"
    assert all(type(p) is Heat2D for p in dev.problem) and all(type(p) is ReferenceHeat2D for p in ref.problem)
    for x, y in zip(dev.t, ref.t):
        assert np.array_equal(x, y)
    return dev, ref


def _random_states(ref, seed):
    """standard-normal rows for every list of every level, rims included"""
    rng = np.random.default_rng(seed)
    out = {}
    for lvl in range(ref.lvl_max):
        app = ref.problem[lvl]
        for name, lst in _lists(ref, lvl):
            out[(name, lvl)] = rng.standard_normal((len(lst), app.nx * app.ny))
    return out


def _phi_term(app, row, t_start, t_stop):
    return phi_bound(app, babs_norm(app, row, t_start, t_stop))


def _tol(app, t, inputs):
    """the largest per-Phi term among the steps t[i-1] -> t[i] with input inputs[i-1], i = 1 .. len(t) - 1"""
    return max(_phi_term(app, inputs[i - 1], t[i - 1], t[i]) for i in range(1, len(t)))


def _lip(app, dt):
    return 1.0 if app.theta != 0 else max(1.0, abs(1.0 - dt * 4.0 * (app.fx + app.fy)))


def _chain(app, t, inputs, slack):
    """e_k = Lip e_(k-1) + per-Phi term + SLACK over the steps t[k-1] -> t[k], inputs[k-1] the reference's input of step k"""
    e = 0.0
    for k in range(1, len(t)):
        e = _lip(app, t[k] - t[k - 1]) * e + _phi_term(app, inputs[k - 1], t[k - 1], t[k]) + slack
    return e


def _run_sweeps(dev, ref, w, seed, sweeps, levels=None, record=None):
    """each sweep on fresh standard-normal states, the device hierarchy against the reference hierarchy"""
    record = {} if record is None else record
    top = dev.lvl_max - 1
    levels = list(range(top)) if levels is None else levels
    seeds = iter(range(seed, seed + 1000))

    def fresh():
        st = _random_states(ref, next(seeds))
        _set_states(dev, ref, st)
        return st

    for lvl in levels:
        app, t = ref.problem[lvl], ref.t[lvl]
        if "f_relax" in sweeps:
            st = fresh()
            slack = 8 * EPS * 3 * _row_norm(*st.values())
            dev.f_relax(lvl); ref.f_relax(lvl)
            cpts = [int(i) for i in np.asarray(ref.cpts[lvl])]
            m = max(np.diff(cpts)) if len(cpts) > 1 else 1
            if m <= 2:      # every Phi acts on a stored state
                allowed = _tol(app, t, st[("u", lvl)]) + slack
            else:           # F-points of one interval are chained
                after, allowed = _host_state(ref, "u", lvl), 0.0
                for a, z in zip(cpts[:-1], cpts[1:]):
                    allowed = max(allowed, _chain(app, t[a:z], [st[("u", lvl)][a]] + [after[i] for i in range(a + 1, z - 1)], slack))
            _ratio(record, "f_relax", _compare(dev, ref, lvl, allowed, "f_relax"), allowed)
        if "c_relax" in sweeps:
            st = fresh()
            slack = 8 * EPS * 3 * _row_norm(*st.values())
            dev.c_relax(lvl); ref.c_relax(lvl)
            allowed = max(1.0, w) * _tol(app, t, st[("u", lvl)]) + slack * (abs(w) + abs(1 - w))
            _ratio(record, "c_relax", _compare(dev, ref, lvl, allowed, f"c_relax w={w}"), allowed)
        if "fas_residual" in sweeps:
            st = fresh()
            slack = 8 * EPS * 3 * _row_norm(*st.values())
            dev.fas_residual(lvl); ref.fas_residual(lvl)
            # g of the coarse level: one Phi of the fine level, one of the coarse level on restricted (= copied) rows of the fine u
            cpts = [int(i) for i in np.asarray(ref.cpts[lvl])]
            assert np.array_equal(t[cpts], ref.t[lvl + 1])
            allowed = _tol(app, t, st[("u", lvl)]) + _tol(ref.problem[lvl + 1], ref.t[lvl + 1], st[("u", lvl)][cpts]) + slack
            _ratio(record, "fas_residual", _compare(dev, ref, lvl + 1, allowed, "fas_residual"), allowed)
    if "forward_solve" in sweeps:
        st = fresh()
        dev.forward_solve(top); ref.forward_solve(top)
        uh = _host_state(ref, "u", top)
        allowed = _chain(ref.problem[top], ref.t[top], uh, 8 * EPS * 3 * _row_norm(uh, st[("g", top)]))
        _ratio(record, "forward_solve", _compare(dev, ref, top, allowed, "forward_solve"), allowed)
    if "error_correction" in sweeps:
        for lvl in reversed(levels):
            st = fresh()
            dev.error_correction(lvl); ref.error_correction(lvl)
            allowed = 8 * EPS * 3 * _row_norm(*st.values())
            _ratio(record, "error_correction", _compare(dev, ref, lvl, allowed, "error_correction"), allowed)
    if "compute_residual" in sweeps:
        st = fresh()
        app = ref.problem[0]
        got, want = np.asarray(dev.compute_residual()), np.asarray(ref.compute_residual())
        allowed = _tol(app, ref.t[0], st[("u", 0)]) + 8 * EPS * 3 * _row_norm(st[("u", 0)]) + (app.nx * app.ny + 2) * EPS * want
        assert got.shape == want.shape and got.size == len(ref.cpts[0]) - 1
        print(f"residual norms: worst deviation {np.abs(got - want).max():.3e}, allowed {allowed.min():.3e}")
        assert np.all(np.abs(got - want) <= allowed), np.abs(got - want).max()
        _ratio(record, "compute_residual", float(np.max(np.abs(got - want) / allowed)), 1.0)
    return record


def _both_weights(nx, ny, ts, seed, sweeps=ALL_SWEEPS, **kw):
    """the sweeps with w = 1.0, then C-relaxation (the one sweep that reads w) with w = 1.3"""
    record = {}
    dev, ref = _pair(nx, ny, ts, weight_c=1.0, **kw)
    _run_sweeps(dev, ref, 1.0, seed, sweeps, record=record)
    dev, ref = _pair(nx, ny, ts, weight_c=1.3, **kw)
    _run_sweeps(dev, ref, 1.3, seed + 500, ("c_relax",), record=record)
    return record


# ---- a. every sweep at the size edges ------------------------------------------------------------------------------------------------
EDGES = [("BE", 4, 3, "separable"), ("BE", 34, 35, "separable"), ("BE", 66, 67, "separable"), ("BE", 129, 130, "separable"),
         ("BE", 131, 132, "separable"), ("BE", 5, 200, "separable"), ("CN", 66, 67, "separable"), ("CN", 131, 132, "separable"),
         ("FE", 20, 17, "separable"), ("BE", 66, 67, "general")]


@pytest.mark.parametrize("method,nx,ny,forcing", EDGES, ids=[f"{m}-{x}x{y}-{f}" for m, x, y, f in EDGES])
def test_every_sweep_at_the_size_edges(method, nx, ny, forcing):
    assert torch.cuda.is_available()
    record = _both_weights(nx, ny, UNIFORM, 100 * nx + ny, method=method, forcing=forcing)
    _report(f"size_edges[{method},{nx}x{ny},{forcing}]", record)


def test_general_forcing_runs_from_rows():
    dev, _ = _pair(66, 67, UNIFORM, forcing="general")
    assert dev.backend.desc[0]["forcing_rows"] is not None


# ---- b. the homogeneous backward-Euler step ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx,ny", [(4, 3), (5, 4), (66, 67), (131, 129)])
def test_every_sweep_of_the_homogeneous_step(nx, ny):
    assert torch.cuda.is_available()
    dev, ref = _pair(nx, ny, UNIFORM, forcing="none", with_bc=False)
    d = dev.problem[0].device_stepper()
    assert len(d["forcing_time"]) == 0 and d["forcing_rows"] is None and not np.any(d["bc"])
    record = _run_sweeps(dev, ref, 1.0, 300 * nx + ny, ALL_SWEEPS)
    _report(f"homogeneous[{nx}x{ny}]", record)


# ---- c. several step sizes per level -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["BE", "CN"])
@pytest.mark.parametrize("nx,ny", [(20, 17), (66, 67)])
@pytest.mark.parametrize("grid", sorted(RAGGED_GRIDS))
def test_every_sweep_with_several_step_sizes_per_level(grid, nx, ny, method):
    assert torch.cuda.is_available()
    ts = RAGGED_GRIDS[grid]
    for t in ts:
        assert _distinct_steps(t) >= 3 and len(set(np.round(np.diff(t) / 1e-4, 6))) >= 3, np.diff(t)
    if grid == "by4_2lvl":      # the three F-points of one interval do not share one D table (steps 1, 1, 1.5 and 2, 1, 1 of 1e-4)
        assert sum(len(set(np.round(np.diff(ts[0][a:a + 4]) / 1e-4, 6))) >= 2 for a in range(0, 16, 4)) >= 2
    record = _both_weights(nx, ny, ts, 500 * nx + ny + (7 if method == "CN" else 0), method=method)
    _report(f"step_sizes[{grid},{method},{nx}x{ny}]", record)


# ---- d. sweeps that split into several batches ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", sorted(BATCH_GROUPS))
def test_sweeps_of_more_than_one_batch(grid):
    assert torch.cuda.is_available()
    nx, ny, w = 9, 9, 1.3
    ts = [g["t_interval"] for g in BATCH_GRIDS[grid]()]
    dev, ref = _pair(nx, ny, ts, weight_c=w)
    t = np.asarray(dev.t[0])
    assert len(t) in (2051, 2053) and len(dev.t[1]) == (len(t) + 1) // 2 and t[1] - t[0] == H
    for groups in dt_groups(t):      # F-points, relaxed C-points
        print(f"{grid}: dt groups of {sum(groups)} points: {groups}")
        assert sum(groups) >= 1025 and groups == BATCH_GROUPS[grid], groups
    record = _run_sweeps(dev, ref, w, 77, STORED_STATE_SWEEPS, levels=[0])
    _report(f"batches[{grid}]", record)


# ---- e. one Phi at larger grids ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx,ny", [(259, 258), (258, 259)])
def test_one_phi_at_larger_grids(nx, ny):
    assert torch.cuda.is_available()
    ts = [np.linspace(0, 2.0 ** -9, n) for n in (5, 3)]      # steps of 2^-11, exact: one factorisation on the reference side
    assert _distinct_steps(ts[0]) == 1
    dev, ref = _pair(nx, ny, ts, a=coefficient(nx, ny, "BE", 2.0 ** -11, "mild"))
    st = _random_states(ref, nx)
    _set_states(dev, ref, st)
    dev.f_relax(0); ref.f_relax(0)
    allowed = _tol(ref.problem[0], ref.t[0], st[("u", 0)]) + 8 * EPS * 3 * _row_norm(*st.values())
    worst = _compare(dev, ref, 0, allowed, "f_relax")
    print(f"RATIO larger_grids[{nx}x{ny}] f_relax: worst error/allowed {worst / allowed:.4f}")


# ---- f. the time-parallel forward solve ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,a", [("BE", cases.H2D_A), ("CN", 0.1)])
def test_time_parallel_forward_solve(method, a):
    """77 coarsest steps = 3 blocks of 16 and one of 29. The states carry the boundary values on their rims (and g zero there), as
    every state a Phi has produced does: Crank-Nicolson takes the modal form for such states only"""
    assert torch.cuda.is_available()
    nx, ny = 12, 10
    t0 = np.linspace(0, 1, 309)
    dev, ref = _pair(nx, ny, [t0, t0[::4]], method=method, a=a)
    assert len(dev.t[1]) == 78 and dev.backend.block_r[1] == (nx - 2) * (ny - 2)
    st = _random_states(ref, 12)
    rim = np.ones((nx, ny), dtype=bool)
    rim[1:-1, 1:-1] = False
    st[("u", 1)][:, rim.ravel()] = ref.problem[1].boundary_values()[rim]
    st[("g", 1)][:, rim.ravel()] = 0.0
    _set_states(dev, ref, st)
    dev.forward_solve(1); ref.forward_solve(1)
    assert dev.backend.block_solve_form(1) != 0
    uh = _host_state(ref, "u", 1)
    allowed = _chain(ref.problem[1], ref.t[1], uh, 8 * EPS * 3 * _row_norm(uh, st[("g", 1)])) + cases.BLK_K * EPS * cases.spacetime_norm(uh)
    worst = _compare(dev, ref, 1, allowed, "forward_solve, time-parallel")
    print(f"RATIO time_parallel[{method}] forward_solve: worst error/allowed {worst / allowed:.4f}")
