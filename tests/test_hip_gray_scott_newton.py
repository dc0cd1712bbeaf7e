"""GPU tests of the Gray-Scott Newton-BiCGStab device path (method='IMPL', linear_solver='bicgstab'; DESIGN.md 3.11, gsn_* in
csrc/mgrit_hip_grayscott.inc): every sweep of the device hierarchy against the SAME hierarchy on the plugin path over
``ReferenceGrayScottNewton`` (tests/gray_scott_newton_reference.py), whose step solves the non-linear system in long double with
corrections from a sparse LU of a Jacobian it assembles itself -- no table, none of the steppers' code.

Inputs: states (the lists u and v) rough and in the box, u plane uniform in [0, 1], v plane uniform in [0, 0.5], fresh per sweep; the
FAS right-hand sides g rough, signed and small (|g| <= 0.01 / 0.005), so that the chained steps of forward_solve stay in the box as
well. Every level of every hierarchy has max dt <= 0.25: dt mu(1.05, 0.55) = 0.25 * 1.97 < 0.5, the regime where the step has one
solution (gray_scott_newton_reference.py derives mu; the coarsest dt = 2 at nx = 4 of the IMEX tests' _t_sweep is the two-root case and
is not used). The box is not assumed: every tolerance takes it from the data and asserts dt mu < 1.

Tolerances, nothing of them measured on the device but its own residual in long double (gray_scott_newton_reference.py states them):

  a Phi that a sweep's row holds (F-relaxation, C-relaxation, forward_solve on every level: row = w (g + Phi) + (1 - w) old, so Phi is
      recovered from the row in long double by subtracting the same g and old on both sides; on level 0 the row IS Phi):
      tau = (norm_2(F(x_dev)) + norm_2(F(x_ref))) / (1 - dt mu) + EPS norm_2(x), both residuals in long double by the reference's code,
      each for its own side's input, mu from the largest |u|, |v| over both Phi and both inputs. Any two points of the box satisfy
      this; it gets its teeth from the exit criterion asserted beside it for every such Phi, max|F(x_dev)| < newton_tol + E_g + E_add:
      E_g = C_G EPS S from the operation count of gsn_residual_kernel (C_G = 8; gray_scott_newton_reference.py), E_add the sweep's own
      roundings between the device's Phi and the recovered one (_measured; zero where the row is Phi).
  a Phi that is not recoverable (fas_residual: the coarse g mixes one Phi of each level; compute_residual: only the norm of Phi - u is
      seen): the same tau with the two residuals replaced by what each side guarantees -- the device sqrt(2) nx (newton_tol + E_g) by
      its exit criterion on 2 nx^2 values (at_newton_maxiter == 0 is asserted), the reference the largest long-double residual it
      recorded during the sweep --, the box the one the reference recorded, widened by 5 % (u) and 10 % (v): a device result outside
      the widened box misses the reference by more than any allowance here.
  + SLACK    8 EPS * 3 * the largest row norm involved, for the sweep's own arithmetic, as tests/test_hip_gray_scott.py;
  fas_residual: the sum over the two levels;
  chained steps (forward_solve, F-relaxation over 3 F-points): e_k = e_(k-1) / (1 - dt_k mu) + tau_k + SLACK -- Phi is Lipschitz with
      1 / (1 - dt mu) on the box by the same inequality; tau_k measured with each side's own previous row as its input.
Every comparison covers all rows of a list. Each sweep prints its worst error / allowed ("RATIO" lines); the largest ratio of the first
run on an MI355X is in DESIGN.md 3.11.
"""
import ctypes as C

import numpy as np
import pytest

import cases
from gray_scott_newton_reference import (C_G_DEVICE, LD, PARS, e_g, exit_criterion, history_allowance, margin, mu, norm2, par_of, residual, tau,
                                         tau_phi_a_priori)
from periodic2d_kinds import GSN_RAGGED as RAGGED_GRIDS, dyadic
from periodic2d_sweeps import (STORED_STATE_SWEEPS, both_weights, compare as _compare, distinct_steps, dt_groups, host_state as _host_state,
                               intervals as _intervals, pair, random_states, ratio as _ratio, report as _report, row_norm as _row_norm,
                               set_states as _set_states)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

EPS = cases.EPS
GSN_MAX_BATCH = 2 * 1024 // (2 * 11)      # csrc/mgrit_hip.hip: 11 two-plane work rows within 2 x H2D_MAX_BATCH work slab items


def _uniform(nts, t_stop=1.0):
    """coarsest step 0.25 for nts = (17, 9, 5)"""
    return [dict(t_start=0, t_stop=t_stop, nt=nt) for nt in nts]


def _pair(nx, grids, par=None, app=None, **opts):
    """(device Mgrit, plugin Mgrit over ReferenceGrayScottNewton) on the same hierarchy"""
    dev, ref = pair("grayscott", nx, grids, side="reference", newton=True, par=par, dev_par=app, **opts)
    for t in dev.t:
        assert np.max(np.diff(t)) <= 0.25
    return dev, ref


def _random_states(ref, seed):
    """per list and level [n_pts][2 nx^2]: states in the box, right-hand sides small and signed (module docstring)"""
    return random_states("grayscott", ref, seed, newton=True)


def _reset(ref):
    for app in ref.problem:
        app.reset_record()


def _tol(dev, ref, lvl):
    """the a-priori tau of one Phi of the level inside a sweep, from what the reference recorded since _reset"""
    return tau_phi_a_priori(dev.problem[lvl], float(np.max(np.diff(ref.t[lvl]))), [ref.problem[lvl]], C_G_DEVICE)


def _recover(row, g=None, old=None, w=1.0):
    """Phi as a sweep's row holds it, in long double: row = w (g + Phi) + (1 - w) old (g absent on level 0, w = 1 but for the weighted
    C-relaxation). For the rows of both sides the SAME g and old are subtracted, so the difference of two recovered Phi is the
    difference of the rows over w, exactly."""
    x = np.asarray(row, dtype=LD)
    if w != 1.0:
        x = (x - (LD(1) - LD(w)) * np.asarray(old, dtype=LD)) / LD(w)
    return x if g is None else x - np.asarray(g, dtype=LD)


def _measured(app, dt, w_dev, x_dev, w_ref, x_ref, c_add, what):
    """(tau, 1 / (1 - dt mu)) of one recovered Phi by the measured form of the module docstring -- each side's residual for ITS input,
    which on a chain is its own previous row --, after asserting the exit criterion of the device's Phi:
        max|F(x_dev)| < newton_tol + E_g + E_add,   E_add = M_F c_add EPS R,
    E_add for the roundings of the sweep's own arithmetic that lie between the device's Phi and the recovered one (c_add of them, EPS
    each on values of magnitude <= R = the largest |value| involved; none where the row IS Phi: c_add = 0), carried into F by its
    Lipschitz constant in the maximum norm, M_F = 1 + dt (8 max(du, dv) / dx^2 + |a| + |b| + 3 R^2)"""
    nx, par = app.nx, par_of(app)
    f_dev, f_ref = residual(x_dev, w_dev, dt, nx, par), residual(x_ref, w_ref, dt, nx, par)
    m = margin(app, dt, x_dev, x_ref, w_dev, w_ref)
    R = float(max(np.abs(x_dev).max(), np.abs(np.asarray(w_dev)).max()))
    m_f = 1.0 + dt * (8.0 * max(app.du, app.dv) / app.dx ** 2 + abs(app.a) + abs(app.b) + 3.0 * R * R)
    g, allowed_g = float(np.abs(f_dev).max()), app.newton_tol + e_g(app, dt, R, C_G_DEVICE) + m_f * c_add * EPS * R
    assert g < allowed_g, (what, "exit criterion", g, allowed_g)
    return (norm2(f_dev) + norm2(f_ref)) / m + EPS * float(np.linalg.norm(np.asarray(x_ref, dtype=np.float64))), 1.0 / m, g / allowed_g


def _check_chains(dev, ref, lvl, st, chains, slack, record, what, w=1.0):
    """every row i of every chain (a list of point indices, each row Phi of the row in front; chains of one are stored-state steps)
    against the reference's row: e_k = e_(k-1) / (1 - dt_k mu) + |w| tau_k + SLACK, tau_k measured; then the other rows and lists"""
    app, t, n_g = dev.problem[lvl], np.asarray(ref.t[lvl]), st.get(("g", lvl))
    got, want = dev.backend.natural("u", lvl), _host_state(ref, "u", lvl)
    c_add = 0.0 if (n_g is None and w == 1.0) else 3.0 * (abs(w) + abs(1.0 - w)) / abs(w)
    worst_allowed = slack
    for chain in chains:
        e = 0.0
        for i in chain:
            g_i, old = (None if n_g is None else n_g[i]), st[("u", lvl)][i]
            tau_i, lip, r_g = _measured(app, float(t[i] - t[i - 1]), got[i - 1], _recover(got[i], g_i, old, w), want[i - 1],
                                        _recover(want[i], g_i, old, w), c_add, (what, lvl, i))
            e = lip * e + abs(w) * tau_i + slack
            err = float(np.linalg.norm(got[i] - want[i]))
            assert err <= e, (what, lvl, i, err, e)
            _ratio(record, what, err, e)
            _ratio(record, what + " max|F(x_dev)|", r_g, 1.0)
            worst_allowed = max(worst_allowed, e)
    _compare(dev, ref, lvl, worst_allowed, what)      # (all rows of all lists, the untouched ones included)


def _run_sweeps(dev, ref, w, seed, sweeps, levels=None, record=None):
    """the named sweeps on fresh random states, each against the reference hierarchy"""
    record = {} if record is None else record
    top = dev.lvl_max - 1
    levels = list(range(top)) if levels is None else levels
    seeds = iter(range(seed, seed + 1000))

    def fresh():
        st = _random_states(ref, next(seeds))
        _set_states(dev, ref, st)
        _reset(ref)
        return st

    for lvl in levels:
        if "f_relax" in sweeps:
            st = fresh()
            slack = 8 * EPS * 3 * _row_norm(*st.values())
            dev.f_relax(lvl); ref.f_relax(lvl)
            cpts = [int(i) for i in np.asarray(ref.cpts[lvl])]
            assert cpts[0] == 0 and cpts[-1] == len(ref.t[lvl]) - 1
            _check_chains(dev, ref, lvl, st, [list(range(a + 1, z)) for a, z in zip(cpts[:-1], cpts[1:])], slack, record, "f_relax")
        if "c_relax" in sweeps:
            st = fresh()
            slack = 8 * EPS * 3 * _row_norm(*st.values())
            dev.c_relax(lvl); ref.c_relax(lvl)
            cpts = [int(i) for i in np.asarray(ref.cpts[lvl])]
            _check_chains(dev, ref, lvl, st, [[i] for i in cpts[1:]], slack * (abs(w) + abs(1 - w)), record, f"c_relax w={w}", w)
        if "fas_residual" in sweeps:
            st = fresh()
            slack = 8 * EPS * 3 * _row_norm(*st.values())
            dev.fas_residual(lvl); ref.fas_residual(lvl)
            # (g of the coarse level mixes one Phi of each level: neither is recoverable, the a-priori tau of both)
            allowed = _tol(dev, ref, lvl) + _tol(dev, ref, lvl + 1) + slack
            _ratio(record, "fas_residual", _compare(dev, ref, lvl + 1, allowed, "fas_residual"), allowed)
    if "forward_solve" in sweeps:
        st = fresh()
        dev.forward_solve(top); ref.forward_solve(top)
        uh = _host_state(ref, "u", top)
        _check_chains(dev, ref, top, st, [list(range(1, len(ref.t[top])))], 8 * EPS * 3 * _row_norm(uh, st[("g", top)]), record, "forward_solve")
    if "error_correction" in sweeps:
        for lvl in reversed(levels):
            st = fresh()
            dev.error_correction(lvl); ref.error_correction(lvl)
            allowed = 8 * EPS * 3 * _row_norm(*st.values())
            _ratio(record, "error_correction", _compare(dev, ref, lvl, allowed, "error_correction"), allowed)
    if "compute_residual" in sweeps:
        st = fresh()
        n = ref.problem[0].nx ** 2
        got, want = np.asarray(dev.compute_residual()), np.asarray(ref.compute_residual())
        # (a point's Phi is seen through the norm of Phi - u alone: not recoverable, the a-priori tau)
        allowed = _tol(dev, ref, 0) + 8 * EPS * 3 * _row_norm(st[("u", 0)]) + (2 * n + 2) * EPS * want
        assert got.shape == want.shape and got.size == len(ref.cpts[0]) - 1
        assert np.all(np.abs(got - want) <= allowed), np.abs(got - want).max()
        _ratio(record, "compute_residual", float(np.max(np.abs(got - want) / allowed)), 1.0)
    for lvl in range(dev.lvl_max):
        assert dev.backend.newton_stats(lvl)["at_newton_maxiter"] == 0
    return record


def _run(dev, ref, bounds, w, seed, sweeps, record):
    return _run_sweeps(dev, ref, w, seed, sweeps, record=record)


# ---- every sweep at the edge sizes of the new kernels ------------------------------------------------------------------------------
@pytest.mark.parametrize("nx", [4, 33, 66])
def test_every_sweep_at_the_size_edges(nx):
    """nx = 4: the stencil wraps onto itself, one workgroup per item; 33: odd, 1089 points, no multiple of a wave; 66: past one 64-tile"""
    assert torch.cuda.is_available()

    def check(dev):
        assert dev.problem[0].du == 100 * dev.problem[0].dv and dev.problem[0].device_stepper()["theta"] == 1.0
    both_weights(lambda w: _pair(nx, _uniform((9, 5, 3), 0.5), weight_c=w), None, 100 * nx, 100 * nx + 7, f"size_edges[nx={nx}]",      # coarsest step 0.25
                 check=check, run=_run)


def test_every_sweep_with_equal_diffusion_coefficients():
    """du = dv: with the default du = 100 dv beside it (above), a table or a coefficient taken for the wrong species shows in one of the two"""
    assert torch.cuda.is_available()
    both_weights(lambda w: _pair(20, _uniform((17, 9, 5)), par=PARS["du=dv"], weight_c=w), None, 4242, 4242 + 7, "equal_diffusion[nx=20]", run=_run)


# ---- one observable Phi: the measured tau and the exit criterion -------------------------------------------------------------------
def _check_observable_phi(dev, ref, st, what):
    """level-0 F-relaxation of a coarsening-2 hierarchy done on both sides: every F-point row against the reference's by the measured
    tau, and the exit criterion of the device's row in long double"""
    app, t = dev.problem[0], np.asarray(dev.t[0])
    got, want = dev.backend.natural("u", 0), _host_state(ref, "u", 0)
    worst, worst_g = 0.0, 0.0
    for i in range(1, len(t), 2):
        w_in, dt = st[("u", 0)][i - 1], float(t[i] - t[i - 1])
        err, allowed = float(np.linalg.norm(got[i] - want[i])), tau(app, w_in, dt, got[i], want[i])
        g, allowed_g = exit_criterion(app, w_in.reshape(2, app.nx, app.nx), dt, got[i].reshape(2, app.nx, app.nx), C_G_DEVICE)
        worst, worst_g = max(worst, err / allowed), max(worst_g, g / allowed_g)
        assert err <= allowed, (what, i, err, allowed)
        assert g < allowed_g, (what, i, g, allowed_g)
    print(f"RATIO {what} f_relax, measured tau: worst error/allowed {worst:.4f}")
    print(f"RATIO {what} max|F(x_dev)|: worst value/allowed {worst_g:.4f}")


def test_one_f_relaxation_at_a_larger_grid():
    assert torch.cuda.is_available()
    nx = 129
    dev, ref = _pair(nx, _uniform((5, 3), 2.0 ** -9))      # steps of 2^-11: dt du / dx^2 = 2
    st = _random_states(ref, nx)
    _set_states(dev, ref, st)
    dev.backend.newton_stats(0)
    dev.f_relax(0); ref.f_relax(0)
    stats = dev.backend.newton_stats(0)
    print(f"nx={nx}: {stats}")
    assert stats["phi"] == 2 and stats["at_newton_maxiter"] == 0 and stats["newton_iterations"] >= 2
    _check_observable_phi(dev, ref, st, f"larger_grid[nx={nx}]")


@pytest.mark.parametrize("par", sorted(PARS))
def test_the_exit_criterion_holds_for_the_returned_rows(par):
    assert torch.cuda.is_available()
    dev, ref = _pair(33, _uniform((17, 9, 5)), par=PARS[par])
    st = _random_states(ref, 21)
    _set_states(dev, ref, st)
    dev.backend.newton_stats(0)
    dev.f_relax(0); ref.f_relax(0)
    assert dev.backend.newton_stats(0)["at_newton_maxiter"] == 0
    _check_observable_phi(dev, ref, st, f"exit_criterion[{par}]")


# ---- items that converge at different times in one batch ---------------------------------------------------------------------------
def test_mixed_convergence_in_one_batch():
    """every second C-point of level 0 is the fixed point (u, v) = (1, 0): g = 0 exactly there (the stencil of a constant, a (1 - 1) and
    u * 0 are exact zeros), so those items freeze at their first test and come back bit for bit; the rough ones beside them in the
    same batch are within tau and satisfy their exit criterion"""
    assert torch.cuda.is_available()
    nx = 33
    n = nx * nx
    dev, ref = _pair(nx, _uniform((17, 9, 5)))
    st = _random_states(ref, 5)
    fixed = np.concatenate((np.ones(n), np.zeros(n)))
    st[("u", 0)][0::4] = fixed
    _set_states(dev, ref, st)
    dev.backend.newton_stats(0)
    dev.f_relax(0); ref.f_relax(0)
    stats = dev.backend.newton_stats(0)
    print(f"mixed batch: {stats}")
    _check_observable_phi(dev, ref, st, "mixed_batch")
    got = dev.backend.natural("u", 0)
    for i in range(1, 17, 4):
        assert np.array_equal(got[i], fixed), i
    assert stats["phi"] == 8 and stats["at_newton_maxiter"] == 0
    assert 4 * 2 <= stats["newton_iterations"] <= 4 * 4 and stats["newton_iterations"] <= stats["cg_iterations"] <= 4 * 16
    assert dev.backend.newton_stats(0) == dict(phi=0, newton_iterations=0, cg_iterations=0, at_newton_maxiter=0)      # the call resets


# ---- the result of an item does not depend on its batch ----------------------------------------------------------------------------
def test_an_item_is_the_same_bits_alone_and_among_others():
    from pymgrit_amd import GrayScott, Mgrit
    assert torch.cuda.is_available()
    nx, h = 33, 2.0 ** -4
    rng = np.random.default_rng(11)
    row = np.concatenate((rng.uniform(0.0, 1.0, size=nx * nx), rng.uniform(0.0, 0.5, size=nx * nx)))

    def run(n_fine, n_coarse, at):
        prob = [GrayScott(nx=nx, method="IMPL", linear_solver="bicgstab", t_interval=h * np.arange(0.0, n, s))
                for n, s in ((n_fine, 1.0), (n_fine, 2.0))]
        assert len(prob[1].t) == n_coarse
        mg = Mgrit(prob, nested_iteration=False, logging_lvl=30)
        assert type(mg.backend).__name__ == "HipBackend"
        r2 = np.random.default_rng(12)
        rows = np.concatenate((r2.uniform(0.0, 1.0, size=(n_fine, nx * nx)), r2.uniform(0.0, 0.5, size=(n_fine, nx * nx))), axis=1)
        rows[at] = row
        out = []
        for rep in range(2):
            mg.backend.set_natural("u", 0, rows)
            mg.f_relax(0)
            out.append(mg.backend.natural("u", 0)[at + 1])
        assert np.array_equal(out[0], out[1])      # the same sweep twice: identical bits
        return out[0]

    alone, among = run(3, 2, 0), run(17, 9, 6)
    assert np.abs(alone - row).max() > 1e-3
    assert np.array_equal(alone, among)


# ---- several step sizes per level --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", sorted(RAGGED_GRIDS))
def test_every_sweep_with_several_step_sizes_per_level(grid):
    """batch_make_plans groups a sweep's items by the bit pattern of dt, one [2][P][P] preconditioner table per group; coarsening 4 puts
    the three F-points of one interval into different groups"""
    assert torch.cuda.is_available()

    def check(dev):      # (the ragged grid's largest step is 6.25 units = 0.244)
        for t in dev.t:
            assert distinct_steps(t) >= 3
    both_weights(lambda w: _pair(20, _intervals(RAGGED_GRIDS[grid]), weight_c=w), None, 10000, 10000 + 3, f"step_sizes[{grid}]", check=check, run=_run)


# ---- a dt group larger than the Newton batch cap -----------------------------------------------------------------------------------
def test_sweeps_of_more_than_one_batch():
    """201 points with the exact step 2^-7 (one bit pattern of dt): 100 F-points and 100 relaxed C-points, each ONE dt group = one plan
    of 100 states, which the Newton arm cuts into a batch of GSN_MAX_BATCH = 93 and one of 7 -- the index lists, the sweep's arithmetic
    and the row sums of the residual offset per batch"""
    assert torch.cuda.is_available()
    nx, w = 4, 1.3
    dev, ref = _pair(nx, _intervals(dyadic("grayscott", 201)), weight_c=w)
    assert len(dev.t[0]) == 201 and len(dev.t[1]) == 101
    for groups in dt_groups(dev.t[0]):      # F-points, relaxed C-points
        assert groups == [100] and GSN_MAX_BATCH == 93 and 100 > GSN_MAX_BATCH, groups
    record = _run_sweeps(dev, ref, w, 77, STORED_STATE_SWEEPS, levels=[0])
    _report("batches[dyadic_201]", record)


# ---- iteration caps ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lin_maxiter", [1, 100])
def test_the_caps_equal_the_host_step(lin_maxiter):
    """newton_maxiter = 1 on device and host (``_step_bicgstab``, the same algorithm) from the same rows.
    lin_maxiter = 1: both add delta = alpha y + omega z of one inner iteration and differ by rounding alone, each side within
    (2 (4 nx + 8) + 4 (2 nx^2 + 2) + 16) EPS norm(J) norm_2(delta) of the exact one (test_gray_scott_newton_cpu.py counts it).
    lin_maxiter = 100: both solve J delta = g to norm_2(r) <= lin_tol norm_2(g) for the recurrence residual; each side's delta is within
    (lin_tol norm_2(g) + n_it 4 EPS norm(J) norm_2(delta)) / (1 - dt mu) of J^-1 g, as test_hip_allen_cahn_newton.py derives for CG.
    norm(J) <= 1 + dt (8 du / dx^2 + |a| + |b| + 3 R^2). The fixed point among the rows needs no iteration and is not counted at the cap."""
    from pymgrit_amd import GrayScott, Mgrit
    assert torch.cuda.is_available()
    nx, h = 20, 2.0 ** -3
    n = nx * nx
    grids = [h * np.arange(9.0), h * np.arange(0.0, 9.0, 2.0)]
    caps = dict(newton_maxiter=1, lin_maxiter=lin_maxiter)
    dev = Mgrit([GrayScott(nx=nx, method="IMPL", linear_solver="bicgstab", t_interval=t, **caps) for t in grids], nested_iteration=False, logging_lvl=30)
    assert type(dev.backend).__name__ == "HipBackend"
    rng = np.random.default_rng(3)
    rows = np.concatenate((rng.uniform(0.0, 1.0, size=(9, n)), rng.uniform(0.0, 0.5, size=(9, n))), axis=1)
    rows[4] = np.concatenate((np.ones(n), np.zeros(n)))
    dev.backend.set_natural("u", 0, rows)
    dev.backend.newton_stats(0)
    dev.f_relax(0)
    got, stats = dev.backend.natural("u", 0), dev.backend.newton_stats(0)
    app = dev.problem[0]
    norm_j = 1.0 + h * (8.0 * app.du / app.dx ** 2 + abs(app.a) + abs(app.b) + 3.0)
    m = 1.0 - h * mu(app.a, app.b, 1.05, 0.55)
    worst, n_lin = 0.0, 0
    for i in range(0, 8, 2):
        w_in, counts = rows[i].reshape(2, nx, nx), {}
        x = app._step_bicgstab(w_in, h, counts)
        n_lin += counts["cg_iterations"]
        assert max(np.abs(x[0]).max(), np.abs(got[i + 1][:n]).max()) <= 1.05 and max(np.abs(x[1]).max(), np.abs(got[i + 1][n:]).max()) <= 0.55
        if i == 4:
            assert counts == dict(newton_iterations=0, cg_iterations=0) and np.array_equal(got[5], rows[4])
            continue
        delta, g = np.linalg.norm(x - w_in), np.linalg.norm(np.asarray(residual(w_in, w_in, h, nx, par_of(app)), dtype=np.float64))
        if lin_maxiter == 1:
            allowed = 2 * (2 * (4 * nx + 8) + 4 * (2 * n + 2) + 16) * EPS * norm_j * delta
        else:
            allowed = 2 * (app.lin_tol * g + counts["cg_iterations"] * 4 * EPS * norm_j * delta) / m
        err = float(np.linalg.norm(got[i + 1] - x.ravel()))
        worst = max(worst, err / allowed)
        assert err <= allowed and delta > 1e-3, (i, err, allowed)
    print(f"RATIO caps[lin_maxiter={lin_maxiter}] f_relax against the host step: worst error/allowed {worst:.4f}")
    print(f"caps: {stats}, host inner iterations {n_lin}")
    assert stats["phi"] == 4 and stats["newton_iterations"] == 3 and stats["at_newton_maxiter"] == 3
    # (an item's count may differ by one from the host's where norm_2(r) lands within rounding of the stop value: one per item)
    assert abs(stats["cg_iterations"] - n_lin) <= (0 if lin_maxiter == 1 else 3) and (lin_maxiter > 1 or n_lin == 3)


# ---- solves ------------------------------------------------------------------------------------------------------------------------
def test_solve_matches_the_reference_hierarchy():
    """from the initial guess on (nx = 20, [0, 1], nt 17 / 9 / 5, newton_tol = 1e-12 on the device): the residual histories by
    history_allowance (gray_scott_newton_reference.py)"""
    assert torch.cuda.is_available()
    dev, ref = _pair(20, _uniform((17, 9, 5)), app=dict(newton_tol=1e-12), max_iter=8, tol=1e-9, nested_iteration=True)
    conv, rconv = np.asarray(dev.solve()["conv"]), np.asarray(ref.solve()["conv"])
    u = dev.backend.natural("u", 0)
    assert len(conv) == len(rconv) >= 2 and rconv[-1] < 1e-9, (conv, rconv)
    tau_phi = tau_phi_a_priori(dev.problem[0], 0.25, ref.problem, C_G_DEVICE)
    allowed = history_allowance(ref, rconv, cases.spacetime_norm(u), tau_phi)
    print(f"RATIO solve conv ({len(conv)} iterations): worst deviation/allowed {np.max(np.abs(conv - rconv) / allowed):.4f}")
    assert np.all(np.abs(conv - rconv) <= allowed), (conv, rconv, allowed)
    last = _host_state(ref, "u", 0)[-1]
    assert np.linalg.norm(u[-1] - last) <= len(conv) * np.sqrt(len(ref.t[0])) * tau_phi
    stats = [dev.backend.newton_stats(lvl) for lvl in range(dev.lvl_max)]
    print(f"solve: {stats}")
    assert all(s["at_newton_maxiter"] == 0 and s["phi"] > 0 for s in stats)


def test_an_imex_coarse_level_under_an_impl_bicgstab_level():
    """a hierarchy may mix the two device forms; against the same classes on the plugin path (the host statements of both steps). Both
    sides stop at their own Newton test: tau_phi from both guarantees, on the box (1.05, 0.55), which the final states are asserted in"""
    from pymgrit_amd import GrayScott, Mgrit
    assert torch.cuda.is_available()
    nx = 20

    class HostGrayScott(GrayScott):     # overriding step sends the hierarchy to the plugin path
        def step(self, u_start, t_start, t_stop):
            return super().step(u_start, t_start, t_stop)

    def prob(cls):
        return [cls(nx=nx, method="IMPL", linear_solver="bicgstab", newton_tol=1e-12, t_start=0, t_stop=1.0, nt=33),
                cls(nx=nx, method="IMEX", t_start=0, t_stop=1.0, nt=9)]
    opts = dict(tol=1e-8, max_iter=12, cycle_type="V", nested_iteration=False, logging_lvl=30)
    dev, host = Mgrit(prob(GrayScott), **opts), Mgrit(prob(HostGrayScott), **opts)
    assert type(dev.backend).__name__ == "HipBackend" and type(host.backend).__name__ == "PluginBackend"
    assert "theta" in dev.backend.desc[0] and "theta" not in dev.backend.desc[1]
    conv, hconv = np.asarray(dev.solve()["conv"]), np.asarray(host.solve()["conv"])
    u = dev.backend.natural("u", 0)
    assert len(conv) == len(hconv) < 12 and hconv[-1] < 1e-8, (conv, hconv)
    assert np.abs(u[:, :nx * nx]).max() <= 1.05 and np.abs(u[:, nx * nx:]).max() <= 0.55
    app, dt = dev.problem[0], 1.0 / 32
    tau_phi = 2 * np.sqrt(2.0) * nx * (app.newton_tol + e_g(app, dt, 1.05, 9.5)) / (1.0 - dt * mu(app.a, app.b, 1.05, 0.55)) + EPS * _row_norm(u)
    allowed = history_allowance(host, hconv, cases.spacetime_norm(u), tau_phi)
    print(f"RATIO solve[impl_over_imex] conv: worst deviation/allowed {np.max(np.abs(conv - hconv) / allowed):.4f}")
    assert np.all(np.abs(conv - hconv) <= allowed), (conv, hconv)
    assert dev.backend.newton_stats(0)["at_newton_maxiter"] == 0
    with pytest.raises(Exception, match="not an Allen-Cahn Newton level"):
        dev.backend.newton_stats(1)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_selection_and_refusals():
    from pymgrit_amd import AtMgrit, GrayScott, GridTransfer, Mgrit
    from pymgrit_amd.core.hip_lib import MgritHipError

    def prob(nxs=(12, 12), solver="bicgstab"):
        return [GrayScott(nx=nx, method="IMPL", linear_solver=solver, t_start=0, t_stop=0.5, nt=nt) for nx, nt in zip(nxs, (9, 3))]

    class GridTransferGrayScott(GridTransfer):
        def restriction(self, u):
            return u

        def interpolation(self, u):
            return u
    assert type(Mgrit(prob(), logging_lvl=30).backend).__name__ == "HipBackend"
    assert type(Mgrit(prob(solver="direct"), logging_lvl=30).backend).__name__ == "PluginBackend"
    with pytest.raises(MgritHipError, match="same nx"):
        Mgrit(prob((12, 6)), transfer=[GridTransferGrayScott()], logging_lvl=30)
    with pytest.raises(MgritHipError, match="GridTransferCopy only"):
        Mgrit(prob(), transfer=[GridTransferGrayScott()], logging_lvl=30)
    with pytest.raises(MgritHipError, match="AT-MGRIT is not supported"):
        AtMgrit(k=2, problem=prob(), logging_lvl=30)
    with pytest.raises(MgritHipError, match="global convergence criteria only"):
        Mgrit(prob(), conv_crit=2, logging_lvl=30)


def test_level_entry_point_refuses_bad_arguments():
    """mgrit_hip_level_grayscott2d_newton through raw ctypes: the codes and texts of mgrit_hip_level_grayscott2d, the solver's
    parameters, and what follows from the level's kind"""
    assert torch.cuda.is_available()
    from pymgrit_amd.core import hip_lib
    lib = hip_lib.load()
    EINVAL, EUNSUPPORTED = -1, -4
    gs, cfg, msg = lib.mgrit_hip_level_grayscott2d_newton, lib.mgrit_hip_block_solve_config, lib.mgrit_hip_last_error
    eng = C.c_void_p()
    assert lib.mgrit_hip_create(C.byref(eng), 3, C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    try:
        t9 = np.ascontiguousarray(np.linspace(0.0, 1.0, 9))
        tp, null = C.c_void_p(t9.ctypes.data), C.c_void_p(0)
        ok, sol = (20, 800, 100.0, 1.0, 0.01, 0.09, 0.086), (1e-10, 100, 1e-10, 100)
        assert gs(None, 0, 9, tp, *ok, *sol) < 0 and gs(eng, 5, 9, tp, *ok, *sol) < 0 and gs(eng, -1, 9, tp, *ok, *sol) < 0
        assert gs(eng, 0, 9, tp, 3, 32, 100.0, 1.0, 0.01, 0.09, 0.086, *sol) == EUNSUPPORTED and b"Gray-Scott grid" in msg()
        assert gs(eng, 0, 9, tp, 20, 400, 100.0, 1.0, 0.01, 0.09, 0.086, *sol) == EINVAL and b"2*nx*nx" in msg()
        assert gs(eng, 0, 9, tp, 20, 800, 100.0, 0.0, 0.01, 0.09, 0.086, *sol) == EINVAL and b"Gray-Scott parameters" in msg()
        assert gs(eng, 0, 9, null, *ok, *sol) == EINVAL and gs(eng, 0, -1, tp, *ok, *sol) == EINVAL
        for bad in ((-1e-10, 100, 1e-10, 100), (1e-10, -1, 1e-10, 100), (1e-10, 100, float("nan"), 100), (1e-10, 100, 1e-10, -1)):
            assert gs(eng, 0, 9, tp, *ok, *bad) == EINVAL and b"bad Newton / BiCGStab parameters" in msg(), bad
        out = (C.c_int64 * 4)()
        assert lib.mgrit_hip_newton_stats(eng, 0, out) == EINVAL                                  # no level was made
        assert gs(eng, 0, 9, tp, *ok, *sol) == 0 and gs(eng, 1, 9, tp, *ok, *sol) == 0 and lib.mgrit_hip_level_grayscott2d(eng, 2, 9, tp, *ok) == 0
        assert gs(eng, 0, 9, tp, *ok, *sol) < 0 and b"already" in msg()
        assert lib.mgrit_hip_newton_stats(eng, 0, out) == 0 and list(out) == [0, 0, 0, 0]
        assert lib.mgrit_hip_newton_stats(eng, 2, out) == EINVAL and b"not an Allen-Cahn Newton level" in msg()      # the IMEX level
        # non-linear Phi: no time-parallel forward solve; no spatial transfer joins two such levels, the copy does
        assert cfg(eng, 1, 4, 1, 0, null, null) == EUNSUPPORTED
        assert cfg(eng, 1, -1, 1, 0, null, null) == 0
        assert lib.mgrit_hip_level_transfer(eng, 0, hip_lib.TRANSFER_PERIODIC2D) == EUNSUPPORTED
        assert lib.mgrit_hip_level_transfer(eng, 0, hip_lib.TRANSFER_COPY) == 0
    finally:
        assert lib.mgrit_hip_destroy(eng) == 0
