"""GPU tests of the Allen-Cahn Newton-PCG device path (methods IMPL and CN with linear_solver='pcg'; DESIGN.md 3.9, acn_* in
csrc/mgrit_hip_allencahn.inc): every sweep of the device hierarchy against the SAME hierarchy on the plugin path over
``ReferenceAllenCahnNewton`` (tests/allen_cahn_newton_reference.py), whose step solves the non-linear system in long double with
corrections from a sparse LU -- no table, no ``space_disc``, none of the steppers' code.

Allowance per device Phi, nothing of it measured on the device. With fac = theta dt, m = 1 - fac / eps^2 (the strong-monotonicity
constant of F(x) = x - fac (L x + r(x) / eps^2) - rhs: forward error <= norm_2(F) / m), R the largest |value| of the input rows:

  tau = (nx newton_tol + E_g) / m + EPS norm_2(x)

  * nx newton_tol: the device stops at max|g| < newton_tol for ITS g, and norm_2 <= nx norm_inf on nx^2 values;
  * EPS norm_2(x): the reference (allen_cahn_newton_reference.py derives it);
  * E_g = C_G EPS M norm_2(x), M = 1 + 8 fac nx^2 + fac (1 + R^nu) / eps^2: the rounding of the device's own g in the 2-norm. M bounds
    the sum of the magnitudes of the terms of g per unit of |x| (x itself; the stencil, whose five terms sum to at most 8 |x| / dx^2;
    the reaction |x| (1 + |x|^nu) / eps^2). Operation count of acn_residual_kernel per value, half an EPS each, every one on a
    quantity of magnitude <= M |x|: stencil 3 additions, the subtraction of 4 x and the scaling by 1 / dx^2 (5 roundings: 2.5 EPS);
    reaction nu - 1 multiplications for the power, 1 - p and x (1 - p) (nu + 1 roundings: (nu + 1) / 2 EPS); the two fma's and the
    subtraction of rhs (3 roundings: 1.5 EPS); and 2 EPS for the parameters the device receives rounded to float64 (1 / dx^2, 1 / eps^2,
    each a division: relative EPS, where the reference forms them in long double):  C_G = 6 + (nu + 1) / 2.
    CN evaluates its right-hand side once with the same kernel: E_g twice.
  * norm_2(x): IMPL  <= norm_2(u) / m  (take the inner product of F(x) = 0 with x: x . r(x) <= norm_2(x)^2, x . (-L x) >= 0);
               CN    <= M norm_2(u) / m  (the same with norm_2(rhs) <= M norm_2(u)).

Sweeps: SLACK = 8 EPS * 3 * the largest row norm involved for the sweep's own arithmetic, chained steps (forward_solve, F-points of one
interval) e_k = Lip e_(k-1) + tau + SLACK, Lip = (1 + (1 - theta) / theta * fac / eps^2) / (1 - fac / eps^2), as test_hip_allen_cahn_reference.py
does for IMEX. Every comparison covers all rows of a list. Each sweep prints its worst error / allowed ("RATIO" lines).
"""
import ctypes as C
import types

import numpy as np
import pytest

import allen_cahn_fixtures
import cases
from allen_cahn_fixtures import EPS, apply_step, check_history
from allen_cahn_newton_reference import residual
from periodic2d_kinds import KINDS, TWO_SIZES
from periodic2d_sweeps import (ALL_SWEEPS, both_weights, check_one_phi, distinct_steps, dt_groups, host_class, intervals as _intervals, pair,
                               compare as _compare, random_states, report as _report, row_norm as _row_norm, run_sweeps, set_states as _set_states, tol,
                               uniform as _uniform)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

META = cases.load_json("allen_cahn_newton.json")
ARR = np.load(cases.GOLDEN + "/allen_cahn_newton.npz")
THETA = {"IMPL": 1.0, "CN": 0.5}
T_SWEEP = KINDS["allencahn"].t_sweep(None)
RAGGED_GRIDS = KINDS["allencahn"].ragged(None)      # largest step 6e-4: fac / eps^2 <= 0.375


def _pair(nx, grids, method, nu=2, app=None, **opts):
    """(device Mgrit, plugin Mgrit over ReferenceAllenCahnNewton) on the same hierarchy"""
    return pair("allencahn", nx, grids, side="reference", newton=True, par=dict(nu=nu, method=method), dev_par=app, **opts)


def _random_states(ref, seed):
    return random_states("allencahn", ref, seed)


def _c_g(nu):
    return 6 + (nu + 1) / 2


def _terms(app, dt, rows):
    """(m, M, bound of norm_2(x), E_g) of one Phi with the step dt for inputs among rows"""
    theta = THETA[app.method]
    fac = theta * dt
    m = 1.0 - fac / app.eps ** 2
    R = float(np.abs(rows).max())
    M = 1.0 + 8.0 * fac * app.nx ** 2 + fac * (1.0 + R ** app.nu) / app.eps ** 2
    x_norm = (1.0 if theta == 1.0 else M) * _row_norm(rows) / m
    return m, M, x_norm, _c_g(app.nu) * EPS * M * x_norm


def _tau(app, dt, rows):
    m, _, x_norm, e_g = _terms(app, dt, rows)
    return (app.nx * app.newton_tol + (1 if app.method == "IMPL" else 2) * e_g) / m + EPS * x_norm


def _lip(app, dt):
    theta = THETA[app.method]
    c = theta * dt / app.eps ** 2
    return (1.0 + (1.0 - theta) / theta * c) / (1.0 - c)


def _no_item_at_newton_maxiter(dev):
    for lvl in range(dev.lvl_max):
        assert dev.backend.newton_stats(lvl)["at_newton_maxiter"] == 0


BOUNDS = types.SimpleNamespace(random_states=_random_states, phi_term=lambda ref, app, rows, dt: _tau(app, dt, rows),
                               lip=lambda app, dt, rows: _lip(app, dt), values_per_state=lambda app: app.nx * app.nx,
                               coarse_rows=lambda ref, st, lvl: st[("u", lvl)], weight_in_key=False, after=_no_item_at_newton_maxiter)


# ---- every sweep at the edge sizes of the new kernels ------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["IMPL", "CN"])
@pytest.mark.parametrize("nx,nu", [(4, 2), (33, 2), (66, 2), (20, 4)])
def test_every_sweep_at_the_size_edges(nx, nu, method):
    """nx = 4: the stencil wraps onto itself; 33: odd, 1089 values, no multiple of a wave; 66: past one 64-tile; nu = 4 at nx = 20"""
    assert torch.cuda.is_available()

    def check(dev):
        d = dev.problem[0].device_stepper()
        assert d["theta"] == THETA[method] and d["nu"] == nu
    both_weights(lambda w: _pair(nx, _uniform((17, 9, 5), T_SWEEP), method, nu=nu, weight_c=w), BOUNDS, 100 * nx, 100 * nx + 7,
                 f"size_edges[nx={nx},nu={nu},{method}]", sweeps13=ALL_SWEEPS, check=check)


def test_one_f_relaxation_at_a_larger_grid():
    assert torch.cuda.is_available()
    nx = 129
    dev, ref = _pair(nx, _uniform((5, 3), 2.0 ** -9), "IMPL")      # steps of 2^-11: fac / eps^2 = 0.31
    check_one_phi(dev, ref, BOUNDS, nx, f"larger_grid[nx={nx}]")
    stats = dev.backend.newton_stats(0)
    print(f"nx={nx}: {stats}")
    assert stats["phi"] == 2 and stats["at_newton_maxiter"] == 0 and stats["newton_iterations"] >= 2


# ---- items that converge at different times in one batch ---------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["IMPL", "CN"])
def test_mixed_convergence_in_one_batch(method):
    """level-0 rows alternate constants 0, +1, -1 with random rows: g = 0 exactly for a constant (the stencil of a constant and
    c (1 - c^2) are exact zeros), so those items freeze at the first test and come back bit for bit; the random ones are within tau"""
    assert torch.cuda.is_available()
    nx = 33
    dev, ref = _pair(nx, _uniform((17, 9, 5), T_SWEEP), method)
    st = _random_states(ref, 5)
    const = np.array([0.0, 1.0, -1.0])[np.arange(17) % 3]
    is_const = (np.arange(17) // 2) % 2 == 0                       # C-point 2 k and the F-point behind it: constant for even k
    for i in range(17):
        if is_const[i]:
            st[("u", 0)][i] = const[i - i % 2]
    st[("u", 0)][1::2] += 0.25                                     # (what F-relaxation has to overwrite)
    _set_states(dev, ref, st)
    dev.backend.newton_stats(0)
    dev.f_relax(0); ref.f_relax(0)
    allowed = tol(BOUNDS, ref, 0, st[("u", 0)][0::2]) + 8 * EPS * 3 * _row_norm(*st.values())
    worst = _compare(dev, ref, 0, allowed, "f_relax, mixed batch")
    print(f"RATIO mixed_batch[{method}] f_relax: worst error/allowed {worst / allowed:.4f}")
    got = dev.backend.natural("u", 0)
    n_const = 0
    for i in range(1, 17, 2):
        if is_const[i]:
            assert np.array_equal(got[i], np.full(nx * nx, const[i - 1])), i
            n_const += 1
    stats = dev.backend.newton_stats(0)
    print(f"mixed batch: {stats}")
    assert n_const == 4 and stats["phi"] == 8 and stats["at_newton_maxiter"] == 0
    assert stats["newton_iterations"] >= 4 and stats["cg_iterations"] >= stats["newton_iterations"]


# ---- the result of an item does not depend on its batch ----------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["IMPL", "CN"])
def test_an_item_is_the_same_bits_alone_and_among_others(method):
    from pymgrit_amd import AllenCahn, Mgrit
    assert torch.cuda.is_available()
    nx, h = 33, 2.0 ** -13
    rng = np.random.default_rng(11)
    row = rng.uniform(-1.0, 1.0, size=nx * nx)

    def run(n_fine, n_coarse, at):
        prob = [AllenCahn(nx=nx, method=method, linear_solver="pcg", t_interval=h * np.arange(0.0, n, s))
                for n, s in ((n_fine, 1.0), (n_fine, 2.0))]
        assert len(prob[1].t) == n_coarse
        mg = Mgrit(prob, nested_iteration=False, logging_lvl=30)
        assert type(mg.backend).__name__ == "HipBackend"
        rows = np.random.default_rng(12).uniform(-1.0, 1.0, size=(n_fine, nx * nx))
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
@pytest.mark.parametrize("method", ["IMPL", "CN"])
@pytest.mark.parametrize("grid", sorted(RAGGED_GRIDS))
def test_every_sweep_with_several_step_sizes_per_level(grid, method):
    assert torch.cuda.is_available()
    nx = 20

    def check(dev):
        for t in dev.t:
            assert distinct_steps(t) >= 3
            assert THETA[method] * np.max(np.diff(t)) / 0.04 ** 2 < 1.0
    both_weights(lambda w: _pair(nx, _intervals(RAGGED_GRIDS[grid]), method, weight_c=w), BOUNDS, 500 * nx, 500 * nx + 3,
                 f"step_sizes[{grid},{method}]", sweeps13=ALL_SWEEPS, check=check)


# ---- sweeps of more than H2D_MAX_BATCH items ---------------------------------------------------------------------------------------
def test_sweeps_of_more_than_one_batch():
    """2050 steps H, then two steps 2 H: a dt group of 1025 items (a plan of 1024 and one of 1, each cut into Newton batches) and a
    second group of 1 in one sweep"""
    assert torch.cuda.is_available()
    nx, w = 9, 1.3
    dev, ref = _pair(nx, _intervals([TWO_SIZES, TWO_SIZES[::2]]), "IMPL", weight_c=w)
    assert len(dev.t[0]) == 2053 and len(dev.t[1]) == 1027
    for groups in dt_groups(dev.t[0]):      # F-points, relaxed C-points
        assert sum(groups) >= 1025 and groups == [1, 1025], groups
    dev.backend.newton_stats(0)
    record = run_sweeps(dev, ref, BOUNDS, w, 77, ("f_relax",), levels=[0])
    assert dev.backend.newton_stats(0)["phi"] == 0      # (run_sweeps has read the counts: the call resets them)
    run_sweeps(dev, ref, BOUNDS, w, 78, ("c_relax", "fas_residual", "compute_residual"), levels=[0], record=record)
    _report("batches[dyadic_2053_two_sizes]", record)


# ---- iteration caps ----------------------------------------------------------------------------------------------------------------
def test_newton_maxiter_2_is_counted_and_equals_the_host_step():
    """The one place host pcg step and device are compared directly: both run exactly two Newton updates on items that need more.
    Per Newton update both sides solve J delta = g by CG to norm_2(r) <= lin_tol norm_2(g) for the recurrence residual r; the true
    residual is off by at most 4 EPS norm(J) norm_2(delta) per CG iteration (the rounding of one product with J and of the two
    vector updates), so each side's delta is within (lin_tol norm_2(g) + n_cg 4 EPS norm(J) norm_2(delta)) / m of the exact one,
    norm(J) <= M' = 1 + 8 fac nx^2 + fac (nu + 1) R^nu / eps^2, m = 1 - fac / eps^2, plus E_g / m for the two evaluations of g:
        e_lin = 2 (lin_tol norm_2(g) + lin_maxiter 4 EPS M' norm_2(delta) + E_g) / m.
    A difference e of the first iterates reaches the second through the Newton map x - J(x)^-1 F(x), whose derivative is
    J^-1 (dJ/dx) delta: K = fac nu (nu + 1) R^(nu - 1) / eps^2 * max|delta_2| / m.   e_2 = K e_1 + e_lin,2."""
    from pymgrit_amd import AllenCahn, Mgrit
    assert torch.cuda.is_available()
    nx, h = 20, 2.0 ** -12
    grids = [h * np.arange(17.0), h * np.arange(0.0, 17.0, 2.0)]
    caps = dict(newton_maxiter=2)
    dev = Mgrit([AllenCahn(nx=nx, method="IMPL", linear_solver="pcg", t_interval=t, **caps) for t in grids], nested_iteration=False, logging_lvl=30)
    assert type(dev.backend).__name__ == "HipBackend"
    rows = np.random.default_rng(3).uniform(-1.0, 1.0, size=(17, nx * nx))
    rows[4] = 1.0                                                   # one item that needs no iteration at all
    dev.backend.set_natural("u", 0, rows)
    dev.backend.newton_stats(0)
    dev.f_relax(0)
    got, stats = dev.backend.natural("u", 0), dev.backend.newton_stats(0)
    app = dev.problem[0]
    one = AllenCahn(nx=nx, method="IMPL", linear_solver="pcg", newton_maxiter=1, t_interval=grids[0])
    fac, inv = h, 1.0 / app.eps ** 2
    m = 1.0 - fac * inv
    worst, capped = 0.0, 0
    for i in range(0, 16, 2):
        u = rows[i].reshape(nx, nx)
        x1, x2 = apply_step(one, u, h), apply_step(app, u, h)
        g1 = np.abs(np.asarray(residual(x1, u, h, 1.0, nx, 2, app.eps), dtype=np.float64)).max()
        assert g1 > 2 * app.newton_tol or g1 < 0.5 * app.newton_tol      # (no item sits at the threshold of the second test)
        capped += g1 > 2 * app.newton_tol
        R = float(max(np.abs(u).max(), np.abs(x1).max(), np.abs(x2).max()))
        M_j = 1.0 + 8.0 * fac * nx ** 2 + fac * 3.0 * R ** 2 * inv
        e_g = _terms(app, h, rows[i])[3]
        e = 0.0
        for a, b in ((u, x1), (x1, x2)):
            g = np.asarray(residual(a, u, h, 1.0, nx, 2, app.eps), dtype=np.float64)
            delta = b - a
            K = fac * 6.0 * R * inv * float(np.abs(delta).max()) / m
            e = K * e + 2.0 * (app.lin_tol * np.linalg.norm(g) + app.lin_maxiter * 4 * EPS * M_j * np.linalg.norm(delta) + e_g) / m
        err = float(np.linalg.norm(got[i + 1] - x2.ravel()))
        worst = max(worst, err / e if e > 0 else 0.0)
        assert err <= e, (i, err, e)
    print(f"RATIO newton_maxiter_2 f_relax against the host step: worst error/allowed {worst:.4f}")
    print(f"newton_maxiter = 2: {stats}, expected at the cap {capped}")
    assert np.array_equal(got[5], np.ones(nx * nx))
    assert capped >= 6 and stats["at_newton_maxiter"] == capped and stats["phi"] == 8 and stats["newton_iterations"] <= 14


# ---- the stopping test really holds ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["IMPL", "CN"])
def test_the_exit_criterion_holds_for_the_returned_rows(method):
    """g of every returned row, evaluated here in long double: max|g| <= newton_tol + E_g_inf, E_g_inf = C_G EPS M max|x| -- the
    pointwise form of E_g (module docstring), twice for CN whose right-hand side the device has rounded as well"""
    assert torch.cuda.is_available()
    nx = 33
    dev, ref = _pair(nx, _uniform((17, 9, 5), T_SWEEP), method)
    st = _random_states(ref, 21)
    _set_states(dev, ref, st)
    dev.backend.newton_stats(0)
    dev.f_relax(0)
    got, app, t = dev.backend.natural("u", 0), dev.problem[0], dev.t[0]
    assert dev.backend.newton_stats(0)["at_newton_maxiter"] == 0
    worst = 0.0
    for i in range(1, 17, 2):
        dt = float(t[i] - t[i - 1])
        g = residual(got[i], st[("u", 0)][i - 1], dt, THETA[method], nx, app.nu, app.eps)
        M = _terms(app, dt, np.vstack((st[("u", 0)][i - 1], got[i])))[1]
        big = float(max(np.abs(got[i]).max(), np.abs(st[("u", 0)][i - 1]).max()))
        allowed = app.newton_tol + (1 if method == "IMPL" else 2) * _c_g(app.nu) * EPS * M * big
        worst = max(worst, float(np.abs(g).max()) / allowed)
        assert float(np.abs(g).max()) <= allowed, (i, float(np.abs(g).max()), allowed)
    print(f"RATIO exit_criterion[{method}] max|g|: worst value/allowed {worst:.4f}")


# ---- solves ------------------------------------------------------------------------------------------------------------------------
SOLVES = {**META["solve"], "impl_2lvl_V": allen_cahn_fixtures.META["solve"]["impl_2lvl_V"]}


@pytest.mark.parametrize("name", sorted(SOLVES))
def test_solves_match_the_reference_histories(name):
    from pymgrit_amd import AllenCahn, Mgrit
    assert torch.cuda.is_available()
    rec = SOLVES[name]
    last = (ARR if name in META["solve"] else allen_cahn_fixtures.ARR)["last_" + name].ravel()
    prob = [AllenCahn(nx=rec["nx"], method=rec["method"], linear_solver="pcg", t_start=0, t_stop=META["t_stop"], nt=nt) for nt in rec["nts"]]
    dev = Mgrit(prob, logging_lvl=30, **rec["opts"])
    assert type(dev.backend).__name__ == "HipBackend"
    conv = dev.solve()["conv"]
    u = dev.backend.natural("u", 0)
    check_history(name, conv, cases.spacetime_norm(u), ref=rec["conv"])
    print(f"RATIO solve[{name}] last state: relative deviation {np.abs(u[-1] - last).max() / np.abs(last).max():.3e} (allowed 1e-9)")
    assert np.abs(u[-1] - last).max() <= 1e-9 * np.abs(last).max()
    stats = [dev.backend.newton_stats(lvl) for lvl in range(dev.lvl_max)]
    print(f"{name}: {stats}")
    assert all(s["at_newton_maxiter"] == 0 and s["phi"] > 0 for s in stats)


def test_an_imex_coarse_level_under_an_impl_fine_level():
    from pymgrit_amd import AllenCahn, Mgrit
    assert torch.cuda.is_available()

    HostAllenCahn = host_class(AllenCahn)

    def prob(cls):
        return [cls(nx=32, method="IMPL", linear_solver="pcg", t_start=0, t_stop=META["t_stop"], nt=33),
                cls(nx=32, method="IMEX", t_start=0, t_stop=META["t_stop"], nt=9)]
    opts = dict(tol=1e-8, max_iter=12, cycle_type="V", nested_iteration=False, logging_lvl=30)
    dev, host = Mgrit(prob(AllenCahn), **opts), Mgrit(prob(HostAllenCahn), **opts)
    assert type(dev.backend).__name__ == "HipBackend" and type(host.backend).__name__ == "PluginBackend"
    conv, hconv = np.asarray(dev.solve()["conv"]), np.asarray(host.solve()["conv"])
    u = dev.backend.natural("u", 0)
    norm_u = cases.spacetime_norm(u)
    assert len(conv) == len(hconv)
    d = np.abs(conv - hconv)
    print(f"RATIO solve[impl_over_imex] conv: largest deviation {np.max(d) / (EPS * norm_u):.2f} units of eps*norm(u) (allowed {cases.BLK_K} beyond 1e-10 relative)")
    assert np.all(d <= 1e-10 * hconv + cases.BLK_K * EPS * norm_u), (conv, hconv)
    last = np.asarray(host.u[0][-1].get_values()).ravel()
    assert np.abs(u[-1] - last).max() <= 1e-9 * np.abs(last).max()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_what_is_not_covered_is_refused():
    from pymgrit_amd import AllenCahn, AtMgrit, Mgrit
    from pymgrit_amd.core import hip_lib
    from pymgrit_amd.core.backend_hip import HipBackend
    from pymgrit_amd.core.hip_lib import MgritHipError

    def prob():
        return [AllenCahn(nx=12, method="IMPL", linear_solver="pcg", t_start=0, t_stop=0.002, nt=nt) for nt in (9, 3)]
    with pytest.raises(MgritHipError, match="AT-MGRIT is not supported"):
        AtMgrit(k=2, problem=prob(), logging_lvl=30)
    with pytest.raises(MgritHipError, match="global convergence criteria only"):
        Mgrit(prob(), conv_crit=2, logging_lvl=30)
    stub = types.SimpleNamespace(desc=[p.device_stepper() for p in prob()])
    with pytest.raises(MgritHipError, match="one time rank only"):
        HipBackend._check_periodic(stub, types.SimpleNamespace(comm_time_size=2, global_conv_crit=True), "allencahn2d")
    # the raw ABI: a step with theta dt / eps^2 >= 1, an odd nu, another theta
    lib = hip_lib.load()
    eng = C.c_void_p()
    assert lib.mgrit_hip_create(C.byref(eng), 1, C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    try:
        t = np.array([0.0, 1e-3, 3e-3])
        ptr = C.c_void_p(t.ctypes.data)
        args = (eng, 0, 3, ptr, 12, 144, 144.0, 625.0)
        EINVAL = -1
        assert lib.mgrit_hip_level_allencahn2d_newton(*args, 2, 1.0, 1e-12, 100, 1e-12, 100) == EINVAL      # 2e-3 * 625 = 1.25
        assert b"dt <" in lib.mgrit_hip_last_error()
        assert lib.mgrit_hip_level_allencahn2d_newton(*args, 3, 0.5, 1e-12, 100, 1e-12, 100) == EINVAL
        assert lib.mgrit_hip_level_allencahn2d_newton(*args, 2, 0.0, 1e-12, 100, 1e-12, 100) == EINVAL
        out = (C.c_int64 * 4)()
        assert lib.mgrit_hip_newton_stats(eng, 0, out) == EINVAL                                              # no level was made
        assert lib.mgrit_hip_level_allencahn2d_newton(*args, 2, 0.5, 1e-12, 100, 1e-12, 100) == 0             # CN: 1e-3 * 625 < 1
        assert lib.mgrit_hip_newton_stats(eng, 0, out) == 0 and list(out) == [0, 0, 0, 0]
    finally:
        assert lib.mgrit_hip_destroy(eng) == 0
