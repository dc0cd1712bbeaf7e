"""GPU tests of the Allen-Cahn IMEX device path against a second implementation of Phi: every sweep of the device hierarchy against the
SAME hierarchy on the plugin path over ``ReferenceAllenCahn`` (tests/allen_cahn_reference.py), whose step is a transform-free solve of
(I - dt L) x = b refined in long double. It shares neither the Hartley table nor the eigenvalues nor the reaction term's code with the
device or the host step, so a mistake common to those two (test_hip_allen_cahn.py compares exactly those two) shows here. What the
cases are chosen for:

  a. the size edges of the tile product: nx = 4 (smallest grid), 33 / 97 (just past a K step of 32), 96 (KP = 96 < P = 128), 129 (just
     past a tile of 64);
  b. exponents nu = 1, 3, 4 in every sweep (odd nu: only sweeps in which every Phi acts on a stored state -- u = -1 is unstable then);
  c. several step sizes on one level: batch_make_plans groups a sweep's items by the bit pattern of dt, one D table and one c = dt / eps^2
     per group. Coarsening 4 puts F-points of one interval into different groups;
  d. sweeps of more than H2D_MAX_BATCH = 1024 items: several launches with blockIdx.z restarting and the index arrays offset per plan.
     A uniform grid given as nt = / linspace holds a dozen bit patterns of dt (the differences k h - (k - 1) h round differently), so no
     group of such a grid reaches 1024 items: the grids that do split are the dyadic ones, whose steps 2^-17 are exact. The test
     asserts the group sizes it relies on;
  e. one Phi at nx = 256, 257 (P = 256, 320);
  f. constant rows 0, +1, -1: mode 0, D = 1, b = u.

Tolerances: those of test_hip_allen_cahn.py with ONE device evaluation instead of two, nothing measured on the device:
  per Phi:     (4 nx + 8) EPS bnorm  (the device)  +  EPS bnorm  (the rounding of the reference to float64),
               bnorm = _b_norm of the input rows with the level's largest c. (For odd nu and negative u, _b_norm is below norm_F(b):
               it takes |u| first, and |u| (1 - |u|^nu) < |u| (1 + |u|^nu). The check is then tighter than derived, never wider.)
  + SLACK      8 EPS * 3 * the largest row norm involved, for the sweep's own arithmetic
  fas_residual: the sum over the two levels;  chained steps (forward_solve, F-relaxation over 3 F-points):
               e_k = Lip_k e_(k-1) + the step's per-Phi term + SLACK, Lip_k as in test_hip_allen_cahn.py.
Every comparison covers all rows of a list. Each sweep prints its worst error / allowed ("RATIO" lines).
"""
import collections
import types

import numpy as np
import pytest

import cases
from allen_cahn_reference import ReferenceAllenCahn
from periodic2d_sweeps import (ALL_SWEEPS, STORED_STATE_SWEEPS, compare as _compare, distinct_steps as _distinct_steps, host_state as _host_state,
                               intervals as _intervals, ratio as _ratio, report as _report, row_norm as _row_norm, run_sweeps,
                               set_states as _set_states, tol, uniform as _uniform)      # (_ratio: for test_hip_heat2d_reference.py)
from test_allen_cahn_cpu import EPS
from test_hip_allen_cahn import T_SWEEP, _b_norm, _random_states

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _pair(nx, grids, nu=2, **opts):
    """(device Mgrit, plugin Mgrit over ReferenceAllenCahn) on the same hierarchy"""
    from pymgrit_amd import AllenCahn, Mgrit
    opts.setdefault("nested_iteration", False)
    dev = Mgrit([AllenCahn(nx=nx, nu=nu, method="IMEX", **g) for g in grids], logging_lvl=30, **opts)
    ref = Mgrit([ReferenceAllenCahn(nx=nx, nu=nu, method="IMEX", **g) for g in grids], logging_lvl=30, **opts)
    assert type(dev.backend).__name__ == "HipBackend" and type(ref.backend).__name__ == "PluginBackend"
    for a, b in zip(dev.t, ref.t):
        assert np.array_equal(a, b)
    return dev, ref


def _phi_term(app, rows, c):
    """one device evaluation and the reference's rounding: (4 nx + 8) EPS bnorm + EPS bnorm"""
    return ((4 * app.nx + 8) + 1) * EPS * _b_norm(app, rows, c)


def _lip(app, c, rows):
    R = float(np.abs(rows).max())
    return max(abs(1 + c), abs(1 + c * (1 - (app.nu + 1) * R ** app.nu)))


# the formulas above take c = dt / eps^2
BOUNDS = types.SimpleNamespace(random_states=_random_states, phi_term=lambda ref, app, rows, dt: _phi_term(app, rows, dt / app.eps ** 2),
                               lip=lambda app, dt, rows: _lip(app, dt / app.eps ** 2, rows), values_per_state=lambda app: app.nx * app.nx,
                               coarse_rows=lambda ref, st, lvl: st[("u", lvl)], weight_in_key=False)


def _tol(ref, lvl, rows):
    return tol(BOUNDS, ref, lvl, rows)


# ---- a. every sweep at the size edges of the tile product --------------------------------------------------------------------------
@pytest.mark.parametrize("nx", [4, 33, 96, 97, 129])
def test_every_sweep_at_the_size_edges(nx):
    assert torch.cuda.is_available()
    record = {}
    for w in (1.0, 1.3):
        dev, ref = _pair(nx, _uniform((17, 9, 5), T_SWEEP), weight_c=w)
        run_sweeps(dev, ref, BOUNDS, w, 100 * nx + (7 if w != 1.0 else 0), ALL_SWEEPS, record=record)
    _report(f"size_edges[nx={nx}]", record)


# ---- b. every sweep for other exponents --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nu", [1, 3, 4])
@pytest.mark.parametrize("nx", [20, 66])
def test_every_sweep_for_other_exponents(nx, nu):
    assert torch.cuda.is_available()
    record = {}
    for w in (1.0, 1.3):
        dev, ref = _pair(nx, _uniform((17, 9, 5), T_SWEEP), nu=nu, weight_c=w)
        assert dev.problem[0].device_stepper()["nu"] == nu
        run_sweeps(dev, ref, BOUNDS, w, 1000 * nx + 10 * nu + (5 if w != 1.0 else 0), ALL_SWEEPS if nu % 2 == 0 else STORED_STATE_SWEEPS, record=record)
    _report(f"exponents[nx={nx},nu={nu}]", record)


# ---- c. several step sizes per level -----------------------------------------------------------------------------------------------
RAGGED = np.concatenate(([0.0], np.cumsum(1e-4 * np.array([1, 1, 1.5, .5, 2, 1, 1, .75, 1, 1, 1, 1.25, 3, 1, 1, 1]))))
RAGGED_GRIDS = {"by2_3lvl": [RAGGED, RAGGED[::2], RAGGED[::4]], "by4_2lvl": [RAGGED, RAGGED[::4]]}


@pytest.mark.parametrize("nu", [2, 4])
@pytest.mark.parametrize("nx", [20, 66])
@pytest.mark.parametrize("grid", sorted(RAGGED_GRIDS))
def test_every_sweep_with_several_step_sizes_per_level(grid, nx, nu):
    assert torch.cuda.is_available()
    record = {}
    for w in (1.0, 1.3):
        dev, ref = _pair(nx, _intervals(RAGGED_GRIDS[grid]), nu=nu, weight_c=w)
        for t in dev.t:
            assert _distinct_steps(t) >= 3 and len(set(np.round(np.diff(t) / 1e-4, 6))) >= 3, np.diff(t)
        if grid == "by4_2lvl":      # the three F-points of one interval do not share one D table (steps 1, 1, 1.5 and 2, 1, 1 of 1e-4)
            assert sum(len(set(np.round(np.diff(dev.t[0][a:a + 4]) / 1e-4, 6))) >= 2 for a in range(0, 16, 4)) >= 2
        run_sweeps(dev, ref, BOUNDS, w, 500 * nx + 10 * nu + (3 if w != 1.0 else 0), ALL_SWEEPS, record=record)
    _report(f"step_sizes[{grid},nx={nx},nu={nu}]", record)


@pytest.mark.parametrize("nu", [2, 4])
@pytest.mark.parametrize("nx", [20, 66])
def test_solve_with_several_step_sizes_per_level(nx, nu):
    """three iterations from the tanh profile on the ragged grid: residual histories by the rule of check_history, the last state to 1e-9"""
    assert torch.cuda.is_available()
    dev, ref = _pair(nx, _intervals(RAGGED_GRIDS["by2_3lvl"]), nu=nu, max_iter=3, tol=0.0)
    for t in dev.t:
        assert _distinct_steps(t) >= 3
    conv, rconv = np.asarray(dev.solve()["conv"]), np.asarray(ref.solve()["conv"])
    u = dev.backend.natural("u", 0)
    norm_u = cases.spacetime_norm(u)
    assert len(conv) == len(rconv) == 3
    dev_ref = np.abs(conv - rconv)
    print(f"RATIO solve[nx={nx},nu={nu}] conv: largest deviation {np.max(dev_ref) / (EPS * norm_u):.2f} units of eps*norm(u) "
          f"(allowed {cases.BLK_K} beyond 1e-10 relative)")
    assert np.all(dev_ref <= 1e-10 * rconv + cases.BLK_K * EPS * norm_u), (conv, rconv)
    last = _host_state(ref, "u", 0)[-1]
    print(f"RATIO solve[nx={nx},nu={nu}] last state: relative deviation {np.abs(u[-1] - last).max() / np.abs(last).max():.3e}")
    assert np.abs(u[-1] - last).max() <= 1e-9 * np.abs(last).max()


# ---- d. sweeps that split into several batches -------------------------------------------------------------------------------------
H = 2.0 ** -17          # 7.6e-6: every t_k = k H and every difference is exact, one bit pattern of dt
BATCH_GRIDS = {
    # as nt = / linspace: a dozen bit patterns of dt per level, the largest group has some 620 items (one launch each)
    "linspace_2051": lambda: _uniform((2051, 1026), 2050e-5),
    "cumsum_2051": lambda: _levels_by2(np.concatenate(([0.0], np.cumsum([1e-5] * 2048 + [2e-5] * 2)))),
    # exact steps: 1025 F-points / C-points of one dt = a batch of 1024 and one of 1
    "dyadic_2051": lambda: _levels_by2(H * np.arange(2051.0)),
    # 2050 steps H, then two steps 2 H: a full batch, a remainder of 1 and a second dt group in one sweep
    "dyadic_2053_two_sizes": lambda: _levels_by2(np.concatenate((H * np.arange(2051.0), H * np.array([2052.0, 2054.0])))),
}
BATCH_GROUPS = {"dyadic_2051": [1025], "dyadic_2053_two_sizes": [1, 1025]}      # sizes of the dt groups among the level-0 F-points


def _levels_by2(t):
    return _intervals([t, t[::2]])


@pytest.mark.parametrize("grid", sorted(BATCH_GRIDS))
def test_sweeps_of_more_than_one_batch(grid):
    assert torch.cuda.is_available()
    nx, w = 9, 1.3
    dev, ref = _pair(nx, BATCH_GRIDS[grid](), weight_c=w)
    t = np.asarray(dev.t[0])
    assert len(t) in (2051, 2053) and len(dev.t[1]) == (len(t) + 1) // 2
    for pts in (np.arange(1, len(t), 2), np.arange(2, len(t), 2)):      # F-points, relaxed C-points
        groups = sorted(collections.Counter((t[pts] - t[pts - 1]).view(np.int64).tolist()).values())
        print(f"{grid}: dt groups of {len(pts)} points: {groups}")
        assert len(pts) >= 1025
        if grid in BATCH_GROUPS:
            assert groups == BATCH_GROUPS[grid], groups
    record = run_sweeps(dev, ref, BOUNDS, w, 77, STORED_STATE_SWEEPS, levels=[0])
    _report(f"batches[{grid}]", record)


# ---- e. one Phi at larger grids ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx", [256, 257])
def test_one_phi_at_larger_grids(nx):
    assert torch.cuda.is_available()
    dev, ref = _pair(nx, _uniform((5, 3), 2.0 ** -9))      # (steps of 2^-11, exact: one factorisation on the reference side)
    st = _random_states(ref, nx)
    _set_states(dev, ref, st)
    dev.f_relax(0); ref.f_relax(0)
    allowed = _tol(ref, 0, st[("u", 0)]) + 8 * EPS * 3 * _row_norm(*st.values())
    worst = _compare(dev, ref, 0, allowed, "f_relax")
    print(f"RATIO larger_grids[nx={nx}] f_relax: worst error/allowed {worst / allowed:.4f}")


# ---- f. constants ------------------------------------------------------------------------------------------------------------------
def test_constant_rows_are_returned():
    """u = 0, +1, -1 (nu = 2): mode 0 with D = 1 and u (1 - u^2) = 0, so Phi(u) = b = u"""
    assert torch.cuda.is_available()
    nx = 33
    dev, ref = _pair(nx, _uniform((17, 9, 5), T_SWEEP))
    st = _random_states(ref, 5)
    const = np.array([0.0, 1.0, -1.0])[(np.arange(17) // 2) % 3]          # the C-point 2 k and the F-point behind it: the same constant
    st[("u", 0)] = np.repeat(const[:, None], nx * nx, axis=1)
    st[("u", 0)][1::2] = 0.5                                               # (what F-relaxation has to overwrite)
    _set_states(dev, ref, st)
    dev.f_relax(0); ref.f_relax(0)
    allowed = _tol(ref, 0, st[("u", 0)][0::2]) + 8 * EPS * 3 * _row_norm(*st.values())
    worst = _compare(dev, ref, 0, allowed, "f_relax, constant rows")
    got = dev.backend.natural("u", 0)
    err = float(np.max(np.linalg.norm(got - const[:, None], axis=1)))
    print(f"RATIO constants f_relax: worst error/allowed {max(worst, err) / allowed:.4f}")
    assert err <= allowed, (err, allowed)
    for i in np.flatnonzero(const == 0.0):
        assert np.array_equal(got[i], np.zeros(nx * nx)), i
