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
import numpy as np
import pytest

from periodic2d_kinds import AC_BATCH_GRIDS as BATCH_GRIDS, AC_BATCH_GROUPS as BATCH_GROUPS, KINDS
from periodic2d_sweeps import (ALL_SWEEPS, EPS, STORED_STATE_SWEEPS, both_weights, bounds_of, check_history, check_one_phi, check_ragged,
                               compare as _compare, distinct_steps as _distinct_steps, dt_groups, intervals as _intervals, pair, report as _report,
                               row_norm as _row_norm, run_sweeps, set_states as _set_states, tol, uniform as _uniform)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

T_SWEEP = KINDS["allencahn"].t_sweep(None)
RAGGED_GRIDS = KINDS["allencahn"].ragged(None)
BOUNDS = bounds_of("allencahn", "reference")      # (the formulas of the module docstring take c = dt / eps^2)


def _pair(nx, grids, nu=2, **opts):
    """(device Mgrit, plugin Mgrit over ReferenceAllenCahn) on the same hierarchy"""
    return pair("allencahn", nx, grids, side="reference", par=dict(nu=nu), **opts)


# ---- a. every sweep at the size edges of the tile product --------------------------------------------------------------------------
@pytest.mark.parametrize("nx", [4, 33, 96, 97, 129])
def test_every_sweep_at_the_size_edges(nx):
    assert torch.cuda.is_available()
    both_weights(lambda w: _pair(nx, _uniform((17, 9, 5), T_SWEEP), weight_c=w), BOUNDS, 100 * nx, 100 * nx + 7, f"size_edges[nx={nx}]",
                 sweeps13=ALL_SWEEPS)


# ---- b. every sweep for other exponents --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nu", [1, 3, 4])
@pytest.mark.parametrize("nx", [20, 66])
def test_every_sweep_for_other_exponents(nx, nu):
    assert torch.cuda.is_available()
    sweeps = ALL_SWEEPS if nu % 2 == 0 else STORED_STATE_SWEEPS

    def check(dev):
        assert dev.problem[0].device_stepper()["nu"] == nu
    both_weights(lambda w: _pair(nx, _uniform((17, 9, 5), T_SWEEP), nu=nu, weight_c=w), BOUNDS, 1000 * nx + 10 * nu, 1000 * nx + 10 * nu + 5,
                 f"exponents[nx={nx},nu={nu}]", sweeps=sweeps, sweeps13=sweeps, check=check)


# ---- c. several step sizes per level -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nu", [2, 4])
@pytest.mark.parametrize("nx", [20, 66])
@pytest.mark.parametrize("grid", sorted(RAGGED_GRIDS))
def test_every_sweep_with_several_step_sizes_per_level(grid, nx, nu):
    assert torch.cuda.is_available()
    both_weights(lambda w: _pair(nx, _intervals(RAGGED_GRIDS[grid]), nu=nu, weight_c=w), BOUNDS, 500 * nx + 10 * nu, 500 * nx + 10 * nu + 3,
                 f"step_sizes[{grid},nx={nx},nu={nu}]", sweeps13=ALL_SWEEPS, check=lambda dev: check_ragged(dev, grid, unit=1e-4))


@pytest.mark.parametrize("nu", [2, 4])
@pytest.mark.parametrize("nx", [20, 66])
def test_solve_with_several_step_sizes_per_level(nx, nu):
    """three iterations from the tanh profile on the ragged grid: residual histories by the rule of check_history, the last state to 1e-9"""
    assert torch.cuda.is_available()
    dev, ref = _pair(nx, _intervals(RAGGED_GRIDS["by2_3lvl"]), nu=nu, max_iter=3, tol=0.0)
    for t in dev.t:
        assert _distinct_steps(t) >= 3
    check_history(dev, ref, f"solve[nx={nx},nu={nu}]", 3)


# ---- d. sweeps that split into several batches -------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", sorted(BATCH_GRIDS))
def test_sweeps_of_more_than_one_batch(grid):
    assert torch.cuda.is_available()
    nx, w = 9, 1.3
    dev, ref = _pair(nx, BATCH_GRIDS[grid](), weight_c=w)
    t = np.asarray(dev.t[0])
    assert len(t) in (2051, 2053) and len(dev.t[1]) == (len(t) + 1) // 2
    for groups in dt_groups(t):      # F-points, relaxed C-points
        print(f"{grid}: dt groups of {sum(groups)} points: {groups}")
        assert sum(groups) >= 1025
        if grid in BATCH_GROUPS:
            assert groups == BATCH_GROUPS[grid], groups
    record = run_sweeps(dev, ref, BOUNDS, w, 77, STORED_STATE_SWEEPS, levels=[0])
    _report(f"batches[{grid}]", record)


# ---- e. one Phi at larger grids ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx", [256, 257])
def test_one_phi_at_larger_grids(nx):
    assert torch.cuda.is_available()
    dev, ref = _pair(nx, _uniform((5, 3), 2.0 ** -9))      # (steps of 2^-11, exact: one factorisation on the reference side)
    check_one_phi(dev, ref, BOUNDS, nx, f"larger_grids[nx={nx}]")


# ---- f. constants ------------------------------------------------------------------------------------------------------------------
def test_constant_rows_are_returned():
    """u = 0, +1, -1 (nu = 2): mode 0 with D = 1 and u (1 - u^2) = 0, so Phi(u) = b = u"""
    assert torch.cuda.is_available()
    nx = 33
    dev, ref = _pair(nx, _uniform((17, 9, 5), T_SWEEP))
    st = BOUNDS.random_states(ref, 5)
    const = np.array([0.0, 1.0, -1.0])[(np.arange(17) // 2) % 3]          # the C-point 2 k and the F-point behind it: the same constant
    st[("u", 0)] = np.repeat(const[:, None], nx * nx, axis=1)
    st[("u", 0)][1::2] = 0.5                                               # (what F-relaxation has to overwrite)
    _set_states(dev, ref, st)
    dev.f_relax(0); ref.f_relax(0)
    allowed = tol(BOUNDS, ref, 0, st[("u", 0)][0::2]) + 8 * EPS * 3 * _row_norm(*st.values())
    worst = _compare(dev, ref, 0, allowed, "f_relax, constant rows")
    got = dev.backend.natural("u", 0)
    err = float(np.max(np.linalg.norm(got - const[:, None], axis=1)))
    print(f"RATIO constants f_relax: worst error/allowed {max(worst, err) / allowed:.4f}")
    assert err <= allowed, (err, allowed)
    for i in np.flatnonzero(const == 0.0):
        assert np.array_equal(got[i], np.zeros(nx * nx)), i
