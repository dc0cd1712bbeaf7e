"""The cases test_hip_cahn_hilliard.py (the device path against the host step) and test_hip_cahn_hilliard_reference.py (against the
long-double solve of cahn_hilliard_reference.py) share, each taking the side, "host" or "reference". test_hip_cahn_hilliard.py's
docstring states the tolerances and the parameters. A plain helper like cases.py: no tests, no fixtures."""
import numpy as np

import cases
from periodic2d_kinds import KINDS, dyadic
from periodic2d_sweeps import (STORED_STATE_SWEEPS, both_weights, bounds_of, check_one_phi, check_ragged, compare as _compare, dt_groups,
                               intervals as _intervals, pair, report as _report, row_norm as _row_norm, run_sweeps, set_states as _set_states, tol,
                               uniform as _uniform)

EPS = cases.EPS
KIND = KINDS["cahnhilliard"]
T_SWEEP = KIND.t_sweep(None)
RAGGED_GRIDS = KIND.ragged(None)      # the grid of the Allen-Cahn reference test
BOUNDS = {side: bounds_of("cahnhilliard", side) for side in ("host", "reference")}


def ch_pair(side, nxs, grids, transfer=None, app=None, **opts):
    """(device Mgrit, plugin Mgrit over the side's class) on the same hierarchy; nxs: one nx, or one per level (on one square: L is the
    finest level's nx / 16); app: eps, stab, mean, amplitude other than the table's"""
    return pair("cahnhilliard", nxs, grids, side=side, par=app, transfer=transfer, **opts)


def check_size_edges(side, nx):
    """every sweep with weight_c = 1; C-relaxation, the one sweep the weight enters, with 1.3 as well"""
    both_weights(lambda w: ch_pair(side, nx, _uniform((17, 9, 5), T_SWEEP), weight_c=w), BOUNDS[side], 100 * nx, 100 * nx + 50, f"size_edges[{side},nx={nx}]")


def check_several_step_sizes(side, grid, nx):
    both_weights(lambda w: ch_pair(side, nx, _intervals(RAGGED_GRIDS[grid]), weight_c=w), BOUNDS[side], 500 * nx, 500 * nx + 3,
                 f"step_sizes[{side},{grid},nx={nx}]", check=lambda dev: check_ragged(dev, grid, unit=1e-4))


def check_split_at_the_batch_cap(side):
    """2051 points with the exact step 2^-17: 1025 F-points and 1025 relaxed C-points, each ONE dt group -- a state owns two work slab
    items through the first two products, so a launch holds 512 states: batches of 512, 512 and 1"""
    nx, w = 8, 1.3
    dev, host = ch_pair(side, nx, _intervals(dyadic("cahnhilliard", 2051)), weight_c=w)
    assert len(dev.t[0]) == 2051 and len(dev.t[1]) == 1026
    for groups in dt_groups(dev.t[0]):      # F-points, relaxed C-points
        assert groups == [1025] and 1025 > 2 * 512, groups
    record = run_sweeps(dev, host, BOUNDS[side], w, 77, STORED_STATE_SWEEPS, levels=[0])
    _report(f"batches[{side},dyadic_2051]", record)


def check_one_phi_at_larger_grids(side, nx):
    dev, host = ch_pair(side, nx, _uniform((5, 3), 2.0 ** -9))      # (steps of 2^-11, exact)
    check_one_phi(dev, host, BOUNDS[side], nx, f"larger_grids[{side},nx={nx}]")


def check_constant_rows(side):
    """u = 0, +0.5, -0.5: w is constant, only mode (0, 0) is non-zero, D1 = 1 and D2 = 0 there: Phi(u) = u. Zeros bit for bit"""
    nx = 33
    dev, host = ch_pair(side, nx, _uniform((17, 9, 5), T_SWEEP))
    st = BOUNDS[side].random_states(host, 5)
    const = np.array([0.0, 0.5, -0.5])[(np.arange(17) // 2) % 3]          # the C-point 2 k and the F-point behind it: the same constant
    st[("u", 0)] = np.repeat(const[:, None], nx * nx, axis=1)
    st[("u", 0)][1::2] = 0.25                                              # (what F-relaxation has to overwrite)
    _set_states(dev, host, st)
    dev.f_relax(0); host.f_relax(0)
    allowed = tol(BOUNDS[side], host, 0, st[("u", 0)][0::2]) + 8 * EPS * 3 * _row_norm(*st.values())
    worst = _compare(dev, host, 0, allowed, "f_relax, constant rows")
    got = dev.backend.natural("u", 0)
    err = float(np.max(np.linalg.norm(got - const[:, None], axis=1)))
    print(f"RATIO constants[{side}] f_relax: worst error/allowed {max(worst, err) / allowed:.4f}")
    assert err <= allowed, (err, allowed)
    for i in np.flatnonzero(const == 0.0):
        assert np.array_equal(got[i], np.zeros(nx * nx)), i
