"""GPU tests of the Cahn-Hilliard IMEX device path against a second implementation of Phi: every sweep of the device hierarchy against the
SAME hierarchy on the plugin path over ``ReferenceCahnHilliard`` (tests/cahn_hilliard_reference.py), whose step is a transform-free solve
of (I + dt (eps^2 Lh^2 - s Lh)) x = u + dt Lh w refined in long double. It shares neither the Hartley table nor the eigenvalues nor the
D tables nor the code of w with the device or the host step, so a mistake common to those two (test_hip_cahn_hilliard.py compares exactly
those two) shows here. The cases are those of test_hip_cahn_hilliard.py (tests/cahn_hilliard_cases.py), whose docstring states the tolerances; here
a Phi is allowed C(nx) EPS bnorm for the device and EPS bnorm for the reference, which asserts its own forward error bound on every call.

  a. the size edges of the tile product: nx = 4 (smallest grid), 33 / 97 (just past a K step of 32), 96 (KP = 96 < P = 128), 129 (just
     past a tile of 64);
  b. several step sizes on one level (the ragged grid of the Allen-Cahn reference test): batch_make_plans groups a sweep's items by the
     bit pattern of dt, one [2][P][P] table per group. Coarsening 4 puts F-points of one interval into different groups;
  c. a dt group of 1025 states: launches of 512, 512 and 1 states, blockIdx.z restarting and the index arrays offset per plan;
  d. one Phi at nx = 256, 257 (P = 256, 320);
  e. constant rows 0, +0.5, -0.5: mode (0, 0) alone, D1 = 1, D2 = 0.
"""
import pytest

from cahn_hilliard_cases import (RAGGED_GRIDS, T_SWEEP, ch_pair as _pair, check_constant_rows, check_one_phi_at_larger_grids, check_several_step_sizes,
                                 check_size_edges, check_split_at_the_batch_cap)
from periodic2d_sweeps import check_history, intervals as _intervals, uniform as _uniform

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.mark.parametrize("nx", [4, 33, 96, 97, 129])
def test_every_sweep_at_the_size_edges(nx):
    assert torch.cuda.is_available()
    check_size_edges("reference", nx)


@pytest.mark.parametrize("nx", [20, 66])
@pytest.mark.parametrize("grid", sorted(RAGGED_GRIDS))
def test_every_sweep_with_several_step_sizes_per_level(grid, nx):
    assert torch.cuda.is_available()
    check_several_step_sizes("reference", grid, nx)


def test_sweeps_split_at_the_batch_cap():
    assert torch.cuda.is_available()
    check_split_at_the_batch_cap("reference")


@pytest.mark.parametrize("nx", [256, 257])
def test_one_phi_at_larger_grids(nx):
    assert torch.cuda.is_available()
    check_one_phi_at_larger_grids("reference", nx)


def test_constant_rows_are_returned():
    assert torch.cuda.is_available()
    check_constant_rows("reference")


def test_solve_matches_the_reference_hierarchy():
    """three iterations from the initial state on the ragged grid (several D tables per sweep): histories by the project's rule"""
    assert torch.cuda.is_available()
    dev, ref = _pair("reference", 20, _intervals(RAGGED_GRIDS["by2_3lvl"]), max_iter=3, tol=0.0)
    check_history(dev, ref, "solve[reference,ragged]", 3)
    dev, ref = _pair("reference", 16, _uniform((17, 9, 5), T_SWEEP), max_iter=3, tol=0.0, cycle_type="F")
    check_history(dev, ref, "solve[reference,F]", 3)
