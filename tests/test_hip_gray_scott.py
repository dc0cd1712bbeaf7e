"""GPU tests of the Gray-Scott IMEX device path (csrc/mgrit_hip_grayscott.inc): every sweep of the device hierarchy
against the SAME hierarchy on the plugin path over ``ReferenceGrayScott`` (tests/gray_scott_reference.py), whose step is a
transform-free solve of (I - dt d_c Lap) x_c = b_c refined in long double. It shares neither the Hartley table nor the eigenvalues nor
the reaction term's code with the device or the host step. States are fresh random, u in [0, 1], v in [0, 0.5]: the planes differ and
are not symmetric in (i, j), so swapped planes, swapped tables or a transposed product miss by orders of magnitude. What the cases are
chosen for:

  a. the size edges of the tile product: nx = 4 (smallest grid), 33 / 97 (just past a K step of 32), 96 (KP = 96 < P = 128), 129 (just
     past a tile of 64); the default du = 100 dv, and one case with du = dv;
  b. several step sizes on one level (nx = 20, 66): batch_make_plans groups a sweep's items by the bit pattern of dt, one pair of D
     tables per group; coarsening 4 puts F-points of one interval into different groups;
  c. a dt group of more than one batch: a launch holds at most H2D_MAX_BATCH = 1024 work slab items = 512 states, so 513 F-points of
     one exact (dyadic) step are a batch of 512 and one of 1, blockIdx.z restarting and the index arrays offset per plan. The test
     asserts the group size it relies on;
  d. one Phi at nx = 256, 257 (P = 256, 320);
  e. the fixed point (u, v) = (1, 0) and a constant state: mode 0, D = 1, Phi = b.

Tolerances, nothing in them measured on the device (test_gray_scott_cpu.py states the per-species bound):
  per Phi:     sqrt(tol_u^2 + tol_v^2),  tol_c = ((4 nx + 8) + 1) EPS bnorm_c  -- (4 nx + 8) EPS bnorm_c for the device's four products
               and pointwise work, EPS bnorm_c for the rounding of the reference to float64; the species are independent solves, a
               state's error is the two combined in quadrature. bnorm_c bounds norm_F(b_c) from the input rows with the level's largest
               dt:  bnorm_u = norm_F(|u| + dt (|a| |1 - u| + |u| v^2)),  bnorm_v = norm_F(|v| + dt (|u| v^2 + |b| |v|)), the largest row;
  + SLACK      8 EPS * 3 * the largest row norm involved, for the sweep's own arithmetic (a handful of additions per value);
  fas_residual: the sum over the two levels;
  chained steps (forward_solve, F-relaxation over 3 F-points): both sides apply Phi to their own previous result, so
               e_k = Lip_k e_(k-1) + the step's per-Phi term + SLACK.  Phi = (solve) o (pointwise map); each solve is a contraction
               (all eigenvalues of I - dt d_c Lap are >= 1), and the pointwise map (u, v) -> (b_u, b_v) has the Jacobian
                   [[1 - dt (a + v^2), -2 dt u v], [dt v^2, 1 + dt (2 u v - b)]],
               whose Frobenius norm bounds its 2-norm at every point. With R = max|state| of the step's input,
                   Lip_k = norm_F([[1 + dt (|a| + R^2), 2 dt R^2], [dt R^2, 1 + dt (2 R^2 + |b|)]]).
Every comparison covers all rows of a list. Each sweep prints its worst error / allowed ("RATIO" lines). Largest ratio of the first
run on an MI355X: see DESIGN.md 3.11.
"""
import types

import numpy as np
import pytest

import cases
from periodic2d_kinds import KINDS, dyadic
from periodic2d_sweeps import (STORED_STATE_SWEEPS, both_weights, bounds_of, check_history, check_jump_criterion, check_level_entry_point,
                               check_one_phi, check_ragged, compare as _compare, dt_groups, intervals as _intervals, pair, report as _report,
                               row_norm as _row_norm, run_sweeps, set_states as _set_states, tol, uniform as _uniform)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

EPS = cases.EPS
KIND = KINDS["grayscott"]
BOUNDS = bounds_of("grayscott", "reference")


def _pair(nx, grids, **opts):
    """(device Mgrit, plugin Mgrit over ReferenceGrayScott) on the same hierarchy"""
    return pair("grayscott", nx, grids, side="reference", **opts)


def _default_ratio(dev):
    assert dev.problem[0].du == 100 * dev.problem[0].dv


# ---- a. every sweep at the size edges of the tile product --------------------------------------------------------------------------
@pytest.mark.parametrize("nx", [4, 33, 96, 97, 129])
def test_every_sweep_at_the_size_edges(nx):
    assert torch.cuda.is_available()
    both_weights(lambda w: _pair(nx, _uniform((17, 9, 5), KIND.t_sweep(nx)), weight_c=w), BOUNDS, 100 * nx, 100 * nx + 7, f"size_edges[nx={nx}]",
                 check=_default_ratio)


def test_every_sweep_with_equal_diffusion_coefficients():
    """du = dv: with the default du = 100 dv beside it (above), a table taken for the wrong species shows in one of the two"""
    assert torch.cuda.is_available()
    nx = 33
    both_weights(lambda w: _pair(nx, _uniform((17, 9, 5), KIND.t_sweep(nx)), par=dict(du=0.5, dv=0.5, a=0.04, b=0.1), weight_c=w), BOUNDS,
                 4242, 4242 + 7, "equal_diffusion[nx=33]")


# ---- b. several step sizes per level -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx", [20, 66])
@pytest.mark.parametrize("grid", ["by2_3lvl", "by4_2lvl"])
def test_every_sweep_with_several_step_sizes_per_level(grid, nx):
    assert torch.cuda.is_available()
    both_weights(lambda w: _pair(nx, _intervals(KIND.ragged(nx)[grid]), weight_c=w), BOUNDS, 500 * nx, 500 * nx + 3, f"step_sizes[{grid},nx={nx}]",
                 check=lambda dev: check_ragged(dev, grid))


# ---- c. a dt group larger than one batch -------------------------------------------------------------------------------------------
def test_sweeps_of_more_than_one_batch():
    """1027 points with the exact step 2^-7 (every t_k = k 2^-7 and every difference is exact: one bit pattern of dt): 513 F-points and
    513 relaxed C-points, each one dt group = a batch of 512 states (1024 work slab items) and a batch of 1"""
    assert torch.cuda.is_available()
    nx, w = 4, 1.3
    dev, ref = _pair(nx, _intervals(dyadic("grayscott", 1027)), weight_c=w)
    assert len(dev.t[0]) == 1027 and len(dev.t[1]) == 514
    for groups in dt_groups(dev.t[0]):      # F-points, relaxed C-points
        assert groups == [513] and 513 > 1024 // 2, groups
    record = run_sweeps(dev, ref, BOUNDS, w, 77, STORED_STATE_SWEEPS, levels=[0])
    _report("batches[dyadic_1027]", record)


# ---- d. one Phi at larger grids ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx", [256, 257])
def test_one_phi_at_larger_grids(nx):
    assert torch.cuda.is_available()
    dev, ref = _pair(nx, _uniform((5, 3), 2.0 ** -9))      # (steps of 2^-11, exact: one factorisation per species; r = 8)
    check_one_phi(dev, ref, BOUNDS, nx, f"larger_grids[nx={nx}]")


# ---- e. the fixed point and a constant state ---------------------------------------------------------------------------------------
def test_fixed_point_and_constant_rows():
    """(u, v) = (1, 0) is a fixed point of the system: b = (1, 0) and mode 0 has D = 1. A constant state (0.5, 0.25): b is constant per
    plane, so Phi = b = (0.5 + dt (a / 2 - 1 / 32), 0.25 + dt (1 / 32 - b / 4))."""
    assert torch.cuda.is_available()
    nx = 33
    dev, ref = _pair(nx, _uniform((17, 9, 5), KIND.t_sweep(nx)))
    app, n, dt = ref.problem[0], nx * nx, float(ref.t[0][1] - ref.t[0][0])
    st = BOUNDS.random_states(ref, 5)
    fixed = np.concatenate((np.ones(n), np.zeros(n)))
    const = np.concatenate((np.full(n, 0.5), np.full(n, 0.25)))
    st[("u", 0)][0::4], st[("u", 0)][2::4] = fixed, const      # C-points 0, 4, .. the fixed point, 2, 6, .. the constant state
    _set_states(dev, ref, st)
    dev.f_relax(0); ref.f_relax(0)
    allowed = tol(BOUNDS, ref, 0, st[("u", 0)][0::2]) + 8 * EPS * 3 * _row_norm(*st.values())
    worst = _compare(dev, ref, 0, allowed, "f_relax, fixed point and constant rows")
    got = dev.backend.natural("u", 0)
    want_const = np.concatenate((np.full(n, 0.5 + dt * (app.a * 0.5 - 0.5 * 0.0625)), np.full(n, 0.25 + dt * (0.5 * 0.0625 - app.b * 0.25))))
    err = max(float(np.max(np.linalg.norm(got[1::4] - fixed, axis=1))), float(np.max(np.linalg.norm(got[3::4] - want_const, axis=1))))
    print(f"RATIO constants f_relax: worst error/allowed {max(worst, err) / allowed:.4f}")
    assert err <= allowed, (err, allowed)
    assert np.array_equal(got[1::4][:, n:], np.zeros_like(got[1::4][:, n:]))      # v = 0 stays 0 exactly


# ---- Mgrit.solve() -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cycle", ["V", "F"])
def test_solve_matches_the_reference_hierarchy(cycle):
    """from the initial guess on (nx = 20, [0, 6], nt 65 / 17 / 5): residual histories by the rule of tests/cases.py"""
    assert torch.cuda.is_available()
    dev, ref = _pair(20, _uniform((65, 17, 5), 6.0), cycle_type=cycle, max_iter=6, tol=1e-9, nested_iteration=True)
    check_history(dev, ref, f"solve[{cycle}]", last_state=False)


def test_jump_criterion_matches_the_reference_hierarchy():
    """conv_crit = 1: the norms of u_i - previous u_i over both planes (h2d_rowsq_kernel<false, 2>), three iterations from the
    initial guess; the same rule as for the residual histories"""
    assert torch.cuda.is_available()
    dev, ref = _pair(20, _uniform((33, 17, 9), 4.0), conv_crit=1, max_iter=3, tol=0.0)
    check_jump_criterion(dev, ref, 3)


# ---- what is refused ---------------------------------------------------------------------------------------------------------------
def test_what_is_not_covered_is_refused():
    from pymgrit_amd import AtMgrit, GrayScott, GridTransfer, GridTransferCopy, Mgrit
    from pymgrit_amd.core.backend_hip import HipBackend
    from pymgrit_amd.core.hip_lib import MgritHipError

    def prob(nxs=(12, 12)):
        return [GrayScott(nx=nx, method="IMEX", t_start=0, t_stop=0.5, nt=nt) for nx, nt in zip(nxs, (9, 3))]

    class GridTransferGrayScott(GridTransfer):      # a spatial coarsening of the user's
        def restriction(self, u):
            return u

        def interpolation(self, u):
            return u
    with pytest.raises(MgritHipError, match="same nx"):
        Mgrit(prob((12, 6)), transfer=[GridTransferGrayScott()], logging_lvl=30)
    with pytest.raises(MgritHipError, match="GridTransferCopy only"):
        Mgrit(prob(), transfer=[GridTransferGrayScott()], logging_lvl=30)
    with pytest.raises(MgritHipError, match="AT-MGRIT is not supported"):
        AtMgrit(k=2, problem=prob(), logging_lvl=30)
    with pytest.raises(MgritHipError, match="global convergence criteria only"):
        Mgrit(prob(), conv_crit=2, logging_lvl=30)
    stub = types.SimpleNamespace(desc=[p.device_stepper() for p in prob()])
    with pytest.raises(MgritHipError, match="one time rank only"):
        HipBackend._check_periodic(stub, types.SimpleNamespace(comm_time_size=2, global_conv_crit=True, transfer_objects=[GridTransferCopy()]), "grayscott2d")
    with pytest.raises(MgritHipError, match="outside"):
        Mgrit([GrayScott(nx=3, method="IMEX", t_start=0, t_stop=0.5, nt=nt) for nt in (9, 3)], logging_lvl=30)
    # the host steppers have no device form: such a hierarchy runs on the plugin path
    for method in ("EXPL", "IMPL"):
        mg = Mgrit([GrayScott(nx=8, method=method, t_start=0, t_stop=0.01, nt=nt) for nt in (9, 3)], logging_lvl=30, max_iter=1)
        assert type(mg.backend).__name__ == "PluginBackend"


def test_level_entry_point_refuses_bad_arguments():
    """mgrit_hip_level_grayscott2d through raw ctypes: negative codes with a message, and what follows from the level's kind"""
    assert torch.cuda.is_available()
    from pymgrit_amd.core import hip_lib
    ok = (20, 800, 100.0, 1.0, 0.01, 0.09, 0.086)

    def transfers(lib, eng, fn, tp, msg):      # no spatial transfer joins two such levels; the copy does
        assert lib.mgrit_hip_level_transfer(eng, 0, hip_lib.TRANSFER_PERIODIC2D) == -4
        assert lib.mgrit_hip_level_transfer(eng, 0, hip_lib.TRANSFER_COPY) == 0
    check_level_entry_point(
        "mgrit_hip_level_grayscott2d", 3, 5, 1.0, ok, small=(3, 32) + ok[2:], large=(2049, 2 * 2049 * 2049 + 14) + ok[2:], large_says_grid=False,
        short=(20, 400) + ok[2:], odd=(20, 808) + ok[2:],      # one plane's worth; not a multiple of 16
        bad=((20, 800, 0.0, 1.0, 0.01, 0.09, 0.086), (20, 800, 100.0, 0.0, 0.01, 0.09, 0.086), (20, 800, 100.0, 1.0, -0.01, 0.09, 0.086),
             (20, 800, 100.0, 1.0, 0.01, float("nan"), 0.086), (20, 800, 100.0, 1.0, 0.01, 0.09, float("inf"))),
        grid_msg=b"Gray-Scott grid", ld_msg=b"2*nx*nx", bad_msg=b"Gray-Scott parameters", describe=[(0, ok), (1, ok)], then=transfers)
