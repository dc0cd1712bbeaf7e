"""GPU tests of the Burgers2D IMEX device path (csrc/mgrit_hip_burgers.inc): every sweep of the device hierarchy against
the SAME hierarchy on the plugin path, over ``HostBurgers2D`` (the numpy statement of the step, Burgers2D.step) and -- one case --
over ``ReferenceBurgers2D`` (tests/burgers_reference.py: the right-hand side in long double, a transform-free refined solve). States
are fresh random, uniform in [-1, 1] in both planes: the planes differ and are not symmetric in (i, j), so swapped planes, swapped
axes of the stencil or a transposed product miss by orders of magnitude. L = nx / 16 (dx = 1 / 16 for every nx), nu = 0.1, sweep grids
nt 17 / 9 / 5 on [0, 0.004]: on the coarsest step dt / dx = 0.016 -- the transport term carries over a percent of the result -- and
8 dt nu / dx^2 = 0.2, both far above the tolerances; r = dt nu / dx^2 <= 50, inside the reference solver's certificate. What the cases
are chosen for:

  a. the size edges: nx = 4 (one tile, KP > nx; with the wrap every neighbour is another rim point), 33 (odd: the v plane is only
     8-byte aligned; pads inside the tile), 66 (two tiles per axis: the wrap and the halo cross a tile border, the last tile is mostly
     pad), 97 (KP = P);
  b. several step sizes on one level (nx = 33), against the host step and against the reference;
  c. a dt group of more than one batch: 513 states = a batch of 512 (1024 work slab items) and a batch of 1 -- blockIdx.z of the
     stencil pass and the work-item index must agree across batches. The test asserts the group size it relies on;
  d. one Phi at nx = 129 (P = 192: three tiles per axis);
  e. a constant state (a fixed point) and a state independent of y with v = 0;
  f. the same bits from a sweep run twice, and from the same state in a batch of 3 and in batches of 512 and 1.

Tolerances, nothing in them measured on the device (test_burgers_cpu.py derives C(nx) = 4 nx + 12 and the majorant):
  per Phi:     device against host 2 C(nx) EPS m (each side C(nx) EPS m), device against reference (C(nx) + 1) EPS m, m the largest
               row majorant, both planes joined in the row norm: m = max over rows of sqrt(m_u^2 + m_v^2),
               m_c = norm_F(|c| + dt inv_2dx (|u| (|c[i+1]| + |c[i-1]|) + |v| (|c[j+1]| + |c[j-1]|)));
  + SLACK      8 EPS * 3 * the largest row norm involved, the harness's, for the sweep's own arithmetic;
  chained steps (forward_solve, F-relaxation over 3 F-points): e_k = Lip_k e_(k-1) + the step's per-Phi term + SLACK with
               Lip_k = 1 + 4 dt R / dx, R the largest |value| of the step's input. Phi = (solve) o (stencil map). The solve contracts
               (all eigenvalues of I - dt nu Lh are >= 1). For two states (u, v), (u', v') in the box |values| <= R with difference
               delta, per plane  u ax_c - u' ax'_c = delta_u ax_c + u' ax_delta  (ax_delta: the x difference of delta_c), likewise
               for v ay_c, so  delta b_c = delta_c - dt (delta_u ax_c + u' ax_delta + delta_v ay_c + v' ay_delta)  with
               |ax_c|, |ay_c| <= R / dx (two values <= R over 2 dx) and norm(ax_delta), norm(ay_delta) <= norm(delta_c) / dx (two
               shifted copies over 2 dx):  norm(delta b_c) <= norm(delta_c) + dt (R / dx) (norm(delta_u) + norm(delta_v) + 2 norm(delta_c)).
               Over both planes, with norm(delta_u) + norm(delta_v) <= sqrt(2) norm(delta) appearing in each of the two:
               norm(delta b) <= (1 + dt (R / dx) (sqrt(2) sqrt(2) + 2)) norm(delta) = (1 + 4 dt R / dx) norm(delta).
Every comparison covers all rows of a list. Each sweep prints its worst error / allowed ("RATIO" lines).
"""
import types

import numpy as np
import pytest

import cases
from periodic2d_kinds import KINDS, dyadic
from periodic2d_sweeps import (STORED_STATE_SWEEPS, both_weights, bounds_of, check_history, check_jump_criterion, check_level_0_twice,
                               check_level_entry_point, check_one_phi, check_ragged, compare as _compare, dt_groups, f_relaxed_rows,
                               intervals as _intervals, pair, report as _report, row_norm as _row_norm, run_sweeps, set_states as _set_states, tol,
                               uniform as _uniform)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

EPS = cases.EPS
KIND = KINDS["burgers"]
T_SWEEP = KIND.t_sweep(None)
BOUNDS = {side: bounds_of("burgers", side) for side in ("host", "reference")}


def _pair(nx, grids, side="host", **opts):
    """(device Mgrit, plugin Mgrit over HostBurgers2D or ReferenceBurgers2D) on the same hierarchy"""
    return pair("burgers", nx, grids, side=side, **opts)


# ---- a. every sweep at the size edges ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx", [4, 33, 66, 97])
def test_every_sweep_at_the_size_edges(nx):
    assert torch.cuda.is_available()

    def check(dev):
        assert dev.problem[0].dx == 1.0 / 16
    both_weights(lambda w: _pair(nx, _uniform((17, 9, 5), T_SWEEP), weight_c=w), BOUNDS["host"], 100 * nx, 100 * nx + 7, f"size_edges[nx={nx}]",
                 check=check)


# ---- b. several step sizes per level -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", ["host", "reference"])
@pytest.mark.parametrize("grid", ["by2_3lvl", "by4_2lvl"])
def test_every_sweep_with_several_step_sizes_per_level(grid, side):
    assert torch.cuda.is_available()
    nx = 33
    both_weights(lambda w: _pair(nx, _intervals(KIND.ragged(nx)[grid]), side=side, weight_c=w), BOUNDS[side], 500 * nx, 500 * nx + 3,
                 f"step_sizes[{grid},{side}]", check=lambda dev: check_ragged(dev, grid))


# ---- c. a dt group larger than one batch -------------------------------------------------------------------------------------------
def test_sweeps_of_more_than_one_batch():
    """1027 points with the exact step 2^-18 (every t_k = k 2^-18 and every difference is exact: one bit pattern of dt; [0, 0.0039]):
    513 F-points and 513 relaxed C-points, each one dt group = a batch of 512 states (1024 work slab items) and a batch of 1"""
    assert torch.cuda.is_available()
    nx, w = 4, 1.3
    dev, ref = _pair(nx, _intervals(dyadic("burgers", 1027)), weight_c=w)
    assert len(dev.t[0]) == 1027 and len(dev.t[1]) == 514
    for groups in dt_groups(dev.t[0]):      # F-points, relaxed C-points
        assert groups == [513] and 513 > 1024 // 2, groups
    record = run_sweeps(dev, ref, BOUNDS["host"], w, 77, STORED_STATE_SWEEPS, levels=[0])
    _report("batches[dyadic_1027]", record)


# ---- d. one Phi at a larger grid ---------------------------------------------------------------------------------------------------
def test_one_phi_at_a_larger_grid():
    assert torch.cuda.is_available()
    nx = 129
    dev, ref = _pair(nx, _uniform((5, 3), 2.0 ** -8))      # (steps of 2^-10, exact)
    check_one_phi(dev, ref, BOUNDS["host"], nx, f"larger_grid[nx={nx}]")


# ---- e. the fixed point and the y-independent state ----------------------------------------------------------------------------------
def test_constant_and_y_independent_rows():
    """C-points 0, 4, ..: the constant state (0.75, -1.25), a fixed point of Phi (b = c exactly, mode 0 has D = 1), which must come
    back within the per-Phi term. C-points 2, 6, ..: u = f(x), v = 0 -- compared with the host step of that same state like every
    other row, and v must stay 0 exactly (b_v = 0 exactly, the products of zeros are zeros). Swapped axes make the second state's
    result depend on y and move the first one's transport term to the other difference; swapped planes give a non-zero v."""
    assert torch.cuda.is_available()
    nx = 33
    dev, ref = _pair(nx, _uniform((17, 9, 5), T_SWEEP))
    n = nx * nx
    st = BOUNDS["host"].random_states(ref, 5)
    const = np.concatenate((np.full(n, 0.75), np.full(n, -1.25)))
    f = np.random.default_rng(11).uniform(-1.0, 1.0, size=nx)
    yind = np.concatenate((np.repeat(f, nx), np.zeros(n)))      # u[i][j] = f[i]: axis 0 is x
    st[("u", 0)][0::4], st[("u", 0)][2::4] = const, yind
    _set_states(dev, ref, st)
    dev.f_relax(0); ref.f_relax(0)
    allowed = tol(BOUNDS["host"], ref, 0, st[("u", 0)][0::2]) + 8 * EPS * 3 * _row_norm(*st.values())
    worst = _compare(dev, ref, 0, allowed, "f_relax, constant and y-independent rows")
    got = dev.backend.natural("u", 0)
    err = float(np.max(np.linalg.norm(got[1::4] - const, axis=1)))
    print(f"RATIO constants f_relax: worst error/allowed {max(worst, err) / allowed:.4f}")
    assert err <= allowed, (err, allowed)
    after = got[3::4]
    assert np.array_equal(after[:, n:], np.zeros_like(after[:, n:]))      # v = 0 stays 0 exactly
    u_after = after[:, :n].reshape(-1, nx, nx)
    assert float(np.max(np.abs(u_after - u_after[:, :, :1]))) <= allowed      # and u stays independent of y
    assert float(np.max(np.abs(u_after[:, :, 0] - f))) > 1e3 * allowed        # while the step moved it


# ---- f. the same bits ----------------------------------------------------------------------------------------------------------------
def test_a_sweep_run_twice_gives_the_same_bits():
    assert torch.cuda.is_available()
    dev, ref = _pair(33, _uniform((17, 9, 5), T_SWEEP))
    check_level_0_twice(dev, ref, BOUNDS["host"].random_states(ref, 21))


def test_a_rows_bits_do_not_depend_on_its_batch():
    """the same state behind the step 2^-18 as one of 3 F-points (one batch of 3) and as the first and the last of 513 (the batch of
    512 and the batch of 1): the same row, bit for bit"""
    assert torch.cuda.is_available()
    nx = 4
    big, ref_big = _pair(nx, _intervals(dyadic("burgers", 1027)))
    small, ref_small = _pair(nx, _intervals(dyadic("burgers", 7)))
    state = np.random.default_rng(3).uniform(-1.0, 1.0, size=2 * nx * nx)
    rows = {name: f_relaxed_rows(dev, ref, BOUNDS["host"].random_states(ref, 9), state, at)
            for name, dev, ref, at in (("small", small, ref_small, (0,)), ("big", big, ref_big, (0, 1024)))}
    assert torch.equal(rows["small"][0], rows["big"][0]) and torch.equal(rows["small"][0], rows["big"][1])
    assert not torch.equal(rows["small"][0][:2 * nx * nx], torch.from_numpy(state).to(rows["small"][0].device))


# ---- Mgrit.solve() -----------------------------------------------------------------------------------------------------------------
SOLVE = dict(par=dict(nu=0.05, L=1.0))


def _solve_grids():
    return _uniform((17, 9, 5), 0.25)


@pytest.mark.parametrize("cycle", ["V", "F"])
def test_solve_matches_the_plugin_path(cycle):
    """from the initial guess on (nx = 12, nu = 0.05, [0, 0.25], nt 17 / 9 / 5): residual histories by the rule of tests/cases.py"""
    assert torch.cuda.is_available()
    dev, ref = _pair(12, _solve_grids(), cycle_type=cycle, max_iter=6, tol=1e-10, nested_iteration=True, **SOLVE)
    check_history(dev, ref, f"solve[{cycle}]", last_state=False)


def test_jump_criterion_matches_the_plugin_path():
    """conv_crit = 1: the norms of u_i - previous u_i over both planes, three iterations from the initial guess; the same rule"""
    assert torch.cuda.is_available()
    dev, ref = _pair(12, _solve_grids(), conv_crit=1, max_iter=3, tol=0.0, **SOLVE)
    check_jump_criterion(dev, ref, 2)


# ---- what is refused ---------------------------------------------------------------------------------------------------------------
def test_what_is_not_covered_is_refused():
    from pymgrit_amd import AtMgrit, Burgers2D, GrayScott, GridTransfer, GridTransferCopy, Mgrit
    from pymgrit_amd.core.backend_hip import HipBackend
    from pymgrit_amd.core.hip_lib import MgritHipError
    name = "Burgers levels on the HIP engine"

    def prob(nxs=(12, 12)):
        return [Burgers2D(nx=nx, t_start=0, t_stop=0.25, nt=nt) for nx, nt in zip(nxs, (9, 3))]

    class GridTransferBurgers(GridTransfer):      # a spatial coarsening of the user's
        def restriction(self, u):
            return u

        def interpolation(self, u):
            return u
    with pytest.raises(MgritHipError, match=name + ".*same nx"):
        Mgrit(prob((12, 6)), transfer=[GridTransferBurgers()], logging_lvl=30)
    with pytest.raises(MgritHipError, match=name + ": GridTransferCopy only"):
        Mgrit(prob(), transfer=[GridTransferBurgers()], logging_lvl=30)
    with pytest.raises(MgritHipError, match=name + ": AT-MGRIT is not supported"):
        AtMgrit(k=2, problem=prob(), logging_lvl=30)
    with pytest.raises(MgritHipError, match=name + ": the global convergence criteria only"):
        Mgrit(prob(), conv_crit=2, logging_lvl=30)
    stub = types.SimpleNamespace(desc=[p.device_stepper() for p in prob()])
    one_rank = types.SimpleNamespace(comm_time_size=1, global_conv_crit=True, transfer_objects=[GridTransferCopy()])
    with pytest.raises(MgritHipError, match=name + ": one time rank only"):
        HipBackend._check_periodic(stub, types.SimpleNamespace(comm_time_size=2, global_conv_crit=True, transfer_objects=[GridTransferCopy()]), "burgers2d")
    mixed = types.SimpleNamespace(desc=[prob()[0].device_stepper(), GrayScott(nx=12, method="IMEX", t_start=0, t_stop=0.25, nt=3).device_stepper()])
    with pytest.raises(MgritHipError, match=name + ": every level of the hierarchy must be a Burgers2D application"):
        HipBackend._check_periodic(mixed, one_rank, "burgers2d")
    with pytest.raises(MgritHipError, match="levels on the HIP engine: every level of the hierarchy must be"):
        Mgrit([prob()[0], GrayScott(nx=12, method="IMEX", t_start=0, t_stop=0.25, nt=3)], logging_lvl=30)
    HipBackend._check_periodic(stub, one_rank, "burgers2d")      # (and what is covered passes the same check)


def test_level_entry_point_refuses_bad_arguments():
    """mgrit_hip_level_burgers2d through raw ctypes: negative codes with a message, and what follows from the level's kind"""
    assert torch.cuda.is_available()
    from pymgrit_amd.core import hip_lib
    ok = (20, 800, 256.0, 8.0, 0.1)      # nx, ld, 1 / dx^2, 1 / (2 dx), nu

    def transfers(lib, eng, fn, tp, msg):      # no spatial transfer joins two such levels; the copy does
        assert lib.mgrit_hip_level_transfer(eng, 0, hip_lib.TRANSFER_PERIODIC2D) == -4
        assert lib.mgrit_hip_level_transfer(eng, 0, hip_lib.TRANSFER_COPY) == 0
    check_level_entry_point(
        "mgrit_hip_level_burgers2d", 3, 5, 0.01, ok, small=(3, 32) + ok[2:], large=(2049, 2 * 2049 * 2049 + 14) + ok[2:],
        short=(20, 400) + ok[2:], odd=(20, 808) + ok[2:],      # one plane's worth; not a multiple of 16
        bad=((20, 800, 256.0, 8.0, 0.0), (20, 800, 256.0, 8.0, -0.1), (20, 800, 256.0, 8.0, float("nan")), (20, 800, 256.0, 8.0, float("inf")),
             (20, 800, 0.0, 8.0, 0.1), (20, 800, 256.0, 0.0, 0.1), (20, 800, 256.0, float("inf"), 0.1)),
        grid_msg=b"Burgers grid", ld_msg=b"2*nx*nx", bad_msg=b"Burgers parameters", describe=[(0, ok), (1, ok)], then=transfers)
