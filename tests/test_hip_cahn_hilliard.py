"""GPU tests of the Cahn-Hilliard IMEX stepper (csrc/mgrit_hip_cahnhilliard.inc, p2d_combine_kernel): every sweep of the device path
against the SAME hierarchy on the plugin path over the host ``step`` -- the same formula in numpy, so a mistake common to both does not
show here; tests/test_hip_cahn_hilliard_reference.py holds the device path against the transform-free long-double solve of
tests/cahn_hilliard_reference.py with the machinery of this file. Then solves, the jump criterion, a spatially coarsened hierarchy,
the mass, and everything that is refused.

Tolerances, none measured on the device (cahn_hilliard_reference.py derives C(nx) = 4 nx + 36 and bnorm):
  per Phi, one evaluation:          norm_F(error) <= C(nx) EPS bnorm,   bnorm = norm_F(u) + d2max norm_F(|u|^3 + (1 + s) |u|) of the
                                    input rows, d2max = max over the modes of dt mu / (1 + dt (eps^2 mu^2 + s mu)) at the level's LARGEST
                                    dt (D2 grows with dt)
  host and device, two evaluations: twice that;   device and reference: C(nx) EPS bnorm + EPS bnorm (the reference's asserted error)
  SLACK:                            8 EPS * 3 * the largest row norm involved, for the sweep's own arithmetic (done on both sides)
  chained steps (forward_solve, F-relaxation over several F-points): e_k <= Lip_k e_(k-1) + the step's per-Phi term + SLACK,
                                    Lip_k <= 1 + d2max_k max|3 u^2 - (1 + s)| over |u| <= R, R the largest |value| of the step's input
                                    (the u path is a contraction, |D1| <= 1; the w path has the Lipschitz constant of w times d2max)
Every comparison covers all rows of a list. Each sweep prints its worst error / allowed ("RATIO" lines).

Parameters. Random states in [-1, 1]. The grid spacing is held at dx = 1 / 16 (L = nx / 16) with eps = 0.1 and stab = 2, so that
absrow(A) = 1 + dt (64 eps^2 / dx^4 + 8 s / dx^2) = 1 + 4.6e4 dt stays near 25 at the coarsest step 5e-4 for every nx: inside the
range in which the reference certifies its own error (cahn_hilliard_reference.py), while D2 reaches 0.09 -- the w path carries a tenth
of the result, six orders above the tolerances.
"""
import types

import numpy as np
import pytest

import cases
from cahn_hilliard_reference import b_norm, c_of
from cahn_hilliard_cases import (BOUNDS, RAGGED_GRIDS, T_SWEEP, ch_pair as _pair, check_constant_rows, check_one_phi_at_larger_grids, check_several_step_sizes,
                                 check_size_edges, check_split_at_the_batch_cap)
from periodic2d_sweeps import (ALL_SWEEPS, check_every_sweep_twice, check_history, check_level_entry_point, intervals as _intervals, report as _report,
                               row_norm as _row_norm, run_sweeps, uniform as _uniform)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

EPS = cases.EPS


# ---- against the host step ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx", [4, 33, 96, 97, 129])
def test_every_sweep_at_the_size_edges(nx):
    """nx = 4 (smallest grid), 33 / 97 (just past a K step of 32), 96 (KP = 96 < P = 128), 129 (just past a tile of 64)"""
    assert torch.cuda.is_available()
    check_size_edges("host", nx)


@pytest.mark.parametrize("nx", [20, 66])
@pytest.mark.parametrize("grid", sorted(RAGGED_GRIDS))
def test_every_sweep_with_several_step_sizes_per_level(grid, nx):
    assert torch.cuda.is_available()
    check_several_step_sizes("host", grid, nx)


def test_sweeps_split_at_the_batch_cap():
    assert torch.cuda.is_available()
    check_split_at_the_batch_cap("host")


@pytest.mark.parametrize("nx", [256, 257])
def test_one_phi_at_larger_grids(nx):
    assert torch.cuda.is_available()
    check_one_phi_at_larger_grids("host", nx)


def test_constant_rows_are_returned():
    assert torch.cuda.is_available()
    check_constant_rows("host")


@pytest.mark.parametrize("nx", [20, 97])
def test_a_sweep_run_twice_gives_the_same_bits(nx):
    """a race in the staging of the two items or in the combine product's two passes through LDS would show here"""
    assert torch.cuda.is_available()
    dev, host = _pair("host", nx, _uniform((17, 9, 5), T_SWEEP), weight_c=1.3)
    check_every_sweep_twice(dev, BOUNDS["host"].random_states(host, nx))


@pytest.mark.parametrize("cycle", ["V", "F"])
def test_solves_match_the_plugin_path(cycle):
    """three iterations from the initial state, copy transfer, nt = 17 / 9 / 5, on the default square (L = 1, nx = 16, eps = 0.05)"""
    assert torch.cuda.is_available()
    dev, host = _pair("host", 16, _uniform((17, 9, 5), 0.01), app=dict(eps=0.05), cycle_type=cycle, max_iter=3, tol=0.0)
    check_history(dev, host, f"solve[{cycle}]", 3)


def test_jump_criterion_matches_the_plugin_path():
    """conv_crit = 1: the norms of u_i - previous u_i (h2d_rowsq_kernel<false>), three iterations; the same rule"""
    assert torch.cuda.is_available()
    dev, host = _pair("host", 16, _uniform((17, 9, 5), 0.01), app=dict(eps=0.05), conv_crit=1, max_iter=3, tol=0.0)
    check_history(dev, host, "solve[jump]", 3)


def test_spatially_coarsened_hierarchy():
    """nx = 16 -> 8 with GridTransferCahnHilliard (the periodic 2-D transfer kernels between two Cahn-Hilliard levels): the sweeps, and
    three iterations by the rule of the residual histories. Such a hierarchy converges slowly (eps is fixed while dx doubles)."""
    from pymgrit_amd import GridTransferCahnHilliard
    assert torch.cuda.is_available()
    record = {}
    for w in (1.0, 1.3):
        dev, host = _pair("host", (16, 8), _uniform((17, 9), T_SWEEP), transfer=[GridTransferCahnHilliard()], weight_c=w)
        assert dev.backend._device_transfer(0) and dev.problem[1].dx == 2 * dev.problem[0].dx
        run_sweeps(dev, host, BOUNDS["host"], w, 900 + (3 if w != 1.0 else 0), ALL_SWEEPS, record=record)
    _report("coarsened[16->8]", record)
    dev, host = _pair("host", (16, 8), _uniform((17, 9), 0.01), transfer=[GridTransferCahnHilliard()], app=dict(eps=0.05), max_iter=3, tol=0.0)
    check_history(dev, host, "solve[16->8]", 3)


def test_a_users_transfer_runs_through_its_python_methods():
    """a user's GridTransfer between two Cahn-Hilliard levels: the caller route, exactly as for Allen-Cahn levels"""
    from pymgrit_amd import GridTransfer, GridTransferCahnHilliard
    assert torch.cuda.is_available()

    class Mine(GridTransfer):
        def __init__(self):
            super().__init__()
            self.inner = GridTransferCahnHilliard()

        def restriction(self, u):
            return self.inner.restriction(u)

        def interpolation(self, u):
            return self.inner.interpolation(u)
    t = 2.0 ** -11 * np.arange(17.0)      # (exact steps: the caller route takes one time-step size per level, as for Allen-Cahn)
    dev, host = _pair("host", (16, 8), _intervals([t, t[::2]]), transfer=[Mine()], app=dict(eps=0.05), max_iter=2, tol=0.0)
    assert not dev.backend._device_transfer(0)
    check_history(dev, host, "solve[user transfer]", 2)


def test_mass_after_a_device_solve():
    """|mean(u_i) - mean(u_0)| <= i * (per-Phi bound) / nx: every state of the solution is at most i Phis from u_0 (the C-points through
    the coarse levels' steps, whose bound at their larger dt is the one used), and norm_F / nx bounds the mean of a grid"""
    assert torch.cuda.is_available()
    nx = 16
    dev, host = _pair("host", nx, _uniform((17, 9, 5), 0.01), app=dict(eps=0.05, mean=0.2), max_iter=3, tol=0.0)
    dev.solve()
    u = dev.backend.natural("u", 0)
    per_phi = max(c_of(nx) * EPS * b_norm(host.problem[lvl], u, float(np.max(np.diff(host.t[lvl])))) for lvl in range(3)) + 8 * EPS * 3 * _row_norm(u)
    drift = np.abs(u.mean(axis=1) - u[0].mean())
    print(f"RATIO mass: largest drift {drift.max():.3e}, allowed at the last point {16 * per_phi / nx:.3e}")
    assert abs(u[0].mean() - 0.2) <= 4 * EPS
    assert np.all(drift <= np.arange(17) * per_phi / nx), drift


# ---- what is refused ---------------------------------------------------------------------------------------------------------------
def test_what_is_not_covered_is_refused():
    from pymgrit_amd import AllenCahn, AtMgrit, CahnHilliard, GridTransferAllenCahn, GridTransferCahnHilliard, Mgrit
    from pymgrit_amd.core.backend_hip import HipBackend
    from pymgrit_amd.core.hip_lib import MgritHipError

    def prob(nxs=(12, 12)):
        return [CahnHilliard(nx=nx, t_start=0, t_stop=0.002, nt=nt) for nx, nt in zip(nxs, (9, 3))]
    with pytest.raises(MgritHipError, match="AT-MGRIT is not supported"):
        AtMgrit(k=2, problem=prob(), logging_lvl=30)
    with pytest.raises(MgritHipError, match="Cahn-Hilliard levels on the HIP engine: the global convergence criteria only"):
        Mgrit(prob(), conv_crit=2, logging_lvl=30)
    stub = types.SimpleNamespace(desc=[p.device_stepper() for p in prob()])
    with pytest.raises(MgritHipError, match="Cahn-Hilliard levels on the HIP engine: one time rank only"):
        HipBackend._check_periodic(stub, types.SimpleNamespace(comm_time_size=2, global_conv_crit=True), "cahnhilliard2d")
    with pytest.raises(Exception, match="nx=3"):
        CahnHilliard(nx=3, t_start=0, t_stop=0.002, nt=9)
    # a hierarchy that mixes Cahn-Hilliard and Allen-Cahn levels: by name, in either order
    mixed = [prob()[0], AllenCahn(nx=12, method="IMEX", t_start=0, t_stop=0.002, nt=3)]
    for levels in (mixed, [AllenCahn(nx=12, method="IMEX", t_start=0, t_stop=0.002, nt=9), prob()[1]]):
        with pytest.raises(MgritHipError, match="every level of the hierarchy must be"):
            Mgrit(levels, logging_lvl=30)
    assert GridTransferAllenCahn().device_transfer() == GridTransferCahnHilliard().device_transfer()


def test_level_entry_point_refuses_bad_arguments():
    """mgrit_hip_level_cahnhilliard2d through raw ctypes: negative codes with a message, and what follows from the level's kind"""
    assert torch.cuda.is_available()
    from pymgrit_amd.core import hip_lib
    EINVAL, EUNSUPPORTED = -1, -4
    ok = (20, 400, 400.0, 0.0025, 2.0)

    def transfers(lib, eng, ch, tp, msg):
        # the periodic transfer joins two Cahn-Hilliard levels with n_fine = 2 n_coarse, and the copy joins equal ones
        assert lib.mgrit_hip_level_transfer(eng, 0, hip_lib.TRANSFER_PERIODIC2D) == 0
        assert lib.mgrit_hip_level_transfer(eng, 0, hip_lib.TRANSFER_COPY) == EINVAL and b"equal DOFs" in msg()
        assert ch(eng, 2, 9, tp, 12, 144, 144.0, 0.0025, 2.0) == 0
        assert lib.mgrit_hip_level_transfer(eng, 1, hip_lib.TRANSFER_PERIODIC2D) == EINVAL and b"n_fine = 2*n_coarse" in msg()
        # never a Cahn-Hilliard level with an Allen-Cahn level, in either order: the refusal of the other pairings, verbatim
        assert lib.mgrit_hip_level_allencahn2d(eng, 3, 9, tp, 8, 64, 64.0, 625.0, 2) == 0 and ch(eng, 4, 9, tp, 4, 16, 16.0, 0.0025, 2.0) == 0
        for lvl in (2, 3):      # Cahn-Hilliard 12 over Allen-Cahn 8 (the kind is looked at first), Allen-Cahn 8 over Cahn-Hilliard 4
            assert lib.mgrit_hip_level_transfer(eng, lvl, hip_lib.TRANSFER_PERIODIC2D) == EUNSUPPORTED
            assert b"the periodic 2-D transfer joins two Allen-Cahn levels" in msg()
        assert lib.mgrit_hip_level_transfer(eng, 2, hip_lib.TRANSFER_HEAT2D) == EUNSUPPORTED
    check_level_entry_point(
        "mgrit_hip_level_cahnhilliard2d", 5, 6, 1e-3, ok, small=(3, 16, 9.0, 0.0025, 2.0), large=(2049, 2049 * 2049 + 15) + ok[2:], large_says_grid=False,
        short=(20, 384) + ok[2:], odd=(20, 408) + ok[2:],      # shorter than a state; not a multiple of 16
        bad=((20, 400, 0.0, 0.0025, 2.0), (20, 400, 400.0, 0.0, 2.0), (20, 400, 400.0, -1.0, 2.0), (20, 400, 400.0, 0.0025, -0.5),
             (20, 400, float("inf"), 0.0025, 2.0), (20, 400, 400.0, float("nan"), 2.0), (20, 400, 400.0, float("inf"), 2.0),
             (20, 400, 400.0, 0.0025, float("nan")), (20, 400, 400.0, 0.0025, float("inf"))),
        grid_msg=b"Cahn-Hilliard grid", ld_msg=b"nx*nx", bad_msg=b"bad Cahn-Hilliard parameters",
        describe=[(0, ok), (1, (10, 112, 100.0, 0.0025, 0.0))], then=transfers)      # (stab = 0 is allowed)
