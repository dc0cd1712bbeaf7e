"""GPU tests of the NavierStokes2D IMEX device path (csrc/mgrit_hip_navierstokes.inc): every sweep of the device hierarchy
against the SAME hierarchy on the plugin path, over ``HostNavierStokes2D`` (the numpy statement of the step, NavierStokes2D.step) and --
one case -- over ``ReferenceNavierStokes2D`` (tests/navier_stokes_reference.py: a transform-free bordered solve for the stream function,
the stencil in long double, a transform-free refined diffusion solve). States are fresh random vorticities, uniform in [-1, 1]: not
symmetric in (i, j), so swapped axes of the stencil, a wrong sign of the Jacobian or a transposed product miss by orders of magnitude
(test_navier_stokes_cpu.py asserts the condition from the reference's numbers: the transport term is 1e9 relative tolerances).
L = nx / 16 (dx = 1 / 16 for every nx), nu = 0.1, sweep grids nt 17 / 9 / 5 on [0, 0.004]: steps 2.5e-4 .. 1e-3, r = dt nu / dx^2 <= 50,
inside the reference solver's certificate. What the cases are chosen for:

  a. the size edges: nx = 4 (one tile, KP > nx; with the wrap every neighbour is another rim point), 33 (odd: a grid row is only 8-byte
     aligned; pads inside the tile), 66 (two tiles per axis: the wrap and the halo cross a tile border, and the psi item wraps at nx = 66
     inside its leading dimension P = 128), 97 (KP = P);
  b. several step sizes on one level (nx = 33), against the host step and against the reference;
  c. a dt group of more than one batch. A state owns ONE work slab item, so a launch holds 1024 states: 1025 states are a full batch and
     a batch of one -- blockIdx.z of the stencil pass and the work-item index must agree across batches. 513 states (the split point of
     the two-item kinds) are one batch here; both run. The test asserts the group size it relies on;
  d. one Phi at nx = 129 (P = 192: three tiles per axis);
  e. the known answers: a constant state (a fixed point), Taylor-Green (J = 0, decays by the discrete factor), a state depending on y only;
  f. the same bits from a sweep run twice;
  g. the same bits from the same state in a batch of 3, in the one batch of 513 and in the batches of 1024 and 1;
  h. a forcing on every level, and a level whose forcing is None beside one that has it;
  i. states with mean 5;
  j. GridTransferNavierStokes hierarchies 12 -> 6 and 66 -> 33: the kernels against the same transfer through its Python methods, bit for bit;
  k. a V-cycle solve to 1e-10 against the plugin path over the host step;
  l. what is refused.

Tolerances, nothing in them measured on the device (navier_stokes_reference.py derives C(nx) = 4 nx + 17 and the majorant M = M1 + M2,
M1 the stencil's own terms on |w| and the reference's |psi|, M2 = dt (norm(w) / (lam_1 dx)) (max |wx| + max |wy|) the propagated psi error):
  per Phi:     device against host 2 C(nx) EPS M (each side C(nx) EPS M), device against reference (C(nx) + ALLOWANCE) EPS M, M the
               largest over the rows;
  + SLACK      8 EPS * 3 * the largest row norm involved, the harness's, for the sweep's own arithmetic;
  chained steps (forward_solve, F-relaxation over 3 F-points): e_k = Lip_k e_(k-1) + the step's per-Phi term + SLACK with
               Lip_k = 1 + 2 dt (1 + 1e-6) (U / dx + R / (lam_1 dx^2)),
               U the largest |psi_x|, |psi_y| (the velocity) and R the largest |value| of the step's reference input. Phi = (solve) o
               (stencil map). The solve contracts (all eigenvalues of I - dt nu Lh are >= 1). For the reference's state w and the
               device's w' = w + delta the Jacobian is bilinear: J(psi', w') - J(psi, w) = J(psi_delta, w') + J(psi, delta).
               J(psi, delta) = psi_y delta_x - psi_x delta_y with |psi_x|, |psi_y| <= U and norm(delta_x), norm(delta_y) <= norm(delta) / dx
               (two shifted copies over 2 dx): at most 2 U norm(delta) / dx. J(psi_delta, w'): |w'_x|, |w'_y| <= R' / dx (two values
               <= R' over 2 dx), norm(psi_delta) <= norm(delta) / lam_1 and a difference of it over 2 dx at most norm(delta) / (lam_1 dx):
               at most 2 (R' / dx) norm(delta) / (lam_1 dx). R' <= (1 + 1e-6) R: the device's state lies within the allowances, six
               orders below 1e-6 R; the same factor covers U, which is evaluated from the reference's long-double psi rounded.
Every comparison covers all rows of a list. Each sweep prints its worst error / allowed ("RATIO" lines).
"""
import ctypes as C
import types

import numpy as np
import pytest

import cases
from navier_stokes_reference import C as _coef, kolmogorov, majorant
from periodic2d_kinds import KINDS, dyadic
from periodic2d_sweeps import (ALL_SWEEPS, STORED_STATE_SWEEPS, both_weights, bounds_of, check_level_0_twice, check_level_entry_point, check_one_phi,
                               check_ragged, compare as _compare, distinct_steps as _distinct_steps, dt_groups, f_relaxed_rows,
                               host_class, intervals as _intervals, pair, report as _report, row_norm as _row_norm, run_sweeps,
                               set_states as _set_states, tol, uniform as _uniform)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

EPS = cases.EPS
KIND = KINDS["navierstokes"]
NU = KIND.par(16)["nu"]
T_SWEEP = KIND.t_sweep(None)
BOUNDS = {side: bounds_of("navierstokes", side) for side in ("host", "reference")}


def _pair(nx, grids, side="host", forcing=None, **opts):
    """(device Mgrit, plugin Mgrit over HostNavierStokes2D or ReferenceNavierStokes2D) on the same hierarchy; forcing: one per level"""
    return pair("navierstokes", nx, grids, side=side, levels=[dict(forcing=f) for f in forcing or [None] * len(grids)], **opts)


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
BATCH_CAP = 1024      # states of a launch: H2D_MAX_BATCH work slab items, one per state


def _dyadic(n_states):
    """2 n_states + 1 points with the exact step 2^-19 (every t_k = k 2^-19 and every difference is exact: one bit pattern of dt;
    at most [0, 0.0039]): n_states F-points and n_states relaxed C-points"""
    return dyadic("navierstokes", 2 * n_states + 1)


@pytest.mark.parametrize("n_states", [513, 1025])
def test_sweeps_of_one_dt_group(n_states):
    """n_states F-points and n_states relaxed C-points, each one dt group: 513 = one batch, 1025 = a batch of 1024 and a batch of 1"""
    assert torch.cuda.is_available()
    nx, w = 4, 1.3
    dev, ref = _pair(nx, _intervals(_dyadic(n_states)), weight_c=w)
    assert len(dev.t[0]) == 2 * n_states + 1 and len(dev.t[1]) == n_states + 1
    for groups in dt_groups(dev.t[0]):      # F-points, relaxed C-points
        assert groups == [n_states], groups
    assert (n_states > BATCH_CAP) == (n_states == 1025) and 1025 == BATCH_CAP + 1
    record = run_sweeps(dev, ref, BOUNDS["host"], w, 77, STORED_STATE_SWEEPS, levels=[0])
    _report(f"batches[{n_states} states]", record)


# ---- d. one Phi at a larger grid ---------------------------------------------------------------------------------------------------
def test_one_phi_at_a_larger_grid():
    assert torch.cuda.is_available()
    nx = 129
    dev, ref = _pair(nx, _uniform((5, 3), 2.0 ** -8))      # (steps of 2^-10, exact)
    check_one_phi(dev, ref, BOUNDS["host"], nx, f"larger_grid[nx={nx}]")


# ---- e. the known answers ------------------------------------------------------------------------------------------------------------
def test_known_answers():
    """C-points 0, 6, 12: the constant state 5, a fixed point of Phi (its mean never reaches psi, mode 0 has D = 1), which must come back
    within the per-Phi term. C-points 2, 8, 14: Taylor-Green w = 2 cos(k X) cos(k Y), an eigenfunction of the discrete Laplacian with
    J = 0, which one step multiplies by 1 / (1 + dt nu mu_k), mu_k = 2 (4 / dx^2) sin^2(pi k / nx) from the stencil. C-points 4, 10:
    w = g(y), J = 0, the result independent of x. All rows are compared with the host step like every other row as well"""
    assert torch.cuda.is_available()
    nx, k = 33, 2
    dev, ref = _pair(nx, _uniform((17, 9, 5), T_SWEEP))
    app, dt = ref.problem[0], float(np.max(np.diff(ref.t[0])))
    st = BOUNDS["host"].random_states(ref, 5)
    X = 2 * np.pi * np.arange(nx) / nx
    const = np.full(nx * nx, 5.0)
    tg = (2.0 * np.cos(k * X)[:, None] * np.cos(k * X)[None, :]).ravel()
    g = np.random.default_rng(11).uniform(-1.0, 1.0, size=nx)
    yonly = np.tile(g, nx)      # w[i][j] = g[j]: axis 1 is y
    st[("u", 0)][0::6], st[("u", 0)][2::6], st[("u", 0)][4::6] = const, tg, yonly
    _set_states(dev, ref, st)
    dev.f_relax(0); ref.f_relax(0)
    slack = 8 * EPS * 3 * _row_norm(*st.values())
    allowed = tol(BOUNDS["host"], ref, 0, st[("u", 0)][0::2]) + slack
    worst = _compare(dev, ref, 0, allowed, "f_relax, known answers")
    got = dev.backend.natural("u", 0)
    assert np.all(np.isfinite(got))
    one = _coef(nx) * EPS      # against an exact answer the device alone is off: C(nx) EPS M
    err_const = float(np.max(np.linalg.norm(got[1::6] - const, axis=1)))
    allowed_const = one * majorant(const, dt, nx, app.L) + slack
    mu_k = 2.0 * (4.0 / app.dx ** 2) * np.sin(np.pi * k / nx) ** 2
    err_tg = float(np.max(np.linalg.norm(got[3::6] - tg / (1.0 + dt * NU * mu_k), axis=1)))
    allowed_tg = (one + 4 * EPS) * majorant(tg, dt, nx, app.L) + slack      # (4 EPS: the yardstick's own quotient, mu_k and its product)
    after = got[5::6][:2].reshape(-1, nx, nx)
    err_y = float(np.max(np.linalg.norm((after - after[:, :1, :]).reshape(2, -1), axis=1)))
    allowed_y = 2 * one * majorant(yonly, dt, nx, app.L) + slack            # (a difference of two rows of the result)
    print(f"RATIO known_answers f_relax: worst error/allowed {worst / allowed:.4f}, constant {err_const / allowed_const:.4f}, "
          f"Taylor-Green {err_tg / allowed_tg:.4f}, y only {err_y / allowed_y:.4f}")
    assert err_const <= allowed_const and err_tg <= allowed_tg and err_y <= allowed_y
    assert float(np.max(np.abs(after[0][0] - g))) > 1e3 * allowed_y      # while the diffusion moved it
    assert float(np.linalg.norm(got[3] - tg)) > 1e3 * allowed_tg


# ---- f, g. the same bits -------------------------------------------------------------------------------------------------------------
def test_a_sweep_run_twice_gives_the_same_bits():
    assert torch.cuda.is_available()
    nx = 33
    dev, ref = _pair(nx, _uniform((17, 9, 5), T_SWEEP), forcing=[kolmogorov(nx)] * 3)
    check_level_0_twice(dev, ref, BOUNDS["host"].random_states(ref, 21))


def test_a_rows_bits_do_not_depend_on_its_batch():
    """the same state behind the step 2^-19 as one of 3 F-points (one batch of 3), as the first and the last of 513 (one batch) and as
    the first and the last of 1025 (the batch of 1024 and the batch of 1): the same row, bit for bit"""
    assert torch.cuda.is_available()
    nx = 4
    state = np.random.default_rng(3).uniform(-1.0, 1.0, size=nx * nx)
    rows = []
    for n_pts, at in ((7, (0,)), (2 * 513 + 1, (0, 1024)), (2 * 1025 + 1, (0, 2048))):
        dev, ref = _pair(nx, _intervals(dyadic("navierstokes", n_pts)))
        rows += f_relaxed_rows(dev, ref, BOUNDS["host"].random_states(ref, 9), state, at)
    assert len(rows) == 5 and all(torch.equal(rows[0], r) for r in rows[1:])
    assert not torch.equal(rows[0][:nx * nx], torch.from_numpy(state).to(rows[0].device))


# ---- h. forcing ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", ["every level", "level 1 without"])
def test_every_sweep_with_a_forcing(levels):
    """a Kolmogorov forcing with a part that depends on x (a transposed plane shows) of amplitude 6: dt f is 6e-3 of the state at the
    coarsest step, 1e10 allowances. 'level 1 without': the engine keeps the forcing per level, None beside a plane"""
    assert torch.cuda.is_available()
    nx, record = 33, {}
    f = kolmogorov(nx)
    forcing = [f, f, f] if levels == "every level" else [f, None, f]
    for side in ("host", "reference"):
        dev, ref = _pair(nx, _uniform((17, 9, 5), T_SWEEP), side=side, forcing=forcing)
        run_sweeps(dev, ref, BOUNDS[side], 1.0, 900 + len(side), ALL_SWEEPS, record=record)
    _report(f"forcing[{levels}]", record)


# ---- i. a mean ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", ["host", "reference"])
def test_every_sweep_on_states_with_mean_5(side):
    """w uniform in [4, 6]: the mean leaves in the second product (S[0][0] = 0) and comes back through b = w - dt J"""
    assert torch.cuda.is_available()
    nx = 33
    dev, ref = _pair(nx, _uniform((17, 9, 5), T_SWEEP), side=side)
    record = run_sweeps(dev, ref, bounds_of("navierstokes", side, mean=5.0), 1.0, 1234, ALL_SWEEPS)
    _report(f"mean_5[{side}]", record)


# ---- j. the device transfer ------------------------------------------------------------------------------------------------------------
def _via_python():
    from pymgrit_amd import GridTransferNavierStokes

    class NavierStokesViaPython(GridTransferNavierStokes):      # overridden methods: the caller's path
        def restriction(self, u):
            return super().restriction(u)

        def interpolation(self, u):
            return super().interpolation(u)
    return NavierStokesViaPython


def _coarsened(sizes, nts, t_stop, cls=None, forcing=0.0, nu=NU, L=None):
    from pymgrit_amd import NavierStokes2D
    cls = cls or NavierStokes2D
    n0 = nts[0] - 1
    assert n0 & (n0 - 1) == 0 and np.log2(t_stop) == int(np.log2(t_stop))      # dyadic: every t_k and every step is exact
    t = t_stop * (np.arange(n0 + 1.0) / n0)
    out = []
    for nx, nt in zip(sizes, nts):
        s = n0 // (nt - 1)
        out.append(cls(nx=nx, nu=nu, L=L or sizes[0] / 16, forcing=forcing * kolmogorov(nx) if forcing else None, t_interval=t[::s]))
        assert len(out[-1].t) == nt and _distinct_steps(out[-1].t) == 1
    return out


@pytest.mark.parametrize("sizes", [(12, 6), (66, 33)])
def test_device_transfer_bit_identical_to_the_callers_path(sizes):
    """the pattern of test_hip_transfer2d.py::both: the library transfer as kernels against a subclass that overrides restriction and
    interpolation by calling super() -- applied row by row on the host between the kernels, every Phi the same device code"""
    assert torch.cuda.is_available()
    from pymgrit_amd import GridTransferNavierStokes, Mgrit
    out = []
    for tr in (GridTransferNavierStokes, _via_python()):
        mg = Mgrit(problem=_coarsened(sizes, (9, 5), 2.0 ** -8, forcing=1.0), transfer=[tr()], logging_lvl=30, nested_iteration=False, max_iter=3, tol=0.0)
        conv = np.asarray(mg.solve()["conv"])
        assert mg.backend.name == "hip" and mg.backend._device_transfer(0) == (tr is GridTransferNavierStokes)
        out.append((conv, mg.backend.natural("u", 0)))
    (c0, u0), (c1, u1) = out
    print("residual histories:", c0, c1)
    assert len(c0) == len(c1) == 3 and np.all(np.isfinite(c0)) and np.array_equal(c0, c1), (c0, c1)
    assert np.array_equal(u0, u1)


# ---- k. Mgrit.solve() ------------------------------------------------------------------------------------------------------------------
def test_v_cycle_solve_matches_the_plugin_path():
    """nx = 12 on three levels (copy transfers), nt 33 / 17 / 9 on [0, 1], L = 2 pi, nu = 0.05, from the initial guess with a forcing, to
    1e-10: the residual histories and three level-0 states with the tolerances of
    test_hip_transfer2d.py::test_heat2d_against_the_plugin_path. (Spatial coarsening 12 -> 6 converges by 0.4 per cycle only on the
    plugin path: it is covered bit for bit above, not solved to 1e-10 here)"""
    assert torch.cuda.is_available()
    from pymgrit_amd import Mgrit, NavierStokes2D
    out = {}
    for host in (True, False):
        prob = _coarsened((12, 12, 12), (33, 17, 9), 1.0, cls=host_class(NavierStokes2D) if host else None, forcing=0.1, nu=0.05, L=2 * np.pi)
        mg = Mgrit(problem=prob, logging_lvl=30, tol=1e-10, max_iter=12)
        conv = np.asarray(mg.solve()["conv"])
        assert (type(mg.backend).__name__ == "HipBackend") != host
        out[host] = (conv, np.array([np.asarray(mg.u[0][i].get_values()) for i in (5, 16, 32)]))
    (ch, uh), (cd, ud) = out[True], out[False]
    print("plugin", ch, "device", cd, "largest state deviation", np.max(np.abs(uh - ud)))
    assert len(ch) == len(cd) < 12 and ch[-1] < 1e-10, (ch, cd)
    assert np.all(np.abs(ch - cd) <= 1e-9 * ch + 2e-11), (ch, cd)
    assert np.max(np.abs(uh - ud)) <= 1e-11 * max(1.0, np.max(np.abs(uh)))


# ---- l. what is refused ------------------------------------------------------------------------------------------------------------------
def test_what_is_not_covered_is_refused():
    from pymgrit_amd import AllenCahn, AtMgrit, GridTransferAllenCahn, GridTransferNavierStokes, Mgrit, NavierStokes2D
    from pymgrit_amd.core.backend_hip import HipBackend
    from pymgrit_amd.core.hip_lib import MgritHipError
    name = "Navier-Stokes levels on the HIP engine"

    def prob():
        return [NavierStokes2D(nx=12, t_start=0, t_stop=0.25, nt=nt) for nt in (9, 3)]
    with pytest.raises(MgritHipError, match=name + ": AT-MGRIT is not supported"):
        AtMgrit(k=2, problem=prob(), logging_lvl=30)
    with pytest.raises(MgritHipError, match=name + ": the global convergence criteria only"):
        Mgrit(prob(), conv_crit=2, logging_lvl=30)
    stub = types.SimpleNamespace(desc=[p.device_stepper() for p in prob()])
    with pytest.raises(MgritHipError, match=name + ": one time rank only"):
        HipBackend._check_periodic(stub, types.SimpleNamespace(comm_time_size=2, global_conv_crit=True), "navierstokes2d")
    # a hierarchy that mixes Navier-Stokes and Allen-Cahn levels: by name, in either order
    mixed = [prob()[0], AllenCahn(nx=12, method="IMEX", t_start=0, t_stop=0.25, nt=3)]
    for levels in (mixed, [AllenCahn(nx=12, method="IMEX", t_start=0, t_stop=0.25, nt=9), prob()[1]]):
        with pytest.raises(MgritHipError, match="every level of the hierarchy must be"):
            Mgrit(levels, logging_lvl=30)
    assert GridTransferAllenCahn().device_transfer() == GridTransferNavierStokes().device_transfer()
    HipBackend._check_periodic(stub, types.SimpleNamespace(comm_time_size=1, global_conv_crit=True), "navierstokes2d")      # (what is covered passes)
    # the engine is usable afterwards
    mg = Mgrit(_coarsened((12, 12), (9, 5), 2.0 ** -8), logging_lvl=30, nested_iteration=False, max_iter=3, tol=0.0)
    conv = np.asarray(mg.solve()["conv"])
    # (two levels with four coarse intervals: MGRIT with FCF relaxation is exact after two cycles, and residuals that are exactly
    # zero are not reported)
    assert type(mg.backend).__name__ == "HipBackend" and 1 <= len(conv) <= 3 and np.all(np.isfinite(conv)) and conv[0] > 0.0, conv


def test_level_entry_point_refuses_bad_arguments():
    """mgrit_hip_level_navierstokes2d through raw ctypes: negative codes with a message, and what follows from the level's kind -- the
    periodic 2-D transfer joins two Navier-Stokes levels and refuses a Navier-Stokes level above an Allen-Cahn level by name"""
    assert torch.cuda.is_available()
    from pymgrit_amd.core import hip_lib
    EINVAL, EUNSUPPORTED = -1, -4
    null = C.c_void_p(0)
    f20, f10 = np.ascontiguousarray(kolmogorov(20)), np.ascontiguousarray(kolmogorov(10))
    bad_f = f20.copy()
    bad_f[7, 3] = np.inf
    ok = (20, 400, 256.0, 8.0, 0.1)      # nx, ld, 1 / dx^2, 1 / (2 dx), nu

    def transfers(lib, eng, fn, tp, msg):
        # the periodic transfer joins two such levels of sizes 2 n and n, the copy two of one size; not the Heat2D transfer
        assert lib.mgrit_hip_level_transfer(eng, 0, hip_lib.TRANSFER_PERIODIC2D) == 0
        assert lib.mgrit_hip_level_transfer(eng, 1, hip_lib.TRANSFER_COPY) == 0
        assert lib.mgrit_hip_level_transfer(eng, 1, hip_lib.TRANSFER_PERIODIC2D) == EINVAL and b"2*n_coarse per axis" in msg()
        assert lib.mgrit_hip_level_transfer(eng, 0, hip_lib.TRANSFER_HEAT2D) == EUNSUPPORTED
        # an Allen-Cahn level below a Navier-Stokes level: refused by name, and the engine goes on
        assert lib.mgrit_hip_level_allencahn2d(eng, 3, 9, tp, 5, 32, 16.0, 1.0, 2) == 0
        assert lib.mgrit_hip_level_transfer(eng, 2, hip_lib.TRANSFER_PERIODIC2D) == EUNSUPPORTED
        assert b"the periodic 2-D transfer joins two Allen-Cahn levels" in msg()
        assert lib.mgrit_hip_level_transfer(eng, 0, hip_lib.TRANSFER_PERIODIC2D) == 0
    check_level_entry_point(
        "mgrit_hip_level_navierstokes2d", 4, 5, 0.01, ok, tail=(null,), small=(3, 16) + ok[2:], large=(2049, 2049 * 2049 + 15) + ok[2:],
        short=(20, 384) + ok[2:], odd=(20, 408) + ok[2:],      # too short; not a multiple of 16
        bad=((20, 400, 256.0, 8.0, 0.0), (20, 400, 256.0, 8.0, -0.1), (20, 400, 256.0, 8.0, float("nan")), (20, 400, 256.0, 8.0, float("inf")),
             (20, 400, 0.0, 8.0, 0.1), (20, 400, 256.0, 0.0, 0.1), (20, 400, 256.0, float("inf"), 0.1)),
        also_invalid=[(ok + (C.c_void_p(bad_f.ctypes.data),), b"forcing is not finite at value 143")],
        grid_msg=b"Navier-Stokes grid", ld_msg=b"nx*nx", bad_msg=b"Navier-Stokes parameters",
        describe=[(0, ok + (C.c_void_p(f20.ctypes.data),)), (1, (10, 112, 64.0, 4.0, 0.1, C.c_void_p(f10.ctypes.data))), (2, (10, 112, 64.0, 4.0, 0.1, null))],
        then=transfers)
