"""GPU tests of the GinzburgLandau2D IMEX device path (csrc/mgrit_hip_ginzburglandau.inc): every sweep of the device
hierarchy against the SAME hierarchy on the plugin path, over ``HostGinzburgLandau2D`` (the numpy statement of the step,
GinzburgLandau2D.step) and -- one case -- over ``ReferenceGinzburgLandau2D`` (tests/ginzburg_landau_reference.py: the right-hand side in
long double, a transform-free refined solve of the 2 nx^2 x 2 nx^2 block system). States are fresh random, uniform in [-1, 1] in both
planes: the planes differ and are not symmetric in (i, j), so swapped planes, a wrong sign of Db or of c, or a transposed product miss by
orders of magnitude. (b, c) = (1.5, -0.8) unless a case says otherwise; L = nx (dx = 1 for every nx), sweep grids nt 17 / 9 / 5 on
[0, 0.5]: on the coarsest step dt = 0.125 the implicit block moves the highest mode by 8 dt |1 + i b| = 1.8 and the cubic term a state of
size 1 by about 0.2, both far above the tolerances, and rr sqrt(1 + b^2) = 0.23 <= 1 / 4, the range C(nx) is derived for (asserted for
every hierarchy). What the cases are chosen for:

  a. the size edges: nx = 4 (one tile, KP > nx), 33 (odd: the imaginary plane is only 8-byte aligned; pads inside the tile), 66 (two tiles
     per axis, the last one mostly pad), 97 (KP = P); nx = 33 also against the reference class;
  b. several step sizes on one level (nx = 33) on a ragged grid;
  c. dt groups of more than one launch: a launch holds 1024 work slab items = 512 two-item states, so 513 states are 512 + 1 and 1025
     are 512 + 512 + 1 -- blockIdx.z of the cross product (states) and of its neighbours (items) must agree across launches. The tests
     assert the group sizes they rely on;
  d. one Phi at nx = 129 (P = 192: three tiles per axis);
  e. the known answers: the zero state (exact zeros out), a constant state, a discrete plane wave;
  f. the same bits from a sweep run twice, and from the same state in a batch of 3, on both sides of the 512 border and in the remainder;
  g. the device 2-D transfer plane by plane (GridTransferGinzburgLandau, 12 -> 6 and 66 -> 33) against the same class through its Python
     methods, bit for bit;
  h. Mgrit.solve() against the plugin path, residual and jump criterion;
  i. what is refused.

Tolerances, nothing in them measured on the device (test_ginzburg_landau_cpu.py derives C(nx) = 4 nx + 25 and the majorant):
  per Phi:     device against host 2 C(nx) EPS M (each side C(nx) EPS M), device against reference (C(nx) + ALLOWANCE) EPS M, M the largest
               row majorant over both planes: M = norm((R, S)), R = |x| + dt (|x| + q (|x| + |c| |y|)), S = |y| + dt (|y| + q (|c| |x| + |y|));
  + SLACK      8 EPS * 3 * the largest row norm involved, the harness's, for the sweep's own arithmetic;
  chained steps (forward_solve, F-relaxation over 3 F-points): e_k = Lip_k e_(k-1) + the step's per-Phi term + SLACK with
               Lip_k = 1 + dt (1 + 3 sqrt(1 + c^2) R^2 (1 + 1e-6)), R the largest |A| of the step's reference input. Phi = (modal solve) o
               (pointwise map). The modal solve contracts: per mode the block [[Da, Db], [-Db, Da]] has 2-norm 1 / sqrt(det) <= 1. The map
               is A -> A + dt (A - (1 + i c) |A|^2 A); the Jacobian of A -> |A|^2 A (as a real 2 x 2 map: |A|^2 I + 2 A A^T) has norm
               3 |A|^2, the factor (1 + i c) the modulus sqrt(1 + c^2): norm(Jacobian of the map) <= 1 + dt (1 + 3 sqrt(1 + c^2) |A|^2) on the
               segment between the two states, whose |A| exceeds R by the error itself -- the factor 1 + 1e-6 (errors here are 1e-12).
Every comparison covers all rows of a list. Each sweep prints its worst error / allowed ("RATIO" lines); the MI355X values are in
DESIGN.md 3.15.
"""
import types

import numpy as np
import pytest

import cases
from ginzburg_landau_reference import LD
from periodic2d_kinds import KINDS, dyadic, gl_coef as _coef, gl_majorant as _majorant
from periodic2d_sweeps import (ALL_SWEEPS, STORED_STATE_SWEEPS, both_weights, bounds_of, check_history, check_jump_criterion, check_level_0_twice,
                               check_level_entry_point, check_one_phi, check_ragged, compare as _compare, dt_groups, f_relaxed_rows,
                               intervals as _intervals, pair, report as _report, row_norm as _row_norm, run_sweeps, set_states as _set_states, tol,
                               uniform as _uniform)
from transfer2d_cases import fill as _fill, one_step_size as _one_step_size, raw as _raw, solve as _solve

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

EPS = cases.EPS
KIND = KINDS["ginzburglandau"]
B, CC = KIND.par(1)["b"], KIND.par(1)["c"]
T_SWEEP = KIND.t_sweep(None)
BOUNDS = {side: bounds_of("ginzburglandau", side) for side in ("host", "reference")}


def _pair(nx, grids, side="host", per_phi_bounds=True, **opts):
    """(device Mgrit, plugin Mgrit over HostGinzburgLandau2D or ReferenceGinzburgLandau2D) on the same hierarchy. per_phi_bounds: the
    comparison uses the per-Phi tolerance, so every step must lie in the range C(nx) is derived for (the solve tests below compare
    residual histories by the rule of tests/cases.py instead)"""
    dev, ref = pair("ginzburglandau", nx, grids, side=side, **opts)
    for t, app in zip(dev.t, ref.problem):
        assert not per_phi_bounds or float(np.max(np.diff(t))) / app.dx ** 2 * np.sqrt(1.0 + app.b ** 2) <= 0.25
    return dev, ref


# ---- a. every sweep at the size edges ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx,side", [(4, "host"), (33, "host"), (66, "host"), (97, "host"), (33, "reference")])
def test_every_sweep_at_the_size_edges(nx, side):
    assert torch.cuda.is_available()

    def check(dev):
        assert dev.problem[0].dx == 1.0
    both_weights(lambda w: _pair(nx, _uniform((17, 9, 5), T_SWEEP), side=side, weight_c=w), BOUNDS[side], 100 * nx, 100 * nx + 7,
                 f"size_edges[nx={nx},{side}]", check=check)


@pytest.mark.parametrize("par", [dict(b=0.0, c=0.0), dict(b=-2.0, c=0.5)])
def test_every_sweep_with_other_coefficients(par):
    """the real-coefficient limit (Db = 0: the cross product reduces to two scaled products) and a pair of the other signs"""
    assert torch.cuda.is_available()
    nx = 33
    dev, ref = _pair(nx, _uniform((17, 9, 5), 0.4), par=dict(L=float(nx), **par))
    record = run_sweeps(dev, ref, BOUNDS["host"], 1.0, 4242, ALL_SWEEPS)
    _report(f"coefficients[b={par['b']},c={par['c']}]", record)


# ---- b. several step sizes per level -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", ["by2_3lvl", "by4_2lvl"])
def test_every_sweep_with_several_step_sizes_per_level(grid):
    assert torch.cuda.is_available()
    nx = 33
    both_weights(lambda w: _pair(nx, _intervals(KIND.ragged(nx)[grid]), weight_c=w), BOUNDS["host"], 500 * nx, 500 * nx + 3, f"step_sizes[{grid}]",
                 check=lambda dev: check_ragged(dev, grid))


# ---- c. dt groups larger than one launch -------------------------------------------------------------------------------------------
def _dyadic(n_pts):
    """n_pts points with the exact step 2^-13 (every t_k = k 2^-13 and every difference is exact: one bit pattern of dt; [0, 0.26])"""
    return dyadic("ginzburglandau", n_pts)


@pytest.mark.parametrize("states", [513, 1025])
def test_sweeps_of_more_than_one_launch(states):
    """513 / 1025 F-points and as many relaxed C-points, each ONE dt group: launches of 512 + 1 and 512 + 512 + 1 states"""
    assert torch.cuda.is_available()
    nx, w = 9, 1.3
    dev, ref = _pair(nx, _intervals(_dyadic(2 * states + 1)), weight_c=w)
    assert len(dev.t[0]) == 2 * states + 1 and len(dev.t[1]) == states + 1
    for groups in dt_groups(dev.t[0]):      # F-points, relaxed C-points
        assert groups == [states] and states % 512 == 1 and states > 1024 // 2, groups
    record = run_sweeps(dev, ref, BOUNDS["host"], w, 77, STORED_STATE_SWEEPS, levels=[0])
    _report(f"launches[{states} states]", record)


# ---- d. one Phi at a larger grid ---------------------------------------------------------------------------------------------------
def test_one_phi_at_a_larger_grid():
    assert torch.cuda.is_available()
    nx = 129
    dev, ref = _pair(nx, _uniform((5, 3), 2.0 ** -3))      # (steps of 2^-5, exact)
    check_one_phi(dev, ref, BOUNDS["host"], nx, f"larger_grid[nx={nx}]")


# ---- e. known answers ------------------------------------------------------------------------------------------------------------------
def test_known_answers_on_the_device():
    """C-points 0, 8, ..: the zero state, which must come back as exact zeros (r = s = 0 exactly, the products of zeros are zeros).
    C-points 2, 10, ..: the constant A = 0.75 - 0.5 i, which moves by the pointwise map alone (Lap A = 0, mode (0, 0) has Da = 1, Db = 0).
    C-points 4, 12, ..: the plane wave A = R exp(2 pi i (2 i1 + 3 i2) / nx), an eigenfunction: one step multiplies it by
    (1 + dt (1 - (1 + i c) R^2)) / (1 + dt mu (1 + i b)); with b and c swapped, a sign flipped or the axes swapped the answer is off by
    more than 1e6 times the allowance. The formulas are evaluated here in float64: (C(nx) + 16) EPS M + SLACK"""
    assert torch.cuda.is_available()
    nx, p, q, R = 33, 2, 3, 0.7
    dev, ref = _pair(nx, _uniform((17, 9, 5), T_SWEEP))
    app, n = ref.problem[0], nx * nx
    dt = float(dev.t[0][1] - dev.t[0][0])
    st = BOUNDS["host"].random_states(ref, 5)
    const = np.concatenate((np.full(n, 0.75), np.full(n, -0.5)))
    i1, i2 = np.meshgrid(np.arange(nx), np.arange(nx), indexing="ij")

    def wave(p, q):
        return R * np.exp(2j * np.pi * ((p * i1 + q * i2) % nx) / nx)

    def stepped(A, p, q, b, c):
        mu = float(LD(4) * (np.sin(LD(np.pi) * LD(p) / LD(nx)) ** 2 + np.sin(LD(np.pi) * LD(q) / LD(nx)) ** 2))      # dx = 1
        return A * (1.0 + dt * (1.0 - (1.0 + 1j * c) * R * R)) / (1.0 + dt * mu * (1.0 + 1j * b))

    def row(A):
        return np.concatenate((A.real.ravel(), A.imag.ravel()))
    A = wave(p, q)
    st[("u", 0)][0::8], st[("u", 0)][2::8], st[("u", 0)][4::8] = 0.0, const, row(A)
    _set_states(dev, ref, st)
    dev.f_relax(0); ref.f_relax(0)
    slack = 8 * EPS * 3 * _row_norm(*st.values())
    worst = _compare(dev, ref, 0, tol(BOUNDS["host"], ref, 0, st[("u", 0)][0::2]) + slack, "f_relax, known answers")
    got = dev.backend.natural("u", 0)
    assert np.array_equal(got[1::8], np.zeros_like(got[1::8]))
    m = 0.75 ** 2 + 0.5 ** 2
    want = np.concatenate((np.full(n, 0.75 + dt * (0.75 - m * (0.75 - CC * -0.5))), np.full(n, -0.5 + dt * (-0.5 - m * (CC * 0.75 - 0.5)))))
    allowed = (_coef(nx) + 16) * EPS * _majorant(app, const, dt) + slack
    err = float(np.max(np.linalg.norm(got[3::8] - want, axis=1)))
    print(f"RATIO known_answers constant: worst error/allowed {err / allowed:.4f}")
    assert err <= allowed and float(np.linalg.norm(want - const)) > 1e6 * allowed, (err, allowed)
    allowed = (_coef(nx) + 16) * EPS * _majorant(app, row(A), dt) + slack
    err = float(np.max(np.linalg.norm(got[5::8] - row(stepped(A, p, q, B, CC)), axis=1)))
    print(f"RATIO known_answers plane_wave: worst error/allowed {err / allowed:.4f} (sweep against host {worst:.3e})")
    assert err <= allowed, (err, allowed)
    for what, wrong in (("b and c swapped", stepped(A, p, q, CC, B)), ("sign of b", stepped(A, p, q, -B, CC)), ("sign of c", stepped(A, p, q, B, -CC)),
                        ("conjugate", np.conj(stepped(A, p, q, B, CC))), ("p and q swapped", stepped(wave(q, p), q, p, B, CC))):
        miss = float(np.min(np.linalg.norm(got[5::8] - row(wrong), axis=1)))
        assert miss > 1e6 * allowed, (what, miss, allowed)


# ---- f. the same bits ----------------------------------------------------------------------------------------------------------------
def test_a_sweep_run_twice_gives_the_same_bits():
    assert torch.cuda.is_available()
    dev, ref = _pair(33, _uniform((17, 9, 5), T_SWEEP))
    check_level_0_twice(dev, ref, BOUNDS["host"].random_states(ref, 21))


def test_a_rows_bits_do_not_depend_on_its_launch():
    """the same state behind the step 2^-13 as one of 3 F-points (one launch of 3) and as state 0, 511, 512 and 1024 of 1025 (the last of
    the first launch of 512, the first of the second, the remainder of 1): the same row, bit for bit"""
    assert torch.cuda.is_available()
    nx = 9
    big, ref_big = _pair(nx, _intervals(_dyadic(2051)))
    small, ref_small = _pair(nx, _intervals(_dyadic(7)))
    state = np.random.default_rng(3).uniform(-1.0, 1.0, size=2 * nx * nx)
    rows = {name: f_relaxed_rows(dev, ref, BOUNDS["host"].random_states(ref, 9), state, at)
            for name, dev, ref, at in (("small", small, ref_small, (0,)), ("big", big, ref_big, (0, 2 * 511, 2 * 512, 2 * 1024)))}
    for r in rows["big"]:
        assert torch.equal(rows["small"][0], r)
    assert not torch.equal(rows["small"][0][:2 * nx * nx], torch.from_numpy(state).to(rows["small"][0].device))


# ---- g. the device transfer ------------------------------------------------------------------------------------------------------------
def _transfer_classes():
    from pymgrit_amd import GridTransferGinzburgLandau

    class ViaPython(GridTransferGinzburgLandau):      # overridden methods: the caller's path
        def restriction(self, u):
            return super().restriction(u)

        def interpolation(self, u):
            return super().interpolation(u)
    return GridTransferGinzburgLandau, ViaPython


def _transfer_problem(sizes, nts):
    from pymgrit_amd import GinzburgLandau2D
    return [GinzburgLandau2D(nx=nx, b=B, c=CC, L=float(sizes[0]), t_start=0, t_stop=0.5, nt=nt) for nx, nt in zip(sizes, nts)]


@pytest.mark.parametrize("fine", [12, 66])
def test_device_transfer_solve_is_bit_identical_to_the_python_methods(fine):
    """three V-cycles over [fine, fine / 2] with GridTransferGinzburgLandau as kernels and through its Python methods (a subclass that
    overrides them by calling super(): every Phi stays the same device code): the same residual history and level-0 states, bit for bit"""
    assert torch.cuda.is_available()
    out = []
    for cls in _transfer_classes():
        prob = _transfer_problem([fine, fine // 2], (9, 5))
        assert all(_one_step_size(p.t) for p in prob)
        conv, mg = _solve(prob, [cls()], nested_iteration=False, max_iter=3, tol=0.0)
        assert mg.backend.name == "hip" and mg.backend._device_transfer(0) == (cls.__name__ != "ViaPython")
        out.append((conv, mg.backend.natural("u", 0)))
    (c0, u0), (c1, u1) = out
    print("residual histories:", c0, c1)
    assert len(c0) == len(c1) == 3 and np.array_equal(c0, c1) and np.all(np.isfinite(c0)) and c0[0] > 0.0
    assert u0.shape == (9, 2 * fine * fine) and np.array_equal(u0, u1)


@pytest.mark.parametrize("fine", [12, 66])
def test_device_transfer_sweeps_equal_the_python_methods(fine):
    """restrict_u, interpolate and error_correction against GridTransferGinzburgLandau's Python methods row by row, bit for bit: each plane
    transferred on its own, the border between the planes (66 -> 33: inside a 16-value pad group) respected, pads and other rows untouched"""
    assert torch.cuda.is_available()
    from pymgrit_amd import Mgrit, VectorGinzburgLandau2D
    coarse = fine // 2
    lib_cls, _ = _transfer_classes()
    py = lib_cls()
    mg = Mgrit(problem=_transfer_problem([fine, coarse], (9, 5)), transfer=[lib_cls()], logging_lvl=30, nested_iteration=False)
    assert mg.backend._device_transfer(0)
    nf, nc = 2 * fine * fine, 2 * coarse * coarse
    pairs = [(2 * j, j) for j in range(1, 5)]
    fi, co = [p[0] for p in pairs], [p[1] for p in pairs]

    def apply(method, rows, nx):
        out = []
        for r in rows:
            v = VectorGinzburgLandau2D(nx)
            v.set_values(r.reshape(2, nx, nx).copy())
            out.append(np.asarray(method(v).get_values()).ravel())
        return np.array(out)

    def check(name, lvl, rows, want, n, before):
        got = _raw(mg, name, lvl)
        assert np.array_equal(got[rows, :n], want), name
        assert not got[:, n:].any()         # row pads stay zero
        rest = np.setdiff1d(np.arange(got.shape[0]), rows)
        assert np.array_equal(got[rest], before[rest])
    _fill(mg, 1)
    before_f, before_c = _raw(mg, "u", 0).copy(), _raw(mg, "u", 1).copy()
    mg.backend.restrict_u(0, pairs)
    check("u", 1, co, apply(py.restriction, before_f[fi, :nf], fine), nc, before_c)
    _fill(mg, 2)
    before_f, before_c = _raw(mg, "u", 0).copy(), _raw(mg, "u", 1).copy()
    mg.backend.interpolate(0, pairs)
    check("u", 0, fi, apply(py.interpolation, before_c[co, :nc], coarse), nf, before_f)
    _fill(mg, 3)
    before_f, uc, vc = _raw(mg, "u", 0).copy(), _raw(mg, "u", 1).copy(), _raw(mg, "v", 1).copy()
    mg.backend.error_correction(0, pairs)
    check("u", 0, fi, before_f[fi, :nf] + apply(py.interpolation, uc[co, :nc] - vc[co, :nc], coarse), nf, before_f)


# ---- h. Mgrit.solve() -----------------------------------------------------------------------------------------------------------------
def _solve_grids():
    return _uniform((17, 9, 5), 2.0)


SOLVE = dict(par=dict(b=B, c=CC, L=12.0), per_phi_bounds=False)


def test_v_cycle_solve_matches_the_plugin_path():
    """from the initial guess on (nx = 12, L = 12, [0, 2], nt 17 / 9 / 5) to 1e-10: residual histories by the rule of tests/cases.py"""
    assert torch.cuda.is_available()
    dev, ref = _pair(12, _solve_grids(), cycle_type="V", max_iter=8, tol=1e-10, nested_iteration=True, **SOLVE)
    conv, rconv, _ = check_history(dev, ref, "solve[V]")
    assert rconv[-1] < 1e-10 and conv[-1] < 1e-10, (conv, rconv)


def test_jump_criterion_matches_the_plugin_path():
    """conv_crit = 1: the norms of u_i - previous u_i over both planes, three iterations from the initial guess; the same rule"""
    assert torch.cuda.is_available()
    dev, ref = _pair(12, _solve_grids(), conv_crit=1, max_iter=3, tol=0.0, **SOLVE)
    check_jump_criterion(dev, ref, 2)


# ---- i. what is refused ---------------------------------------------------------------------------------------------------------------
def test_what_is_not_covered_is_refused():
    from pymgrit_amd import AtMgrit, GinzburgLandau2D, GrayScott, GridTransfer, GridTransferBurgers, GridTransferCopy, Mgrit
    from pymgrit_amd.core.backend_hip import HipBackend
    from pymgrit_amd.core.hip_lib import MgritHipError
    name = "Ginzburg-Landau levels on the HIP engine"

    def prob(nxs=(12, 12)):
        return [GinzburgLandau2D(nx=nx, L=12.0, t_start=0, t_stop=0.25, nt=nt) for nx, nt in zip(nxs, (9, 3))]

    class Mine(GridTransfer):      # a spatial coarsening of the user's
        def restriction(self, u):
            return u

        def interpolation(self, u):
            return u
    with pytest.raises(MgritHipError, match=name + ".*same nx"):
        Mgrit(prob((12, 6)), transfer=[Mine()], logging_lvl=30)
    with pytest.raises(MgritHipError, match=name + ": GridTransferCopy only"):
        Mgrit(prob(), transfer=[Mine()], logging_lvl=30)
    with pytest.raises(MgritHipError, match=name + ".*GridTransferBurgers.*not this application's transfer"):
        Mgrit(prob((12, 6)), transfer=[GridTransferBurgers()], logging_lvl=30)      # another application's library class
    with pytest.raises(MgritHipError, match=name + ": AT-MGRIT is not supported"):
        AtMgrit(k=2, problem=prob(), logging_lvl=30)
    with pytest.raises(MgritHipError, match=name + ": the global convergence criteria only"):
        Mgrit(prob(), conv_crit=2, logging_lvl=30)
    stub = types.SimpleNamespace(desc=[p.device_stepper() for p in prob()])
    one_rank = types.SimpleNamespace(comm_time_size=1, global_conv_crit=True, transfer_objects=[GridTransferCopy()])
    with pytest.raises(MgritHipError, match=name + ": one time rank only"):
        HipBackend._check_periodic(stub, types.SimpleNamespace(comm_time_size=2, global_conv_crit=True, transfer_objects=[GridTransferCopy()]),
                                   "ginzburglandau2d")
    gs = GrayScott(nx=12, method="IMEX", t_start=0, t_stop=0.25, nt=3)
    mixed = types.SimpleNamespace(desc=[prob()[0].device_stepper(), gs.device_stepper()])
    with pytest.raises(MgritHipError, match=name + ": every level of the hierarchy must be a GinzburgLandau2D application"):
        HipBackend._check_periodic(mixed, one_rank, "ginzburglandau2d")
    with pytest.raises(MgritHipError, match="levels on the HIP engine: every level of the hierarchy must be"):
        Mgrit([prob()[0], gs], logging_lvl=30)
    HipBackend._check_periodic(stub, one_rank, "ginzburglandau2d")      # (and what is covered passes the same check)


def test_level_entry_point_refuses_bad_arguments():
    """mgrit_hip_level_ginzburglandau2d through raw ctypes: negative codes with a message, and what follows from the level's kind"""
    assert torch.cuda.is_available()
    from pymgrit_amd.core import hip_lib
    ok = (20, 800, 1.0, 1.5, -0.8)      # nx, ld, 1 / dx^2, b, c

    def transfers(lib, eng, fn, tp, msg):      # two levels of one nx: the periodic 2-D transfer is not theirs, the copy is
        assert lib.mgrit_hip_level_transfer(eng, 0, hip_lib.TRANSFER_PERIODIC2D) == -4
        assert lib.mgrit_hip_level_transfer(eng, 0, hip_lib.TRANSFER_COPY) == 0
    check_level_entry_point(
        "mgrit_hip_level_ginzburglandau2d", 3, 5, 0.5, ok, small=(3, 32) + ok[2:], large=(2049, 2 * 2049 * 2049 + 14) + ok[2:],
        short=(20, 400) + ok[2:], odd=(20, 808) + ok[2:],      # one plane's worth; not a multiple of 16
        bad=((20, 800, 0.0, 1.5, -0.8), (20, 800, -1.0, 1.5, -0.8), (20, 800, float("inf"), 1.5, -0.8), (20, 800, float("nan"), 1.5, -0.8),
             (20, 800, 1.0, float("nan"), -0.8), (20, 800, 1.0, float("inf"), -0.8), (20, 800, 1.0, 1.5, float("nan")),
             (20, 800, 1.0, 1.5, -float("inf"))),
        grid_msg=b"Ginzburg-Landau grid", ld_msg=b"2*nx*nx", bad_msg=b"Ginzburg-Landau parameters", describe=[(0, ok), (1, ok)], then=transfers)
