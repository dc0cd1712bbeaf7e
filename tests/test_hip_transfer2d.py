"""GPU: the 2-D library transfers as kernels (csrc/mgrit_hip_transfer2d.inc; MGRIT_HIP_TRANSFER_HEAT2D / _PERIODIC2D).

Yardstick of the bit-identity tests: the same hierarchy with a subclass that overrides restriction and interpolation by calling
super() -- the backend then applies the Python methods row by row on the host between the kernels (MGRIT_HIP_TRANSFER_CALLER), every Phi
stays the same device code, so the kernels must reproduce the Python spec bit for bit. That path takes one time-step size (one bit
pattern of dt) per level, so every grid compared with it is one whose steps are equal bit for bit: linspace(0, 1, 2^k + 1), and
linspace(0, T_SWEEP, nt) for nt <= 9 (asserted)."""
import ctypes as C

import numpy as np
import pytest

import cases
from transfer2d_cases import fill as _fill, one_step_size as _one_step_size, raw as _raw, solve

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

EPS = cases.EPS

T_SWEEP = 0.002     # as tests/test_hip_allen_cahn.py


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU visible")


def _classes():
    from pymgrit_amd import GridTransferAllenCahn, GridTransferHeat2D

    class Heat2DViaPython(GridTransferHeat2D):      # overridden methods: the caller's path
        def restriction(self, u):
            return super().restriction(u)

        def interpolation(self, u):
            return super().interpolation(u)

    class AllenCahnViaPython(GridTransferAllenCahn):
        def restriction(self, u):
            return super().restriction(u)

        def interpolation(self, u):
            return super().interpolation(u)
    return {"heat": (GridTransferHeat2D, Heat2DViaPython), "ac": (GridTransferAllenCahn, AllenCahnViaPython)}


def heat_problem(shapes, nt0, strides, method="BE", host=False):
    from pymgrit_amd.heat.heat_2d import Heat2D
    t0 = np.linspace(0, 1, nt0)
    prob = [Heat2D(x_start=0, x_end=cases.H2D_X_END, y_start=0, y_end=cases.H2D_Y_END, nx=nx, ny=ny, a=cases.H2D_A, method=method,
                   rhs_separable=[(cases.h2d_s0, lambda t: 1.0)], t_interval=t0[::s]) for (nx, ny), s in zip(shapes, strides)]
    if host:
        for p in prob:
            p.device_stepper = lambda: None
    return prob


def ac_problem(sizes, nts, nu=2, app=None):
    from pymgrit_amd import AllenCahn
    app = app or AllenCahn
    return [app(nx=nx, nu=nu, method="IMEX", t_start=0, t_stop=T_SWEEP, nt=nt) for nx, nt in zip(sizes, nts)]


def transfers(kind, n_levels, via_python, copies=()):
    from pymgrit_amd import GridTransferCopy
    lib, py = _classes()[kind]
    return [GridTransferCopy() if lvl in copies else (py if via_python else lib)() for lvl in range(n_levels - 1)]


def both(kind, make_problem, n_levels, copies=(), solver=None, **opts):
    """(library transfer, the same through the Python methods): residual histories and all level-0 states"""
    out = []
    for via_python in (False, True):
        prob = make_problem()
        for p in prob:
            assert _one_step_size(p.t)
        conv, mg = solve(prob, transfers(kind, n_levels, via_python, copies), solver=solver, **opts)
        assert mg.backend.name == "hip"
        for lvl in range(n_levels - 1):
            assert mg.backend._device_transfer(lvl) == (not via_python or lvl in copies)
        out.append((conv, mg.backend.natural("u", 0)))
    (c0, u0), (c1, u1) = out
    print("residual histories:", c0, c1)
    assert len(c0) == len(c1) and np.array_equal(c0, c1), (c0, c1)
    assert np.array_equal(u0, u1)
    return c0


HEAT_CASES = {
    "5x7_2lvl": dict(shapes=[(5, 7), (3, 4)], nt0=17, strides=(1, 4)),
    "17x21_copy_below": dict(shapes=[(17, 21), (9, 11), (9, 11)], nt0=33, strides=(1, 2, 4), copies=(1,)),
    "33x33_F_nested": dict(shapes=[(33, 33), (17, 17), (9, 9)], nt0=33, strides=(1, 2, 4), opts=dict(cycle_type="F", nested_iteration=True)),
    "67x35_tile_edge": dict(shapes=[(67, 35), (34, 18)], nt0=17, strides=(1, 4)),
}


@pytest.mark.parametrize("method", ["BE", "CN"])
@pytest.mark.parametrize("case", sorted(HEAT_CASES))
def test_heat2d_bit_identical_to_the_callers_path(case, method):
    c = HEAT_CASES[case]
    opts = dict(nested_iteration=False, max_iter=3, tol=0.0)
    opts.update(c.get("opts", {}))
    conv = both("heat", lambda: heat_problem(c["shapes"], c["nt0"], c["strides"], method), len(c["shapes"]), c.get("copies", ()), **opts)
    assert len(conv) == 3 and np.all(np.isfinite(conv))


AC_CASES = {"12": ([12, 6], (9, 5), ()), "20_copy_below": ([20, 10, 10], (9, 5, 3), (1,)), "66": ([66, 33], (9, 5), ())}


@pytest.mark.parametrize("nu", [2, 4])
@pytest.mark.parametrize("case", sorted(AC_CASES))
def test_allen_cahn_bit_identical_to_the_callers_path(case, nu):
    sizes, nts, copies = AC_CASES[case]
    conv = both("ac", lambda: ac_problem(sizes, nts, nu), len(sizes), copies, nested_iteration=False, max_iter=3, tol=0.0)
    assert len(conv) == 3 and np.all(np.isfinite(conv))


def test_conv_crit_1_bit_identical():
    both("heat", lambda: heat_problem([(17, 21), (9, 11)], 33, (1, 2)), 2, nested_iteration=False, max_iter=3, tol=0.0, conv_crit=1)
    both("ac", lambda: ac_problem([12, 6], (9, 5)), 2, nested_iteration=False, max_iter=3, tol=0.0, conv_crit=1)


def test_at_mgrit_bit_identical():
    """AT-MGRIT passes through the same sweeps (restrict_u, fas_rhs, error_correction); its truncated solves are the coarse level's own"""
    from pymgrit_amd import AtMgrit
    both("heat", lambda: heat_problem([(17, 21), (9, 11)], 33, (1, 2)), 2, solver=lambda **kw: AtMgrit(k=4, **kw),
         nested_iteration=False, max_iter=3, tol=0.0)


# ---- the sweeps alone ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,fine,coarse", [("heat", (5, 7), (3, 4)), ("heat", (67, 35), (34, 18)), ("ac", (66, 66), (33, 33))])
def test_sweeps_alone_equal_the_python_methods(kind, fine, coarse):
    from pymgrit_amd import Mgrit
    lib_cls, _ = _classes()[kind]
    py = lib_cls()

    def make(via_python):
        prob = heat_problem([fine, coarse], 9, (1, 2)) if kind == "heat" else ac_problem([fine[0], coarse[0]], (9, 5))
        return Mgrit(problem=prob, transfer=transfers(kind, 2, via_python), logging_lvl=30, nested_iteration=False)
    mg, twin = make(False), make(True)
    assert mg.backend._device_transfer(0) and not twin.backend._device_transfer(0)
    nf, nc = fine[0] * fine[1], coarse[0] * coarse[1]
    pairs = [(2 * j, j) for j in range(1, 5)]
    vec = type(mg.problem[0].vector_template)

    def apply(method, rows, shape):
        out = []
        for r in rows:
            v = vec(*shape)
            v.set_values(r.reshape(shape).copy())
            out.append(np.asarray(method(v).get_values()).ravel())
        return np.array(out)
    fi, co = [p[0] for p in pairs], [p[1] for p in pairs]

    def check(name, lvl, rows, want, n):
        got = _raw(mg, name, lvl)
        assert np.array_equal(got[rows, :n], want), name
        assert not got[:, n:].any()         # row pads stay zero
        untouched = np.setdiff1d(np.arange(got.shape[0]), rows)
        return got, untouched

    # restrict_u: u^{l+1}_j = R(u^l_i)
    _fill(mg, 1)
    before_f, before_c = _raw(mg, "u", 0).copy(), _raw(mg, "u", 1).copy()
    mg.backend.restrict_u(0, pairs)
    got, rest = check("u", 1, co, apply(py.restriction, before_f[fi, :nf], fine), nc)
    assert np.array_equal(got[rest], before_c[rest])
    # interpolate: u^l_i = P(u^{l+1}_j)
    _fill(mg, 2)
    before_f, before_c = _raw(mg, "u", 0).copy(), _raw(mg, "u", 1).copy()
    mg.backend.interpolate(0, pairs)
    got, rest = check("u", 0, fi, apply(py.interpolation, before_c[co, :nc], coarse), nf)
    assert np.array_equal(got[rest], before_f[rest])
    # error_correction: u^l_i = u^l_i + P(u^{l+1}_j - v^{l+1}_j)
    _fill(mg, 3)
    before_f, uc, vc = _raw(mg, "u", 0).copy(), _raw(mg, "u", 1).copy(), _raw(mg, "v", 1).copy()
    mg.backend.error_correction(0, pairs)
    got, rest = check("u", 0, fi, before_f[fi, :nf] + apply(py.interpolation, uc[co, :nc] - vc[co, :nc], coarse), nf)
    assert np.array_equal(got[rest], before_f[rest])
    # fas_rhs: the fine half, the Python restriction of the downloaded rows, the coarse half -- what the caller's path does
    _fill(mg, 4)
    _fill(twin, 4)
    mg.backend.fas_rhs(0, pairs)
    twin.backend.fas_rhs(0, pairs)
    assert np.array_equal(_raw(mg, "g", 1), _raw(twin, "g", 1))
    assert not _raw(mg, "g", 1)[:, nc:].any()
    for name, lvl in (("u", 0), ("u", 1), ("v", 1)):
        assert np.array_equal(_raw(mg, name, lvl), _raw(twin, name, lvl))


# ---- against the host plugin path ----------------------------------------------------------------------------------------------------
def test_heat2d_against_the_plugin_path():
    from pymgrit_amd import GridTransferCopy, GridTransferHeat2D
    out = {}
    for host in (True, False):
        prob = heat_problem([(17, 21), (9, 11), (9, 11)], 33, (1, 2, 4), host=host)
        conv, mg = solve(prob, [GridTransferHeat2D(), GridTransferCopy()], tol=1e-9, max_iter=8)
        assert (type(mg.backend).__name__ == "HipBackend") != host
        out[host] = (conv, np.array([np.asarray(mg.u[0][i].get_values()) for i in (5, 16, 32)]))
    (ch, uh), (cd, ud) = out[True], out[False]
    print("plugin", ch, "device", cd, "largest state deviation", np.max(np.abs(uh - ud)))
    assert len(ch) == len(cd) and np.all(np.abs(ch - cd) <= 1e-9 * ch + 2e-11), (ch, cd)
    assert np.max(np.abs(uh - ud)) <= 1e-11 * max(1.0, np.max(np.abs(uh)))


def test_allen_cahn_against_the_reference_solve():
    """20 -> 10 against the plugin path over ReferenceAllenCahn (transform-free long-double solve) on both levels: the tolerance of
    tests/test_hip_allen_cahn_reference.py::test_solve_with_several_step_sizes_per_level"""
    from allen_cahn_reference import ReferenceAllenCahn
    from pymgrit_amd import GridTransferAllenCahn
    opts = dict(nested_iteration=False, max_iter=3, tol=0.0)
    conv, dev = solve(ac_problem([20, 10], (17, 9)), [GridTransferAllenCahn()], **opts)
    rconv, ref = solve(ac_problem([20, 10], (17, 9), app=ReferenceAllenCahn), [GridTransferAllenCahn()], **opts)
    assert type(dev.backend).__name__ == "HipBackend" and type(ref.backend).__name__ == "PluginBackend"
    u = dev.backend.natural("u", 0)
    norm_u = cases.spacetime_norm(u)
    print("device", conv, "reference", rconv, "allowed beyond 1e-10 relative", cases.BLK_K * EPS * norm_u)
    assert len(conv) == len(rconv) == 3
    assert np.all(np.abs(conv - rconv) <= 1e-10 * rconv + cases.BLK_K * EPS * norm_u), (conv, rconv)
    last = np.asarray(ref.u[0][-1].get_values()).ravel()
    assert np.abs(u[-1] - last).max() <= 1e-9 * np.abs(last).max()


# ---- planned cycle -------------------------------------------------------------------------------------------------------------------
def test_planned_cycle_bit_identical_to_program_order():
    """Heat2D 17 x 21 -> 9 x 11, nt = 513 / 129, the coarse level solved step by step: two blocks (sweeps and the coarse solve on two
    streams; the FAS sweep's scratch rows are written and read on the sweep stream only) against program order"""
    from pymgrit_amd import GridTransferHeat2D
    from pymgrit_amd.core.options import options
    out = {}
    try:
        options.coarse_solve = "sequential"
        for blocks in (1, 2):
            options.plan_blocks_heat2d = blocks
            conv, mg = solve(heat_problem([(17, 21), (9, 11)], 513, (1, 4)), [GridTransferHeat2D()], nested_iteration=False, max_iter=3, tol=0.0)
            assert not mg.backend._host_transfers() and mg.plan_blocks() == blocks
            if blocks > 1:
                assert any(p is not None for p in mg._plans.values())      # the cycle was recorded and ran as a plan
            out[blocks] = (conv, mg.backend.natural("u", 0))
    finally:
        options.reset("coarse_solve", "plan_blocks_heat2d")
    print(out[1][0], out[2][0])
    assert np.array_equal(out[1][0], out[2][0])
    assert np.array_equal(out[1][1], out[2][1])


# ---- ranks ---------------------------------------------------------------------------------------------------------------------------
def test_heat2d_on_ranks_bit_identical_to_one_rank():
    from pymgrit_amd import GridTransferHeat2D, Mgrit
    from pymgrit_amd.core.comm import run_loopback_ranks

    def target(comm):
        mg = Mgrit(heat_problem([(17, 21), (9, 11)], 33, (1, 4)), transfer=[GridTransferHeat2D()], logging_lvl=30, comm_time=comm,
                   nested_iteration=False, max_iter=3, tol=0.0)
        conv = mg.solve()["conv"]
        return conv, np.array([np.asarray(mg.u[0][int(i)].pack()).ravel() for i in mg.index_local[0]])
    _, (one,) = run_loopback_ranks(1, target)
    for world in (2, 3):
        w, res = run_loopback_ranks(world, target)
        w.close()
        assert all(np.array_equal(r[0], one[0]) for r in res)
        assert np.array_equal(np.concatenate([r[1] for r in res if r[1].size], axis=0), one[1])


def test_allen_cahn_on_ranks_stays_refused():
    """Allen-Cahn levels run on one time rank (tests/test_hip_allen_cahn.py::test_what_is_not_covered_is_refused pins the refusal): a
    hierarchy 12 -> 6, nt = 33 / 9 with the library transfer on two ranks is refused by that name, not run differently"""
    from pymgrit_amd import GridTransferAllenCahn, Mgrit
    from pymgrit_amd.core.comm import run_loopback_ranks
    from pymgrit_amd.core.hip_lib import MgritHipError

    def target(comm):
        Mgrit(ac_problem([12, 6], (33, 9)), transfer=[GridTransferAllenCahn()], logging_lvl=30, comm_time=comm, nested_iteration=False)
    with pytest.raises(MgritHipError, match="one time rank only"):
        run_loopback_ranks(2, target, timeout=60)


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_level_transfer_refusals_leave_the_engine_usable():
    from pymgrit_amd.core import hip_lib
    lib = hip_lib.load()

    def ptr(a):
        return C.c_void_p(a.ctypes.data)

    def heat2d(eng, lvl, nx, ny, t):
        ld = ((nx * ny + 15) // 16) * 16
        bc = np.zeros(nx * ny)
        assert lib.mgrit_hip_level_heat2d(eng, lvl, t.size, ptr(t), nx, ny, ld, 1.0, 1.0, 1.0, ptr(bc), 0, None, None) == 0
        return ld
    eng = C.c_void_p()
    assert lib.mgrit_hip_create(C.byref(eng), 4, C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    try:
        t0 = np.ascontiguousarray(np.linspace(0, 1, 9))
        t1 = np.ascontiguousarray(t0[::2])
        ldf = heat2d(eng, 0, 9, 11, t0)
        ldc = heat2d(eng, 1, 5, 7, t1)            # 2*7 - 1 = 13, not 11
        n1 = 13
        s, tau = np.zeros((0, n1)), np.zeros((0, t1.size))
        assert lib.mgrit_hip_level_heat1d(eng, 2, t1.size, ptr(t1), n1, lib.mgrit_hip_row_stride(n1), 1.0, 0, ptr(s), ptr(tau)) == 0
        assert lib.mgrit_hip_level_heat1d(eng, 3, t1.size, ptr(t1), n1, lib.mgrit_hip_row_stride(n1), 1.0, 0, ptr(s), ptr(tau)) == 0
        rc = lib.mgrit_hip_level_transfer(eng, 0, hip_lib.TRANSFER_HEAT2D)
        msg = lib.mgrit_hip_last_error().decode()
        assert rc == -1 and "9x11" in msg and "5x7" in msg, (rc, msg)            # MGRIT_HIP_EINVAL with the sizes
        rc = lib.mgrit_hip_level_transfer(eng, 2, hip_lib.TRANSFER_HEAT2D)      # 1-D levels
        assert rc == -4 and "Heat2D transfer joins two Heat2D levels" in lib.mgrit_hip_last_error().decode()
        rc = lib.mgrit_hip_level_transfer(eng, 1, hip_lib.TRANSFER_HEAT2D)      # Heat2D above a 1-D level
        assert rc == -4
        rc = lib.mgrit_hip_level_transfer(eng, 0, hip_lib.TRANSFER_PERIODIC2D)  # the periodic kind on Heat2D levels
        assert rc == -4 and "two Allen-Cahn levels" in lib.mgrit_hip_last_error().decode()
        for kind in (hip_lib.TRANSFER_HEAT1D, 2):                                # the messages of the 1-D kinds on 2-D levels stay
            assert lib.mgrit_hip_level_transfer(eng, 0, kind) == -4
            assert "Heat2D levels support the copy transfer only" in lib.mgrit_hip_last_error().decode()
        # the engine is still usable: an F-relaxation of the fine level (zero state, zero rim, no forcing) leaves zeros
        u = torch.zeros((t0.size, ldf), dtype=torch.float64, device="cuda")
        assert lib.mgrit_hip_level_bind(eng, 0, C.c_void_p(u.data_ptr()), None, None) == 0
        start, length, rid = np.array([1], dtype=np.int32), np.array([3], dtype=np.int32), C.c_int(-1)
        assert lib.mgrit_hip_runs_create(eng, 0, 1, ptr(start), ptr(length), C.byref(rid)) == 0
        assert lib.mgrit_hip_relax(eng, 0, rid.value, hip_lib.RELAX_F, 1.0) == 0
        assert lib.mgrit_hip_sync(eng) == 0
        assert not u.cpu().numpy().any() and ldc > 0
    finally:
        assert lib.mgrit_hip_destroy(eng) == 0
