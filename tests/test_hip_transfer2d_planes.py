"""GPU: the periodic 2-D library transfer on rows of two planes (csrc/mgrit_hip_transfer2d.inc): Gray-Scott and Burgers
hierarchies with spatial coarsening, GridTransferGrayScott / GridTransferBurgers as kernels.

Yardstick of the bit-identity tests, as in tests/test_hip_transfer2d.py: the same hierarchy with a subclass that overrides restriction and
interpolation by calling super() -- the backend then applies the Python methods row by row on the host between the kernels
(MGRIT_HIP_TRANSFER_CALLER), every Phi stays the same device code, so the kernels must reproduce the Python spec bit for bit. That path
takes one bit pattern of dt per level: [0, 0.25] (Burgers) and [0, 0.5] (Gray-Scott) in 8, 4 and 2 steps (asserted).

Sizes: 12 -> 6 (one tile per coarse row), 20 -> 10 -> 10 (the copy transfer below), 66 -> 33: a coarse plane is 1089 values and a fine one
4356, so the border between the planes falls inside a 256-wide tile and inside a 16-value pad group, and nx is no multiple of the 64 the
products pad to."""
import ctypes as C

import numpy as np
import pytest

import cases
from transfer2d_cases import fill as _fill, one_step_size as _one_step_size, raw as _raw, solve

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

EPS = cases.EPS
T_STOP = {"burgers": 0.25, "grayscott": 0.5, "grayscott_impl": 0.5}


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU visible")


def _classes(kind):
    """(the library class, a subclass of it on the caller's path)"""
    from pymgrit_amd import GridTransferBurgers, GridTransferGrayScott
    lib = GridTransferBurgers if kind == "burgers" else GridTransferGrayScott

    class ViaPython(lib):      # overridden methods: the caller's path
        def restriction(self, u):
            return super().restriction(u)

        def interpolation(self, u):
            return super().interpolation(u)
    return lib, ViaPython


def problem(kind, sizes, nts, host=False):
    from pymgrit_amd import Burgers2D, GrayScott
    grid = dict(t_start=0, t_stop=T_STOP[kind])
    if kind == "burgers":
        cls = Burgers2D
        par = {}
    else:
        cls = GrayScott
        par = dict(method="IMPL", linear_solver="bicgstab") if kind == "grayscott_impl" else dict(method="IMEX")
    if host:
        class Host(cls):     # overriding step sends the hierarchy to the plugin path (_host_class in tests/test_hip_burgers.py)
            def step(self, u_start, t_start, t_stop):
                return super().step(u_start, t_start, t_stop)
        cls = Host
    return [cls(nx=nx, nt=nt, **par, **grid) for nx, nt in zip(sizes, nts)]


def transfers(kind, n_levels, via_python, copies=()):
    from pymgrit_amd import GridTransferCopy
    lib, py = _classes(kind)
    return [GridTransferCopy() if lvl in copies else (py if via_python else lib)() for lvl in range(n_levels - 1)]


def both(kind, sizes, nts, copies=(), **opts):
    """(library transfer, the same through the Python methods): residual histories and all level-0 states"""
    out = []
    for via_python in (False, True):
        prob = problem(kind, sizes, nts)
        for p in prob:
            assert _one_step_size(p.t)
        conv, mg = solve(prob, transfers(kind, len(sizes), via_python, copies), **opts)
        assert mg.backend.name == "hip"
        for lvl in range(len(sizes) - 1):
            assert mg.backend._device_transfer(lvl) == (not via_python or lvl in copies)
        out.append((conv, mg.backend.natural("u", 0)))
    (c0, u0), (c1, u1) = out
    print("residual histories:", c0, c1)
    assert len(c0) == len(c1) and np.array_equal(c0, c1), (c0, c1)
    assert u0.shape == (nts[0], 2 * sizes[0] ** 2) and np.array_equal(u0, u1)
    return c0


CASES = {"12": ([12, 6], (9, 5), ()), "20_copy_below": ([20, 10, 10], (9, 5, 3), (1,)), "66": ([66, 33], (9, 5), ())}
OPTS = dict(nested_iteration=False, max_iter=3, tol=0.0)


@pytest.mark.parametrize("kind,case", [(k, c) for k in ("burgers", "grayscott") for c in sorted(CASES)] + [("grayscott_impl", "12")])
def test_bit_identical_to_the_callers_path(kind, case):
    sizes, nts, copies = CASES[case]
    conv = both(kind, sizes, nts, copies, **OPTS)
    assert len(conv) == 3 and np.all(np.isfinite(conv)) and conv[0] > 0.0


@pytest.mark.parametrize("kind", ["burgers", "grayscott"])
def test_conv_crit_1_bit_identical(kind):
    both(kind, [12, 6], (9, 5), conv_crit=1, **OPTS)


# ---- the sweeps alone ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,fine,coarse", [(k, f, f // 2) for k in ("burgers", "grayscott") for f in (12, 66)])
def test_sweeps_alone_equal_the_python_methods(kind, fine, coarse):
    from pymgrit_amd import Mgrit
    lib_cls, _ = _classes(kind)
    py = lib_cls()

    def make(via_python):
        return Mgrit(problem=problem(kind, [fine, coarse], (9, 5)), transfer=transfers(kind, 2, via_python), logging_lvl=30, nested_iteration=False)
    mg, twin = make(False), make(True)
    assert mg.backend._device_transfer(0) and not twin.backend._device_transfer(0)
    nf, nc = 2 * fine * fine, 2 * coarse * coarse
    assert mg.backend.n[:2] == [nf, nc] and mg.backend.ld[:2] == [(nf + 15) // 16 * 16, (nc + 15) // 16 * 16]
    pairs = [(2 * j, j) for j in range(1, 5)]
    vec = type(mg.problem[0].vector_template)

    def apply(method, rows, nx):
        out = []
        for r in rows:
            v = vec(nx)
            v.set_values(r.reshape(2, nx, nx).copy())
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
    g = _raw(mg, "g", 1)
    assert np.array_equal(g, _raw(twin, "g", 1)) and np.all(np.isfinite(g)) and g[co, :nc].any()
    assert not g[:, nc:].any()
    for name, lvl in (("u", 0), ("u", 1), ("v", 1)):
        assert np.array_equal(_raw(mg, name, lvl), _raw(twin, name, lvl))


@pytest.mark.parametrize("kind", ["burgers", "grayscott"])
def test_error_correction_to_rows_of_its_own(kind):
    """the rows_out form (mgrit_hip_error_correction_to): the corrected rows land in a buffer of the caller's, u of the fine level keeps
    every bit, and the rows are those the in-place sweep writes"""
    from pymgrit_amd import Mgrit
    fine, coarse = 66, 33
    mg = Mgrit(problem=problem(kind, [fine, coarse], (9, 5)), transfer=transfers(kind, 2, False), logging_lvl=30, nested_iteration=False)
    b = mg.backend
    _fill(mg, 5)
    nf, ld = 2 * fine * fine, b.ld[0]
    pairs = [(2 * j, j) for j in range(1, 5)]
    before = _raw(mg, "u", 0).copy()
    rows = torch.full((len(pairs), ld), 7.0, dtype=torch.float64, device="cuda")
    from pymgrit_amd.core.hip_lib import check
    check(b.lib.mgrit_hip_error_correction_to(b.h, 0, b._list_id("pairs", 0, pairs), C.c_void_p(rows.data_ptr()), ld))
    b.sync()
    assert np.array_equal(_raw(mg, "u", 0), before)
    b.error_correction(0, pairs)
    got, out = _raw(mg, "u", 0), rows.cpu().numpy()
    assert np.array_equal(out[:, :nf], got[[p[0] for p in pairs], :nf]) and not np.array_equal(out[:, :nf], before[[p[0] for p in pairs], :nf])
    assert np.all(out[:, nf:] == 7.0)       # behind the two planes nothing is written


# ---- against the host plugin path ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["burgers", "grayscott"])
def test_solve_matches_the_plugin_path(kind):
    """[12, 6, 6], nt 17 / 9 / 5, V cycle, three iterations from the initial guess, the plugin side over a subclass that overrides step:
    residual histories by the rule of the applications' own solve tests (tests/cases.py)"""
    from pymgrit_amd import GridTransferCopy
    lib_cls, _ = _classes(kind)
    opts = dict(cycle_type="V", **OPTS)
    conv, dev = solve(problem(kind, [12, 6, 6], (17, 9, 5)), [lib_cls(), GridTransferCopy()], **opts)
    rconv, ref = solve(problem(kind, [12, 6, 6], (17, 9, 5), host=True), [lib_cls(), GridTransferCopy()], **opts)
    assert type(dev.backend).__name__ == "HipBackend" and type(ref.backend).__name__ == "PluginBackend"
    for a, b in zip(dev.t, ref.t):
        assert np.array_equal(a, b)
    norm_u = cases.spacetime_norm(dev.backend.natural("u", 0))
    assert len(conv) == len(rconv) == 3 and np.all(rconv > 0.0), (conv, rconv)
    print(f"RATIO solve[{kind}] conv {conv} plugin {rconv}: largest deviation {np.max(np.abs(conv - rconv)) / (EPS * norm_u):.2f} units of "
          f"eps*norm(u) (allowed {cases.BLK_K} beyond 1e-10 relative)")
    assert np.all(np.abs(conv - rconv) <= 1e-10 * rconv + cases.BLK_K * EPS * norm_u), (conv, rconv)


# ---- what is refused, through Mgrit --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,name", [("burgers", "Burgers"), ("grayscott", "Gray-Scott")])
def test_refused_by_name(kind, name):
    from pymgrit_amd import GridTransferAllenCahn, Mgrit
    from pymgrit_amd.core.comm import run_loopback_ranks
    from pymgrit_amd.core.hip_lib import MgritHipError
    own, _ = _classes(kind)
    other, _ = _classes("grayscott" if kind == "burgers" else "burgers")
    head = name + " levels on the HIP engine: "
    with pytest.raises(MgritHipError, match=head + f"{own.__name__}.*nx_fine = 2 \\* nx_coarse, not nx 12 and 5"):
        Mgrit(problem(kind, [12, 5], (9, 5)), transfer=[own()], logging_lvl=30)
    with pytest.raises(MgritHipError, match=head + f"{own.__name__}.*not nx 12 and 12"):
        Mgrit(problem(kind, [12, 12], (9, 5)), transfer=[own()], logging_lvl=30)
    for cls in (other, GridTransferAllenCahn):
        with pytest.raises(MgritHipError, match=head + f"{cls.__name__} between levels of nx 12 and 6"):
            Mgrit(problem(kind, [12, 6], (9, 5)), transfer=[cls()], logging_lvl=30)

    def target(comm):
        Mgrit(problem(kind, [12, 6], (33, 9)), transfer=[own()], logging_lvl=30, comm_time=comm, nested_iteration=False)
    with pytest.raises(MgritHipError, match=head + "one time rank only"):
        run_loopback_ranks(2, target, timeout=60)


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_level_transfer_on_two_plane_levels():
    from pymgrit_amd import Burgers2D, GrayScott
    from pymgrit_amd.core import hip_lib
    lib = hip_lib.load()

    def ptr(a):
        return C.c_void_p(a.ctypes.data)
    eng = C.c_void_p()
    assert lib.mgrit_hip_create(C.byref(eng), 6, C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    try:
        t0 = np.ascontiguousarray(np.linspace(0, 0.25, 9))
        t1 = np.ascontiguousarray(t0[::2])
        ld = {nx: ((2 * nx * nx + 15) // 16) * 16 for nx in (12, 5, 8, 4)}
        hip_lib.level_2d(eng, 0, t0.size, ptr(t0), ld[12], Burgers2D(nx=12, t_interval=t0).device_stepper())
        hip_lib.level_2d(eng, 1, t1.size, ptr(t1), ld[5], Burgers2D(nx=5, t_interval=t1).device_stepper())       # 2 * 5 = 10, not 12
        hip_lib.level_2d(eng, 2, t1.size, ptr(t1), ld[8], GrayScott(nx=8, method="IMEX", t_interval=t1).device_stepper())
        hip_lib.level_2d(eng, 3, t1.size, ptr(t1), ld[4],
                         GrayScott(nx=4, method="IMPL", linear_solver="bicgstab", t_interval=t1).device_stepper())
        hip_lib.level_2d(eng, 4, t1.size, ptr(t1), ld[4], Burgers2D(nx=4, t_interval=t1).device_stepper())
        hip_lib.level_2d(eng, 5, t1.size, ptr(t1), ld[4], Burgers2D(nx=4, t_interval=t1).device_stepper())
        rc = lib.mgrit_hip_level_transfer(eng, 0, hip_lib.TRANSFER_PERIODIC2D)
        msg = lib.mgrit_hip_last_error().decode()
        assert rc == -1 and "12x12" in msg and "5x5" in msg, (rc, msg)            # MGRIT_HIP_EINVAL with both sizes
        rc = lib.mgrit_hip_level_transfer(eng, 1, hip_lib.TRANSFER_PERIODIC2D)    # a Burgers above a Gray-Scott level
        assert rc == -4, (rc, lib.mgrit_hip_last_error().decode())                # MGRIT_HIP_EUNSUPPORTED
        rc = lib.mgrit_hip_level_transfer(eng, 3, hip_lib.TRANSFER_PERIODIC2D)    # a Gray-Scott above a Burgers level of the same nx
        assert rc == -4, (rc, lib.mgrit_hip_last_error().decode())
        rc = lib.mgrit_hip_level_transfer(eng, 4, hip_lib.TRANSFER_PERIODIC2D)    # two Burgers levels of one nx: the copy is theirs
        assert rc == -4 and "copy transfer" in lib.mgrit_hip_last_error().decode()
        assert lib.mgrit_hip_level_transfer(eng, 4, hip_lib.TRANSFER_COPY) == 0
        assert lib.mgrit_hip_level_transfer(eng, 0, hip_lib.TRANSFER_HEAT2D) == -4     # the Heat2D kind on periodic levels
        assert "Heat2D transfer joins two Heat2D levels" in lib.mgrit_hip_last_error().decode()
        assert lib.mgrit_hip_level_transfer(eng, 2, hip_lib.TRANSFER_PERIODIC2D) == 0  # the two forms of Gray-Scott, 8 -> 4
        # the engine is still usable: an F-relaxation of the fine Burgers level from zeros leaves zeros
        u = torch.zeros((t0.size, ld[12]), dtype=torch.float64, device="cuda")
        assert lib.mgrit_hip_level_bind(eng, 0, C.c_void_p(u.data_ptr()), None, None) == 0
        start, length, rid = np.array([1], dtype=np.int32), np.array([3], dtype=np.int32), C.c_int(-1)
        assert lib.mgrit_hip_runs_create(eng, 0, 1, ptr(start), ptr(length), C.byref(rid)) == 0
        assert lib.mgrit_hip_relax(eng, 0, rid.value, hip_lib.RELAX_F, 1.0) == 0
        assert lib.mgrit_hip_sync(eng) == 0
        assert not u.cpu().numpy().any()
    finally:
        assert lib.mgrit_hip_destroy(eng) == 0
