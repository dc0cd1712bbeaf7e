"""GPU: the FAS sweep of a coarse level with its F-relaxation over chunks of consecutive intervals (ffas_kernel behind
mgrit_hip_fas_fused_opts(MGRIT_HIP_FAS_WITH_F_RELAX), chunk length by mgrit_hip_set_fas_chunk) against the oracle and against the
item-by-item kernel it stands for (fas_fused1_kernel, set_fas_chunk(-1)): the same Phi applications on the same values, so
everything is bit-identical.

Shapes: one state size per compiled instance (one wave / 512 threads / 1024 threads with two padding positions in the last
group); level 1 of the 145-point grid has 9 intervals, so chunks of 1, 2, 3, 4, 16 give full chunks, a ragged last chunk and a
list that is one chunk; the 4-level grid runs the sweep on level 1 (u of the next level stored) and on level 2 (not stored)."""
import ctypes as C

import numpy as np
import pytest

import cases
from parity_cases import need_gpu as _need_gpu, assert_state_equal, heat_problem, make_pair, randomize

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

NXS = [1024, 4099, 16384]
CHUNKS = (0, 1, 2, 3, 4, 16)


def grids_m4():
    t = cases.lin(2, 145)
    return [t, t[::4], t[::16]]


def grids_m2():
    t = cases.lin(2, 65)
    return [t, t[::2], t[::4], t[::8]]


def grids_two_dt():
    """145 points, the step size changes at point 72: inside interval 5 of level 1 (points 16..20 there) and, as a step made of
    both sizes, at step 5 of level 2 -- with chunks of 4 the coefficient set of either level changes inside the second chunk"""
    t = np.concatenate((np.linspace(0.0, 1.0, 73), 1.0 + np.linspace(0.0, 2.0, 73)[1:]))
    return [t, t[::4], t[::16]]


def two_term_pair(oracle, nx, grids):
    from pymgrit_amd import Heat1D, Mgrit
    terms = cases.BDF_FORCING["two"]
    prob = [Heat1D(x_start=0, x_end=1, nx=nx, a=1, init_cond=cases.init_cond, rhs_separable=terms, t_interval=np.asarray(t))
            for t in grids]
    specs = []
    x, _ = cases.heat_grid(nx)
    for t in grids:
        s = cases.heat_level_spec(nx, t, forcing=False)
        s["s"] = np.array([f(x) for f, _ in terms])
        s["tau"] = np.array([[g(tt) for tt in t] for _, g in terms])
        specs.append(s)
    return Mgrit(prob, logging_lvl=30, nested_iteration=False), oracle.OracleProblem(specs, variant=1, nested_iteration=False)


def expected_chunks(mg, lvl, chunk):
    """chunks of a whole level's list (no gaps): ceil(items / chunk); 0 = item by item (-1, and the rule on a one-group level);
    the rule gives every list of these tests (fewer items than the chip holds workgroups) chunks of 1"""
    items = len(mg._coarse_down(lvl)[1])
    if chunk < 0 or (chunk == 0 and mg.backend.n[lvl] <= 1024):
        return 0
    return items if chunk == 0 else -(-items // chunk)


def assert_chunked_kernel_is_routed(mg, chunk):
    """which kernel the sweeps will run: the library's own count of the chunks it launches over (both kernels give the same bits,
    so no comparison of values could tell)"""
    for lvl in range(1, mg.lvl_max - 1):
        assert mg.backend.fas_chunks(lvl, mg._coarse_down(lvl)[1]) == expected_chunks(mg, lvl, chunk), (lvl, chunk)


def cycles_against_oracle(mg, op, chunk, cycle, seed):
    mg.backend.set_fas_chunk(chunk)
    assert all(mg._coarse_down(lvl) is not None for lvl in range(1, mg.lvl_max - 1))   # the sweep under test is on the way down
    assert_chunked_kernel_is_routed(mg, chunk)
    randomize(mg, op, seed=seed)
    for it in range(3):
        mg.iteration(lvl=0, cycle_type=cycle, iteration=it, first_f=True)
        op.iteration(0, cycle, it, True)
        mg.backend.materialise()
        assert_state_equal(mg, op, what=("u",))


@pytest.mark.parametrize("chunk", [1, 2, 3, 4, 16])
@pytest.mark.parametrize("forcing", [False, True], ids=["noforcing", "forcing"])
@pytest.mark.parametrize("nx", NXS)
def test_cycles_match_the_oracle(oracle, nx, forcing, chunk):
    _need_gpu()
    for cycle in ("V", "F"):
        mg, op = make_pair(oracle, "heat", nx, grids_m4(), forcing=forcing)
        cycles_against_oracle(mg, op, chunk, cycle, seed=nx + chunk)


@pytest.mark.parametrize("chunk", [0, 3])
@pytest.mark.parametrize("nx", NXS)
def test_four_levels_match_the_oracle(oracle, nx, chunk):
    """m = 2, 65 points: the sweep on level 1 stores u of level 2, the one on level 2 need not store u of the coarsest level"""
    _need_gpu()
    for cycle in ("V", "F"):
        mg, op = make_pair(oracle, "heat", nx, grids_m2())
        assert mg._coarse_down(1)[3] is False and mg._coarse_down(2)[3] is True
        cycles_against_oracle(mg, op, chunk, cycle, seed=11)


@pytest.mark.parametrize("nx", NXS)
def test_step_size_changes_inside_a_chunk(oracle, nx):
    _need_gpu()
    for cycle in ("V", "F"):
        mg, op = make_pair(oracle, "heat", nx, grids_two_dt())
        cycles_against_oracle(mg, op, 4, cycle, seed=13)


@pytest.mark.parametrize("nx", NXS)
def test_two_forcing_terms_match_the_oracle(oracle, nx):
    _need_gpu()
    for cycle in ("V", "F"):
        mg, op = two_term_pair(oracle, nx, grids_m4())
        cycles_against_oracle(mg, op, 4, cycle, seed=17)


@pytest.mark.parametrize("blocks", [1, 3])
@pytest.mark.parametrize("nx", [1024, 16384])
def test_planned_blocks_match_the_oracle(oracle, nx, blocks):
    """a planned cycle hands the sweep one list per block of time points: each is cut into chunks at its own ends"""
    _need_gpu()
    from pymgrit_amd import Mgrit
    grids = grids_m4()
    _, op = make_pair(oracle, "heat", nx, grids)
    mg = Mgrit(heat_problem(nx, grids), logging_lvl=30, nested_iteration=False, plan_blocks=blocks)
    cycles_against_oracle(mg, op, 2, "V", seed=19)


def sweep_outputs(mg, op, lvl, chunk, seed):
    """u, v, g of level lvl + 1 after ONE sweep from the seeded state"""
    _, triples, _, skip_u = mg._coarse_down(lvl)
    mg.backend.set_fas_chunk(chunk)
    assert mg.backend.fas_chunks(lvl, triples) == expected_chunks(mg, lvl, chunk), (lvl, chunk)
    randomize(mg, op, seed=seed)
    mg.backend.fas_fused(lvl, triples, with_f_relax=True, skip_coarse_u=skip_u)
    return [mg.backend.natural(name, lvl + 1) for name in ("u", "v", "g")]


@pytest.mark.parametrize("grids", [grids_m4, grids_m2, grids_two_dt], ids=["m4", "m2_4lvl", "two_dt"])
@pytest.mark.parametrize("forcing", [False, True], ids=["noforcing", "forcing"])
@pytest.mark.parametrize("nx", NXS)
def test_sweep_equals_the_item_by_item_kernel(oracle, nx, forcing, grids):
    """A/B in one process, sweep by sweep: every chunk setting against set_fas_chunk(-1)"""
    _need_gpu()
    mg, op = make_pair(oracle, "heat", nx, grids(), forcing=forcing)
    for lvl in range(1, mg.lvl_max - 1):
        want = sweep_outputs(mg, op, lvl, -1, seed=lvl)
        for chunk in CHUNKS:
            got = sweep_outputs(mg, op, lvl, chunk, seed=lvl)
            for name, a, b in zip("uvg", got, want):
                assert np.array_equal(a, b), (name, lvl, chunk)


@pytest.mark.parametrize("nx", NXS)
def test_cycles_equal_the_item_by_item_kernel(oracle, nx):
    """A/B in one process, whole cycles: states of every coarse level and the residual history"""
    _need_gpu()

    def run(chunk):
        mg, op = make_pair(oracle, "heat", nx, grids_m4(), max_iter=3)
        mg.backend.set_fas_chunk(chunk)
        randomize(mg, op, seed=23)
        for it in range(3):
            mg.iteration(lvl=0, cycle_type="V", iteration=it, first_f=True)
            mg.convergence_criterion(iteration=it + 1)
        return mg.conv.copy(), [mg.backend.natural(name, lvl) for lvl in (1, 2) for name in ("u", "v", "g")]

    conv0, st0 = run(-1)
    assert np.all(conv0[1:4] > 0)
    for chunk in (0, 3, 4):
        conv, st = run(chunk)
        assert np.array_equal(conv, conv0), (chunk, conv, conv0)
        for a, b in zip(st, st0):
            assert np.array_equal(a, b), chunk


def test_set_fas_chunk_rejects_a_length_below_minus_one(oracle):
    _need_gpu()
    from pymgrit_amd.core import hip_lib
    lib = hip_lib.load()
    mg, _ = make_pair(oracle, "heat", 33, [cases.lin(2, 17), cases.lin(2, 5)])
    assert lib.mgrit_hip_set_fas_chunk(mg.backend.h, -2) != 0
    assert b"chunk" in lib.mgrit_hip_last_error()
    assert lib.mgrit_hip_set_fas_chunk(C.c_void_p(None), 0) != 0
    for ok in (-1, 0, 5):
        assert lib.mgrit_hip_set_fas_chunk(mg.backend.h, ok) == 0


def test_chunk_count_of_a_list_with_a_gap(oracle):
    """the library's cut of a list: items join only while each starts where the one before ends, a gap ends a chunk, and a length
    asked for a second time is served from the views made before"""
    _need_gpu()
    from pymgrit_amd.core import hip_lib
    from pymgrit_amd.core.hip_lib import check
    lib = hip_lib.load()
    mg, _ = make_pair(oracle, "heat", 4099, grids_m4())
    h = mg.backend.h
    # level 1 has 37 points, C-points 0, 4, .., 36: the items ending on 4 .. 20 and on 28 .. 36 -- the item ending on 24 is left out
    fine = np.array([4, 8, 12, 16, 20, 28, 32, 36], dtype=np.int32)
    prev, coarse = fine - 4, fine // 4
    tid, n = C.c_int(-1), C.c_int(-1)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    check(lib.mgrit_hip_triples_create(h, 1, len(fine), ptr(fine), ptr(prev), ptr(coarse), C.byref(tid)))
    for chunk, want in ((-1, 0), (0, 8), (1, 8), (2, 5), (3, 3), (4, 3), (16, 2), (2, 5), (-1, 0), (16, 2)):
        check(lib.mgrit_hip_set_fas_chunk(h, chunk))
        check(lib.mgrit_hip_fas_chunks(h, 1, tid.value, C.byref(n)))
        assert n.value == want, (chunk, n.value, want)
    # a list of level 0 is never chunked (the sweep with its F-relaxation is for levels > 0)
    f0 = np.array([4, 8], dtype=np.int32)
    check(lib.mgrit_hip_triples_create(h, 0, 2, ptr(f0), ptr(f0 - 4), ptr(f0 // 4), C.byref(tid)))
    check(lib.mgrit_hip_fas_chunks(h, 0, tid.value, C.byref(n)))
    assert n.value == 0
