"""What the host-side table builders of libmgrit_hip.so produce, pinned bit for bit where the oracle comparison is by tolerance or
absent: every case describes one small level through the raw C ABI (ctypes only), binds seeded u / v / g, runs F-relaxation,
C-relaxation, the residual of the C-points and, on a level > 0, the MGRIT_HIP_RELAX_CHAIN forward solve over all steps, and compares
the sha256 of u at the live positions (after the relaxations and after the forward solve) and of the residual values with
tests/golden/level_tables.json. The residual is taken twice: after the C-relaxation, where the sequence asks for it, it is exactly
zero at every C-point (weight 1: u_i = Phi(u_{i-1}) was just assigned), so it is also taken between the two relaxations, where it is
not. The recording was made on an MI355X with the library as it stood before the host side got one builder per table (two
recordings, byte-identical); a refactor of the builders must reproduce it unchanged.

The shapes are the smallest at which a builder can go wrong: a partial last group, several coefficient sets with one that comes
back, a second group of 6 values (the overlapped chain's tables), five time blocks the last of which has a remainder, both Fourier
forms of Advection1D, both BDF orders, a Heat2D grid with a non-zero rim and two block step-size sequences, the Hartley table of
Allen-Cahn, and one state wider than a workgroup holds."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "level_tables.json")
M = 4                                  # coarsening factor of the run lists: C-points at 4, 8, ...
RELAX_F, RELAX_C, RELAX_CHAIN = 0, 1, 2


def _ptr(a):
    return C.c_void_p(a.ctypes.data) if a is not None else C.c_void_p(0)


def _dev(t):
    return C.c_void_p(t.data_ptr())


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest()


def _grid(dts):
    return np.ascontiguousarray(np.concatenate(([0.0], np.cumsum(np.asarray(dts, dtype=np.float64)))))


def _perm(lib, n):
    return np.array([lib.mgrit_hip_row_position(n, j) for j in range(n)])


# --- the time grids -------------------------------------------------------------------------------------------------
# (step sizes with a few mantissa bits: the grid points are exact, so equal steps are equal bit for bit -- one coefficient set each)
DT = 2.0 ** -7


def t_three_sizes():      # nt = 17: three distinct step sizes, the first of them comes back behind the other two
    return _grid([DT] * 4 + [1.5 * DT] * 4 + [0.75 * DT] * 4 + [DT] * 4)


def t_uniform(nt):
    return _grid([DT] * (nt - 1))


def t_nonuniform(nt):     # every step its own size
    return _grid(0.01 * (1.0 + 0.25 * np.sin(np.arange(nt - 1))))


def t_two_sequences():    # nt = 84: 83 steps = blocks of 16 with the same sequence of two sizes, and a last block of 19
    return _grid([DT if (i % 16) < 8 else 1.25 * DT for i in range(83)])


def t_pairs(nt):          # two-point steppers: two step sizes, both above dtau
    return _grid([2 * DT if (i % 3) else 3 * DT for i in range(nt - 1)])


# --- the descriptors: each returns (live positions of a row, ld) after describing level lvl ---------------------------
def heat1d(lib, eng, lvl, t, rng, n, fac, K):
    ld, perm = lib.mgrit_hip_row_stride(n), _perm(lib, n)
    s = np.ascontiguousarray(rng.standard_normal((K, n))) if K else None
    tau = np.ascontiguousarray(rng.standard_normal((K, t.size))) if K else None
    assert lib.mgrit_hip_level_heat1d(eng, lvl, t.size, _ptr(t), n, ld, fac, K, _ptr(s), _ptr(tau)) == 0
    return perm, ld


def advection1d(lib, eng, lvl, t, rng, n, fac):
    ld = lib.mgrit_hip_row_stride(n)
    assert lib.mgrit_hip_level_advection1d(eng, lvl, t.size, _ptr(t), n, ld, fac) == 0
    return _perm(lib, n), ld


def heat1d_2pts(lib, eng, lvl, t, rng, n, fac, dtau, order, K):
    half, perm = lib.mgrit_hip_row_stride(n), _perm(lib, n)
    s = np.ascontiguousarray(rng.standard_normal((K, n)))
    tau, tau2 = (np.ascontiguousarray(rng.standard_normal((K, t.size))) for _ in range(2))
    assert lib.mgrit_hip_level_heat1d_2pts(eng, lvl, t.size, _ptr(t), n, 2 * half, fac, dtau, order, K, _ptr(s), _ptr(tau), _ptr(tau2)) == 0
    return np.concatenate((perm, half + perm)), 2 * half


def heat2d(lib, eng, lvl, t, rng, nx, ny, theta, K):
    ld = (nx * ny + 15) // 16 * 16
    bc = rng.standard_normal((nx, ny))
    bc[1:-1, 1:-1] = 0.0                  # boundary values on the rim, zero inside
    bc = np.ascontiguousarray(bc.reshape(-1))
    S = np.ascontiguousarray(rng.standard_normal((K, (nx - 2) * (ny - 2))))
    tau = np.ascontiguousarray(rng.standard_normal((K, t.size)))
    assert lib.mgrit_hip_level_heat2d(eng, lvl, t.size, _ptr(t), nx, ny, ld, 64.0, 121.0, theta, _ptr(bc), K, _ptr(S), _ptr(tau)) == 0
    return np.arange(nx * ny), ld, bc


def allencahn2d(lib, eng, lvl, t, rng, nx):
    ld = (nx * nx + 15) // 16 * 16
    assert lib.mgrit_hip_level_allencahn2d(eng, lvl, t.size, _ptr(t), nx, ld, float(nx * nx), 25.0, 2) == 0
    return np.arange(nx * nx), ld


def _heat1d_blk(lib, eng, lvl, t, rng):
    # fac large enough that all but a few sine modes decay below 2^-60 over one block: the rule takes the time-parallel form
    n, fac, r = 100, 1.0e4, C.c_int(-1)
    assert lib.mgrit_hip_block_solve_rank(1, n, fac, t.size, _ptr(t), C.byref(r)) == 0     # MGRIT_HIP_STEPPER_HEAT1D
    assert r.value > 0, r.value
    return heat1d(lib, eng, lvl, t, rng, n, fac, 1)


CASES = {
    # name: (level, time grid, describe(lib, eng, lvl, t, rng), scale of the seeded states)
    "heat1d_n100_nt17_K0": (0, t_three_sizes(), lambda *a: heat1d(*a, 100, 10201.0, 0), 1.0),
    "heat1d_n100_nt17_K2": (0, t_three_sizes(), lambda *a: heat1d(*a, 100, 10201.0, 2), 1.0),
    "heat1d_n1030_uniform_K1_lvl1": (1, t_uniform(17), lambda *a: heat1d(*a, 1030, 1062961.0, 1), 1.0),
    "heat1d_n100_nt84_blocks_lvl1": (1, t_nonuniform(84), _heat1d_blk, 1.0),
    "advection1d_n64_nt84_lvl1": (1, t_nonuniform(84), lambda *a: advection1d(*a, 64, 64.0), 1.0),
    "advection1d_n96_nt84_lvl1": (1, t_nonuniform(84), lambda *a: advection1d(*a, 96, 96.0), 1.0),
    "heat1d_2pts_n100_order1": (0, t_pairs(13), lambda *a: heat1d_2pts(*a, 100, 10201.0, 2.0 ** -8, 1, 1), 1.0),
    "heat1d_2pts_n100_order2": (0, t_pairs(13), lambda *a: heat1d_2pts(*a, 100, 10201.0, 2.0 ** -8, 2, 1), 1.0),
    "heat2d_9x12_theta1_lvl1": (1, t_two_sequences(), lambda *a: heat2d(*a, 9, 12, 1.0, 1), 1.0),
    "heat2d_9x12_theta05_lvl1": (1, t_two_sequences(), lambda *a: heat2d(*a, 9, 12, 0.5, 1), 1.0),
    "allencahn2d_nx20_nt9": (0, _grid([1e-3 * (1 + (i % 2)) for i in range(8)]), lambda *a: allencahn2d(*a, 20), 0.5),
    "heat1d_wide_n16390_nt5": (0, t_nonuniform(5), lambda *a: heat1d(*a, 16390, 268599321.0, 1), 1.0),
}


def run_case(lib, name):
    """-> {"residual_after_f": sha256, "u_relaxed": sha256, "residual": sha256[, "u_chain": sha256]} of the case"""
    lvl, t, describe, scale = CASES[name]
    nt = t.size
    rng = np.random.default_rng(int(hashlib.sha256(name.encode()).hexdigest()[:8], 16))
    eng = C.c_void_p()
    assert lib.mgrit_hip_create(C.byref(eng), lvl + 1, C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    try:
        live, ld, *rest = describe(lib, eng, lvl, t, rng)
        host = []
        for _ in range(3):     # u, v, g: seeded at the live positions, padding zero
            a = np.zeros((nt, ld))
            a[:, live] = scale * rng.standard_normal((nt, live.size))
            host.append(a)
        if rest:               # Heat2D: every state carries the boundary values on its rim (what any Phi leaves there), g none
            rim = rest[0] != 0.0
            for a, val in zip(host, (rest[0][rim], rest[0][rim], 0.0)):
                a[:, np.flatnonzero(rim)] = val
        u, v, g = (torch.from_numpy(a).cuda() for a in host)
        assert lib.mgrit_hip_level_bind(eng, lvl, _dev(u), _dev(v), _dev(g)) == 0
        if name.startswith("heat1d_n1030"):     # the overlapped chain keeps its running state in a buffer of the caller
            slen = C.c_int(0)
            assert lib.mgrit_hip_chain_state_len(eng, lvl, C.byref(slen)) == 0 and slen.value == ld + 64
            state = torch.zeros(slen.value, dtype=torch.float64, device="cuda")
            assert lib.mgrit_hip_chain_bind(eng, lvl, _dev(state)) == 0

        def runs(start, length):
            start, length, rid = np.asarray(start, dtype=np.int32), np.asarray(length, dtype=np.int32), C.c_int(-1)
            assert lib.mgrit_hip_runs_create(eng, lvl, start.size, _ptr(start), _ptr(length), C.byref(rid)) == 0, lib.mgrit_hip_last_error()
            return rid.value, start.size

        f_start = np.arange(1, nt, M)
        fid, _ = runs(f_start, np.minimum(M - 1, nt - f_start))
        c_start = np.arange(M, nt, M)
        cid, n_c = runs(c_start, np.ones_like(c_start))
        assert lib.mgrit_hip_relax(eng, lvl, fid, RELAX_F, 1.0) == 0, lib.mgrit_hip_last_error()
        sumsq_f, sumsq = (torch.zeros(n_c, dtype=torch.float64, device="cuda") for _ in range(2))
        assert lib.mgrit_hip_residual(eng, lvl, cid, _dev(sumsq_f)) == 0, lib.mgrit_hip_last_error()
        assert lib.mgrit_hip_relax(eng, lvl, cid, RELAX_C, 1.0) == 0, lib.mgrit_hip_last_error()
        assert lib.mgrit_hip_residual(eng, lvl, cid, _dev(sumsq)) == 0, lib.mgrit_hip_last_error()
        assert lib.mgrit_hip_sync(eng) == 0
        assert (sumsq_f.cpu().numpy() > 0.0).all() and np.isfinite(sumsq_f.cpu().numpy()).all()
        if lvl == 0:     # (no g: the C-relaxation has just stored the very value the residual compares with; its hash pins only that)
            assert not sumsq.cpu().numpy().any()
        out = {"residual_after_f": _sha(sumsq_f.cpu().numpy()), "u_relaxed": _sha(u.cpu().numpy()[:, live]),
               "residual": _sha(sumsq.cpu().numpy())}
        if lvl > 0:
            whole, _ = runs([1], [nt - 1])
            assert lib.mgrit_hip_relax(eng, lvl, whole, RELAX_CHAIN, 1.0) == 0, lib.mgrit_hip_last_error()
            assert lib.mgrit_hip_sync(eng) == 0
            r = C.c_int(-1)
            assert lib.mgrit_hip_block_solve_state(eng, lvl, C.byref(r)) == 0
            assert (r.value > 0) == (nt == 84), (name, r.value)     # the time-parallel form exactly where the case is about it
            out["u_chain"] = _sha(u.cpu().numpy()[:, live])
        got = u.cpu().numpy()
        assert np.isfinite(got).all() and np.isfinite(sumsq.cpu().numpy()).all()
        return out
    finally:
        assert lib.mgrit_hip_destroy(eng) == 0


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU visible")
    from pymgrit_amd.core import hip_lib
    return hip_lib.load()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_names_the_cases(golden):
    assert sorted(golden) == sorted(CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_level_tables_reproduce_the_recording(lib, golden, name):
    got = run_case(lib, name)
    print(name, got)
    assert got == golden[name]
