"""The refusals of the level descriptors, of mgrit_hip_block_solve_config and of the three list constructors, pinned call by call:
return code and the full text of mgrit_hip_last_error against tests/golden/abi_errors.json, recorded on an MI355X with the library as
it stood before the descriptors got a shared opening. ctypes only, like test_hip_abi.py.

The table holds at least one call per fail(...) of those functions that arguments alone can reach and, for every two neighbouring
checks of a function, one call that violates both -- the text that comes back says which check runs first. Calls run in table order
on a handful of engines (SETUP); a refused call must leave its level as it was, so later entries also pin that.

Left out, because no argument reaches them: every refusal behind a failed allocation or upload ("no memory for an upload", any
hipMalloc / hipMemcpyAsync / hipFuncSetAttribute error of register_lds_limits, dev_upload, blk_config, scratch_reserve), and
"mgrit_hip_block_solve_config inside a stream capture" (needs a capturing stream, not an argument)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "abi_errors.json")
NULL = C.c_void_p(0)


def _ptr(a):
    return C.c_void_p(a.ctypes.data)


def _i32(*v):
    return np.array(v, dtype=np.int32)


T9 = np.ascontiguousarray(np.linspace(0.0, 1.0, 9))
T84 = np.ascontiguousarray(np.linspace(0.0, 1.0, 84))
# step sizes (1 + i) * 2^-30: the grid points and their differences are exact, so every step has a size of its own
T_DISTINCT = np.ascontiguousarray(np.concatenate(([0.0], np.cumsum((1.0 + np.arange(262145)) * 2.0 ** -30))))
T_DISTINCT_2PTS = np.ascontiguousarray(T_DISTINCT[:4100] * 2.0 ** 20)     # (steps well above dtau)
S100, TAU9, BC = np.ones((1, 100)), np.ones((1, 9)), np.ones(9 * 12)
S2D = np.ones((1, 7 * 10))
LD = 1024          # mgrit_hip_row_stride(100)


def build_table(lib, E):
    """[(name, thunk)]: E maps an engine's name to its handle (None: the null engine)."""
    h1 = lib.mgrit_hip_level_heat1d
    adv = lib.mgrit_hip_level_advection1d
    p2 = lib.mgrit_hip_level_heat1d_2pts
    h2 = lib.mgrit_hip_level_heat2d
    ac = lib.mgrit_hip_level_allencahn2d
    cfg = lib.mgrit_hip_block_solve_config
    rid = C.c_int(-1)
    out = C.byref(rid)
    t9, s, tau, bc, s2 = _ptr(T9), _ptr(S100), _ptr(TAU9), _ptr(BC), _ptr(S2D)
    D, A, B, H = E["D"], E["A"], E["B"], E["H"]
    buf = C.c_void_p(T9.ctypes.data)      # any non-null address: the refusals below come before anything reads it
    runs, pairs, ivals = lib.mgrit_hip_runs_create, lib.mgrit_hip_pairs_create, lib.mgrit_hip_intervals_create
    one, three, four, zero, minus1, minus2, far = (_ptr(ONE_ELEMENT[v]) for v in (1, 3, 4, 0, -1, -2, 99))

    def iv(e, lvl, n, cs, ce, csc, cec, rp, res_len, chunk, o=out):
        return ivals(e, lvl, n, cs, ce, csc, cec, rp, res_len, chunk, NULL, o)

    return [
        # ---- mgrit_hip_level_heat1d: engine, level, n, ld, time grid, forcing, "already described", distinct step sizes
        ("heat1d/null_engine", lambda: h1(None, 0, 9, t9, 100, LD, 1.0, 0, NULL, NULL)),
        ("heat1d/null_engine+level", lambda: h1(None, 7, 9, t9, 100, LD, 1.0, 0, NULL, NULL)),
        ("heat1d/level_high", lambda: h1(D, 8, 9, t9, 100, LD, 1.0, 0, NULL, NULL)),
        ("heat1d/level_negative", lambda: h1(D, -1, 9, t9, 100, LD, 1.0, 0, NULL, NULL)),
        ("heat1d/level+n", lambda: h1(D, 8, 9, t9, 0, LD, 1.0, 0, NULL, NULL)),
        ("heat1d/n_zero", lambda: h1(D, 0, 9, t9, 0, 0, 1.0, 0, NULL, NULL)),
        ("heat1d/n_above_wide", lambda: h1(D, 0, 9, t9, 70000, 70656, 1.0, 0, NULL, NULL)),
        ("heat1d/n+ld", lambda: h1(D, 0, 9, t9, 70000, 5, 1.0, 0, NULL, NULL)),
        ("heat1d/ld", lambda: h1(D, 0, 9, t9, 100, LD + 16, 1.0, 0, NULL, NULL)),
        ("heat1d/ld+time_grid", lambda: h1(D, 0, -1, t9, 100, LD + 16, 1.0, 0, NULL, NULL)),
        ("heat1d/time_grid_negative", lambda: h1(D, 0, -1, t9, 100, LD, 1.0, 0, NULL, NULL)),
        ("heat1d/time_grid_null", lambda: h1(D, 0, 9, NULL, 100, LD, 1.0, 0, NULL, NULL)),
        ("heat1d/time_grid+forcing", lambda: h1(D, 0, 9, NULL, 100, LD, 1.0, 9, NULL, NULL)),
        ("heat1d/forcing_K_high", lambda: h1(D, 0, 9, t9, 100, LD, 1.0, 9, s, tau)),
        ("heat1d/forcing_K_negative", lambda: h1(D, 0, 9, t9, 100, LD, 1.0, -1, s, tau)),
        ("heat1d/forcing_s_null", lambda: h1(D, 0, 9, t9, 100, LD, 1.0, 1, NULL, tau)),
        ("heat1d/forcing_tau_null", lambda: h1(D, 0, 9, t9, 100, LD, 1.0, 1, s, NULL)),
        ("heat1d/ok", lambda: h1(D, 0, 9, t9, 100, LD, 1.0, 1, s, tau)),
        ("heat1d/already", lambda: h1(D, 0, 9, t9, 100, LD, 1.0, 0, NULL, NULL)),
        ("heat1d/forcing+already", lambda: h1(D, 0, 9, t9, 100, LD, 1.0, 9, NULL, NULL)),
        ("heat1d/ld+already", lambda: h1(D, 0, 9, t9, 100, LD + 16, 1.0, 0, NULL, NULL)),
        ("heat1d/already+distinct_steps", lambda: h1(D, 0, T_DISTINCT.size, _ptr(T_DISTINCT), 100, LD, 1.0, 0, NULL, NULL)),
        ("heat1d/distinct_steps", lambda: h1(D, 1, T_DISTINCT.size, _ptr(T_DISTINCT), 100, LD, 1.0, 0, NULL, NULL)),
        ("heat1d/after_distinct_steps_ok", lambda: h1(D, 1, 9, t9, 100, LD, 1.0, 0, NULL, NULL)),
        # ---- mgrit_hip_level_advection1d (no forcing arguments)
        ("advection1d/null_engine", lambda: adv(None, 0, 9, t9, 100, LD, 1.0)),
        ("advection1d/level", lambda: adv(D, 9, 9, t9, 100, LD, 1.0)),
        ("advection1d/level+n", lambda: adv(D, 9, 9, t9, 70000, LD, 1.0)),
        ("advection1d/n", lambda: adv(D, 2, 9, t9, 70000, 70656, 1.0)),
        ("advection1d/n+ld", lambda: adv(D, 2, 9, t9, -3, 77, 1.0)),
        ("advection1d/ld", lambda: adv(D, 2, 9, t9, 100, 2 * LD, 1.0)),
        ("advection1d/ld+time_grid", lambda: adv(D, 2, 9, NULL, 100, 2 * LD, 1.0)),
        ("advection1d/time_grid", lambda: adv(D, 2, 9, NULL, 100, LD, 1.0)),
        ("advection1d/time_grid+already", lambda: adv(D, 0, 9, NULL, 100, LD, 1.0)),
        ("advection1d/already", lambda: adv(D, 0, 9, t9, 100, LD, 1.0)),
        ("advection1d/distinct_steps", lambda: adv(D, 2, T_DISTINCT.size, _ptr(T_DISTINCT), 100, LD, 1.0)),
        ("advection1d/ok", lambda: adv(D, 2, 9, t9, 100, LD, 1.0)),
        # ---- mgrit_hip_level_heat1d_2pts: engine, level, n, ld, order, time grid, forcing, "already described", distinct step sizes
        ("2pts/null_engine", lambda: p2(None, 3, 9, t9, 100, 2 * LD, 1.0, 0.01, 1, 0, NULL, NULL, NULL)),
        ("2pts/level", lambda: p2(D, 64, 9, t9, 100, 2 * LD, 1.0, 0.01, 1, 0, NULL, NULL, NULL)),
        ("2pts/level+n", lambda: p2(D, 64, 9, t9, 0, 2 * LD, 1.0, 0.01, 1, 0, NULL, NULL, NULL)),
        ("2pts/n", lambda: p2(D, 3, 9, t9, 70000, 2 * 70656, 1.0, 0.01, 1, 0, NULL, NULL, NULL)),
        ("2pts/n+ld", lambda: p2(D, 3, 9, t9, 0, 2 * LD, 1.0, 0.01, 1, 0, NULL, NULL, NULL)),
        ("2pts/ld_of_one_half", lambda: p2(D, 3, 9, t9, 100, LD, 1.0, 0.01, 1, 0, NULL, NULL, NULL)),
        ("2pts/ld+order", lambda: p2(D, 3, 9, t9, 100, LD, 1.0, 0.01, 3, 0, NULL, NULL, NULL)),
        ("2pts/order", lambda: p2(D, 3, 9, t9, 100, 2 * LD, 1.0, 0.01, 3, 0, NULL, NULL, NULL)),
        ("2pts/order+time_grid", lambda: p2(D, 3, -2, t9, 100, 2 * LD, 1.0, 0.01, 0, 0, NULL, NULL, NULL)),
        ("2pts/time_grid", lambda: p2(D, 3, 9, NULL, 100, 2 * LD, 1.0, 0.01, 2, 0, NULL, NULL, NULL)),
        ("2pts/time_grid+forcing", lambda: p2(D, 3, 9, NULL, 100, 2 * LD, 1.0, 0.01, 2, 12, NULL, NULL, NULL)),
        ("2pts/forcing_K_high", lambda: p2(D, 3, 9, t9, 100, 2 * LD, 1.0, 0.01, 2, 12, s, tau, tau)),
        ("2pts/forcing_tau2_null", lambda: p2(D, 3, 9, t9, 100, 2 * LD, 1.0, 0.01, 2, 1, s, tau, NULL)),
        ("2pts/forcing_tau_null", lambda: p2(D, 3, 9, t9, 100, 2 * LD, 1.0, 0.01, 2, 1, s, NULL, tau)),
        ("2pts/forcing_s_null", lambda: p2(D, 3, 9, t9, 100, 2 * LD, 1.0, 0.01, 2, 1, NULL, tau, tau)),
        ("2pts/forcing+already", lambda: p2(D, 0, 9, t9, 100, 2 * LD, 1.0, 0.01, 2, 1, NULL, tau, tau)),
        ("2pts/already", lambda: p2(D, 0, 9, t9, 100, 2 * LD, 1.0, 0.01, 2, 0, NULL, NULL, NULL)),
        ("2pts/already+distinct_steps", lambda: p2(D, 0, T_DISTINCT_2PTS.size, _ptr(T_DISTINCT_2PTS), 100, 2 * LD, 1.0, 2.0 ** -12, 1, 0, NULL, NULL, NULL)),
        ("2pts/distinct_steps", lambda: p2(D, 3, T_DISTINCT_2PTS.size, _ptr(T_DISTINCT_2PTS), 100, 2 * LD, 1.0, 2.0 ** -12, 1, 0, NULL, NULL, NULL)),
        ("2pts/distinct_steps_order2", lambda: p2(D, 4, T_DISTINCT_2PTS.size, _ptr(T_DISTINCT_2PTS), 100, 2 * LD, 1.0, 2.0 ** -12, 2, 0, NULL, NULL, NULL)),
        ("2pts/ok", lambda: p2(D, 5, 9, t9, 100, 2 * LD, 1.0, 0.01, 2, 1, s, tau, tau)),
        # ---- mgrit_hip_level_heat2d: engine, level, grid, ld, theta, arguments, forcing, "already described"
        ("heat2d/null_engine", lambda: h2(None, 6, 9, t9, 9, 12, 112, 64.0, 64.0, 1.0, bc, 0, NULL, NULL)),
        ("heat2d/level", lambda: h2(D, 70, 9, t9, 9, 12, 112, 64.0, 64.0, 1.0, bc, 0, NULL, NULL)),
        ("heat2d/level+grid", lambda: h2(D, 70, 9, t9, 2, 12, 112, 64.0, 64.0, 1.0, bc, 0, NULL, NULL)),
        ("heat2d/grid_small", lambda: h2(D, 6, 9, t9, 2, 12, 112, 64.0, 64.0, 1.0, bc, 0, NULL, NULL)),
        ("heat2d/grid_large", lambda: h2(D, 6, 9, t9, 9, 2051, 112, 64.0, 64.0, 1.0, bc, 0, NULL, NULL)),
        ("heat2d/grid+ld", lambda: h2(D, 6, 9, t9, 2, 12, 8, 64.0, 64.0, 1.0, bc, 0, NULL, NULL)),
        ("heat2d/ld_short", lambda: h2(D, 6, 9, t9, 9, 12, 96, 64.0, 64.0, 1.0, bc, 0, NULL, NULL)),
        ("heat2d/ld_not_16", lambda: h2(D, 6, 9, t9, 9, 12, 110, 64.0, 64.0, 1.0, bc, 0, NULL, NULL)),
        ("heat2d/ld+theta", lambda: h2(D, 6, 9, t9, 9, 12, 110, 64.0, 64.0, 0.25, bc, 0, NULL, NULL)),
        ("heat2d/theta", lambda: h2(D, 6, 9, t9, 9, 12, 112, 64.0, 64.0, 0.25, bc, 0, NULL, NULL)),
        ("heat2d/theta+arguments", lambda: h2(D, 6, 9, t9, 9, 12, 112, 64.0, 64.0, float("nan"), NULL, 0, NULL, NULL)),
        ("heat2d/bc_null", lambda: h2(D, 6, 9, t9, 9, 12, 112, 64.0, 64.0, 1.0, NULL, 0, NULL, NULL)),
        ("heat2d/time_grid_null", lambda: h2(D, 6, 9, NULL, 9, 12, 112, 64.0, 64.0, 1.0, bc, 0, NULL, NULL)),
        ("heat2d/time_grid_negative", lambda: h2(D, 6, -1, t9, 9, 12, 112, 64.0, 64.0, 1.0, bc, 0, NULL, NULL)),
        ("heat2d/arguments+forcing", lambda: h2(D, 6, 9, t9, 9, 12, 112, 64.0, 64.0, 1.0, NULL, 9, NULL, NULL)),
        ("heat2d/forcing_K_high", lambda: h2(D, 6, 9, t9, 9, 12, 112, 64.0, 64.0, 1.0, bc, 9, s2, tau)),
        ("heat2d/forcing_S_null", lambda: h2(D, 6, 9, t9, 9, 12, 112, 64.0, 64.0, 1.0, bc, 1, NULL, tau)),
        ("heat2d/forcing_tau_null", lambda: h2(D, 6, 9, t9, 9, 12, 112, 64.0, 64.0, 1.0, bc, 1, s2, NULL)),
        ("heat2d/forcing+already", lambda: h2(D, 0, 9, t9, 9, 12, 112, 64.0, 64.0, 1.0, bc, 1, s2, NULL)),
        ("heat2d/already", lambda: h2(D, 0, 9, t9, 9, 12, 112, 64.0, 64.0, 1.0, bc, 0, NULL, NULL)),
        ("heat2d/ok", lambda: h2(D, 6, 9, t9, 9, 12, 112, 64.0, 64.0, 0.5, bc, 1, s2, tau)),
        ("heat2d/already_heat2d", lambda: h2(D, 6, 9, t9, 9, 12, 112, 64.0, 64.0, 0.5, bc, 1, s2, tau)),
        # ---- mgrit_hip_level_allencahn2d: engine, level, grid, ld, parameters, arguments, "already described"
        ("allencahn/null_engine", lambda: ac(None, 7, 9, t9, 20, 400, 400.0, 25.0, 2)),
        ("allencahn/level", lambda: ac(D, -5, 9, t9, 20, 400, 400.0, 25.0, 2)),
        ("allencahn/level+grid", lambda: ac(D, -5, 9, t9, 3, 400, 400.0, 25.0, 2)),
        ("allencahn/grid_small", lambda: ac(D, 7, 9, t9, 3, 400, 400.0, 25.0, 2)),
        ("allencahn/grid_large", lambda: ac(D, 7, 9, t9, 2049, 2049 * 2049 + 15, 400.0, 25.0, 2)),
        ("allencahn/grid+ld", lambda: ac(D, 7, 9, t9, 3, 7, 400.0, 25.0, 2)),
        ("allencahn/ld_short", lambda: ac(D, 7, 9, t9, 20, 384, 400.0, 25.0, 2)),
        ("allencahn/ld_not_16", lambda: ac(D, 7, 9, t9, 20, 404, 400.0, 25.0, 2)),
        ("allencahn/ld+parameters", lambda: ac(D, 7, 9, t9, 20, 404, 400.0, 25.0, 0)),
        ("allencahn/nu_low", lambda: ac(D, 7, 9, t9, 20, 400, 400.0, 25.0, 0)),
        ("allencahn/nu_high", lambda: ac(D, 7, 9, t9, 20, 400, 400.0, 25.0, 65)),
        ("allencahn/inv_dx2", lambda: ac(D, 7, 9, t9, 20, 400, 0.0, 25.0, 2)),
        ("allencahn/inv_eps2_nan", lambda: ac(D, 7, 9, t9, 20, 400, 400.0, float("nan"), 2)),
        ("allencahn/parameters+arguments", lambda: ac(D, 7, 9, NULL, 20, 400, 400.0, -1.0, 2)),
        ("allencahn/time_grid_null", lambda: ac(D, 7, 9, NULL, 20, 400, 400.0, 25.0, 2)),
        ("allencahn/time_grid_negative", lambda: ac(D, 7, -1, t9, 20, 400, 400.0, 25.0, 2)),
        ("allencahn/arguments+already", lambda: ac(D, 0, 9, NULL, 20, 400, 400.0, 25.0, 2)),
        ("allencahn/already", lambda: ac(D, 6, 9, t9, 20, 400, 400.0, 25.0, 2)),
        ("allencahn/ok", lambda: ac(D, 7, 9, t9, 20, 400, 400.0, 25.0, 2)),
        # ---- mgrit_hip_block_solve_config. Engine A: Heat1D n = 100, levels 0 (9 points), 1 (84), 2 (9), 3 not described;
        # engine B: Advection1D, levels 0 and 1 n = 64 with 84 points, level 2 n = 32; engine H: Heat2D 9x12 levels 0 (84 points), 1 (84,
        # theta = 0), 2 (9 points), Allen-Cahn level 3
        ("blk/null_engine", lambda: cfg(None, 1, 4, 1, 0, NULL, NULL)),
        ("blk/level", lambda: cfg(A, 4, 4, 1, 0, NULL, NULL)),
        ("blk/no_stepper", lambda: cfg(A, 3, 4, 1, 0, NULL, NULL)),
        ("blk/r_zero_ok", lambda: cfg(A, 0, 0, 0, 1, NULL, NULL)),
        ("blk/level0", lambda: cfg(A, 0, 4, 1, 0, NULL, NULL)),
        ("blk/level0_by_rule_ok", lambda: cfg(A, 0, -1, 1, 0, NULL, NULL)),
        ("blk/level0+steps", lambda: cfg(A, 0, 4, 0, 1, NULL, NULL)),
        ("blk/two_point_level", lambda: cfg(D, 5, 4, 1, 0, NULL, NULL)),
        ("blk/steps", lambda: cfg(A, 2, 4, 1, 0, NULL, NULL)),
        ("blk/steps+uh_in", lambda: cfg(A, 2, 4, 0, 0, NULL, NULL)),
        ("blk/uh_in", lambda: cfg(A, 1, 4, 0, 0, NULL, NULL)),
        ("blk/uh_in+uh_out", lambda: cfg(A, 1, 4, 0, 1, NULL, NULL)),
        ("blk/uh_out", lambda: cfg(A, 1, 4, 1, 1, NULL, NULL)),
        ("blk/uh_out+r", lambda: cfg(A, 1, 300, 1, 1, buf, NULL)),
        ("blk/r_above_rmax", lambda: cfg(A, 1, 257, 1, 0, NULL, NULL)),
        ("blk/r_above_n", lambda: cfg(A, 1, 101, 1, 0, NULL, NULL)),
        ("blk/advection_uh_out+r", lambda: cfg(B, 1, 32, 1, 1, NULL, NULL)),
        ("blk/advection_r_not_n", lambda: cfg(B, 1, 32, 1, 0, NULL, NULL)),
        ("blk/advection_n_small", lambda: cfg(B, 2, 32, 1, 0, NULL, NULL)),
        ("blk/advection_n_small_by_rule_ok", lambda: cfg(B, 2, -1, 1, 0, NULL, NULL)),
        ("blk/heat2d_first_real", lambda: cfg(H, 0, 4, 0, 0, NULL, NULL)),
        ("blk/heat2d_successor", lambda: cfg(H, 0, -1, 1, 1, NULL, NULL)),
        ("blk/heat2d_ranks+level0", lambda: cfg(H, 0, 4, 0, 1, NULL, NULL)),
        ("blk/heat2d_level0", lambda: cfg(H, 0, 4, 1, 0, NULL, NULL)),
        ("blk/heat2d_level0_by_rule_ok", lambda: cfg(H, 0, -1, 1, 0, NULL, NULL)),
        ("blk/heat2d_explicit", lambda: cfg(H, 1, 4, 1, 0, NULL, NULL)),
        ("blk/heat2d_steps", lambda: cfg(H, 2, 4, 1, 0, NULL, NULL)),
        ("blk/allencahn", lambda: cfg(H, 3, 4, 1, 0, NULL, NULL)),
        ("blk/allencahn_by_rule_ok", lambda: cfg(H, 3, -1, 1, 0, NULL, NULL)),
        # ---- mgrit_hip_runs_create (engine A)
        ("runs/null_engine", lambda: runs(None, 0, 1, one, one, out)),
        ("runs/level", lambda: runs(A, 9, 1, one, one, out)),
        ("runs/no_stepper", lambda: runs(A, 3, 1, one, one, out)),
        ("runs/no_stepper+list", lambda: runs(A, 3, -1, one, one, out)),
        ("runs/n_negative", lambda: runs(A, 0, -1, one, one, out)),
        ("runs/id_out_null", lambda: runs(A, 0, 1, one, one, None)),
        ("runs/start_null", lambda: runs(A, 0, 1, NULL, one, out)),
        ("runs/len_null", lambda: runs(A, 0, 1, one, NULL, out)),
        ("runs/list+run", lambda: runs(A, 0, 1, zero, NULL, out)),
        ("runs/start_zero", lambda: runs(A, 0, 1, zero, one, out)),
        ("runs/len_zero", lambda: runs(A, 0, 1, one, zero, out)),
        ("runs/leaves_grid", lambda: runs(A, 0, 1, one, far, out)),
        ("runs/second_run_bad", lambda: runs(A, 0, 2, _ptr(RUN2_START), _ptr(RUN2_LEN), out)),
        ("runs/empty_ok", lambda: runs(A, 0, 0, NULL, NULL, out)),
        ("runs/ok", lambda: runs(A, 0, 1, one, three, out)),
        # ---- mgrit_hip_pairs_create (engine A: levels 0-2 described, level 3 not)
        ("pairs/null_engine", lambda: pairs(None, 0, 1, one, one, out)),
        ("pairs/level", lambda: pairs(A, -1, 1, one, one, out)),
        ("pairs/no_stepper", lambda: pairs(A, 3, 1, one, one, out)),
        ("pairs/last_level", lambda: pairs(E["L"], 0, 1, one, one, out)),
        ("pairs/coarser_not_described", lambda: pairs(A, 2, 1, one, one, out)),
        ("pairs/coarser+list", lambda: pairs(A, 2, -1, one, one, out)),
        ("pairs/n_negative", lambda: pairs(A, 0, -1, one, one, out)),
        ("pairs/id_out_null", lambda: pairs(A, 0, 1, one, one, None)),
        ("pairs/fine_null", lambda: pairs(A, 0, 1, NULL, one, out)),
        ("pairs/coarse_null", lambda: pairs(A, 0, 1, one, NULL, out)),
        ("pairs/list+pair", lambda: pairs(A, 0, 1, far, NULL, out)),
        ("pairs/fine_negative", lambda: pairs(A, 0, 1, minus1, one, out)),
        ("pairs/fine_high", lambda: pairs(A, 0, 1, far, one, out)),
        ("pairs/coarse_negative", lambda: pairs(A, 0, 1, one, minus1, out)),
        ("pairs/coarse_high", lambda: pairs(A, 0, 1, one, far, out)),
        ("pairs/empty_ok", lambda: pairs(A, 0, 0, NULL, NULL, out)),
        ("pairs/ok", lambda: pairs(A, 0, 1, four, one, out)),
        # ---- mgrit_hip_intervals_create (engine A; arguments: cstart, cend, cstart_coarse, cend_coarse, res_pos, res_len, chunk)
        ("intervals/null_engine", lambda: iv(None, 0, 1, zero, four, zero, one, zero, 1, 0)),
        ("intervals/level", lambda: iv(A, 4, 1, zero, four, zero, one, zero, 1, 0)),
        ("intervals/no_stepper", lambda: iv(A, 3, 1, zero, four, zero, one, zero, 1, 0)),
        ("intervals/coarser_not_described", lambda: iv(A, 2, 1, zero, four, zero, one, zero, 1, 0)),
        ("intervals/coarser+list", lambda: iv(A, 2, -1, zero, four, zero, one, zero, 1, 0)),
        ("intervals/n_negative", lambda: iv(A, 0, -1, zero, four, zero, one, zero, 1, 0)),
        ("intervals/chunk_below_long", lambda: iv(A, 0, 1, zero, four, zero, one, zero, 1, -2)),
        ("intervals/res_len_short", lambda: iv(A, 0, 1, zero, four, zero, one, zero, 0, 0)),
        ("intervals/id_out_null", lambda: iv(A, 0, 1, zero, four, zero, one, zero, 1, 0, None)),
        ("intervals/cstart_null", lambda: iv(A, 0, 1, NULL, four, zero, one, zero, 1, 0)),
        ("intervals/cend_null", lambda: iv(A, 0, 1, zero, NULL, zero, one, zero, 1, 0)),
        ("intervals/cstart_coarse_null", lambda: iv(A, 0, 1, zero, four, NULL, one, zero, 1, 0)),
        ("intervals/cend_coarse_null", lambda: iv(A, 0, 1, zero, four, zero, NULL, zero, 1, 0)),
        ("intervals/res_pos_null", lambda: iv(A, 0, 1, zero, four, zero, one, NULL, 1, 0)),
        ("intervals/list+interval", lambda: iv(A, 0, 1, minus1, four, zero, one, NULL, 1, 0)),
        ("intervals/cstart_negative", lambda: iv(A, 0, 1, minus1, four, zero, one, zero, 1, 0)),
        ("intervals/cend_high", lambda: iv(A, 0, 1, zero, far, zero, one, zero, 1, 0)),
        ("intervals/no_f_point", lambda: iv(A, 0, 1, three, four, zero, one, zero, 1, 0)),
        ("intervals/interval+coarse", lambda: iv(A, 0, 1, three, four, minus2, one, zero, 1, 0)),
        ("intervals/cstart_coarse_low", lambda: iv(A, 0, 1, zero, four, minus2, one, zero, 1, 0)),
        ("intervals/cstart_coarse_high", lambda: iv(A, 0, 1, one, four, far, one, zero, 1, 0)),
        ("intervals/cend_coarse_negative", lambda: iv(A, 0, 1, zero, four, minus1, minus1, zero, 1, 0)),
        ("intervals/cend_coarse_high", lambda: iv(A, 0, 1, zero, four, minus1, far, zero, 1, 0)),
        ("intervals/start_takes_part_at_slot_0", lambda: iv(A, 0, 1, zero, four, zero, one, zero, 1, 0)),
        ("intervals/res_pos_negative", lambda: iv(A, 0, 1, zero, four, minus1, one, minus1, 1, 0)),
        ("intervals/res_pos_high", lambda: iv(A, 0, 1, zero, four, minus1, one, one, 1, 0)),
        ("intervals/empty_ok", lambda: iv(A, 0, 0, NULL, NULL, NULL, NULL, NULL, 0, 0)),
        ("intervals/ok", lambda: iv(A, 0, 1, zero, four, minus1, one, zero, 1, -1)),
    ]


RUN2_START, RUN2_LEN = _i32(1, 5), _i32(3, 9)
ONE_ELEMENT = {v: _i32(v) for v in (1, 3, 4, 0, -1, -2, 99)}     # the index lists of one entry that the table's pointers name


def setup(lib):
    """The engines the table runs on: D for the descriptors (8 levels, none described), A / B / H with described levels for
    mgrit_hip_block_solve_config and the list constructors, L with one level."""
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    E = {}
    for name, n_levels in (("D", 8), ("A", 4), ("B", 3), ("H", 4), ("L", 1)):
        eng = C.c_void_p()
        assert lib.mgrit_hip_create(C.byref(eng), n_levels, stream) == 0
        E[name] = eng
    t9, t84, bc = _ptr(T9), _ptr(T84), _ptr(BC)
    for lvl, t in ((0, T9), (1, T84), (2, T9)):
        assert lib.mgrit_hip_level_heat1d(E["A"], lvl, t.size, _ptr(t), 100, LD, 1.0e4, 0, NULL, NULL) == 0
    for lvl, n in ((0, 64), (1, 64), (2, 32)):
        assert lib.mgrit_hip_level_advection1d(E["B"], lvl, 84, t84, n, LD, 64.0) == 0
    for lvl, t, theta in ((0, T84, 1.0), (1, T84, 0.0), (2, T9, 1.0)):
        assert lib.mgrit_hip_level_heat2d(E["H"], lvl, t.size, _ptr(t), 9, 12, 112, 64.0, 64.0, theta, bc, 0, NULL, NULL) == 0
    assert lib.mgrit_hip_level_allencahn2d(E["H"], 3, 9, t9, 20, 400, 400.0, 25.0, 2) == 0
    assert lib.mgrit_hip_level_heat1d(E["L"], 0, 9, t9, 100, LD, 1.0, 0, NULL, NULL) == 0
    return E


def run_table(lib):
    """-> {name: [return code, text of mgrit_hip_last_error after a refusal, "" after a success]}"""
    E = setup(lib)
    try:
        got, table = {}, build_table(lib, E)
        for name, call in table:
            rc = call()
            got[name] = [rc, lib.mgrit_hip_last_error().decode() if rc != 0 else ""]
        assert len(got) == len(table), "two entries of the table share a name"
        return got
    finally:
        for eng in E.values():
            assert lib.mgrit_hip_destroy(eng) == 0


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU visible")
    from pymgrit_amd.core import hip_lib
    return hip_lib.load()


def test_refusals_match_the_recording(lib):
    with open(GOLDEN) as f:
        golden = json.load(f)
    got = run_table(lib)
    assert list(got) == list(golden)
    for name in got:
        if got[name] != golden[name]:
            print(name, got[name], "recorded:", golden[name])
    assert got == golden
    # the table is about refusals: all but the entries marked ok are one, and each comes with a text
    for name, (rc, text) in got.items():
        assert (rc == 0) == name.endswith("ok"), (name, rc, text)
        assert rc == 0 or text
