"""ctypes binding of libmgrit_hip.so (C ABI: include/mgrit_hip.h). The library is mandatory for device
applications: there is no CPU fallback -- a missing library or a missing GPU raises."""
import ctypes as C
import os

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("PYMGRIT_AMD_LIB") or os.path.join(_PKG, "lib", "libmgrit_hip.so")   # (override: experiment builds)

RELAX_F, RELAX_C, RELAX_CHAIN, RELAX_FC = 0, 1, 2, 3
FAS_WITH_F_RELAX, FAS_SKIP_COARSE_U = 1, 2
# MGRIT_HIP_T_*: kinds of timed entry-point calls (mgrit_hip_timing_drain)
TIMED_KINDS = ("relax_f", "relax_c", "chain", "residual", "jump", "restrict", "copy", "fas_rhs", "fas_fused",
               "error_correction", "interpolate", "ec_relax", "at_solve", "cf_fas", "ec_relax_res", "relax_fc", "f_fas", "exchange",
               "gen_down", "gen_up")
STEPPER_HEAT1D, STEPPER_ADVECTION1D = 1, 2
STEPPER_ALLENCAHN2D = 5
STEPPER_GRAYSCOTT2D = 6
STEPPER_CAHNHILLIARD2D = 7
STEPPER_BURGERS2D = 8
STEPPER_NAVIERSTOKES2D = 9
STEPPER_GINZBURGLANDAU2D = 10
TRANSFER_COPY, TRANSFER_HEAT1D, TRANSFER_CALLER = 0, 1, 3
TRANSFER_HEAT2D, TRANSFER_PERIODIC2D = 4, 5
MAX_N = 16384
MAX_LINKS = 16
BLOCK_K, BLOCK_RMAX = 16, 256     # time-parallel forward solve
CHUNK_LONG = -1                   # mgrit_hip_intervals_create: the library's rule for the Heat1D whole-level passes (up to 16)

EXPORTS = {
    # name: (restype, argtypes)
    "mgrit_hip_abi_version": (C.c_int, []),
    "mgrit_hip_last_error": (C.c_char_p, []),
    "mgrit_hip_device_count": (C.c_int, []),
    "mgrit_hip_row_stride": (C.c_int, [C.c_int]),
    "mgrit_hip_row_position": (C.c_int, [C.c_int, C.c_int]),
    "mgrit_hip_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_void_p]),
    "mgrit_hip_destroy": (C.c_int, [C.c_void_p]),
    "mgrit_hip_sync": (C.c_int, [C.c_void_p]),
    "mgrit_hip_level_heat1d": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_double,
                                         C.c_int, C.c_void_p, C.c_void_p]),
    "mgrit_hip_level_heat1d_2pts": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_double,
                                              C.c_double, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mgrit_hip_level_forcing_rows": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "mgrit_hip_ec_runs_create": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]),
    "mgrit_hip_ec_relax": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "mgrit_hip_at_solve": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "mgrit_hip_level_advection1d": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_double]),
    "mgrit_hip_level_heat2d": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double,
                                         C.c_double, C.c_double, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "mgrit_hip_heat2d_padded": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "mgrit_hip_level_heat2d_forcing_rows": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "mgrit_hip_level_allencahn2d": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double,
                                              C.c_int]),
    "mgrit_hip_level_allencahn2d_newton": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_double,
                                                     C.c_double, C.c_int, C.c_double, C.c_double, C.c_int, C.c_double, C.c_int]),
    "mgrit_hip_level_grayscott2d": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double,
                                              C.c_double, C.c_double, C.c_double]),
    "mgrit_hip_level_grayscott2d_newton": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double,
                                                     C.c_double, C.c_double, C.c_double, C.c_double, C.c_int, C.c_double, C.c_int]),
    "mgrit_hip_level_cahnhilliard2d": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double,
                                                 C.c_double]),
    "mgrit_hip_level_burgers2d": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double,
                                            C.c_double]),
    "mgrit_hip_level_navierstokes2d": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double,
                                                 C.c_double, C.c_void_p]),
    "mgrit_hip_level_ginzburglandau2d": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double,
                                                   C.c_double]),
    "mgrit_hip_newton_stats": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "mgrit_hip_level_bind": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mgrit_hip_chain_enable": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "mgrit_hip_chain_state_len": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "mgrit_hip_chain_bind": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "mgrit_hip_chain_resume": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "mgrit_hip_block_solve_rank": (C.c_int, [C.c_int, C.c_int, C.c_double, C.c_int, C.c_void_p, C.POINTER(C.c_int)]),
    "mgrit_hip_block_solve_config": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "mgrit_hip_block_solve": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "mgrit_hip_block_solve_state": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "mgrit_hip_block_solve_form": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "mgrit_hip_level_transfer": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "mgrit_hip_runs_create": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]),
    "mgrit_hip_pairs_create": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]),
    "mgrit_hip_relax": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double]),
    "mgrit_hip_residual": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "mgrit_hip_jump": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "mgrit_hip_restrict_u": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "mgrit_hip_copy_u_to_v": (C.c_int, [C.c_void_p, C.c_int]),
    "mgrit_hip_fas_rhs": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "mgrit_hip_triples_create": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.POINTER(C.c_int)]),
    "mgrit_hip_fas_fused": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "mgrit_hip_fas_fused_opts": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "mgrit_hip_set_fas_chunk": (C.c_int, [C.c_void_p, C.c_int]),
    "mgrit_hip_fas_chunks": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "mgrit_hip_copy_pairs_u_to_v": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "mgrit_hip_error_correction": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "mgrit_hip_interpolate": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "mgrit_hip_residual_host": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "mgrit_hip_jump_host": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "mgrit_hip_set_timing": (C.c_int, [C.c_void_p, C.c_int]),
    "mgrit_hip_last_kernel_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "mgrit_hip_timing_drain": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]),
    "mgrit_hip_set_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mgrit_hip_set_reserve": (C.c_int, [C.c_void_p, C.c_int]),
    "mgrit_hip_chain_clock": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "mgrit_hip_intervals_create": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int)]),
    "mgrit_hip_fas_fine_rows": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]),
    "mgrit_hip_fas_coarse": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "mgrit_hip_cf_fas": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "mgrit_hip_ec_relax_res": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "mgrit_hip_deferred": (C.c_int, [C.c_void_p, C.c_int]),
    "mgrit_hip_set_defer": (C.c_int, [C.c_void_p, C.c_int]),
    "mgrit_hip_set_twin": (C.c_int, [C.c_void_p, C.c_int]),
    "mgrit_hip_twin": (C.c_int, [C.c_void_p, C.c_int]),
    "mgrit_hip_settle": (C.c_int, [C.c_void_p, C.c_int]),
    "mgrit_hip_set_lag": (C.c_int, [C.c_void_p, C.c_int]),
    "mgrit_hip_lagged": (C.c_int, [C.c_void_p, C.c_int]),
    "mgrit_hip_lag_settle": (C.c_int, [C.c_void_p, C.c_int]),
    "mgrit_hip_set_up2": (C.c_int, [C.c_void_p, C.c_int]),
    "mgrit_hip_up2_pending": (C.c_int, [C.c_void_p]),
    "mgrit_hip_up2_settle": (C.c_int, [C.c_void_p]),
    "mgrit_hip_set_cfas_form": (C.c_int, [C.c_void_p, C.c_int]),
    "mgrit_hip_cfas_form": (C.c_int, [C.c_void_p, C.c_int]),
    "mgrit_hip_ec_relax_res_to": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "mgrit_hip_gen_down": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "mgrit_hip_gen_down_part": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "mgrit_hip_gen_up": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "mgrit_hip_residual_fetch": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    # ghost exchange under the ABI (links: RCCL two-rank communicators / mailboxes)
    "mgrit_hip_comm_unique_id": (C.c_int, [C.c_void_p]),
    "mgrit_hip_comm_init_rank": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p, C.c_int, C.c_int]),
    "mgrit_hip_comm_destroy": (C.c_int, [C.c_void_p, C.c_int]),
    "mgrit_hip_link_attach": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
    "mgrit_hip_mailbox_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int]),
    "mgrit_hip_mailbox_destroy": (C.c_int, [C.c_void_p]),
    "mgrit_hip_link_mailbox": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "mgrit_hip_link_stats": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "mgrit_hip_links_close": (C.c_int, [C.c_void_p, C.c_int]),
    "mgrit_hip_exchange": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "mgrit_hip_send": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]),
    "mgrit_hip_recv": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]),
    "mgrit_hip_sync_bounded": (C.c_int, [C.c_void_p, C.c_double]),
    "mgrit_hip_error_correction_to": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]),
    "mgrit_hip_residual_stash": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "mgrit_hip_cpoint_mirror": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "mgrit_hip_stream_create_masked": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int]),
    "mgrit_hip_stream_destroy": (C.c_int, [C.c_void_p]),
}

_lib = None


class MgritHipError(RuntimeError):
    pass


def load():
    """dlopen libmgrit_hip.so and type every export; raises MgritHipError when the library is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise MgritHipError(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; "
                                f"g.build()'` (hipcc --offload-arch=gfx950). There is no CPU fallback.")
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in EXPORTS.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        if lib.mgrit_hip_abi_version() != 3:
            raise MgritHipError("libmgrit_hip.so ABI version mismatch")
        _lib = lib
    return _lib


def check(rc):
    if rc != 0:
        raise MgritHipError(f"libmgrit_hip error {rc}: {load().mgrit_hip_last_error().decode()}")


def row_stride(n):
    """slab row stride (doubles) for n DOFs per time point: 1024*ceil(n/1024)"""
    return load().mgrit_hip_row_stride(int(n))


def row_permutation(n):
    """perm[j] = row position of natural spatial index j (the engine's lane-blocked storage order)"""
    import numpy as np
    j = np.arange(int(n), dtype=np.int64)
    perm = ((((j >> 10) * 8 + ((j & 15) >> 1)) * 64 + ((j >> 4) & 63)) << 1) + (j & 1)
    lib = load()
    for probe in (0, n // 2, n - 1):  # the formula must agree with the library
        assert perm[probe] == lib.mgrit_hip_row_position(int(n), int(probe))
    return perm


# The level descriptions of the periodic 2-D kinds, kind -> (the IMEX export, the Newton export or None,
# the keys of the application's description that follow (h, level, n_pts, t, nx, ld) in the export's argument order, the keys the
# Newton export takes after those). A description that carries theta is a Newton level's. The C type of a key is its argument's in EXPORTS.
_NEWTON = ("newton_tol", "newton_maxiter", "lin_tol", "lin_maxiter")
LEVEL_2D = {
    "allencahn2d": ("mgrit_hip_level_allencahn2d", "mgrit_hip_level_allencahn2d_newton", ("inv_dx2", "inv_eps2", "nu"), ("theta",) + _NEWTON),
    "grayscott2d": ("mgrit_hip_level_grayscott2d", "mgrit_hip_level_grayscott2d_newton", ("inv_dx2", "du", "dv", "a", "b"), _NEWTON),
    "cahnhilliard2d": ("mgrit_hip_level_cahnhilliard2d", None, ("inv_dx2", "eps2", "stab"), ()),
    "burgers2d": ("mgrit_hip_level_burgers2d", None, ("inv_dx2", "inv_2dx", "nu"), ()),
    "navierstokes2d": ("mgrit_hip_level_navierstokes2d", None, ("inv_dx2", "inv_2dx", "nu"), ()),      # (+ the forcing plane or NULL)
    "ginzburglandau2d": ("mgrit_hip_level_ginzburglandau2d", None, ("inv_dx2", "b", "c"), ()),
}


def level_2d_call(h, engine_lvl, n_pts, t_ptr, ld, d, *tail):
    """(export name, argument tuple) that describes a periodic 2-D level; d: the application's description, tail: what the export takes
    behind the description's values (Navier-Stokes: the forcing, nx * nx doubles in natural order, which the library copies, or NULL)"""
    imex, newton, keys, newton_keys = LEVEL_2D[d["kind"]]
    name, keys = (newton, keys + newton_keys) if "theta" in d else (imex, keys)
    types = EXPORTS[name][1][6:]
    values = tuple((float if t is C.c_double else int)(d[k]) for k, t in zip(keys, types))
    return name, (h, engine_lvl, n_pts, t_ptr, int(d["nx"]), ld) + values + tail


def level_2d(h, engine_lvl, n_pts, t_ptr, ld, d, *tail):
    """describe a periodic 2-D level (level_2d_call) and raise on refusal"""
    name, args = level_2d_call(h, engine_lvl, n_pts, t_ptr, ld, d, *tail)
    check(getattr(load(), name)(*args))


def settle(h, lvl):
    """rows of u the engine has left unstored on the level or the next coarser one (include/mgrit_hip.h, mgrit_hip_twin) are put
    in place: for a reader or writer of a coarse slab that goes past the engine"""
    check(load().mgrit_hip_settle(h, int(lvl)))


def lag_settle(h, lvl):
    """corrected C-points the level's way up has left unstored (include/mgrit_hip.h, mgrit_hip_lagged) are put in place, and
    nothing else: for a reader of the level-0 slab, or a writer of u of level 1, that goes past the engine"""
    check(load().mgrit_hip_lag_settle(h, int(lvl)))


def set_up2(h, mode):
    """0: the ways up of levels 1 and 0 as two passes; 1: as one pass whenever the level-0 way up lags (include/mgrit_hip.h,
    mgrit_hip_set_up2)"""
    check(load().mgrit_hip_set_up2(h, int(mode)))


def up2_settle(h):
    """u of level 1 is brought up where the ways up of levels 1 and 0 ran as one pass, and nothing else: for a reader of u or g of
    level 1 or of u of level 2, or a writer of g of level 1 or u of level 2, that goes past the engine"""
    check(load().mgrit_hip_up2_settle(h))


def up2_pending(h):
    """0: nothing pending; 1: the level-1 way up is noted and nothing has run; 2: the one-pass way up has run and u of level 1 is
    not brought up (include/mgrit_hip.h, mgrit_hip_up2_pending)"""
    return int(load().mgrit_hip_up2_pending(h))


def newton_stats(h, lvl):
    """{phi, newton_iterations, cg_iterations, at_newton_maxiter} of a Newton level since the last call (which resets them);
    cg_iterations counts the inner iterations: CG (Allen-Cahn) or BiCGStab (Gray-Scott)"""
    out = (C.c_int64 * 4)()
    check(load().mgrit_hip_newton_stats(h, int(lvl), out))
    return dict(zip(("phi", "newton_iterations", "cg_iterations", "at_newton_maxiter"), (int(v) for v in out)))
