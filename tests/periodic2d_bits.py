"""The fixed cases of the bit-for-bit record of the periodic 2-D device paths (Allen-Cahn IMEX and Newton-PCG, Gray-Scott IMEX and
Newton-BiCGStab, Cahn-Hilliard, Burgers, Navier-Stokes and Ginzburg-Landau IMEX; csrc/mgrit_hip_periodic2d.inc and the kinds' own
.inc files), shared by tests/golden/make_golden_periodic2d_bits.py, which records
tests/golden/periodic2d_bits.json, and tests/test_hip_periodic2d_bits.py, which recomputes every digest and compares. Needs a GPU.

A case is one hierarchy on seeded inputs (np.random.default_rng). Before every sweep all lists of all levels are set afresh; after it
the SHA-256 of the bytes of the u, v and g slabs of every level in natural order is taken, of the compute_residual output, and on
Newton levels of the four mgrit_hip_newton_stats counts. The inputs (time grids and every state uploaded) have a digest of their own, so
a changed input is told apart from changed device arithmetic. Every slab digested is finite. Nothing is compared with a tolerance: these kernels have no floating-point
atomics and a sweep run twice gives the same bits (test_a_sweep_run_twice_gives_the_same_bits).

What the cases are chosen for -- the smallest shapes at which the tile product of the periodic grid can go another way:
  nx = 4 (one tile, KP = 32 > nx), 33 (K crosses one 32-step, pads inside the tile), 66 (two tiles per axis, P = 128, the last tile
  mostly pad), Gray-Scott also 97 (KP = P); Newton-PCG (IMPL and CN) also nx = 20 with nu = 4; Gray-Scott Newton-BiCGStab nx = 4, 33;
  Navier-Stokes at nx = 33 also with a forcing plane on every level;
  every kind with the application parameters, the ragged time grid and the ranges of the random states of its entry in the kinds
  table (tests/periodic2d_kinds.py), which its own test_hip_<kind>.py takes them from as well -- no test module is imported here;
  points (17, 9, 5) on a ragged time grid (several D tables per level, a plan grouped by step size), weight_c = 1.3;
  f_relax, c_relax, fas_residual per level, forward_solve on the coarsest level (batches of one on the chain's work buffers, or the
  Newton chain rows), compute_residual, and one solve of two iterations with the jump criterion (h2d_rowsq_kernel with H2D_OP_JUMP);
  at nx = 4 sweeps of more than one batch: Gray-Scott above 512 states, Allen-Cahn IMEX above 1024, Newton above ACN_MAX_BATCH.
"""
import hashlib
import os
import subprocess
import zlib

import numpy as np

import cases
from navier_stokes_reference import kolmogorov
from periodic2d_kinds import GSN_RAGGED, KINDS, TWO_SIZES, dyadic
from periodic2d_sweeps import draw, lists as _lists

GOLDEN_FILE = os.path.join(cases.GOLDEN, "periodic2d_bits.json")
WEIGHT_C = 1.3
STORED_STATE_SWEEPS = ("f_relax", "c_relax", "fas_residual", "compute_residual")
ALL_SWEEPS = ("f_relax", "c_relax", "fas_residual", "forward_solve", "compute_residual", "jump_solve")


def _make_cases():
    """every case from the kinds table (periodic2d_kinds.py): the kind's parameters, its ragged grid by2_3lvl, its dyadic step"""
    out = {}

    def case(name, kind, nx, par=None, grids=None, sweeps=ALL_SWEEPS, **more):
        out[name] = dict(app=kind, nx=nx, par=KINDS[kind].par(nx) if par is None else par,
                         grids=KINDS[kind].ragged(nx)["by2_3lvl"] if grids is None else grids, sweeps=sweeps, **more)
    for nx in (4, 33, 66):
        case(f"allencahn_imex_nx{nx}", "allencahn", nx)
    for nx in (4, 33, 66, 97):
        case(f"grayscott_imex_nx{nx}", "grayscott", nx)
    for method in ("IMPL", "CN"):
        for nx, nu in ((4, 2), (33, 2), (66, 2), (20, 4)):
            case(f"allencahn_{method.lower()}_nx{nx}_nu{nu}", "allencahn", nx, par=dict(nu=nu, method=method, **KINDS["allencahn"].newton))
    for nx in (4, 33, 66):      # the IMEX kinds that came after
        for kind in ("cahnhilliard", "burgers", "navierstokes", "ginzburglandau"):
            case(f"{kind}_imex_nx{nx}", kind, nx)
    case("navierstokes_imex_nx33_forcing", "navierstokes", 33, par=dict(KINDS["navierstokes"].par(33), forcing=kolmogorov(33)))
    for nx in (4, 33):
        case(f"grayscott_impl_nx{nx}", "grayscott", nx, par=dict(KINDS["grayscott"].newton), grids=GSN_RAGGED["by2_3lvl"])
    # more than one batch per sweep, the grids of the test_sweeps_of_more_than_one_batch tests: for Gray-Scott one dt group of 513
    # states, for Allen-Cahn dt groups of 1025 and 1 items
    batches = dict(sweeps=STORED_STATE_SWEEPS, levels=[0])
    case("grayscott_imex_nx4_batches", "grayscott", 4, grids=dyadic("grayscott", 1027), **batches)
    case("allencahn_imex_nx4_batches", "allencahn", 4, grids=[TWO_SIZES, TWO_SIZES[::2]], **batches)
    case("allencahn_impl_nx4_batches", "allencahn", 4, par=dict(nu=2, method="IMPL", **KINDS["allencahn"].newton), grids=[TWO_SIZES, TWO_SIZES[::2]],
         **batches)
    return out


CASES = _make_cases()


def _sha(a, dtype=np.float64):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=dtype).tobytes()).hexdigest()


def _hierarchy(spec, **opts):
    import pymgrit_amd
    from pymgrit_amd import Mgrit
    app = getattr(pymgrit_amd, KINDS[spec["app"]].cls)
    mg = Mgrit([app(nx=spec["nx"], t_interval=np.asarray(t), **spec["par"]) for t in spec["grids"]], nested_iteration=False, logging_lvl=30, **opts)
    assert type(mg.backend).__name__ == "HipBackend"
    return mg


def run_case(name):
    """{"inputs": digest of the time grids and of every state uploaded, "digests": {"<sweep>/<list><level>": digest}}"""
    spec = CASES[name]
    mg = _hierarchy(spec, weight_c=WEIGHT_C)
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    inputs = hashlib.sha256()
    for t in mg.t:
        inputs.update(np.ascontiguousarray(t, dtype=np.float64).tobytes())
    top, digests = mg.lvl_max - 1, {}
    newton = "linear_solver" in spec["par"]

    def fresh():
        for lvl in range(mg.lvl_max):
            for which, lst in _lists(mg, lvl):
                val = draw(spec["app"], rng, which, len(lst), spec["nx"], newton)      # the kind's ranges (periodic2d_kinds.py)
                inputs.update(val.tobytes())
                mg.backend.set_natural(which, lvl, val)

    def record(label, mgr=mg):
        for lvl in range(mgr.lvl_max):
            for which, _ in _lists(mgr, lvl):
                slab = mgr.backend.natural(which, lvl)
                assert np.all(np.isfinite(slab)), (name, label, which, lvl)
                digests[f"{label}/{which}{lvl}"] = _sha(slab)
            if newton:      # (the call resets the counts: they are those of this sweep)
                st = mgr.backend.newton_stats(lvl)
                digests[f"{label}/newton_stats{lvl}"] = _sha([st[k] for k in ("phi", "newton_iterations", "cg_iterations", "at_newton_maxiter")], np.int64)

    if newton:
        for lvl in range(mg.lvl_max):
            mg.backend.newton_stats(lvl)
    for lvl in spec.get("levels", range(top)):
        for sweep in ("f_relax", "c_relax", "fas_residual"):
            if sweep in spec["sweeps"]:
                fresh()
                getattr(mg, sweep)(lvl)
                record(f"{sweep}{lvl}")
    if "forward_solve" in spec["sweeps"]:
        fresh()
        mg.forward_solve(top)
        record("forward_solve")
    if "compute_residual" in spec["sweeps"]:
        fresh()
        digests["compute_residual/norms"] = _sha(np.asarray(mg.compute_residual()))
        record("compute_residual")
    if "jump_solve" in spec["sweeps"]:      # two iterations from the application's own initial guess, the jump criterion
        solve = _hierarchy(spec, weight_c=WEIGHT_C, conv_crit=1, max_iter=2, tol=0.0)
        digests["jump_solve/conv"] = _sha(np.asarray(solve.solve()["conv"]))
        record("jump_solve", solve)
    return {"inputs": inputs.hexdigest(), "digests": digests}


def hipcc_version():
    """the first line of `hipcc --version` that names the HIP version, or 'unknown'"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    try:
        out = subprocess.run([hipcc, "--version"], capture_output=True, text=True, timeout=60).stdout
    except (OSError, subprocess.SubprocessError):
        return "unknown"
    lines = [line.strip() for line in out.splitlines() if line.strip()]
    return next((line for line in lines if line.startswith("HIP version")), lines[0] if lines else "unknown")
