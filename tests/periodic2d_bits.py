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
  every kind with the application parameters, the ragged time grid and the ranges of the random states of its own test_hip_<kind>.py;
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
import test_hip_burgers as bg
import test_hip_cahn_hilliard as ch
import test_hip_ginzburg_landau as gl
import test_hip_gray_scott_newton as gsn
import test_hip_navier_stokes as ns
from test_hip_allen_cahn import _lists
from test_hip_allen_cahn_newton import H, RAGGED_GRIDS
from test_hip_gray_scott import _ragged

GOLDEN_FILE = os.path.join(cases.GOLDEN, "periodic2d_bits.json")
WEIGHT_C = 1.3
STORED_STATE_SWEEPS = ("f_relax", "c_relax", "fas_residual", "compute_residual")
ALL_SWEEPS = ("f_relax", "c_relax", "fas_residual", "forward_solve", "compute_residual", "jump_solve")


def _make_cases():
    out = {}
    ragged = RAGGED_GRIDS["by2_3lvl"]
    for nx in (4, 33, 66):
        out[f"allencahn_imex_nx{nx}"] = dict(app="allencahn", nx=nx, par=dict(nu=2, method="IMEX"), grids=ragged, sweeps=ALL_SWEEPS)
    for nx in (4, 33, 66, 97):
        out[f"grayscott_imex_nx{nx}"] = dict(app="grayscott", nx=nx, par=dict(method="IMEX"), grids=_ragged(nx, "by2_3lvl"), sweeps=ALL_SWEEPS)
    for method in ("IMPL", "CN"):
        for nx, nu in ((4, 2), (33, 2), (66, 2), (20, 4)):
            out[f"allencahn_{method.lower()}_nx{nx}_nu{nu}"] = dict(app="allencahn", nx=nx, par=dict(nu=nu, method=method, linear_solver="pcg"),
                                                                   grids=ragged, sweeps=ALL_SWEEPS)
    for nx in (4, 33, 66):      # the IMEX kinds that came after, each as its own test builds it
        out[f"cahnhilliard_imex_nx{nx}"] = dict(app="cahnhilliard", nx=nx, par=dict(L=nx / 16.0, eps=0.1, stab=2.0), grids=ch.RAGGED_GRIDS["by2_3lvl"], sweeps=ALL_SWEEPS)
        out[f"burgers_imex_nx{nx}"] = dict(app="burgers", nx=nx, par=dict(nu=bg.NU, L=nx / 16), grids=bg._ragged("by2_3lvl"), sweeps=ALL_SWEEPS)
        out[f"navierstokes_imex_nx{nx}"] = dict(app="navierstokes", nx=nx, par=dict(nu=ns.NU, L=nx / 16), grids=ns._ragged("by2_3lvl"), sweeps=ALL_SWEEPS)
        out[f"ginzburglandau_imex_nx{nx}"] = dict(app="ginzburglandau", nx=nx, par=dict(b=gl.B, c=gl.CC, L=float(nx)), grids=gl._ragged("by2_3lvl"),
                                                  sweeps=ALL_SWEEPS)
    out["navierstokes_imex_nx33_forcing"] = dict(app="navierstokes", nx=33, par=dict(nu=ns.NU, L=33 / 16, forcing=ns.kolmogorov(33)),
                                                 grids=ns._ragged("by2_3lvl"), sweeps=ALL_SWEEPS)
    for nx in (4, 33):
        out[f"grayscott_impl_nx{nx}"] = dict(app="grayscott", nx=nx, par=dict(method="IMPL", linear_solver="bicgstab"),
                                             grids=gsn.RAGGED_GRIDS["by2_3lvl"], sweeps=ALL_SWEEPS)
    # more than one batch per sweep, the grids of the test_sweeps_of_more_than_one_batch tests
    two_sizes = np.concatenate((H * np.arange(2051.0), H * np.array([2052.0, 2054.0])))      # dt groups of 1025 and 1 items
    dyadic = 2.0 ** -7 * np.arange(1027.0)                                                   # one dt group of 513 states
    out["grayscott_imex_nx4_batches"] = dict(app="grayscott", nx=4, par=dict(method="IMEX"), grids=[dyadic, dyadic[::2]],
                                             sweeps=STORED_STATE_SWEEPS, levels=[0])
    out["allencahn_imex_nx4_batches"] = dict(app="allencahn", nx=4, par=dict(nu=2, method="IMEX"), grids=[two_sizes, two_sizes[::2]],
                                             sweeps=STORED_STATE_SWEEPS, levels=[0])
    out["allencahn_impl_nx4_batches"] = dict(app="allencahn", nx=4, par=dict(nu=2, method="IMPL", linear_solver="pcg"),
                                             grids=[two_sizes, two_sizes[::2]], sweeps=STORED_STATE_SWEEPS, levels=[0])
    return out


CASES = _make_cases()


def _sha(a, dtype=np.float64):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=dtype).tobytes()).hexdigest()


def _hierarchy(spec, **opts):
    import pymgrit_amd
    from pymgrit_amd import Mgrit
    app = getattr(pymgrit_amd, {"allencahn": "AllenCahn", "grayscott": "GrayScott", "cahnhilliard": "CahnHilliard", "burgers": "Burgers2D",
                                "navierstokes": "NavierStokes2D", "ginzburglandau": "GinzburgLandau2D"}[spec["app"]])
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
    top, n, digests = mg.lvl_max - 1, spec["nx"] ** 2, {}
    newton = "linear_solver" in spec["par"]

    def fresh():
        for lvl in range(mg.lvl_max):
            for which, lst in _lists(mg, lvl):
                if spec["app"] == "grayscott":      # [u plane | v plane], u in [0, 1], v in [0, 0.5]; Newton: g small and signed
                    hi = (0.01, 0.005) if newton and which == "g" else (1.0, 0.5)
                    lo = (-0.01, -0.005) if newton and which == "g" else (0.0, 0.0)
                    val = np.concatenate([rng.uniform(lo[c], hi[c], size=(len(lst), n)) for c in range(2)], axis=1)
                else:                               # one plane, or [plane | plane] of Burgers and Ginzburg-Landau
                    val = rng.uniform(-1.0, 1.0, size=(len(lst), n * (2 if spec["app"] in ("burgers", "ginzburglandau") else 1)))
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
