"""The periodic 2-D application kinds as the tests see them: one entry per kind, keyed as in periodic2d_bits.py. A plain helper like
cases.py: no tests, no fixtures. An entry states once what test_hip_<kind>.py, its *_reference.py sibling and the bit-for-bit record
(periodic2d_bits.py) build their hierarchies from:

  cls, reference, newton_reference   the pymgrit_amd class name; (module, class) of the second implementation of Phi under tests/
  planes, ranges(name, newton)       planes per state; the ranges of the random states, one (lo, hi) per draw of a list's rows
  par(nx)                            the application parameters of the sweep tests
  newton                             Newton variant: the parameters the device side alone takes (the reference classes fix theirs)
  t_sweep(nx), ragged(nx), dyadic_step   the sweep horizon (nt 17 / 9 / 5), the ragged grids, the exact step of the one-dt-group grids
  bounds(side)                       the object run_sweeps takes (periodic2d_sweeps.py), side "host" or "reference"

Every number is the one the kind's test file held before this table; they differ between kinds for stated reasons: each
test_hip_<kind>.py docstring derives its per-Phi term and Lipschitz factor and says which certificate of the reference its ranges
stay inside. Adding a kind: one entry here, a name in periodic2d_bits.CASES, and a test file with the tests that are its own.
"""
import importlib
import types

import numpy as np

import cases
from cahn_hilliard_reference import b_norm as ch_b_norm, c_of as ch_c_of, d2max as ch_d2max
from ginzburg_landau_reference import ALLOWANCE as GL_ALLOWANCE
from navier_stokes_reference import ALLOWANCE as NS_ALLOWANCE, C as ns_coef, lam_1, majorant as ns_majorant, stream_function

EPS = cases.EPS
RAGGED_UNITS = np.array([1, 1, 1.5, .5, 2, 1, 1, .75, 1, 1, 1, 1.25, 3, 1, 1, 1])      # 16 steps, 18 units, at most 6.25 per coarse step
RAGGED = np.concatenate(([0.0], np.cumsum(RAGGED_UNITS)))
RAGGED_1E4 = np.concatenate(([0.0], np.cumsum(1e-4 * RAGGED_UNITS)))                     # Allen-Cahn, Cahn-Hilliard, Heat2D: largest step 6e-4


def by_levels(t):
    return {"by2_3lvl": [t, t[::2], t[::4]], "by4_2lvl": [t, t[::4]]}


def dyadic(kind, n_pts):
    """n_pts points t_k = k * the kind's exact step (every difference is exact: one bit pattern of dt), and every second of them"""
    t = KINDS[kind].dyadic_step * np.arange(float(n_pts))
    return [t, t[::2]]


def reference_class(kind, newton=False):
    module, name = KINDS[kind].newton_reference if newton else KINDS[kind].reference
    return getattr(importlib.import_module(module), name)


def _fine_rows(ref, st, lvl):
    return st[("u", lvl)]


def _bounds(phi_term, lip, planes, coarse_rows=_fine_rows, weight_in_key=True):
    return types.SimpleNamespace(phi_term=lambda ref, app, rows, dt: phi_term(app, rows, dt), lip=lip, coarse_rows=coarse_rows,
                                 values_per_state=lambda app: planes * app.nx ** 2, weight_in_key=weight_in_key)


# ---- Allen-Cahn (test_hip_allen_cahn.py, test_hip_allen_cahn_reference.py) ---------------------------------------------------------
def ac_b_norm(app, rows, c):
    rows = np.abs(np.atleast_2d(rows))
    return float(np.max(np.linalg.norm(rows + c * np.abs(rows * (1.0 - rows ** app.nu)), axis=1)))


def ac_lip(app, dt, rows):
    c, R = dt / app.eps ** 2, float(np.abs(rows).max())
    return max(abs(1 + c), abs(1 + c * (1 - (app.nu + 1) * R ** app.nu)))


def _ac_bounds(side):
    """host: two evaluations of (4 nx + 8) EPS bnorm; reference: one, and EPS bnorm for the reference's rounding. c = dt / eps^2"""
    units = (lambda nx: 2 * (4 * nx + 8)) if side == "host" else (lambda nx: (4 * nx + 8) + 1)
    return _bounds(lambda app, rows, dt: units(app.nx) * EPS * ac_b_norm(app, rows, dt / app.eps ** 2), ac_lip, 1, weight_in_key=False)


# ---- Gray-Scott (test_hip_gray_scott.py) -------------------------------------------------------------------------------------------
def gs_phi_term(app, rows, dt):
    """one device evaluation and the reference's rounding, the two species in quadrature"""
    rows = np.abs(np.atleast_2d(rows))
    n = app.nx ** 2
    u, v = rows[:, :n], rows[:, n:]
    bu = float(np.max(np.linalg.norm(u + dt * (abs(app.a) * np.abs(1.0 - u) + u * v * v), axis=1)))
    bv = float(np.max(np.linalg.norm(v + dt * (u * v * v + abs(app.b) * v), axis=1)))
    return ((4 * app.nx + 8) + 1) * EPS * float(np.hypot(bu, bv))


def gs_lip(app, dt, rows):
    R2 = float(np.abs(rows).max()) ** 2
    return float(np.linalg.norm([[1 + dt * (abs(app.a) + R2), 2 * dt * R2], [dt * R2, 1 + dt * (2 * R2 + abs(app.b))]]))


def _gs_ragged(nx):
    return by_levels(RAGGED * 0.5 * (2.0 / nx) ** 2)      # unit step: r = dt du / dx^2 = 0.5; at most 6.25 units per coarse step


# ---- Cahn-Hilliard (test_hip_cahn_hilliard.py, test_hip_cahn_hilliard_reference.py) ------------------------------------------------
def ch_lip(app, dt, rows):
    R = float(np.abs(rows).max())
    return 1.0 + ch_d2max(app, dt) * max(1.0 + app.stab, abs(3.0 * R * R - (1.0 + app.stab)))


def _ch_bounds(side):
    """the device's C(nx) EPS bnorm and the other side's: C(nx) again for the host step, 1 for the reference (its asserted error).
    fas_residual: the coarse level's Phi acts on the restricted rows of the fine u (full weighting has non-negative weights that sum
    to 1: values stay in [-1, 1], a row norm does not grow beyond the fine row's)"""
    from periodic2d_sweeps import host_state
    other = ch_c_of if side == "host" else (lambda nx: 1)
    return _bounds(lambda app, rows, dt: (ch_c_of(app.nx) + other(app.nx)) * EPS * ch_b_norm(app, rows, dt), ch_lip, 1,
                   coarse_rows=lambda host, st, lvl: host_state(host, "v", lvl + 1), weight_in_key=False)


# ---- Burgers (test_hip_burgers.py) -------------------------------------------------------------------------------------------------
def bg_coef(nx):
    return 4 * nx + 12


def bg_majorant(app, rows, dt):
    """the largest row majorant, both planes joined"""
    nx = app.nx
    w = np.abs(np.atleast_2d(rows)).reshape(-1, 2, nx, nx)
    u, v = w[:, 0], w[:, 1]
    m2 = 0.0
    for c in (u, v):
        m = c + dt * app.inv_2dx * (u * (np.roll(c, -1, 1) + np.roll(c, 1, 1)) + v * (np.roll(c, -1, 2) + np.roll(c, 1, 2)))
        m2 = m2 + np.sum(m * m, axis=(1, 2))
    return float(np.sqrt(np.max(m2)))


def _two_sided(coef, allowance, majorant, lip, planes):
    """device against host 2 C(nx) EPS m, device against reference (C(nx) + the reference's allowance) EPS m"""
    def bounds(side):
        units = (lambda nx: 2 * coef(nx)) if side == "host" else (lambda nx: coef(nx) + allowance)
        return _bounds(lambda app, rows, dt: units(app.nx) * EPS * majorant(app, rows, dt), lip, planes)
    return bounds


# ---- Navier-Stokes (test_hip_navier_stokes.py) -------------------------------------------------------------------------------------
def ns_row_majorant(app, rows, dt):
    """the largest row majorant M1 + M2 (navier_stokes_reference.majorant: the reference's psi, the suite's own formula)"""
    return max(ns_majorant(row, dt, app.nx, app.L, app.forcing) for row in np.atleast_2d(rows))


def ns_lip(app, dt, rows):
    nx, dx = app.nx, app.dx
    U = 0.0
    for row in np.atleast_2d(rows):
        psi = stream_function(row, nx, app.L).astype(np.float64)
        U = max(U, float(np.abs(np.roll(psi, -1, 0) - np.roll(psi, 1, 0)).max()) / (2 * dx),
                float(np.abs(np.roll(psi, -1, 1) - np.roll(psi, 1, 1)).max()) / (2 * dx))
    R = float(np.abs(rows).max())
    return 1.0 + 2.0 * dt * (1.0 + 1e-6) * (U / dx + R / (lam_1(nx, app.L) * dx ** 2))


# ---- Ginzburg-Landau (test_hip_ginzburg_landau.py) ---------------------------------------------------------------------------------
def gl_coef(nx):
    return 4 * nx + 25      # C(nx) of test_ginzburg_landau_cpu.py, valid for rr sqrt(1 + b^2) <= 1 / 4


def gl_majorant(app, rows, dt):
    """the largest row majorant over both planes"""
    w = np.abs(np.atleast_2d(rows)).reshape(-1, 2, app.nx * app.nx)
    x, y = w[:, 0], w[:, 1]
    q = x * x + y * y
    c = abs(app.c)
    R = x + dt * (x + q * (x + c * y))
    S = y + dt * (y + q * (c * x + y))
    return float(np.sqrt(np.max(np.sum(R * R, axis=1) + np.sum(S * S, axis=1))))


def gl_lip(app, dt, rows):
    w = np.atleast_2d(rows).reshape(-1, 2, app.nx * app.nx)
    R2 = float(np.max(w[:, 0] ** 2 + w[:, 1] ** 2))
    return 1.0 + dt * (1.0 + 3.0 * np.sqrt(1.0 + app.c ** 2) * R2 * (1.0 + 1e-6))


SIGNED = [(-1.0, 1.0)]      # one draw over all planes of a list's rows


def _kind(**entry):
    entry.setdefault("newton_reference", None)
    entry.setdefault("newton", None)
    entry.setdefault("ranges", lambda name, newton=False: SIGNED)
    return types.SimpleNamespace(**entry)


KINDS = {
    "allencahn": _kind(
        cls="AllenCahn", reference=("allen_cahn_reference", "ReferenceAllenCahn"),
        newton_reference=("allen_cahn_newton_reference", "ReferenceAllenCahnNewton"), newton=dict(linear_solver="pcg"), planes=1,
        par=lambda nx: dict(nu=2, method="IMEX"), t_sweep=lambda nx: 0.002, ragged=lambda nx: by_levels(RAGGED_1E4),
        dyadic_step=2.0 ** -17, bounds=_ac_bounds),
    "grayscott": _kind(
        cls="GrayScott", reference=("gray_scott_reference", "ReferenceGrayScott"),
        newton_reference=("gray_scott_newton_reference", "ReferenceGrayScottNewton"), newton=dict(method="IMPL", linear_solver="bicgstab"),
        planes=2,      # u in [0, 1], v in [0, 0.5]; the right-hand sides of the Newton variant small and signed
        ranges=lambda name, newton=False: [(-0.01, 0.01), (-0.005, 0.005)] if newton and name == "g" else [(0.0, 1.0), (0.0, 0.5)],
        par=lambda nx: dict(method="IMEX"),
        # [0, T] with 16 fine steps of r = dt du / dx^2 = 2 (du = 1, L = 2): r = 8 on the coarsest of the three levels; dt = 0.5 at nx = 4
        t_sweep=lambda nx: 16 * 2.0 * (2.0 / nx) ** 2, ragged=_gs_ragged, dyadic_step=2.0 ** -7,
        bounds=lambda side: _bounds(gs_phi_term, gs_lip, 2)),
    "cahnhilliard": _kind(
        cls="CahnHilliard", reference=("cahn_hilliard_reference", "ReferenceCahnHilliard"), planes=1,
        par=lambda nx: dict(L=nx / 16.0, eps=0.1, stab=2.0), t_sweep=lambda nx: 0.002, ragged=lambda nx: by_levels(RAGGED_1E4),
        dyadic_step=2.0 ** -17, bounds=_ch_bounds),
    "burgers": _kind(
        cls="Burgers2D", reference=("burgers_reference", "ReferenceBurgers2D"), planes=2,
        par=lambda nx: dict(nu=0.1, L=nx / 16), t_sweep=lambda nx: 0.004,
        ragged=lambda nx: by_levels(RAGGED * 2.0 ** -12),      # 18 units: [0, 0.0044]; at most 6.25 units per coarse step, dt / dx = 0.024
        dyadic_step=2.0 ** -18, bounds=_two_sided(bg_coef, 1, bg_majorant, lambda app, dt, rows: 1.0 + 4.0 * dt * float(np.abs(rows).max()) / app.dx, 2)),
    "navierstokes": _kind(
        cls="NavierStokes2D", reference=("navier_stokes_reference", "ReferenceNavierStokes2D"), planes=1,
        par=lambda nx: dict(nu=0.1, L=nx / 16), t_sweep=lambda nx: 0.004,
        ragged=lambda nx: by_levels(RAGGED * 2.0 ** -12),      # 18 units: [0, 0.0044]; at most 6.25 units per coarse step, dt = 0.0015
        dyadic_step=2.0 ** -19, bounds=_two_sided(ns_coef, NS_ALLOWANCE, ns_row_majorant, ns_lip, 1)),
    "ginzburglandau": _kind(
        cls="GinzburgLandau2D", reference=("ginzburg_landau_reference", "ReferenceGinzburgLandau2D"), planes=2,
        par=lambda nx: dict(b=1.5, c=-0.8, L=float(nx)), t_sweep=lambda nx: 0.5,
        ragged=lambda nx: by_levels(RAGGED * 2.0 ** -6),       # 18 units: [0, 0.28]; at most 6.25 units = 0.098 per coarse step
        dyadic_step=2.0 ** -13, bounds=_two_sided(gl_coef, GL_ALLOWANCE, gl_majorant, gl_lip, 2)),
}
GSN_RAGGED = by_levels(0.039 * RAGGED)      # Gray-Scott Newton-BiCGStab: largest step 6.25 units = 0.244, inside dt <= 0.25

# Allen-Cahn's (and Heat2D's) grids of sweeps that split into several batches, levels [t, t[::2]]
H = KINDS["allencahn"].dyadic_step      # 7.6e-6: every t_k = k H and every difference is exact, one bit pattern of dt
TWO_SIZES = np.concatenate((H * np.arange(2051.0), H * np.array([2052.0, 2054.0])))      # dt groups of 1025 and 1 items


def _levels_by2(t):
    return [dict(t_interval=np.asarray(x)) for x in (t, t[::2])]


AC_BATCH_GRIDS = {
    # as nt = / linspace: a dozen bit patterns of dt per level, the largest group has some 620 items (one launch each)
    "linspace_2051": lambda: [dict(t_start=0, t_stop=2050e-5, nt=nt) for nt in (2051, 1026)],
    "cumsum_2051": lambda: _levels_by2(np.concatenate(([0.0], np.cumsum([1e-5] * 2048 + [2e-5] * 2)))),
    # exact steps: 1025 F-points / C-points of one dt = a batch of 1024 and one of 1
    "dyadic_2051": lambda: _levels_by2(H * np.arange(2051.0)),
    # 2050 steps H, then two steps 2 H: a full batch, a remainder of 1 and a second dt group in one sweep
    "dyadic_2053_two_sizes": lambda: _levels_by2(TWO_SIZES),
}
AC_BATCH_GROUPS = {"dyadic_2051": [1025], "dyadic_2053_two_sizes": [1, 1025]}      # sizes of the dt groups among the level-0 F-points
