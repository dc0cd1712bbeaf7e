"""An independent Phi for the NavierStokes2D IMEX step: no Hartley table, no eigenvalues, no transform of any kind.

    A psi = w - mean w,  mean psi = 0,     A = -Lap = (4 psi - the four neighbours) / dx^2 on the periodic grid, dx = L / nx
    px = (psi[i+1][j] - psi[i-1][j]) / (2 dx),   py = (psi[i][j+1] - psi[i][j-1]) / (2 dx),   wx, wy the same of w   (mod nx, axis 0 = x)
    b = w - dt (py wx - px wy) [+ dt f]                                                       all of it in np.longdouble
    (I - dt nu Lap) x = b

The diffusion solve is ``gray_scott_reference.solve_plane`` (sparse LU start, three refinements with a long-double residual), imported,
not copied: the returned plane is off by at most EPS norm_F(b).

The Poisson solve is singular (constants are the kernel of A), so it cannot use that function. It is a bordered system

    [ dx^2 A   1 ] [psi]   [dx^2 (w - mean w)]
    [ 1^T      0 ] [ s ] = [0]

factorised once per nx by SuperLU in float64 (non-singular: dx^2 A is positive definite on the zero-mean planes and the border pins the
mean), refined with a residual evaluated with ``np.roll`` in long double, psi kept in long double from there on (it is never rounded to
float64: it feeds the stencil directly). The factorisation only preconditions: what the function returns is pinned by its own
certificate, asserted on the zero-mean psi before anything else uses it,

    norm_F((w - mean w) - A psi) <= EPS / 2 norm_F(w - mean w).

On the zero-mean planes the smallest eigenvalue of A is lam_1 = (4 / dx^2) sin^2(pi / nx), so the forward error that certificate earns
is norm_F(psi - exact) <= EPS / 2 norm_F(w - mean w) / lam_1. A difference of psi over 2 dx is then off by at most that over dx in the
Frobenius norm, and b by at most

    EPS / 2 * dt * (norm_F(w) / (lam_1 dx)) * (max |wx| + max |wy|),

half a unit of the second part of the tests' majorant (test_navier_stokes_cpu.py). With solve_plane's EPS norm_F(b) that is the only
allowance the reference gets in a test: ALLOWANCE = 2 units of EPS * majorant (1/2 + 1, rounded up).

The long-double residual floor of the Poisson certificate is about eps_ld * 8 norm(psi) / dx^2, far below EPS / 2 norm(w) at the sizes
the tests use (nx <= 129); solve_plane's certificate holds for r = dt nu / dx^2 <= 50 (gray_scott_reference.py), so the test grids keep
r below that on their coarsest level.

``ReferenceNavierStokes2D`` overrides ``step`` with this Phi, which sends a hierarchy to the plugin path.
"""
import functools

import numpy as np
import scipy.sparse as sp
from scipy.sparse.linalg import splu

from gray_scott_reference import EPS, LD, solve_plane      # noqa: F401  (EPS, LD: re-exported for the tests)
from pymgrit_amd import NavierStokes2D, VectorNavierStokes2D

ALLOWANCE = 2
REFINEMENTS = 3


@functools.lru_cache(maxsize=16)
def _bordered(nx):
    """SuperLU of [[4 I - neighbours, 1], [1^T, 0]] in float64, rows and columns in row-major grid order p = i nx + j, the border last"""
    n = nx * nx
    i, j = np.divmod(np.arange(n), nx)
    p = i * nx + j
    rows, cols, vals = [p], [p], [np.full(n, 4.0)]
    for di, dj in ((1, 0), (-1, 0), (0, 1), (0, -1)):
        rows.append(p)
        cols.append(((i + di) % nx) * nx + (j + dj) % nx)
        vals.append(np.full(n, -1.0))
    rows += [p, np.full(n, n)]
    cols += [np.full(n, n), p]
    vals += [np.ones(n), np.ones(n)]
    A = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n + 1, n + 1))
    return splu(sp.csc_matrix(A))


def _neg_stencil(x):
    """4 x - the four neighbours, in long double"""
    return LD(4) * x - (np.roll(x, 1, axis=0) + np.roll(x, -1, axis=0) + np.roll(x, 1, axis=1) + np.roll(x, -1, axis=1))


def stream_function(w, nx, L):
    """psi in long double with A psi = w - mean w and mean psi = 0, certificate asserted (module docstring)"""
    w = np.asarray(w, dtype=LD).reshape(nx, nx)
    dx2 = (LD(L) / LD(nx)) ** 2
    g = w - np.sum(w) / LD(nx * nx)
    rhs = dx2 * g
    lu = _bordered(int(nx))

    def correction(res):
        return lu.solve(np.append(res.astype(np.float64).ravel(), 0.0))[:-1].reshape(nx, nx).astype(LD)
    psi = correction(rhs)
    for _ in range(REFINEMENTS):
        psi = psi - np.sum(psi) / LD(nx * nx)
        psi = psi + correction(rhs - _neg_stencil(psi))
    psi = psi - np.sum(psi) / LD(nx * nx)
    res = g - _neg_stencil(psi) / dx2
    res_f, g_f = float(np.sqrt(np.sum(res * res))), float(np.sqrt(np.sum(g * g)))
    assert res_f <= 0.5 * EPS * g_f, ("stream_function: residual certificate", nx, res_f, g_f)
    return psi


def right_hand_side(w, dt, nx, L, forcing=None):
    """b in long double from the float64 plane w"""
    psi = stream_function(w, nx, L)
    w = np.asarray(w, dtype=LD).reshape(nx, nx)
    two_dx = LD(2) * LD(L) / LD(nx)
    px = (np.roll(psi, -1, axis=0) - np.roll(psi, 1, axis=0)) / two_dx
    py = (np.roll(psi, -1, axis=1) - np.roll(psi, 1, axis=1)) / two_dx
    wx = (np.roll(w, -1, axis=0) - np.roll(w, 1, axis=0)) / two_dx
    wy = (np.roll(w, -1, axis=1) - np.roll(w, 1, axis=1)) / two_dx
    b = w - LD(dt) * (py * wx - px * wy)
    if forcing is not None:
        b = b + LD(dt) * np.asarray(forcing, dtype=LD).reshape(nx, nx)
    return b


def reference_phi(w, dt, nx, nu, L, forcing=None):
    """Phi(w) for one step of size dt as a float64 [nx][nx] array (w: nx^2 values, any shape)"""
    dt = float(dt)
    w = np.asarray(w, dtype=np.float64).reshape(nx, nx)
    r = LD(dt) * LD(nu) * (LD(nx) / LD(L)) ** 2
    return solve_plane(right_hand_side(w, dt, nx, L, forcing), nx, r)


class ReferenceNavierStokes2D(NavierStokes2D):
    """NavierStokes2D whose ``step`` is ``reference_phi``; overriding step selects the plugin path"""

    def step(self, u_start, t_start, t_stop):
        ret = VectorNavierStokes2D(self.nx, self.ny)
        ret.set_values(reference_phi(u_start.get_values(), t_stop - t_start, self.nx, self.nu, self.L, self.forcing))
        return ret
