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

half a unit of the second part of the tests' majorant (below). With solve_plane's EPS norm_F(b) that is the only
allowance the reference gets in a test: ALLOWANCE = 2 units of EPS * majorant (1/2 + 1, rounded up).

The long-double residual floor of the Poisson certificate is about eps_ld * 8 norm(psi) / dx^2, far below EPS / 2 norm(w) at the sizes
the tests use (nx <= 129); solve_plane's certificate holds for r = dt nu / dx^2 <= 50 (gray_scott_reference.py), so the test grids keep
r below that on their coarsest level.

``ReferenceNavierStokes2D`` overrides ``step`` with this Phi, which sends a hierarchy to the plugin path.

The tolerance of one IMEX step (``C``, ``lam_1``, ``majorant`` below: the bounds the CPU and the GPU tests share), nothing in it measured
on the code under test:

    norm_F(error) <= (C(nx) + ALLOWANCE) EPS M,      C(nx) = 4 nx + 17,      M = M1 + M2

    M1 = norm_F(|w| + dt inv_2dx^2 ((|psi[j+1]| + |psi[j-1]|) (|w[i+1]| + |w[i-1]|) + (|psi[i+1]| + |psi[i-1]|) (|w[j+1]| + |w[j-1]|)) + dt |f|)
    M2 = dt (norm_F(w) / (lam_1 dx)) (max |wx| + max |wy|),      lam_1 = (4 / dx^2) sin^2(pi / nx)

M1 is the row majorant of the stencil's own terms: b = w - dt (py wx - px wy) + dt f with every sign dropped, so |b| <= the expression
under the norm point by point, and so is every intermediate of the evaluation. psi in it is the REFERENCE's stream function (long
double, rounded): the majorant comes from the reference's numbers, not from the code under test.
M2 carries an error of psi into b. If psi is off by delta (Frobenius norm), a central difference of it is off by at most
norm(delta) / dx (two shifted copies over 2 dx), the Jacobian py wx - px wy by (norm(delta) / dx) (max |wx| + max |wy|), b by dt times
that. psi = T ((T w T) o S) T with |S| <= 1 / lam_1 is off by a multiple of EPS norm_F(w) / lam_1 -- norm_F(w) with its mean: the first
two products act on w as it is, the mean leaves with S[0][0] = 0 only after them.
  * 4 nx: a product with an orthogonal n x n matrix is off by at most n eps (1 - n eps)^-1 times the operand's 2-norm
    (allen_cahn_fixtures.py derives the rule). The stream-function solve has four such products: psi is off by 4 nx EPS norm_F(w) / lam_1,
    which is 4 nx EPS M2 in b. The diffusion solve has four more, the table between them has |D| <= 1 and norm_F(b) <= M1: 4 nx EPS M1.
  * 17: b at one point. Each of px, py, wx, wy is a subtraction, a multiplication and the rounded quotient inv_2dx: 3. A term py wx is
    3 + 3 + 1, the difference of the two terms one more, the product with dt and the sum with w two more: 10, each relative to a
    partial result the point's term of M1 bounds; the forcing adds a product and a sum: 12 (one rounding less wherever the device
    fuses). The table D is a number <= 1: lam_i + lam_j carries the eigenvalues' own roundings (four each, relative), damped by
    z / (1 + z)^2 <= 1 / 4 -- two units --, then a sum, a quotient and the scale: 5. Together 17. On the psi side the table S is the
    eigenvalues' roundings (4), their sum, the quotient and the scale: 7 <= 17, in units of EPS M2.
  * ALLOWANCE (2): what the reference itself is off by (above: 1/2 M2 for the stream function's certificate,
    norm_F(b) <= M1 for solve_plane).
The device form fuses multiply-adds of b, which only removes roundings; numpy does not fuse, the bound covers both. (For orientation
only: a prototype against a transform-based long-double step, which is not independent, stayed below 4 EPS M at these sizes.)
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


# ---- the bounds of the tests (module docstring) ------------------------------------------------------------------------------------
def C(nx):
    return 4 * nx + 17


def lam_1(nx, L):
    dx = L / nx
    return 4.0 / dx ** 2 * np.sin(np.pi / nx) ** 2


def majorant(w, dt, nx, L, forcing=None):
    """M = M1 + M2 of the module docstring, evaluated by its own formula from the reference's stream function"""
    dx = L / nx
    inv_2dx = 1.0 / (2.0 * dx)
    a = np.abs(np.asarray(w, dtype=np.float64).reshape(nx, nx))
    p = np.abs(stream_function(w, nx, L).astype(np.float64))
    m = a + dt * inv_2dx ** 2 * ((np.roll(p, -1, 1) + np.roll(p, 1, 1)) * (np.roll(a, -1, 0) + np.roll(a, 1, 0))
                                 + (np.roll(p, -1, 0) + np.roll(p, 1, 0)) * (np.roll(a, -1, 1) + np.roll(a, 1, 1)))
    if forcing is not None:
        m = m + dt * np.abs(forcing)
    w2 = np.asarray(w, dtype=np.float64).reshape(nx, nx)
    wx = np.abs(np.roll(w2, -1, 0) - np.roll(w2, 1, 0)).max() * inv_2dx
    wy = np.abs(np.roll(w2, -1, 1) - np.roll(w2, 1, 1)).max() * inv_2dx
    return float(np.linalg.norm(m)) + dt * float(np.linalg.norm(w2)) / (lam_1(nx, L) * dx) * (wx + wy)


def kolmogorov(nx, k=2, amp=3.0):
    """f = -amp k cos(k Y) + a part that depends on x as well, so that a transposed forcing plane shows"""
    X = 2 * np.pi * np.arange(nx)[:, None] / nx
    Y = 2 * np.pi * np.arange(nx)[None, :] / nx
    return -amp * k * np.cos(k * Y) + 0.5 * amp * np.sin(X) * np.cos(Y)
