"""An independent Phi for the GinzburgLandau2D IMEX step: no Hartley table, no eigenvalues, no transform of any kind.

    q = x^2 + y^2,   r = x + dt (x - q (x - c y)),   s = y + dt (y - q (c x + y))                          in np.longdouble
    [ I - dt Lap     b dt Lap ] [x_new]   [r]
    [ -b dt Lap    I - dt Lap ] [y_new] = [s],       Lap = periodic 5-point stencil / dx^2,   dx = L / nx

The real form of (1 - dt (1 + i b) Lap) A_new = A + dt (A - (1 + i c) |A|^2 A). The ``2 nx^2 x 2 nx^2`` block system is built from the
stencil definition; the solve starts from its float64 SuperLU factorisation and is followed by three steps of iterative refinement
whose residual is evaluated with ``np.roll`` in long double. The factorisation only preconditions: what the function returns is pinned
by its own long-double residual. The block matrix M is normal (its blocks are polynomials of the one symmetric matrix Lap): in the
eigenbasis of Lap it is, per mode mu >= 0, the 2 x 2 block [[a, -beta], [beta, a]], a = 1 + dt mu, beta = b dt mu, whose two singular
values are sqrt(a^2 + beta^2) >= 1. So norm_2(M^-1) <= 1 and the forward error of (x_new, y_new) is at most the residual's 2-norm over
both planes, which is asserted before rounding: norm(residual) <= EPS / 2 norm((r, s)). Rounding to float64 adds at most
EPS / 2 norm((x_new, y_new)) <= EPS / 2 norm((r, s)): the returned state is off by at most ALLOWANCE EPS norm((r, s)) in the 2-norm over
all 2 nx^2 values, ALLOWANCE = 1. That is the only allowance the reference gets in a test.

The assertion limits the step sizes this reference can certify, as in gray_scott_reference.py: the long-double residual floor is about
eps_ld (1 + 8 rr sqrt(1 + b^2)), rr = dt / dx^2; the tests keep rr far below 50.

``ReferenceGinzburgLandau2D`` overrides ``step`` with this Phi, which sends a hierarchy to the plugin path.
"""
import functools

import numpy as np
import scipy.sparse as sp
from scipy.sparse.linalg import splu

from pymgrit_amd import GinzburgLandau2D, VectorGinzburgLandau2D

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
REFINEMENTS = 3
ALLOWANCE = 1


@functools.lru_cache(maxsize=8)
def _factorisation(nx, rr, brr):
    """SuperLU of the block matrix in float64; rr = dt / dx^2, brr = b dt / dx^2; unknown p = i nx + j of the x plane, nx^2 + p of the
    y plane. S = the stencil (neighbours - 4): x - rr S x + brr S y = r,  y - rr S y - brr S x = s"""
    n = nx * nx
    i, j = np.divmod(np.arange(n), nx)
    p = i * nx + j
    rows, cols, vals = [p], [p], [np.full(n, -4.0)]
    for di, dj in ((1, 0), (-1, 0), (0, 1), (0, -1)):
        rows.append(p)
        cols.append(((i + di) % nx) * nx + (j + dj) % nx)
        vals.append(np.ones(n))
    S = sp.csc_matrix(sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n)))
    eye = sp.identity(n, format="csc")
    return splu(sp.csc_matrix(sp.bmat([[eye - rr * S, brr * S], [-brr * S, eye - rr * S]])))


def _stencil(x):
    return (np.roll(x, 1, axis=0) + np.roll(x, -1, axis=0) + np.roll(x, 1, axis=1) + np.roll(x, -1, axis=1)) - LD(4) * x


def residual(x, y, r, s, rr, brr):
    """(r, s) - M (x, y) in long double"""
    sx, sy = _stencil(x), _stencil(y)
    return r - (x - rr * sx + brr * sy), s - (y - rr * sy - brr * sx)


def right_hand_side(w, dt, c):
    """(r, s) in long double from the float64 planes w[0] = Re A, w[1] = Im A"""
    x, y = np.asarray(w[0], dtype=LD), np.asarray(w[1], dtype=LD)
    q = x * x + y * y
    return x + LD(dt) * (x - q * (x - LD(c) * y)), y + LD(dt) * (y - q * (LD(c) * x + y))


def reference_phi(w, dt, nx, b, c, L):
    """Phi(w) for one step of size dt as a float64 [2][nx][nx] array (w: 2 nx^2 values, real plane then imaginary plane, any shape)"""
    dt, nx = float(dt), int(nx)
    w = np.asarray(w, dtype=np.float64).reshape(2, nx, nx)
    r, s = right_hand_side(w, dt, c)
    rr = LD(dt) * (LD(nx) / LD(L)) ** 2
    brr = LD(b) * rr
    lu = _factorisation(nx, float(rr), float(brr))

    def solve(fx, fy):
        z = lu.solve(np.concatenate((fx.astype(np.float64).ravel(), fy.astype(np.float64).ravel())))
        return z[:nx * nx].reshape(nx, nx).astype(LD), z[nx * nx:].reshape(nx, nx).astype(LD)

    x, y = solve(r, s)
    for _ in range(REFINEMENTS):
        dx_, dy_ = solve(*residual(x, y, r, s, rr, brr))
        x, y = x + dx_, y + dy_
    ex, ey = residual(x, y, r, s, rr, brr)
    res_f = float(np.sqrt(np.sum(ex * ex) + np.sum(ey * ey)))
    rhs_f = float(np.sqrt(np.sum(r * r) + np.sum(s * s)))
    assert res_f <= 0.5 * EPS * rhs_f, ("reference_phi: forward error bound", nx, float(rr), float(brr), res_f, rhs_f)
    return np.stack((x.astype(np.float64), y.astype(np.float64)))


class ReferenceGinzburgLandau2D(GinzburgLandau2D):
    """GinzburgLandau2D whose ``step`` is ``reference_phi``; overriding step selects the plugin path"""

    def step(self, u_start, t_start, t_stop):
        ret = VectorGinzburgLandau2D(self.nx)
        ret.set_values(reference_phi(u_start.get_values(), t_stop - t_start, self.nx, self.b, self.c, self.L))
        return ret
