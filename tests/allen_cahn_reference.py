"""An independent Phi for the Allen-Cahn IMEX step: no Hartley table, no eigenvalues, no transform of any kind.

    b = u + (dt / eps^2) u (1 - u^nu)                          in np.longdouble
    (I - dt L) x = b,   L = periodic 5-point stencil / dx^2,   dx = 1 / nx

The solve starts from a float64 SuperLU factorisation of the sparse matrix, which this module builds from the stencil definition
(not from ``AllenCahn.space_disc``), and is followed by three steps of iterative refinement whose residual is evaluated with
``np.roll`` in long double. The factorisation only preconditions: what the function returns is pinned by its own long-double residual,

    max|b - A x| <= 64 eps_ld (1 + 8 dt nx^2) max|b|,

asserted before rounding. A = I - dt L is symmetric with all eigenvalues >= 1, so norm_2(A^-1) <= 1 and the forward error of x is at
most the residual's 2-norm: eps_ld (1 + 8 dt nx^2) norm_F(x) or so, between 1e-3 ulp of a double on the small grids and 0.1 ulp at
nx = 257. That norm is asserted as well, norm_F(b - A x) <= EPS / 2 norm_F(b); rounding to float64 adds at most EPS / 2 norm_F(x) and
norm_F(x) <= norm_F(b), so the returned array is off by at most EPS norm_F(b). That is the only allowance the reference gets in a test.

``ReferenceAllenCahn`` overrides ``step`` with this Phi, which sends a hierarchy to the plugin path: ``Mgrit([ReferenceAllenCahn(..)..])``
is then the reference for every sweep -- the driver's own operand orders applied to an independently computed Phi.
"""
import functools

import numpy as np
import scipy.sparse as sp
from scipy.sparse.linalg import splu

from pymgrit_amd import AllenCahn, VectorAllenCahn2D

LD = np.longdouble
EPS_LD = LD(np.finfo(LD).eps)
REFINEMENTS = 3


@functools.lru_cache(maxsize=64)
def _factorisation(nx, dt):
    """SuperLU of I - dt L in float64, rows and columns in row-major grid order p = i nx + j"""
    r = dt * float(nx) ** 2
    i, j = np.divmod(np.arange(nx * nx), nx)
    p = i * nx + j
    rows, cols, vals = [p], [p], [np.full(nx * nx, 1.0 + 4.0 * r)]
    for di, dj in ((1, 0), (-1, 0), (0, 1), (0, -1)):
        rows.append(p)
        cols.append(((i + di) % nx) * nx + (j + dj) % nx)
        vals.append(np.full(nx * nx, -r))
    A = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(nx * nx, nx * nx))
    return splu(sp.csc_matrix(A))


def _apply(x, r):
    """(I - dt L) x on the periodic grid in long double, r = dt / dx^2"""
    nb = np.roll(x, 1, axis=0) + np.roll(x, -1, axis=0) + np.roll(x, 1, axis=1) + np.roll(x, -1, axis=1)
    return x - r * (nb - LD(4) * x)


def right_hand_side(u, dt, nu, eps):
    """b = u + (dt / eps^2) u (1 - u^nu) in long double"""
    u = np.asarray(u, dtype=LD)
    return u + (LD(dt) / LD(eps) ** 2) * u * (LD(1) - u ** int(nu))


def reference_phi(u, dt, nx, nu, eps):
    """Phi(u) for one step of size dt as a float64 [nx][nx] array (u: nx*nx values in row-major order, any shape)"""
    dt = float(dt)
    b = right_hand_side(np.asarray(u, dtype=np.float64).reshape(nx, nx), dt, nu, eps)
    lu = _factorisation(int(nx), dt)
    r = LD(dt) * LD(nx) ** 2
    x = lu.solve(b.astype(np.float64).ravel()).reshape(nx, nx).astype(LD)
    for _ in range(REFINEMENTS):
        res = b - _apply(x, r)
        x = x + lu.solve(res.astype(np.float64).ravel()).reshape(nx, nx).astype(LD)
    res = b - _apply(x, r)
    worst, allowed = float(np.abs(res).max()), float(LD(64) * EPS_LD * (LD(1) + LD(8) * r) * np.abs(b).max())
    assert worst <= allowed, ("reference_phi: residual of the long-double solve", nx, dt, worst, allowed)
    res_f, b_f = float(np.sqrt(np.sum(res * res))), float(np.sqrt(np.sum(b * b)))
    assert res_f <= 0.5 * float(np.finfo(np.float64).eps) * b_f, ("reference_phi: forward error bound", nx, dt, res_f, b_f)
    return x.astype(np.float64)


class ReferenceAllenCahn(AllenCahn):
    """AllenCahn whose ``step`` is ``reference_phi`` (method 'IMEX' only); overriding step selects the plugin path"""

    def step(self, u_start, t_start, t_stop):
        assert self.method == "IMEX"
        ret = VectorAllenCahn2D(self.nx, self.ny)
        ret.set_values(reference_phi(u_start.get_values(), t_stop - t_start, self.nx, self.nu, self.eps))
        return ret
