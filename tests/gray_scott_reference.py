"""An independent Phi for the Gray-Scott IMEX step: no Hartley table, no eigenvalues, no transform of any kind.

    b_u = u + dt (a (1 - u) - u v^2),   b_v = v + dt (u v^2 - b v)             in np.longdouble
    (I - dt d_c Lap) x_c = b_c,   Lap = periodic 5-point stencil / dx^2,   dx = L / nx,   c = u, v

Per species the solve starts from a float64 SuperLU factorisation of the sparse matrix, which this module builds from the stencil
definition, and is followed by three steps of iterative refinement whose residual is evaluated with ``np.roll`` in long double. The
factorisation only preconditions: what the function returns is pinned by its own long-double residual. A_c = I - dt d_c Lap is
symmetric with all eigenvalues >= 1, so norm_2(A_c^-1) <= 1 and the forward error of x_c is at most the residual's 2-norm, which is
asserted before rounding: norm_F(b_c - A_c x_c) <= EPS / 2 norm_F(b_c). Rounding to float64 adds at most EPS / 2 norm_F(x_c) and
norm_F(x_c) <= norm_F(b_c), so the returned plane is off by at most EPS norm_F(b_c). That is the only allowance the reference gets in
a test.

The assertion limits the step sizes this reference can certify: the long-double residual floor is about eps_ld (1 + 8 r),
r = dt d_c / dx^2. It fails near r = 1000 and holds for every r <= 50 tried, so the test grids keep r = dt du / dx^2 <= 50 on their
coarsest level.

``ReferenceGrayScott`` overrides ``step`` with this Phi, which sends a hierarchy to the plugin path: ``Mgrit([ReferenceGrayScott(..)..])``
is then the reference for every sweep -- the driver's own operand orders applied to an independently computed Phi.
"""
import functools

import numpy as np
import scipy.sparse as sp
from scipy.sparse.linalg import splu

from pymgrit_amd import GrayScott, VectorGrayScott2D

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
REFINEMENTS = 3


@functools.lru_cache(maxsize=64)
def _factorisation(nx, r):
    """SuperLU of I - r (stencil) in float64, r = dt d_c / dx^2, rows and columns in row-major grid order p = i nx + j"""
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
    """(I - dt d_c Lap) x on the periodic grid in long double, r = dt d_c / dx^2"""
    nb = np.roll(x, 1, axis=0) + np.roll(x, -1, axis=0) + np.roll(x, 1, axis=1) + np.roll(x, -1, axis=1)
    return x - r * (nb - LD(4) * x)


def right_hand_side(w, dt, a, b):
    """(b_u, b_v) in long double from the float64 planes w[0] = u, w[1] = v"""
    u, v = np.asarray(w[0], dtype=LD), np.asarray(w[1], dtype=LD)
    uv2 = u * v * v
    return u + LD(dt) * (LD(a) * (LD(1) - u) - uv2), v + LD(dt) * (uv2 - LD(b) * v)


def solve_plane(b, nx, r):
    """x with (I - r stencil) x = b, float64 [nx][nx]; b and r = dt d_c / dx^2 in long double (the factorisation takes r rounded)"""
    lu = _factorisation(int(nx), float(r))
    x = lu.solve(b.astype(np.float64).ravel()).reshape(nx, nx).astype(LD)
    for _ in range(REFINEMENTS):
        res = b - _apply(x, r)
        x = x + lu.solve(res.astype(np.float64).ravel()).reshape(nx, nx).astype(LD)
    res = b - _apply(x, r)
    res_f, b_f = float(np.sqrt(np.sum(res * res))), float(np.sqrt(np.sum(b * b)))
    assert res_f <= 0.5 * EPS * b_f, ("reference_phi: forward error bound", nx, float(r), res_f, b_f)
    return x.astype(np.float64)


def reference_phi(w, dt, nx, du, dv, a, b, L):
    """Phi(w) for one step of size dt as a float64 [2][nx][nx] array (w: 2 nx^2 values, u plane then v plane, any shape)"""
    dt = float(dt)
    w = np.asarray(w, dtype=np.float64).reshape(2, nx, nx)
    inv_dx2 = (LD(nx) / LD(L)) ** 2
    return np.stack([solve_plane(rhs, nx, LD(dt) * LD(d) * inv_dx2) for rhs, d in zip(right_hand_side(w, dt, a, b), (du, dv))])


class ReferenceGrayScott(GrayScott):
    """GrayScott whose ``step`` is ``reference_phi`` (method 'IMEX' only); overriding step selects the plugin path"""

    def step(self, u_start, t_start, t_stop):
        assert self.method == "IMEX"
        ret = VectorGrayScott2D(self.nx)
        ret.set_values(reference_phi(u_start.get_values(), t_stop - t_start, self.nx, self.du, self.dv, self.a, self.b, self.L))
        return ret
