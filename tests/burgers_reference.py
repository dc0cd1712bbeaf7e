"""An independent Phi for the Burgers2D IMEX step: no Hartley table, no eigenvalues, no transform of any kind.

    ax_c[i][j] = (c[i+1][j] - c[i-1][j]) / (2 dx),   ay_c[i][j] = (c[i][j+1] - c[i][j-1]) / (2 dx)     (indices mod nx, axis 0 = x)
    b_c = c - dt (u ax_c + v ay_c)                                                                    in np.longdouble, c = u, v
    (I - dt nu Lap) x_c = b_c,   Lap = periodic 5-point stencil / dx^2,   dx = L / nx

The solve is ``gray_scott_reference.solve_plane`` (sparse LU start, three refinements with a long-double residual), imported, not
copied: it asserts norm_F(b_c - A x_c) <= EPS / 2 norm_F(b_c) before it rounds, and with norm_2(A^-1) <= 1 the returned plane is off by
at most EPS norm_F(b_c). That is the only allowance the reference gets in a test. Its certificate holds for r = dt nu / dx^2 <= 50
(gray_scott_reference.py), so the test grids keep r below that on their coarsest level.

``ReferenceBurgers2D`` overrides ``step`` with this Phi, which sends a hierarchy to the plugin path.
"""
import numpy as np

from gray_scott_reference import EPS, LD, solve_plane      # noqa: F401  (EPS, LD: re-exported for the tests)
from pymgrit_amd import Burgers2D, VectorBurgers2D


def right_hand_side(w, dt, nx, L):
    """(b_u, b_v) in long double from the float64 planes w[0] = u, w[1] = v"""
    u, v = np.asarray(w[0], dtype=LD), np.asarray(w[1], dtype=LD)
    two_dx = LD(2) * LD(L) / LD(nx)
    out = []
    for c in (u, v):
        ax = (np.roll(c, -1, axis=0) - np.roll(c, 1, axis=0)) / two_dx
        ay = (np.roll(c, -1, axis=1) - np.roll(c, 1, axis=1)) / two_dx
        out.append(c - LD(dt) * (u * ax + v * ay))
    return out


def reference_phi(w, dt, nx, nu, L):
    """Phi(w) for one step of size dt as a float64 [2][nx][nx] array (w: 2 nx^2 values, u plane then v plane, any shape)"""
    dt = float(dt)
    w = np.asarray(w, dtype=np.float64).reshape(2, nx, nx)
    r = LD(dt) * LD(nu) * (LD(nx) / LD(L)) ** 2
    return np.stack([solve_plane(rhs, nx, r) for rhs in right_hand_side(w, dt, nx, L)])


class ReferenceBurgers2D(Burgers2D):
    """Burgers2D whose ``step`` is ``reference_phi``; overriding step selects the plugin path"""

    def step(self, u_start, t_start, t_stop):
        ret = VectorBurgers2D(self.nx)
        ret.set_values(reference_phi(u_start.get_values(), t_stop - t_start, self.nx, self.nu, self.L))
        return ret
