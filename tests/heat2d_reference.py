"""An independent Phi for the Heat2D theta scheme: no sine table, no eigenvalues, no fold, no transform of any kind.

    b = u_int - (1 - theta) dt (L u)_int + theta dt f(t_stop) + (1 - theta) dt f(t_start) + theta dt W          in np.longdouble
    (I + theta dt L_int) x = b,      L = the 5-point stencil  2 (fx + fy) c - fx (up + down) - fy (left + right)

``L u`` is taken on the full grid INCLUDING the rim values of u (Crank-Nicolson and forward Euler read them, backward Euler does not),
``L_int`` is the same stencil on the interior with zero Dirichlet values, and W = fx (BC above + BC below) + fy (BC left + BC right) is
what the boundary values of the NEW state contribute; it is built here from the stencil applied to ``boundary_values()``, not taken from
``Heat2D.boundary_coupling()``. f is the application's ``rhs`` callable (float64 values, as the user's code returns them).

theta > 0: the solve starts from a float64 SuperLU factorisation of the sparse interior matrix, which this module builds from the
stencil, and is followed by three steps of iterative refinement whose residual is evaluated with slices in long double. The
factorisation only preconditions: what the function returns is pinned by its own long-double residual, asserted before rounding,

    norm_F(b - A x) <= EPS / 2 norm_F(b).

A = I + theta dt L_int is symmetric with all eigenvalues >= 1, so norm_2(A^-1) <= 1 and the forward error of x is at most that residual;
rounding to float64 adds at most EPS / 2 norm_F(x) and norm_F(x) <= norm_F(b), so the returned interior is off by at most EPS norm_F(b).
That is the only allowance the reference gets in a test (the "+ 1" of ``phi_bound``).

theta = 0 (forward Euler): the explicit formula in long double, rounded once; the rim is ``boundary values + old rim`` (the quirk of
the scheme this application follows).

``right_hand_side`` returns next to b its absolute counterpart babs: the same sum with every term replaced by its absolute value (|L|
applied to |u|, |f|, |W| from |BC|). norm_F(babs) is the scale of every tolerance: it bounds what the roundings of ANY evaluation order
of b can amount to, and it bounds norm_F(b) and norm_F(x).

``ReferenceHeat2D`` overrides ``step`` with this Phi and describes no device stepper, which sends a hierarchy to the plugin path:
``Mgrit([ReferenceHeat2D(..) ..])`` is then the reference for every sweep -- the driver's own operand orders applied to an independently
computed Phi.

The coefficients the tests choose (``coefficient``, ``make_app`` below), two per shape:
  mild:  a such that 4 theta dt (fx + fy) = 8, i.e. theta dt lambda <= 8 for every mode: every mode keeps at least 1 / 9 of its weight,
         so a wrong table entry or eigenvalue of ANY mode shows in the result;
  stiff: the suite's own cases.H2D_A = 3.5 (dt lambda_max of order 1e4 at 66x67: only the low modes survive the step).
Forward Euler: a such that 4 dt (fx + fy) = 0.9 (stable).
"""
import functools

import numpy as np
import scipy.sparse as sp
from scipy.sparse.linalg import splu

import cases
from pymgrit_amd.heat.heat_2d import Heat2D, VectorHeat2D

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
REFINEMENTS = 3


def _bits(x):
    return int(np.float64(x).view(np.int64))


@functools.lru_cache(maxsize=64)
def _factorisation(nx, ny, thdt_bits, fx_bits, fy_bits):
    """SuperLU of I + theta dt L_int in float64, unknowns in row-major order p = a mj + b of the (nx - 2) x (ny - 2) interior"""
    thdt, fx, fy = (float(np.int64(v).view(np.float64)) for v in (thdt_bits, fx_bits, fy_bits))
    mi, mj = nx - 2, ny - 2
    a, b = np.divmod(np.arange(mi * mj), mj)
    p = a * mj + b
    rows, cols, vals = [p], [p], [np.full(mi * mj, 1.0 + thdt * 2.0 * (fx + fy))]
    for da, db, f in ((1, 0, fx), (-1, 0, fx), (0, 1, fy), (0, -1, fy)):
        keep = (a + da >= 0) & (a + da < mi) & (b + db >= 0) & (b + db < mj)
        rows.append(p[keep])
        cols.append(((a + da) * mj + (b + db))[keep])
        vals.append(np.full(int(keep.sum()), -thdt * f))
    A = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(mi * mj, mi * mj))
    return splu(sp.csc_matrix(A))


def _stencil(z, fx, fy, sign):
    """interior of  2 (fx + fy) z + sign (fx (up + down) + fy (left + right))  for a full grid z: sign = -1 is L z, +1 is |L| z for z >= 0"""
    nb = fx * (z[:-2, 1:-1] + z[2:, 1:-1]) + fy * (z[1:-1, :-2] + z[1:-1, 2:])
    return LD(2) * (fx + fy) * z[1:-1, 1:-1] + (nb if sign > 0 else -nb)


def _apply(x, thdt, fx, fy):
    """(I + theta dt L_int) x in long double: x on the interior, zero values around it"""
    z = np.zeros((x.shape[0] + 2, x.shape[1] + 2), dtype=LD)
    z[1:-1, 1:-1] = x
    return x + thdt * _stencil(z, fx, fy, -1)


def _norm(a):
    return float(np.sqrt(np.sum(a * a)))


def _forcing(app, t):
    xi, yi = app.x_2d[1:-1], app.y_2d[:, 1:-1]
    f = np.asarray(app.rhs(x=xi, y=yi, t=t), dtype=np.float64) * np.ones((app.nx - 2, app.ny - 2))
    return f.astype(LD)


def right_hand_side(app, u, t_start, t_stop):
    """(b, babs) on the interior in long double; u: the full nx x ny grid"""
    u = np.asarray(u, dtype=np.float64).reshape(app.nx, app.ny).astype(LD)
    dt, th, fx, fy = LD(np.float64(t_stop) - np.float64(t_start)), LD(app.theta), LD(app.fx), LD(app.fy)
    b, babs = u[1:-1, 1:-1].copy(), np.abs(u[1:-1, 1:-1])
    if th != 1:
        b = b - (LD(1) - th) * dt * _stencil(u, fx, fy, -1)
        babs = babs + (LD(1) - th) * np.abs(dt) * _stencil(np.abs(u), fx, fy, +1)
        f = _forcing(app, t_start)
        b, babs = b + (LD(1) - th) * dt * f, babs + (LD(1) - th) * np.abs(dt) * np.abs(f)
    if th != 0:
        f = _forcing(app, t_stop)
        b, babs = b + th * dt * f, babs + th * np.abs(dt) * np.abs(f)
        bc = np.asarray(app.boundary_values(), dtype=np.float64).astype(LD)
        bc[1:-1, 1:-1] = 0
        for z, into in ((bc, "b"), (np.abs(bc), "babs")):
            w = fx * (z[:-2, 1:-1] + z[2:, 1:-1]) + fy * (z[1:-1, :-2] + z[1:-1, 2:])
            if into == "b":
                b = b + th * dt * w
            else:
                babs = babs + th * np.abs(dt) * w
    return b, babs


def babs_norm(app, u, t_start, t_stop):
    return _norm(right_hand_side(app, u, t_start, t_stop)[1])


def phi_bound(app, babs_f):
    """what one evaluation of Phi in float64 may be off the returned reference, in the Frobenius norm: the four products of the fast
    diagonalisation are fma chains of length mi, mj, mi, mj with orthogonal tables and a division by D >= 1 in between (2 mi + 2 mj), 8 for
    forming b and the tables' own rounding, 1 for the reference (residual and rounding to float64); forward Euler has no products"""
    chains = 2 * (app.nx - 2) + 2 * (app.ny - 2) if app.theta != 0 else 0
    return ((chains + 8) + 1) * EPS * babs_f


def reference_phi(app, u, t_start, t_stop):
    """Phi(u) for the step t_start -> t_stop as a float64 [nx][ny] array"""
    nx, ny = app.nx, app.ny
    u = np.asarray(u, dtype=np.float64).reshape(nx, ny)
    b, _ = right_hand_side(app, u, t_start, t_stop)
    out = np.array(app.boundary_values(), dtype=np.float64)
    if app.theta == 0:
        rim = (out.astype(LD) + u.astype(LD)).astype(np.float64)
        rim[1:-1, 1:-1] = b.astype(np.float64)
        return rim
    thdt64 = float(app.theta) * float(np.float64(t_stop) - np.float64(t_start))
    thdt, fx, fy = LD(app.theta) * LD(np.float64(t_stop) - np.float64(t_start)), LD(app.fx), LD(app.fy)
    lu = _factorisation(nx, ny, _bits(thdt64), _bits(app.fx), _bits(app.fy))
    shape = (nx - 2, ny - 2)
    x = lu.solve(b.astype(np.float64).ravel()).reshape(shape).astype(LD)
    for _ in range(REFINEMENTS):
        res = b - _apply(x, thdt, fx, fy)
        x = x + lu.solve(res.astype(np.float64).ravel()).reshape(shape).astype(LD)
    res_f, b_f = _norm(b - _apply(x, thdt, fx, fy)), _norm(b)
    assert res_f <= 0.5 * EPS * b_f, ("reference_phi: forward error bound", nx, ny, thdt64, res_f, b_f)
    out[1:-1, 1:-1] = x.astype(np.float64)
    return out


class ReferenceHeat2D(Heat2D):
    """Heat2D whose ``step`` is ``reference_phi``; no device description, so a hierarchy of these runs on the plugin path"""

    def step(self, u_start, t_start, t_stop):
        ret = VectorHeat2D(self.nx, self.ny)
        ret.set_values(reference_phi(self, u_start.get_values(), t_start, t_stop))
        return ret

    def device_stepper(self):
        return None


# ---- the applications of the tests (module docstring) ------------------------------------------------------------------------------
def coefficient(nx, ny, method, dt, which):
    """the diffusion coefficient a of the docstring for a step of size dt"""
    if which == "stiff":
        return cases.H2D_A
    per_a = 1.0 / (cases.H2D_X_END / (nx - 1)) ** 2 + 1.0 / (cases.H2D_Y_END / (ny - 1)) ** 2       # (fx + fy) / a
    if method == "FE":
        return 0.9 / (4.0 * dt * per_a)
    return 8.0 / (4.0 * {"BE": 1.0, "CN": 0.5}[method] * dt * per_a)


def make_app(nx, ny, t, method, a, forcing, with_bc, cls=None):
    if forcing == "general":
        assert with_bc
        return cases.h2d_general_app(nx, ny, t, method, a, cls=cls)
    return cases.h2d_app(nx, ny, t, method, with_bc, a, forcing=forcing == "separable", cls=cls)
