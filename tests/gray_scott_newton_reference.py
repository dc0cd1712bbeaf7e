"""An independent Phi for the Gray-Scott backward-Euler step (method 'IMPL'): no Hartley table, no eigenvalues, none of the code of the
host steppers (``_step_impl``, ``_step_bicgstab``, ``_rate``, ``_jacobian``) or of the device kernels.

    rate(u, v) = (du L u - u v^2 + a (1 - u),  dv L v + u v^2 - b v),   L = periodic 5-point stencil / dx^2,  dx = Len / nx
    F(x) = x - dt rate(x) - w = 0                                        solved in np.longdouble from x = w

Newton's method on the long-double iterate: F is evaluated with ``np.roll`` in long double; the corrections come from a float64 SuperLU
factorisation of the Jacobian, which this module assembles from the stencil definition (rows and columns [u plane | v plane], row-major
within a plane):

    J = [[I - dt (du L - diag(v^2 + a)),  diag(2 dt u v)], [diag(-dt v^2),  I - dt (dv L + diag(2 u v - b))]].

A factorisation is kept (it only preconditions) while each correction cuts the residual to a quarter, and made anew where one did not. What the
function returns is pinned by its own long-double residual: the iteration ends, and the function asserts, that

    norm_2(F(x)) <= C_F EPS_LD M norm_2(x'),   x' = (x, w) stacked,

the rounding level of ONE evaluation of F in long double: M = 1 + dt (8 max(du, dv) / dx^2 + |a| + |b| + 3 R^2), R the largest |value| of
x and w, bounds the sum of the magnitudes of the terms of F per unit of |x'|; each value of F takes about 16 roundings of EPS_LD / 2 each
on quantities of that magnitude (the stencil 5, the reaction 6, the products with du / dv and dt and the two subtractions 5): C_F = 8.

Where the answer is unique. On a box |u| <= U, |v| <= V the symmetric part of the Jacobian is at least (1 - dt mu) I,
``mu(U, V) = max(|a| + U V, |b| + 3 U V + V^2 / 2)``: the diffusion blocks are symmetric positive semi-definite; the reaction Jacobian
[[-(v^2 + a), -2 u v], [v^2, 2 u v - b]] has the symmetric part [[-(v^2 + a), (v^2 - 2 u v) / 2], [., 2 u v - b]], whose Gershgorin rows are
-(v^2 + a) + |v^2 - 2 u v| / 2 <= -a - v^2 / 2 + |u v| <= |a| + U V and 2 u v - b + |v^2 - 2 u v| / 2 <= |b| + 3 U V + V^2 / 2. So for dt mu < 1 and
any two points of the box norm_2(x - y) <= norm_2(F(x) - F(y)) / (1 - dt mu): the forward error of the long-double iterate is at most its
residual / (1 - dt mu), and rounding to float64 adds at most EPS / 2 norm_2(x).

``ReferenceGrayScottNewton`` overrides ``step`` with this Phi, which sends a hierarchy to the plugin path. It records, since the last
``reset_record()``, the box of every input and result (``box``), the largest long-double residual norm of a returned float64 state
(``worst_residual``) and the largest norm_2 of a result (``worst_norm``): what the tolerances of the device tests are made of.

The tolerance of the tests (``tau``, ``e_g``, ``exit_criterion`` and the allowances below, shared by the CPU and the GPU tests) between
two states x, y that both claim to solve F = 0 for the same input, nothing of it measured on the code under test but
its own residual, which is evaluated here in long double by the reference's code:

    tau = (norm_2(F(x)) + norm_2(F(y))) / (1 - dt mu) + EPS norm_2(x),

mu from the largest |u|, |v| over both states and the input (the segment between them lies in that box). On its own this is an
inequality any two points of the box satisfy; what gives it teeth is the exit criterion asserted beside it: max|F(x)| < newton_tol +
E_g for the step's result, E_g the rounding of the step's own evaluation of g:

    E_g = C_G EPS S,   S = 2 R + dt (8 max(du, dv) R / dx^2 + R^3 + max(|a| (1 + R), |b| R)),   R the largest |value| of x and w,

S the sum of the magnitudes of the terms of one value of g. Operation count of gsn_residual_kernel per value of the u plane (the v
plane takes fewer), half an EPS each on a quantity of magnitude <= S: stencil 3 additions, the subtraction of 4 u and the scaling by
1 / dx^2 (5 roundings); v v, u (v v), 1 - u, a (1 - u) and their difference (5); the fma's with du and with dt and the subtraction of w
(3); 1 / dx^2 itself arrives rounded three times (L / nx, its square, the reciprocal), relative 1.5 EPS, where the reference forms it in
long double (3 more): C_G = 8. The numpy step does not fuse its three multiply-adds: C_G = 9.5 on the host.
"""
import numpy as np
import scipy.sparse as sp
from scipy.sparse.linalg import splu

import cases
from pymgrit_amd import GrayScott, VectorGrayScott2D

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
EPS_LD = float(np.finfo(LD).eps)
C_F = 8
MAX_ITERATIONS = 80
KEEP_FACTORISATION_BELOW = 0.25      # of the previous residual


def mu(a, b, U, V):
    """the bound of the module docstring on the largest eigenvalue of the symmetric part of the reaction Jacobian on |u| <= U, |v| <= V"""
    return max(abs(a) + U * V, abs(b) + 3.0 * U * V + 0.5 * V * V)


def _neighbours(nx):
    i, j = np.divmod(np.arange(nx * nx), nx)
    return i * nx + j, [((i + di) % nx) * nx + (j + dj) % nx for di, dj in ((1, 0), (-1, 0), (0, 1), (0, -1))]


def jacobian(x, dt, nx, par):
    """the Jacobian of the module docstring as a float64 CSC matrix"""
    du, dv, a, b, length = par
    n = nx * nx
    p, nbs = _neighbours(nx)
    u, v = np.asarray(x[0], dtype=np.float64).ravel(), np.asarray(x[1], dtype=np.float64).ravel()
    rows, cols, vals = [], [], []
    for c, d, diag in ((0, du, 1.0 + dt * (v * v + a)), (1, dv, 1.0 - dt * (2.0 * u * v - b))):
        r = dt * d * (nx / length) ** 2
        rows.append(c * n + p); cols.append(c * n + p); vals.append(diag + 4.0 * r)
        for q in nbs:
            rows.append(c * n + p); cols.append(c * n + q); vals.append(np.full(n, -r))
    rows.append(p); cols.append(n + p); vals.append(2.0 * dt * u * v)
    rows.append(n + p); cols.append(p); vals.append(-dt * v * v)
    A = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(2 * n, 2 * n))
    return sp.csc_matrix(A)


def _lap(p, nx, length):
    nb = np.roll(p, 1, axis=0) + np.roll(p, -1, axis=0) + np.roll(p, 1, axis=1) + np.roll(p, -1, axis=1)
    return (nb - LD(4) * p) * (LD(nx) / LD(length)) ** 2


def residual(x, w, dt, nx, par):
    """F(x) in long double as a [2][nx][nx] array for the input w (both 2 nx^2 values [u plane | v plane], any shape or float type);
    par = (du, dv, a, b, Len)"""
    du, dv, a, b, length = (LD(q) for q in par)
    x, w, dt = np.asarray(x, dtype=LD).reshape(2, nx, nx), np.asarray(w, dtype=LD).reshape(2, nx, nx), LD(dt)
    u, v = x[0], x[1]
    uv2 = u * v * v
    rate = np.stack((du * _lap(u, nx, par[4]) - uv2 + a * (LD(1) - u), dv * _lap(v, nx, par[4]) + uv2 - b * v))
    return x - dt * rate - w


def _norm(a):
    return float(np.sqrt(np.sum(a * a)))


def rounding_level(x, w, dt, nx, par):
    """C_F EPS_LD M norm_2((x, w)) of the module docstring"""
    du, dv, a, b, length = par
    R = float(max(np.abs(x).max(), np.abs(w).max()))
    M = 1.0 + dt * (8.0 * max(du, dv) * (nx / length) ** 2 + abs(a) + abs(b) + 3.0 * R * R)
    return C_F * EPS_LD * M * float(np.hypot(_norm(x), _norm(w)))


def reference_phi(w, dt, nx, par):
    """Phi(w) for one step of size dt as a float64 [2][nx][nx] array"""
    dt = float(dt)
    w = np.asarray(w, dtype=np.float64).reshape(2, nx, nx)
    x = w.astype(LD)
    lu, before = None, np.inf
    for it in range(MAX_ITERATIONS):
        res = residual(x, w, dt, nx, par)
        res_2 = _norm(res)
        if res_2 <= rounding_level(x, w, dt, nx, par):
            break
        if lu is None or res_2 > KEEP_FACTORISATION_BELOW * before:
            lu = splu(jacobian(x, dt, nx, par))
        before = res_2
        x = x - lu.solve(res.astype(np.float64).ravel()).reshape(2, nx, nx).astype(LD)
    res_2 = _norm(residual(x, w, dt, nx, par))
    assert res_2 <= rounding_level(x, w, dt, nx, par), ("reference_phi: residual of the long-double solve", nx, dt, res_2, rounding_level(x, w, dt, nx, par))
    return x.astype(np.float64)


class ReferenceGrayScottNewton(GrayScott):
    """GrayScott(method='IMPL') whose ``step`` is ``reference_phi``; overriding step selects the plugin path"""

    def __init__(self, *args, **kwargs):
        kwargs.setdefault("method", "IMPL")
        super().__init__(*args, **kwargs)
        assert self.method == "IMPL"
        self.par = (self.du, self.dv, self.a, self.b, self.L)
        self.reset_record()

    def reset_record(self):
        self.box, self.worst_residual, self.worst_norm = [0.0, 0.0], 0.0, 0.0

    def step(self, u_start, t_start, t_stop):
        w, dt = np.asarray(u_start.get_values(), dtype=np.float64), t_stop - t_start
        x = reference_phi(w, dt, self.nx, self.par)
        for c in range(2):
            self.box[c] = max(self.box[c], float(np.abs(x[c]).max()), float(np.abs(w[c]).max()))
        self.worst_residual = max(self.worst_residual, _norm(residual(x, w, dt, self.nx, self.par)))
        self.worst_norm = max(self.worst_norm, float(np.linalg.norm(x)))
        ret = VectorGrayScott2D(self.nx)
        ret.set_values(x)
        return ret


# ---- the allowances of the tests (module docstring) --------------------------------------------------------------------------------
C_G_DEVICE, C_G_HOST = 8.0, 9.5
PARS = {"du=100dv": dict(du=1.0, dv=0.01, a=0.09, b=0.086, L=2.0), "du=dv": dict(du=0.5, dv=0.5, a=0.04, b=0.1, L=2.0)}


def par_of(app):
    return (app.du, app.dv, app.a, app.b, app.L)


def norm2(a):
    return float(np.sqrt(np.sum(np.asarray(a, dtype=LD) ** 2)))


def margin(app, dt, *states):
    """1 - dt mu on the box of the states given ([2][nx][nx] each, or rows [u plane | v plane])"""
    U = max(float(np.abs(np.asarray(s).reshape(-1, 2, app.nx ** 2)[:, 0]).max()) for s in states)
    V = max(float(np.abs(np.asarray(s).reshape(-1, 2, app.nx ** 2)[:, 1]).max()) for s in states)
    m = 1.0 - dt * mu(app.a, app.b, U, V)
    assert m > 0.0, ("outside the regime where the step has one solution", dt, U, V)
    return m


def e_g(app, dt, R, c_g):
    """E_g of the module docstring: the rounding of one value of the step's own g"""
    S = 2.0 * R + dt * (8.0 * max(app.du, app.dv) * R / app.dx ** 2 + R ** 3 + max(abs(app.a) * (1.0 + R), abs(app.b) * R))
    return c_g * EPS * S


def tau(app, w, dt, x, y):
    """the tolerance of the module docstring between x and y for the input w"""
    fx, fy = (norm2(residual(s, w, dt, app.nx, par_of(app))) for s in (x, y))
    return (fx + fy) / margin(app, dt, x, y, w) + EPS * float(np.linalg.norm(x))


def exit_criterion(app, w, dt, x, c_g):
    """(max|F(x)| in long double, newton_tol + E_g)"""
    g = float(np.abs(residual(x, w, dt, app.nx, par_of(app))).max())
    return g, app.newton_tol + e_g(app, dt, float(max(np.abs(x).max(), np.abs(w).max())), c_g)


def history_allowance(ref_mg, rconv, norm_u, tau_phi):
    """|conv - reference conv| per iteration k (from 0): 1e-10 reference + 64 EPS norm(u), the project's rule for two exact steppers
    (tests/cases.py), + (k + 1) sqrt(points) tau_phi for two steppers that each stop at their own Newton test: a point's residual holds
    one Phi, which differs by at most tau_phi, and the deviation of the states it is formed from grows by at most as much per iteration
    where the iteration contracts (it converges: asserted by the callers)"""
    n_pts = len(ref_mg.t[0])
    return 1e-10 * rconv + cases.BLK_K * EPS * norm_u + (np.arange(len(rconv)) + 1.0) * np.sqrt(n_pts) * tau_phi


def tau_phi_a_priori(app, dt, ref_apps, c_g):
    """tau with the residuals replaced by what each side guarantees: the step under test max|g| < newton_tol + E_g on 2 nx^2 values,
    the reference its recorded long-double residual; the box from the reference's record, widened by 5 % (u) and 10 % (v)"""
    U, V = 1.05 * max(r.box[0] for r in ref_apps), 1.1 * max(r.box[1] for r in ref_apps)
    m = 1.0 - dt * mu(app.a, app.b, U, V)
    assert m > 0.0, (dt, U, V)
    res = np.sqrt(2.0) * app.nx * (app.newton_tol + e_g(app, dt, max(U, V), c_g)) + max(r.worst_residual for r in ref_apps)
    return res / m + EPS * max(r.worst_norm for r in ref_apps)
