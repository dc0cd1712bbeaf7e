"""2-D Gray-Scott reaction-diffusion system with periodic boundary conditions: state vector and application.

    u_t = du (u_xx + u_yy) - u v^2 + a (1 - u)
    v_t = dv (v_xx + v_yy) + u v^2 - b v            on [0, L)^2 x (t_start, t_end],  periodic,

the one *system* of PDEs the reference ships (reference src/pymgrit/petsc/gray_scott_2d_petsc.py:23-325), there on a PETSc DMDA.
This module is the same problem in numpy / scipy: same parameters ``du, dv, a, b, L``, same methods, same initial guess. What has no
counterpart here: the PETSc arguments ``dmda`` and ``comm_x`` (:28, the distributed grid and its communicator -- the grid is
``nx x nx`` points ``x_i = i dx``, ``dx = L / nx``, on one process) and the KSP / SNES tolerances ``lsol_tol``, ``lsol_maxiter``,
``nlsol_tol``, ``nlsol_maxiter`` (:28-29, :56-72): the IMEX solve below is exact, Newton's method has ``newton_tol`` /
``newton_maxiter`` and its Krylov form ``lin_tol`` / ``lin_maxiter`` (the reference's ``lsol_tol`` / ``lsol_maxiter`` defaults). Three
time integrators:

``method='IMEX'`` (reference :84-89, :198-216)
    the reaction explicit, the diffusion implicit, per species c = u, v::

        b_u = u + dt (a (1 - u) - u v^2),   b_v = v + dt (u v^2 - b v)
        (I - dt d_c Lap) x_c = b_c

    Lap the periodic 5-point Laplacian / dx^2. The reference solves with unpreconditioned CG to 1e-10; here the solve is the
    eigen-decomposition of Lap in the discrete Hartley basis ``T`` (allen_cahn.hartley_matrix), exact up to rounding:
    ``x_c = T ((T b_c T) o D_c) T``, ``D_c[i][j] = 1 / (1 + (dt d_c) (lam_i + lam_j))``. This is the method that runs on the MI355X:
    ``device_stepper()`` describes it (kind ``"grayscott2d"``) and the engine applies the four products for both species in one set of
    launches on the FP64 matrix cores (csrc/mgrit_hip_grayscott.inc). ``step`` is the same formula in numpy, in the
    operand order the kernel shares (``_rhs_imex``, ``_dinv``).
``method='EXPL'`` (reference :99-113)
    forward Euler. Host only.
``method='IMPL'`` (reference :90-97, :218-309)
    backward Euler by Newton's method on the reference's ``formFunction`` with its ``formJacobian``. The Jacobian couples the species
    through ``+2 dt u v`` and ``-dt v^2`` and is not symmetric, so the Newton-PCG route of Allen-Cahn does not apply.
    Two linear solvers:

    ``linear_solver='direct'`` (the default)
        each correction a sparse direct solve of the ``2 nx^2 x 2 nx^2`` Jacobian. Host only.
    ``linear_solver='bicgstab'``
        each correction by right-preconditioned BiCGStab, matrix-free (``_step_bicgstab`` states the algorithm, operand order
        included). This form runs on the MI355X: ``device_stepper()`` describes it (the IMEX keys plus ``theta``, the Newton and the
        BiCGStab parameters) and the engine runs batches of such steps with the ``gsn_*`` kernels; ``step`` is the
        same algorithm in numpy.

    Where the two agree. On a box ``|u| <= U``, ``|v| <= V`` the symmetric part of the Jacobian of F(x) = x - dt rate(x) - w is at
    least ``(1 - dt mu) I`` with ``mu(U, V) = max(|a| + U V, |b| + 3 U V + V^2 / 2)`` (Gershgorin on the symmetric part of the
    reaction Jacobian; the diffusion only adds). For ``dt mu < 1`` the step has one solution in the box and
    ``norm_2(x - y) <= norm_2(F(x) - F(y)) / (1 - dt mu)`` for any two points of it, so every correct solver returns the same state up
    to its residual. The box is a property of the data, not of the parameters: no step size is refused at construction. Outside
    ``dt mu < 1`` the non-linear system can have several roots and ``'bicgstab'`` may return another one than ``'direct'`` (nx = 4,
    dt = 2, a rough state in [0, 1] x [0, 0.5], dt mu about 3.4: both converge to a residual of 1e-13, at two points 1.29 apart).

For ``EXPL`` and for ``IMPL`` with the direct solver ``device_stepper()`` returns ``None`` and a hierarchy that holds such a level runs
through ``step`` on the plugin path like any host application.
"""
import numpy as np
import scipy.sparse as sp
from scipy.sparse.linalg import spsolve

from pymgrit_amd.allen_cahn.allen_cahn import hartley_matrix, periodic_laplacian_eigenvalues
from pymgrit_amd.core.application import Application
from pymgrit_amd.core.plane_vector import TwoPlaneVector


class VectorGrayScott2D(TwoPlaneVector):
    """The two species of one time point: ``values[0]`` is u, ``values[1]`` is v, each an nx x nx grid; the norm is the 2-norm over
    all 2 nx^2 values. The reference interleaves the fields (``xa[i, j, field]``, a DMDA with dof = 2); here they are stored as two
    planes because the engine's tile products want a contiguous nx x nx operand per species -- a device state row is
    ``[u plane | v plane]``, which is ``values.ravel()``."""

    CLONE_COPIES = True


class GrayScott(Application):
    """Gray-Scott in 2-D space with periodic boundary conditions (module docstring). ``method='IMEX'`` and ``method='IMPL'`` with
    ``linear_solver='bicgstab'`` have a device form; ``'EXPL'`` and ``'IMPL'`` with the default ``linear_solver='direct'`` are host
    steppers and send their hierarchy to the plugin path. ``lin_tol`` / ``lin_maxiter``: the relative residual and the iteration cap
    of one BiCGStab solve (the reference's ``lsol_tol`` / ``lsol_maxiter``). Outside ``dt mu < 1`` (module docstring) the answer of
    ``'bicgstab'`` may differ from ``'direct'``'s: the non-linear system can have several roots there."""

    def __init__(self, nx=64, du=1.0, dv=0.01, a=0.09, b=0.086, L=2.0, method='IMEX', newton_tol=1e-10, newton_maxiter=100,
                 *args, linear_solver='direct', lin_tol=1e-10, lin_maxiter=100, **kwargs):
        super().__init__(*args, **kwargs)
        if method not in ('IMPL', 'IMEX', 'EXPL'):
            raise Exception("Unknown method. Choose IMPL (implicit) or IMEX (implicit-explicit)")      # (reference :48)
        if linear_solver not in ('direct', 'bicgstab'):
            raise Exception(f"Unknown linear_solver {linear_solver!r}. Choose 'direct' (sparse LU) or 'bicgstab' (matrix-free)")
        if linear_solver == 'bicgstab' and method != 'IMPL':
            raise Exception(f"linear_solver='bicgstab' is the inner solver of method='IMPL'; method={method!r} solves no such system")
        if int(nx) != nx or nx < 1:
            raise Exception(f"nx={nx!r} must be a positive integer")
        if not (np.isfinite(du) and np.isfinite(dv) and du > 0 and dv > 0):
            raise Exception(f"the diffusion coefficients must be positive and finite (du={du}, dv={dv})")
        if not (np.isfinite(a) and np.isfinite(b)):
            raise Exception(f"the reaction parameters must be finite (a={a}, b={b})")
        if not (np.isfinite(L) and L > 0):
            raise Exception(f"the domain length must be positive and finite (L={L})")
        self.nx = int(nx)
        self.du, self.dv, self.a, self.b, self.L = float(du), float(dv), float(a), float(b), float(L)
        self.method = method
        self.newton_tol = newton_tol
        self.newton_maxiter = newton_maxiter
        self.linear_solver, self.lin_tol, self.lin_maxiter = linear_solver, lin_tol, lin_maxiter
        self.dx = self.L / self.nx
        self.x = self.dx * np.arange(self.nx)
        self._hartley = None
        self._lam = None
        self._lap_matrix = None
        self.vector_template = VectorGrayScott2D(self.nx)
        self.vector_t_start = self.initial_guess()

    # -- IMEX --------------------------------------------------------------------------------------------------------------------
    def _rhs_imex(self, u, v, dt):
        """(b_u, b_v). The operand order is fixed and is the device kernel's (GSPre, csrc/mgrit_hip_grayscott.inc), which fuses the
        last multiplication and addition of each line into one fma: uv2 = u * (v * v); b_u = fma(dt, a * (1 - u) - uv2, u);
        b_v = fma(dt, uv2 - b * v, v)"""
        uv2 = u * (v * v)
        return dt * (self.a * (1.0 - u) - uv2) + u, dt * (uv2 - self.b * v) + v

    def _dinv(self, dt, d):
        """D_c = 1 / (1 + (dt d_c) (lam_i + lam_j)), the engine's table for one bit pattern of dt (h2d_dinv, the same operand order)"""
        return 1.0 / (1.0 + (dt * d) * (self._lam[:, None] + self._lam[None, :]))

    def _step_imex(self, w, dt):
        if self._hartley is None:
            self._hartley = hartley_matrix(self.nx)
            self._lam = periodic_laplacian_eigenvalues(self.nx, self.dx)
        T = self._hartley
        out = np.empty((2, self.nx, self.nx))
        for c, (b, d) in enumerate(zip(self._rhs_imex(w[0], w[1], dt), (self.du, self.dv))):
            out[c] = T @ (((T @ b) @ T) * self._dinv(dt, d)) @ T
        return out

    # -- EXPL, IMPL (host only) ----------------------------------------------------------------------------------------------------
    def _lap(self, p):
        """periodic 5-point Laplacian / dx^2 of one nx x nx plane"""
        s = ((np.roll(p, 1, 0) + np.roll(p, -1, 0)) + (np.roll(p, 1, 1) + np.roll(p, -1, 1))) - 4.0 * p
        return s * (1.0 / self.dx ** 2)

    def _rate(self, w):
        """the right-hand side of the system: (du Lap u - u v^2 + a (1 - u), dv Lap v + u v^2 - b v), reference :106-109, :236-240"""
        u, v = w[0], w[1]
        uv2 = u * v ** 2
        return np.stack((self.du * self._lap(u) - uv2 + self.a * (1.0 - u), self.dv * self._lap(v) + uv2 - self.b * v))

    def _step_expl(self, w, dt):
        return w + dt * self._rate(w)

    def newton_residual(self, x, old, dt):
        """the reference's formFunction (:218-240) minus the right-hand side SNES solves it against: x - dt rate(x) - old"""
        return x - dt * self._rate(x) - old

    def _jacobian(self, x, dt):
        """the reference's formJacobian (:242-309) in plane order: rows / columns [u plane | v plane], row-major within a plane"""
        if self._lap_matrix is None:
            n = self.nx
            one = np.ones(n)
            lap = sp.diags([-2.0 * one, one[:-1], one[:-1], [1.0], [1.0]], [0, 1, -1, n - 1, 1 - n], shape=(n, n), format='csc')
            self._lap_matrix = sp.csc_matrix((sp.kron(lap, sp.eye(n)) + sp.kron(sp.eye(n), lap)) * (1.0 / self.dx ** 2))
        lap, eye = self._lap_matrix, sp.eye(self.nx ** 2)
        u, v = x[0].ravel(), x[1].ravel()
        j_uu = eye - dt * (self.du * lap - sp.diags(v ** 2 + self.a))
        j_uv = sp.diags(dt * 2.0 * u * v)
        j_vu = sp.diags(-dt * v ** 2)
        j_vv = eye - dt * (self.dv * lap + sp.diags(2.0 * u * v - self.b))
        return sp.csc_matrix(sp.bmat([[j_uu, j_uv], [j_vu, j_vv]]))

    def _step_impl(self, w, dt):
        x = w.copy()
        for _ in range(int(self.newton_maxiter)):
            g = self.newton_residual(x, w, dt)
            if np.max(np.abs(g)) < self.newton_tol:
                break
            x = x - spsolve(self._jacobian(x, dt), g.ravel()).reshape(x.shape)
        return x

    # -- IMPL with linear_solver='bicgstab': the specification the device kernels share (gsn_*, csrc/mgrit_hip_grayscott.inc) -------
    def _lap_dev(self, p, inv_dx2):
        """the stencil in the kernel's operand order: ((up + down) + (left + right) - 4 p) * (1 / dx^2), 1 / dx^2 formed once"""
        return (((np.roll(p, 1, 0) + np.roll(p, -1, 0)) + (np.roll(p, 1, 1) + np.roll(p, -1, 1))) - 4.0 * p) * inv_dx2

    def _residual_bicgstab(self, x, w, dt, inv_dx2):
        """g = F(x) = x - dt rate(x) - w. Operand order (the kernel fuses each ``c * y + z`` written below into one fma):
        uv2 = u * (v * v);  rate_u = du * lap(u) + (a * (1 - u) - uv2);  rate_v = dv * lap(v) + (uv2 - b * v);
        g_c = (-dt * rate_c + x_c) - w_c"""
        u, v = x[0], x[1]
        uv2 = u * (v * v)
        rate_u = self.du * self._lap_dev(u, inv_dx2) + (self.a * (1.0 - u) - uv2)
        rate_v = self.dv * self._lap_dev(v, inv_dx2) + (uv2 - self.b * v)
        return np.stack(((-dt * rate_u + u) - w[0], (-dt * rate_v + v) - w[1]))

    def _jac_apply(self, x, p, dt, inv_dx2):
        """J(x) p, the reference's formJacobian (``_jacobian``) matrix-free. Operand order (fma's as above):
        v2 = v * v;  c = 2 * (u * v);
        t_u = du * lap(p_u) - ((v2 + a) * p_u + c * p_v);   t_v = dv * lap(p_v) + (v2 * p_u + (c - b) * p_v);
        (J p)_c = -dt * t_c + p_c"""
        u, v = x[0], x[1]
        v2, c = v * v, 2.0 * (u * v)
        t_u = self.du * self._lap_dev(p[0], inv_dx2) - ((v2 + self.a) * p[0] + c * p[1])
        t_v = self.dv * self._lap_dev(p[1], inv_dx2) + (v2 * p[0] + (c - self.b) * p[1])
        return np.stack((-dt * t_u + p[0], -dt * t_v + p[1]))

    def _precondition(self, p, dt):
        """P^-1 p, P = blockdiag((1 + dt a) I - dt du Lap, (1 + dt b) I - dt dv Lap) -- J at the fixed point (u, v) = (1, 0), where
        the coupling blocks vanish --: per species the four Hartley products with the table 1 / ((1 + dt s_c) + (dt d_c) (lam_i + lam_j)),
        s_u = a, s_v = b (the engine's p2d_fill_dinv, the same operand order)"""
        T, lam = self._hartley, self._lam[:, None] + self._lam[None, :]
        out = np.empty_like(p)
        for c, (s, d) in enumerate(((self.a, self.du), (self.b, self.dv))):
            out[c] = T @ (((T @ p[c]) @ T) * (1.0 / ((1.0 + dt * s) + (dt * d) * lam))) @ T
        return out

    def _bicgstab(self, x, g, dt, inv_dx2):
        """(delta, iterations): right-preconditioned BiCGStab on J(x) delta = g from delta = 0 with the shadow residual r^ = g, so the
        first rho = g . g. Per iteration, with stop = lin_tol norm_2(g):
            p = r (first) or r + beta (p - omega v);   y = P^-1 p;   v = J y;   sigma = r^ . v;   alpha = rho / sigma
            s = r - alpha v;   norm_2(s) <= stop: delta += alpha y, end
            z = P^-1 s;   t = J z;   omega = (t . s) / (t . t)
            delta += alpha y + omega z;   r = s - omega t;   norm_2(r) <= stop or lin_maxiter iterations: end
            rho' = r^ . r;   beta = (rho' / rho) (alpha / omega);   rho = rho'
        Breakdowns end the solve with the delta accumulated so far (the spirit of CG stopping on p . J p <= 0): rho or sigma zero or
        not finite before alpha exists -- nothing added --; t . t = 0, omega = 0 or not finite -- delta += alpha y, the half step,
        whose residual s is known --. An iteration counts once it has added to delta."""
        stop = self.lin_tol * np.sqrt(np.sum(g * g))
        rhat, r, delta = g, g.copy(), np.zeros_like(g)
        rho = float(np.sum(g * g))
        p = v = None
        alpha = omega = beta = 0.0
        k = 0
        while k < int(self.lin_maxiter) and rho != 0.0 and np.isfinite(rho):
            p = r.copy() if k == 0 else r + beta * (p - omega * v)
            y = self._precondition(p, dt)
            v = self._jac_apply(x, y, dt, inv_dx2)
            sigma = float(np.sum(rhat * v))
            if sigma == 0.0 or not np.isfinite(sigma) or not np.isfinite(rho / sigma):
                break
            alpha = rho / sigma
            s = r - alpha * v
            k += 1
            if np.sqrt(np.sum(s * s)) <= stop:
                delta = delta + alpha * y
                break
            z = self._precondition(s, dt)
            t = self._jac_apply(x, z, dt, inv_dx2)
            ts, tt = float(np.sum(t * s)), float(np.sum(t * t))
            omega = ts / tt if tt != 0.0 else 0.0
            if tt == 0.0 or omega == 0.0 or not np.isfinite(omega):
                delta = delta + alpha * y
                break
            delta = delta + (alpha * y + omega * z)
            r = s - omega * t
            if np.sqrt(np.sum(r * r)) <= stop:
                break
            rho_next = float(np.sum(rhat * r))
            beta = (rho_next / rho) * (alpha / omega)
            rho = rho_next
            if not np.isfinite(beta):
                break
        return delta, k

    def _step_bicgstab(self, w, dt, counts=None):
        """Newton's method from x = w: g = F(x); max|g| < newton_tol ends it (the test comes before the solve, as in ``_step_impl``);
        otherwise x <- x - delta with delta from ``_bicgstab``. At most newton_maxiter corrections; an item that reaches the cap
        returns its last iterate. counts: a dict that receives 'newton_iterations' and 'cg_iterations' (the tests read it)"""
        if self._hartley is None:
            self._hartley = hartley_matrix(self.nx)
            self._lam = periodic_laplacian_eigenvalues(self.nx, self.dx)
        inv_dx2 = 1.0 / self.dx ** 2
        x = w.copy()
        n_newton = n_lin = 0
        for _ in range(int(self.newton_maxiter)):
            g = self._residual_bicgstab(x, w, dt, inv_dx2)
            if np.max(np.abs(g)) < self.newton_tol:
                break
            delta, k = self._bicgstab(x, g, dt, inv_dx2)
            n_newton, n_lin = n_newton + 1, n_lin + k
            if k:
                x = x - delta
        if counts is not None:
            counts.update(newton_iterations=n_newton, cg_iterations=n_lin)
        return x

    def step(self, u_start: VectorGrayScott2D, t_start: float, t_stop: float) -> VectorGrayScott2D:
        w = np.asarray(u_start.get_values(), dtype=np.float64)
        dt = t_stop - t_start
        impl = self._step_bicgstab if self.linear_solver == 'bicgstab' else self._step_impl
        ret = VectorGrayScott2D(self.nx)
        ret.set_values({'IMEX': self._step_imex, 'EXPL': self._step_expl, 'IMPL': impl}[self.method](w, dt))
        return ret

    def device_stepper(self):
        """description of Phi for the HIP engine: ``method='IMEX'``, or -- with theta and the solver's parameters beside the same keys
        -- ``method='IMPL'`` with ``linear_solver='bicgstab'``; ``None`` for the host steppers: plugin path"""
        d = {"kind": "grayscott2d", "n": 2 * self.nx ** 2, "nx": self.nx, "inv_dx2": 1.0 / self.dx ** 2, "du": self.du,
             "dv": self.dv, "a": self.a, "b": self.b}
        if self.method == 'IMEX':
            return d
        if self.method == 'IMPL' and self.linear_solver == 'bicgstab':
            return {**d, "theta": 1.0, "newton_tol": self.newton_tol, "newton_maxiter": self.newton_maxiter, "lin_tol": self.lin_tol,
                    "lin_maxiter": self.lin_maxiter}
        return None

    def initial_guess(self):
        """the reference's (:311-325): v = sin^2(4 pi x) sin^2(4 pi y) / 4 on 1 <= x, y <= 1.5 and 0 elsewhere, u = 1 - 2 v"""
        initial = VectorGrayScott2D(self.nx)
        x, y = self.x[:, None], self.x[None, :]
        inside = (x >= 1.0) & (x <= 1.5) & (y >= 1.0) & (y <= 1.5)
        v = np.where(inside, (np.sin(4 * np.pi * x) ** 2) * (np.sin(4 * np.pi * y) ** 2) / 4, 0.0)
        initial.set_values(np.stack((1 - 2 * v, v)))
        return initial
