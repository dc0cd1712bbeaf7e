"""2-D Allen-Cahn equation with periodic boundary conditions: state vector and application.

    u_t = u_xx + u_yy + (1 / eps^2) u (1 - u^nu)   on [-0.5, 0.5]^2 x (t_start, t_end],
    u(x, 0) = tanh((radius - |x|) / (sqrt(2) eps)).

Drop-in for ``pymgrit.allen_cahn.allen_cahn`` (reference src/pymgrit/allen_cahn/allen_cahn.py:16-260): same constructor,
attributes and helpers. Three time integrators:

``method='IMEX'``
    ``Phi(u) = (I - dt L)^-1 (u + dt/eps^2 u (1 - u^nu))``, L the periodic 5-point Laplacian / dx^2. The reference factorises
    ``I - dt L`` with SuperLU on every step; here the solve is the eigen-decomposition of L in the discrete Hartley basis
    ``T[i][k] = (cos(2 pi i k / n) + sin(2 pi i k / n)) / sqrt(n)`` (symmetric, orthogonal, ``T T = I``):
    ``Phi = T ((T b T) / (1 + dt (lam_i + lam_j))) T`` with ``lam_k = (4 / dx^2) sin^2(pi k / n)``. This is the method that
    runs on the MI355X: ``device_stepper()`` describes it (kind ``"allencahn2d"``) and the engine applies the four products on the
    FP64 matrix cores (csrc/mgrit_hip_allencahn.inc). ``step`` is the same formula in numpy (plugin path).
``method='IMPL'`` and ``method='CN'``
    Newton's method on ``x - fac (L x + r(x) / eps^2) = rhs``, ``fac = theta dt`` (theta = 1 / 0.5). The Newton Jacobian
    ``J = I - fac (L + diag((1 - (nu + 1) x^nu) / eps^2))`` changes with the iterate and is not diagonal in any fixed basis, so
    there is no table that inverts it. Two linear solvers:

    ``linear_solver='direct'`` (default, the reference's behaviour)
        a sparse direct solve (SuperLU) per Newton iteration, on the host only: ``device_stepper()`` returns ``None`` and a
        hierarchy that holds such a level runs through ``step`` on the plugin path like any host application.
    ``linear_solver='pcg'``
        conjugate gradients on the symmetric J, preconditioned by ``P = (1 + fac nu / eps^2) I - fac L`` -- J away from the
        interface, where ``|u| = 1`` --, which the Hartley tables invert exactly like the IMEX solve. ``lin_tol`` and
        ``lin_maxiter`` bound the inner iteration. This form has a device description (``theta``, ``newton_tol``, ...) and runs on
        the MI355X as batched Newton-PCG steps; ``step`` states the same algorithm in numpy. Offered only where
        the implicit system is uniquely solvable and J positive definite for every iterate: even ``nu`` and
        ``theta max(dt) / eps^2 < 1`` (L is negative semi-definite and ``1 - (nu + 1) x^nu <= 1``, so ``J >= (1 - fac / eps^2) I``);
        anything else is refused at construction.
"""
import numpy as np
import scipy.sparse as sp
from scipy.sparse.linalg import spsolve

from pymgrit_amd.core.application import Application
from pymgrit_amd.core.plane_vector import OnePlaneVector


class VectorAllenCahn2D(OnePlaneVector):
    """nx x ny grid values of one time point; the norm is the 2-norm over all of them"""


def hartley_matrix(n):
    """T[i][k] = (cos(2 pi i k / n) + sin(2 pi i k / n)) / sqrt(n); the angle is reduced exactly, (i k) mod n"""
    r = np.outer(np.arange(n, dtype=np.int64), np.arange(n, dtype=np.int64)) % n
    a = 2.0 * np.pi * r / n
    return (np.cos(a) + np.sin(a)) / np.sqrt(n)


def periodic_laplacian_eigenvalues(n, dx):
    """eigenvalues of -(periodic [1 -2 1] / dx^2), mode k of the Hartley (or Fourier) basis"""
    return (4.0 / dx ** 2) * np.sin(np.pi * np.arange(n) / n) ** 2


class AllenCahn(Application):
    """Allen-Cahn in 2-D space with periodic boundary conditions (module docstring). ``method='IMEX'`` has a device form, and so
    have ``'IMPL'`` and ``'CN'`` with ``linear_solver='pcg'``; with ``'direct'`` they are host-side Newton solves and send their
    hierarchy to the plugin path."""

    def __init__(self, nx=128, nu=2, eps=0.04, newton_maxiter=100, newton_tol=1e-12, lin_tol=1e-12, lin_maxiter=100,
                 radius=0.25, method='IMPL', linear_solver='direct', *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.nu = nu
        self.eps = eps
        self.newton_maxiter = newton_maxiter
        self.newton_tol = newton_tol
        self.lin_tol = lin_tol
        self.lin_maxiter = lin_maxiter
        self.radius = radius
        self.nx = nx
        self.ny = nx
        self.method = method
        if method not in ('IMPL', 'IMEX', 'CN'):
            raise Exception("Unknown method. Choose IMPL (implicit), IMEX (implicit-explicit) or CN (Crank-Nicolson")
        if linear_solver not in ('direct', 'pcg'):
            raise Exception("Unknown linear_solver. Choose direct (sparse LU per Newton iteration) or pcg (preconditioned "
                            "conjugate gradients)")
        self.linear_solver = linear_solver
        self.theta = 0.5 if method == 'CN' else 1.0
        if linear_solver == 'pcg':
            self._check_pcg()
        self.dx = 1.0 / self.nx
        self.space_disc = self.compute_matrix()
        self.id = sp.eye(self.nx * self.ny)
        self.x = np.linspace(start=-0.5, stop=0.5, num=self.nx)   # (nx points INCLUDING both ends, although dx = 1 / nx: as the reference)
        self._hartley = None
        self._lam = None
        self.vector_t_start = self.initial_guess()
        self.vector_template = VectorAllenCahn2D(nx=self.nx, ny=self.ny)

    def compute_matrix(self):
        """periodic 5-point Laplacian / dx^2 on the row-major nx x ny grid (sparse, csc)"""
        n = self.nx
        one = np.ones(n)
        lap = sp.diags([-2.0 * one, one[:-1], one[:-1], [1.0], [1.0]], [0, 1, -1, n - 1, 1 - n], shape=(n, n), format='csc')
        out = sp.kron(lap, sp.eye(n)) + sp.kron(sp.eye(n), lap)
        return sp.csc_matrix(out * (1.0 / self.dx ** 2))

    def _reaction(self, u):
        """u (1 - u^nu), u^nu by nu - 1 multiplications p = p * u (the device kernel's order)"""
        p = u.copy()
        for _ in range(1, int(self.nu)):
            p = p * u
        return u * (1.0 - p)

    def _step_imex(self, u, dt):
        if self._hartley is None:
            self._hartley = hartley_matrix(self.nx)
            self._lam = periodic_laplacian_eigenvalues(self.nx, self.dx)
        T = self._hartley
        c = dt * (1.0 / self.eps ** 2)
        b = c * self._reaction(u) + u
        dinv = 1.0 / (1.0 + dt * (self._lam[:, None] + self._lam[None, :]))
        return T @ (((T @ b) @ T) * dinv) @ T

    def _step_newton(self, u, dt):
        old = u.ravel()
        new = old.copy()
        inv_eps2 = 1.0 / self.eps ** 2
        if self.method == 'CN':
            fac = dt / 2
            rhs = old + fac * (self.space_disc.dot(old) + inv_eps2 * self._reaction(old))
        else:
            fac = dt
            rhs = old
        for _ in range(int(self.newton_maxiter)):
            g = new - fac * (self.space_disc.dot(new) + inv_eps2 * self._reaction(new)) - rhs
            if np.linalg.norm(g, np.inf) < self.newton_tol:
                break
            jac = self.id - fac * (self.space_disc + inv_eps2 * sp.diags(1.0 - (self.nu + 1) * new ** self.nu, offsets=0))
            new = new - spsolve(sp.csc_matrix(jac), g)
        return new.reshape(self.nx, self.ny)

    def _check_pcg(self):
        """linear_solver='pcg' is offered where J is positive definite for every iterate (module docstring), refused elsewhere"""
        if self.method == 'IMEX':
            raise Exception("linear_solver='pcg' belongs to the Newton methods IMPL and CN; method='IMEX' has no Newton iteration")
        if int(self.nu) != self.nu or int(self.nu) < 2 or int(self.nu) % 2 != 0:
            raise Exception(f"linear_solver='pcg' requires an even nu (nu={self.nu}): for odd nu the Jacobian's diagonal term "
                            "1 - (nu + 1) u^nu is unbounded above for negative u")
        fac_max = self.theta * float(np.max(np.diff(self.t))) if len(self.t) > 1 else 0.0
        if not fac_max / self.eps ** 2 < 1.0:
            raise Exception(f"linear_solver='pcg' requires theta * dt / eps^2 < 1 on every step, i.e. dt < "
                            f"{self.eps ** 2 / self.theta:.6g} for method={self.method!r}, eps={self.eps}; the largest step of this "
                            f"time grid is {fac_max / self.theta:.6g}")

    def _hartley_tables(self):
        if self._hartley is None:
            self._hartley = hartley_matrix(self.nx)
            self._lam = periodic_laplacian_eigenvalues(self.nx, self.dx)
        return self._hartley, self._lam

    def _lap(self, v):
        """periodic 5-point Laplacian of the nx x nx grid v, the device kernels' order"""
        s = ((np.roll(v, 1, 0) + np.roll(v, -1, 0)) + (np.roll(v, 1, 1) + np.roll(v, -1, 1))) - 4.0 * v
        return s * (1.0 / self.dx ** 2)

    def _step_pcg(self, u, dt):
        """Newton with preconditioned conjugate gradients (the specification the device step shares)"""
        T, lam = self._hartley_tables()
        inv_eps2 = 1.0 / self.eps ** 2
        fac = self.theta * dt
        nu = int(self.nu)
        dinv = 1.0 / ((1.0 + fac * nu * inv_eps2) + fac * (lam[:, None] + lam[None, :]))
        rhs = u + fac * (self._lap(u) + inv_eps2 * self._reaction(u)) if self.method == 'CN' else u
        x = u.copy()
        for _ in range(int(self.newton_maxiter)):
            g = (x - fac * (self._lap(x) + inv_eps2 * self._reaction(x))) - rhs
            if np.max(np.abs(g)) < self.newton_tol:
                break
            pw = x.copy()
            for _q in range(1, nu):
                pw = pw * x
            d = (1.0 - (nu + 1) * pw) * inv_eps2
            delta, r, p, rz = np.zeros_like(x), g.copy(), None, 0.0
            stop = self.lin_tol * np.sqrt(np.sum(g * g))
            for _k in range(int(self.lin_maxiter)):
                z = T @ (((T @ r) @ T) * dinv) @ T
                rz_new = float(np.sum(r * z))
                p = z if p is None else z + (rz_new / rz) * p
                rz = rz_new
                jp = p - fac * (self._lap(p) + d * p)
                pjp = float(np.sum(p * jp))
                if not pjp > 0.0:
                    break
                alpha = rz / pjp
                delta = delta + alpha * p
                r = r - alpha * jp
                rr = float(np.sum(r * r))
                if rr == 0.0 or np.sqrt(rr) <= stop:
                    break
            x = x - delta
        return x

    def step(self, u_start: VectorAllenCahn2D, t_start: float, t_stop: float) -> VectorAllenCahn2D:
        u = np.asarray(u_start.get_values(), dtype=np.float64)
        dt = t_stop - t_start
        ret = VectorAllenCahn2D(self.nx, self.ny)
        if self.method == 'IMEX':
            out = self._step_imex(u, dt)
        else:
            out = self._step_pcg(u, dt) if self.linear_solver == 'pcg' else self._step_newton(u, dt)
        ret.set_values(out)
        return ret

    def device_stepper(self):
        """description of Phi for the HIP engine: ``method='IMEX'``, and the Newton methods with ``linear_solver='pcg'`` (extended by
        ``theta`` and the solver's parameters); ``None`` otherwise: plugin path"""
        if self.method != 'IMEX' and self.linear_solver != 'pcg':
            return None
        d = {"kind": "allencahn2d", "n": self.nx * self.ny, "nx": self.nx, "inv_dx2": 1.0 / self.dx ** 2,
             "inv_eps2": 1.0 / self.eps ** 2, "nu": int(self.nu)}
        if self.method != 'IMEX':
            d.update(theta=self.theta, newton_tol=float(self.newton_tol), newton_maxiter=int(self.newton_maxiter),
                     lin_tol=float(self.lin_tol), lin_maxiter=int(self.lin_maxiter))
        return d

    def initial_guess(self):
        initial = VectorAllenCahn2D(nx=self.nx, ny=self.ny)
        r = np.sqrt(self.x[:, None] ** 2 + self.x[None, :] ** 2)
        initial.set_values(np.tanh((self.radius - r) / (np.sqrt(2) * self.eps)))
        return initial

    def exact_radius(self, t):
        return np.sqrt(max(self.radius ** 2 - 2.0 * t, 0))

    def compute_radius(self, u):
        return np.sqrt(np.count_nonzero(u.get_values() >= 0.0) / np.pi) * self.dx
