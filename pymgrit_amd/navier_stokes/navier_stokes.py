"""2-D incompressible Navier-Stokes equations in vorticity form with periodic boundary conditions: state vector and application.

    w_t + u w_x + v w_y = nu Lap w + f,     Lap psi = -w,     u = psi_y,  v = -psi_x          on [0, L)^2 x (t_start, t_end],  periodic.

A state is ONE plane, the vorticity w, on the ``nx x nx`` grid ``x_i = i dx``, ``dx = L / nx``, axis 0 = x, axis 1 = y; the velocity is
never stored: every step recovers the stream function psi from w. The reference ships no such application (as it ships no
Cahn-Hilliard): its non-linear time-dependent PDEs are Allen-Cahn, Gray-Scott and Burgers. One time integrator:

``method='IMEX'``
    the transport explicit with central differences of psi and w, the diffusion implicit. With ``T`` the discrete Hartley matrix
    (allen_cahn.hartley_matrix), ``lam`` the eigenvalues of the periodic 5-point Laplacian / dx^2 (periodic_laplacian_eigenvalues),
    ``mu = lam_i + lam_j`` and ``inv_2dx = 1 / (2 dx)`` (indices mod nx)::

        psi = T ((T w T) o S) T                 S = 1 / mu, S[0][0] = 0      (Lh psi = -(w - mean w); the mean never reaches psi)
        px = (psi[i+1][j] - psi[i-1][j]) * inv_2dx      py = (psi[i][j+1] - psi[i][j-1]) * inv_2dx
        wx, wy: the same differences of w
        jac = fma(py, wx, -(px * wy))           (u = psi_y, v = -psi_x: u w_x + v w_y)
        b   = fma(-dt, jac, w);   with a forcing:  b = fma(dt, f, b)
        x   = T ((T b T) o D) T                 D = 1 / (1 + (dt nu) mu)     (the operand order of Burgers2D._dinv)

    ``device_stepper()`` describes the step (kind ``"navierstokes2d"``) and the engine applies it as nine launches per batch: four
    one-plane Hartley products for psi, a stencil pass that forms b from one staged tile of psi and of w, four more products for x
    (csrc/mgrit_hip_navierstokes.inc). ``step`` is the same formula in numpy, in the operand order the kernel shares
    (``_rhs_imex``, ``_sinv``, ``_dinv``): the plugin path and the specification of the device step.

The forcing ``f`` does not depend on time (a Kolmogorov forcing ``f = -k cos(k y)`` is the use case). It is the first stepper here with
an elliptic solve inside its explicit right-hand side.
"""
import numpy as np

from pymgrit_amd.allen_cahn.allen_cahn import hartley_matrix, periodic_laplacian_eigenvalues
from pymgrit_amd.core.application import Application
from pymgrit_amd.core.plane_vector import OnePlaneVector


class VectorNavierStokes2D(OnePlaneVector):
    """the vorticity of one time point on the nx x ny grid; the norm is the 2-norm over all values"""

    CLONE_COPIES = True


class NavierStokes2D(Application):
    """Incompressible Navier-Stokes in 2-D space, vorticity form, periodic boundary conditions, IMEX step (module docstring)"""

    def __init__(self, nx=32, nu=1e-2, L=2 * np.pi, forcing=None, method='IMEX', *args, **kwargs):
        super().__init__(*args, **kwargs)
        if method != 'IMEX':
            raise Exception(f"Unknown method {method!r}. NavierStokes2D offers IMEX (transport explicit, diffusion implicit)")
        try:
            finite = all(np.isfinite(float(v)) for v in (nu, L))
        except (TypeError, ValueError):
            finite = False
        if not finite or not nu > 0 or not L > 0:
            raise Exception(f"NavierStokes2D: nu and L must be positive and finite (nu={nu}, L={L})")
        if int(nx) != nx or nx < 4:
            raise Exception(f"NavierStokes2D: nx={nx!r} must be an integer >= 4")
        self.nx = int(nx)
        self.ny = self.nx
        self.nu, self.L = float(nu), float(L)
        self.method = method
        self.dx = self.L / self.nx
        self.inv_2dx = 1.0 / (2.0 * self.dx)
        self.x = self.dx * np.arange(self.nx)
        if forcing is not None:
            try:
                if callable(forcing):      # evaluated once on the grid; a function of one coordinate only broadcasts
                    f = np.broadcast_to(np.asarray(forcing(self.x[:, None], self.x[None, :]), dtype=np.float64), (self.nx, self.nx))
                else:
                    f = np.asarray(forcing, dtype=np.float64)
            except (TypeError, ValueError):
                f = None
            if f is None or f.shape != (self.nx, self.nx) or not np.all(np.isfinite(f)):
                raise Exception(f"NavierStokes2D: forcing must be None, a finite ({self.nx}, {self.nx}) array or a callable f(x, y) "
                                f"that gives one")
            forcing = np.array(f, dtype=np.float64, order="C")      # (a copy: the caller's array may change later)
        self.forcing = forcing
        self._hartley = None
        self._lam = None
        self.vector_template = VectorNavierStokes2D(self.nx, self.ny)
        self.vector_t_start = self.initial_guess()

    def _tables(self):
        if self._hartley is None:
            self._hartley = hartley_matrix(self.nx)
            self._lam = periodic_laplacian_eigenvalues(self.nx, self.dx)
        return self._hartley

    def _sinv(self):
        """S = 1 / (lam_i + lam_j), S[0][0] = 0: the engine's table of the level (ns_sinv)"""
        mu = self._lam[:, None] + self._lam[None, :]
        mu[0, 0] = 1.0
        s = 1.0 / mu
        s[0, 0] = 0.0
        return s

    def _dinv(self, dt):
        """D = 1 / (1 + (dt nu) (lam_i + lam_j)), the engine's table for one bit pattern of dt (h2d_dinv; the operand order of
        Burgers2D._dinv)"""
        return 1.0 / (1.0 + (dt * self.nu) * (self._lam[:, None] + self._lam[None, :]))

    def stream_function(self, w):
        """psi with Lh psi = -(w - mean w) and mean 0: T ((T w T) o S) T"""
        T = self._tables()
        return T @ (((T @ w) @ T) * self._sinv()) @ T

    def _rhs_imex(self, w, psi, dt):
        """b. The operand order is fixed and is the device kernel's (ns_rhs_kernel, csrc/mgrit_hip_navierstokes.inc), which fuses the
        multiply-adds numpy rounds separately:  px = (psi[i+1][j] - psi[i-1][j]) * inv_2dx;  py = (psi[i][j+1] - psi[i][j-1]) * inv_2dx;
        wx, wy the same of w;  jac = fma(py, wx, -(px * wy));  b = fma(-dt, jac, w);  with a forcing b = fma(dt, f, b)"""
        px = (np.roll(psi, -1, 0) - np.roll(psi, 1, 0)) * self.inv_2dx
        py = (np.roll(psi, -1, 1) - np.roll(psi, 1, 1)) * self.inv_2dx
        wx = (np.roll(w, -1, 0) - np.roll(w, 1, 0)) * self.inv_2dx
        wy = (np.roll(w, -1, 1) - np.roll(w, 1, 1)) * self.inv_2dx
        b = -dt * (py * wx + -(px * wy)) + w
        if self.forcing is not None:
            b = dt * self.forcing + b
        return b

    def _step_imex(self, w, dt):
        T = self._tables()
        b = self._rhs_imex(w, self.stream_function(w), dt)
        return T @ (((T @ b) @ T) * self._dinv(dt)) @ T

    def step(self, u_start: VectorNavierStokes2D, t_start: float, t_stop: float) -> VectorNavierStokes2D:
        w = np.asarray(u_start.get_values(), dtype=np.float64)
        ret = VectorNavierStokes2D(self.nx, self.ny)
        ret.set_values(self._step_imex(w, t_stop - t_start))
        return ret

    def device_stepper(self):
        """description of Phi for the HIP engine (mgrit_hip_level_navierstokes2d)"""
        return {"kind": "navierstokes2d", "n": self.nx * self.nx, "nx": self.nx, "inv_dx2": 1.0 / self.dx ** 2, "inv_2dx": self.inv_2dx,
                "nu": self.nu, "forcing": self.forcing}

    def initial_guess(self):
        """w = cos(X) cos(Y) + 0.5 sin(2 X) cos(Y) + 0.25 sin(X + 2 Y), X = 2 pi x / L: two wavenumber shells mixed (|k|^2 = 2 and 5),
        so the Jacobian is non-zero from the first step -- a single shell is a steady Euler flow, J(psi, w) = 0"""
        initial = VectorNavierStokes2D(self.nx, self.ny)
        X, Y = 2 * np.pi * self.x[:, None] / self.L, 2 * np.pi * self.x[None, :] / self.L
        initial.set_values(np.cos(X) * np.cos(Y) + 0.5 * np.sin(2 * X) * np.cos(Y) + 0.25 * np.sin(X + 2 * Y))
        return initial
