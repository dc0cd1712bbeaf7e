"""2-D Gray-Scott reaction-diffusion system with periodic boundary conditions: state vector and application.

    u_t = du (u_xx + u_yy) - u v^2 + a (1 - u)
    v_t = dv (v_xx + v_yy) + u v^2 - b v            on [0, L)^2 x (t_start, t_end],  periodic,

the one *system* of PDEs the reference ships (reference src/pymgrit/petsc/gray_scott_2d_petsc.py:23-325), there on a PETSc DMDA.
This module is the same problem in numpy / scipy: same parameters ``du, dv, a, b, L``, same methods, same initial guess. What has no
counterpart here: the PETSc arguments ``dmda`` and ``comm_x`` (:28, the distributed grid and its communicator -- the grid is
``nx x nx`` points ``x_i = i dx``, ``dx = L / nx``, on one process) and the KSP / SNES tolerances ``lsol_tol``, ``lsol_maxiter``,
``nlsol_tol``, ``nlsol_maxiter`` (:28-29, :56-72): the IMEX solve below is exact, and Newton's method has ``newton_tol`` /
``newton_maxiter``. Three time integrators:

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
    backward Euler by Newton's method on the reference's ``formFunction`` with its ``formJacobian``, each correction a sparse direct
    solve of the ``2 nx^2 x 2 nx^2`` Jacobian. Host only: the Jacobian couples the species through ``+2 dt u v`` and ``-dt v^2`` and is
    not symmetric, so the Newton-PCG route of Allen-Cahn does not apply.

For ``EXPL`` and ``IMPL`` ``device_stepper()`` returns ``None`` and a hierarchy that holds such a level runs through ``step`` on the
plugin path like any host application.
"""
import numpy as np
import scipy.sparse as sp
from scipy.sparse.linalg import spsolve

from pymgrit_amd.allen_cahn.allen_cahn import hartley_matrix, periodic_laplacian_eigenvalues
from pymgrit_amd.core.application import Application
from pymgrit_amd.core.vector import Vector


class VectorGrayScott2D(Vector):
    """The two species of one time point: ``values[0]`` is u, ``values[1]`` is v, each an nx x nx grid; the norm is the 2-norm over
    all 2 nx^2 values. The reference interleaves the fields (``xa[i, j, field]``, a DMDA with dof = 2); here they are stored as two
    planes because the engine's tile products want a contiguous nx x nx operand per species -- a device state row is
    ``[u plane | v plane]``, which is ``values.ravel()``."""

    def __init__(self, nx):
        super().__init__()
        self.nx = nx
        self.values = np.zeros((2, nx, nx))

    def _like(self, values):
        out = VectorGrayScott2D(self.nx)
        out.set_values(values)
        return out

    def __add__(self, other):
        return self._like(self.get_values() + other.get_values())

    def __sub__(self, other):
        return self._like(self.get_values() - other.get_values())

    def __mul__(self, other):
        return self._like(self.get_values() * other)

    def norm(self):
        return np.linalg.norm(self.values)

    def clone(self):
        return self._like(self.get_values().copy())

    def clone_zero(self):
        return VectorGrayScott2D(self.nx)

    def clone_rand(self):
        return self._like(np.random.rand(2, self.nx, self.nx))

    def set_values(self, values):
        self.values = values

    def get_values(self):
        return self.values

    def pack(self):
        return self.values

    def unpack(self, values):
        self.values = values


class GrayScott(Application):
    """Gray-Scott in 2-D space with periodic boundary conditions (module docstring). ``method='IMEX'`` has a device form;
    ``'EXPL'`` and ``'IMPL'`` are host steppers and send their hierarchy to the plugin path."""

    def __init__(self, nx=64, du=1.0, dv=0.01, a=0.09, b=0.086, L=2.0, method='IMEX', newton_tol=1e-10, newton_maxiter=100,
                 *args, **kwargs):
        super().__init__(*args, **kwargs)
        if method not in ('IMPL', 'IMEX', 'EXPL'):
            raise Exception("Unknown method. Choose IMPL (implicit) or IMEX (implicit-explicit)")      # (reference :48)
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

    def step(self, u_start: VectorGrayScott2D, t_start: float, t_stop: float) -> VectorGrayScott2D:
        w = np.asarray(u_start.get_values(), dtype=np.float64)
        dt = t_stop - t_start
        ret = VectorGrayScott2D(self.nx)
        ret.set_values({'IMEX': self._step_imex, 'EXPL': self._step_expl, 'IMPL': self._step_impl}[self.method](w, dt))
        return ret

    def device_stepper(self):
        """description of Phi for the HIP engine (``method='IMEX'``); ``None`` for the host steppers: plugin path"""
        if self.method != 'IMEX':
            return None
        return {"kind": "grayscott2d", "n": 2 * self.nx ** 2, "nx": self.nx, "inv_dx2": 1.0 / self.dx ** 2, "du": self.du,
                "dv": self.dv, "a": self.a, "b": self.b}

    def initial_guess(self):
        """the reference's (:311-325): v = sin^2(4 pi x) sin^2(4 pi y) / 4 on 1 <= x, y <= 1.5 and 0 elsewhere, u = 1 - 2 v"""
        initial = VectorGrayScott2D(self.nx)
        x, y = self.x[:, None], self.x[None, :]
        inside = (x >= 1.0) & (x <= 1.5) & (y >= 1.0) & (y <= 1.5)
        v = np.where(inside, (np.sin(4 * np.pi * x) ** 2) * (np.sin(4 * np.pi * y) ** 2) / 4, 0.0)
        initial.set_values(np.stack((1 - 2 * v, v)))
        return initial
