"""2-D complex Ginzburg-Landau equation with periodic boundary conditions: state vector and application.

    A_t = A + (1 + i b) Lap A - (1 + i c) |A|^2 A          on [0, L)^2 x (t_start, t_end],  periodic,  A = x + i y complex

the standard pattern-forming amplitude equation (spiral waves, phase turbulence; b = c = 0 is the real Ginzburg-Landau equation, whose
real solutions follow Allen-Cahn with nu = 2, eps = 1). The reference package has no such class. The problem is stated in numpy on the
``nx x nx`` grid ``x_i = i dx``, ``dx = L / nx``, axis 0 = x, axis 1 = y, in real form: a state is the two planes ``(x, y) = (Re A,
Im A)``. One time integrator:

``method='IMEX'``
    the growth and the cubic term explicit, diffusion and dispersion implicit. With ``q = x*x + y*y``::

        r = x + dt (x - q (x - c y)),    s = y + dt (y - q (c x + y))
        [ I - dt Lh     b dt Lh ] [x_new]   [r]
        [ -b dt Lh    I - dt Lh ] [y_new] = [s]

    Lh the periodic 5-point Laplacian / dx^2. Unlike every other periodic application of this package the implicit operator is not
    diagonal in the planes: the dispersion ``i b Lap`` couples them. The discrete Hartley basis ``T`` (allen_cahn.hartley_matrix)
    diagonalises Lh in each plane and leaves a 2 x 2 block per mode: with ``mu = lam_i + lam_j``, ``a = 1 + dt mu``,
    ``beta = (b dt) mu``, ``det = a a + beta beta``::

        Da = a / det,   Db = beta / det,   X = T r T,   Y = T s T
        x_new = T (X o Da + Y o Db) T,     y_new = T (Y o Da - X o Db) T

    exact up to rounding. ``Da^2 + Db^2 = 1 / det <= 1``: the modal solve contracts in the 2-norm; mode (0, 0) has Da = 1, Db = 0.
    ``device_stepper()`` describes the step (kind ``"ginzburglandau2d"``) and the engine applies it as four launches on the FP64 matrix
    cores, the second of which reads both spectra of a state and writes both (p2d_cross_kernel, csrc/mgrit_hip_ginzburglandau.inc,
    DESIGN.md 3.15). ``step`` is the same formula in numpy, in the operand order the kernels share (``_rhs_imex``, ``_dinv``, the join
    in ``_step_imex``: each table product rounded, then the sum or the difference): the plugin path and the specification of the device
    step.
"""
import numpy as np

from pymgrit_amd.allen_cahn.allen_cahn import hartley_matrix, periodic_laplacian_eigenvalues
from pymgrit_amd.core.application import Application
from pymgrit_amd.core.plane_vector import TwoPlaneVector


class VectorGinzburgLandau2D(TwoPlaneVector):
    """The complex amplitude of one time point as two planes: ``values[0]`` is Re A, ``values[1]`` is Im A, each an nx x nx grid; the
    norm is the 2-norm over all 2 nx^2 values (the 2-norm of A). A device state row is ``[Re A plane | Im A plane]``, which is
    ``values.ravel()``."""

    CLONE_COPIES = True


class GinzburgLandau2D(Application):
    """Complex Ginzburg-Landau in 2-D space with periodic boundary conditions, IMEX step (module docstring). ``init``: a callable
    ``(X, Y) -> complex array`` on the grid's coordinates (``X[i][j] = x_i``, ``Y[i][j] = y_j``); the default is a fixed smooth pattern
    of amplitude 0.1."""

    def __init__(self, nx=64, b=1.0, c=-1.2, L=32.0, init=None, method='IMEX', *args, **kwargs):
        super().__init__(*args, **kwargs)
        if method != 'IMEX':
            raise Exception(f"Unknown method {method!r}. GinzburgLandau2D offers IMEX (growth and cubic term explicit, diffusion and "
                            f"dispersion implicit)")
        try:
            finite = all(np.isfinite(float(v)) for v in (b, c, L))
        except (TypeError, ValueError):
            finite = False
        if not finite or not L > 0:
            raise Exception(f"GinzburgLandau2D: b and c must be finite, L positive and finite (b={b}, c={c}, L={L})")
        try:
            whole = int(nx) == nx
        except (TypeError, ValueError):
            whole = False
        if not whole or nx < 1:
            raise Exception(f"GinzburgLandau2D: nx={nx!r} must be a positive integer (the device path takes 4 <= nx <= 2048)")
        if init is not None and not callable(init):
            raise Exception("GinzburgLandau2D: init must be a callable (X, Y) -> complex array, or None")
        self.nx = int(nx)
        self.b, self.c, self.L = float(b), float(c), float(L)
        self.method = method
        self.init = init
        self.dx = self.L / self.nx
        self.x = self.dx * np.arange(self.nx)
        self._hartley = None
        self._lam = None
        self.vector_template = VectorGinzburgLandau2D(self.nx)
        self.vector_t_start = self.initial_guess()

    def _rhs_imex(self, x, y, dt):
        """(r, s). The operand order is fixed and is the device map's (GLPre, csrc/mgrit_hip_ginzburglandau.inc), no fma:
        q = x * x + y * y;  r = x + dt * (x - q * (x - c * y));  s = y + dt * (y - q * (c * x + y))"""
        q = x * x + y * y
        return x + dt * (x - q * (x - self.c * y)), y + dt * (y - q * (self.c * x + y))

    def _dinv(self, dt):
        """(Da, Db), the engine's [2][P][P] table for one bit pattern of dt (h2d_dinv, the same operand order): mu = lam_i + lam_j;
        a = 1 + dt * mu;  beta = (b * dt) * mu;  det = a * a + beta * beta;  Da = a / det;  Db = beta / det"""
        mu = self._lam[:, None] + self._lam[None, :]
        a = 1.0 + dt * mu
        beta = (self.b * dt) * mu
        det = a * a + beta * beta
        return a / det, beta / det

    def _step_imex(self, w, dt):
        if self._hartley is None:
            self._hartley = hartley_matrix(self.nx)
            self._lam = periodic_laplacian_eigenvalues(self.nx, self.dx)
        T = self._hartley
        Da, Db = self._dinv(dt)
        r, s = self._rhs_imex(w[0], w[1], dt)
        X, Y = (T @ r) @ T, (T @ s) @ T
        # each table product rounded, then the sum or the difference (p2d_cross_kernel)
        return np.stack((T @ (X * Da + Y * Db) @ T, T @ (Y * Da - X * Db) @ T))

    def step(self, u_start: VectorGinzburgLandau2D, t_start: float, t_stop: float) -> VectorGinzburgLandau2D:
        w = np.asarray(u_start.get_values(), dtype=np.float64)
        ret = VectorGinzburgLandau2D(self.nx)
        ret.set_values(self._step_imex(w, t_stop - t_start))
        return ret

    def device_stepper(self):
        """description of Phi for the HIP engine (mgrit_hip_level_ginzburglandau2d)"""
        return {"kind": "ginzburglandau2d", "n": 2 * self.nx ** 2, "nx": self.nx, "inv_dx2": 1.0 / self.dx ** 2, "b": self.b, "c": self.c}

    def initial_guess(self):
        """``init(X, Y)`` where given; otherwise A = 0.1 (cos(2 pi x / L) + i sin(2 pi (x + 2 y) / L)) + 0.05 cos(4 pi y / L): smooth,
        small, both planes non-trivial and not symmetric in (x, y), the same for every run"""
        initial = VectorGinzburgLandau2D(self.nx)
        X, Y = np.meshgrid(self.x, self.x, indexing="ij")
        if self.init is not None:
            A = np.asarray(self.init(X, Y), dtype=np.complex128)
            if A.shape != (self.nx, self.nx) or not np.all(np.isfinite(A)):
                raise Exception(f"GinzburgLandau2D: init must return finite complex values of shape ({self.nx}, {self.nx}), not {A.shape}")
        else:
            k = 2.0 * np.pi / self.L
            A = 0.1 * (np.cos(k * X) + 1j * np.sin(k * (X + 2.0 * Y))) + 0.05 * np.cos(2.0 * k * Y)
        initial.set_values(np.stack((np.ascontiguousarray(A.real), np.ascontiguousarray(A.imag))))
        return initial
