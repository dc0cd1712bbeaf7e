"""2-D Cahn-Hilliard equation with periodic boundary conditions: state vector and application.

    u_t = Lap(u^3 - u - eps^2 Lap u)   on [0, L)^2 x (t_start, t_end],
    u(x, y, 0) = mean + amplitude (cos(4 pi x / L) cos(2 pi y / L) + 0.5 sin(2 pi x / L) sin(6 pi y / L)).

The mass-conserving sibling of Allen-Cahn (no reference class: the reference ships Allen-Cahn only). Fourth-order stiff, so the one
method is the linearly stabilised IMEX step (an Eyre-type splitting with stabilisation ``s = stab >= 0``) on the ``nx x nx`` grid
``x_i = i dx``, ``dx = L / nx``, with ``Lh`` the periodic 5-point Laplacian / dx^2 of ``AllenCahn.compute_matrix``:

    (I + dt (eps^2 Lh^2 - s Lh)) u+ = u + dt Lh w,     w = u^3 - (1 + s) u   (pointwise)

In the discrete Hartley basis ``T`` of ``allen_cahn.hartley_matrix`` (symmetric, orthogonal, ``T T = I``), with
``lam_k = (4 / dx^2) sin^2(pi k / nx)`` the eigenvalues of ``-Lh`` and ``mu_ab = lam_a + lam_b``:

    u+ = T ((T u T) o D1 + (T w T) o D2) T,     D1 = 1 / (1 + dt (eps^2 mu^2 + s mu)),     D2 = -(dt mu) D1

Mode (0, 0) has ``D1 = 1`` and ``D2 = 0``: the mean of u is conserved. ``device_stepper()`` describes the step (kind
``"cahnhilliard2d"``) and the engine applies it as six batched item-products per state on the FP64 matrix cores
(csrc/mgrit_hip_cahnhilliard.inc); ``step`` is the same formula in numpy, in the kernels' operand order: the plugin
path and the specification of the device step.
"""
import numpy as np

from pymgrit_amd.allen_cahn.allen_cahn import hartley_matrix, periodic_laplacian_eigenvalues
from pymgrit_amd.core.application import Application
from pymgrit_amd.core.plane_vector import OnePlaneVector


class VectorCahnHilliard2D(OnePlaneVector):
    """nx x ny grid values of one time point; the norm is the 2-norm over all of them"""


class CahnHilliard(Application):
    """Cahn-Hilliard in 2-D space with periodic boundary conditions, linearly stabilised IMEX step (module docstring)"""

    def __init__(self, nx=64, eps=0.05, stab=2.0, L=1.0, mean=0.0, amplitude=0.1, method='IMEX', *args, **kwargs):
        super().__init__(*args, **kwargs)
        if method != 'IMEX':
            raise Exception("Unknown method. CahnHilliard offers IMEX (linearly stabilised implicit-explicit) only")
        try:
            finite = all(np.isfinite(float(v)) for v in (eps, stab, L, mean, amplitude))
        except (TypeError, ValueError):
            finite = False
        if not finite:
            raise Exception(f"CahnHilliard: eps, stab, L, mean and amplitude must be finite numbers "
                            f"(eps={eps}, stab={stab}, L={L}, mean={mean}, amplitude={amplitude})")
        if int(nx) != nx or nx < 4:
            raise Exception(f"CahnHilliard: nx={nx} must be an integer >= 4")
        if not eps > 0:
            raise Exception(f"CahnHilliard: eps={eps} must be positive")
        if stab < 0:
            raise Exception(f"CahnHilliard: stab={stab} must not be negative")
        if not L > 0:
            raise Exception(f"CahnHilliard: L={L} must be positive")
        self.nx = int(nx)
        self.ny = self.nx
        self.eps = float(eps)
        self.stab = float(stab)
        self.L = float(L)
        self.mean = float(mean)
        self.amplitude = float(amplitude)
        self.method = method
        self.dx = self.L / self.nx
        self.x = np.arange(self.nx) * self.dx
        self._hartley = None
        self._mu = None
        self.vector_t_start = self.initial_guess()
        self.vector_template = VectorCahnHilliard2D(self.nx, self.ny)

    def _w(self, u):
        """w = u^3 - (1 + s) u, the device kernel's operand order (CHPre): (u * u) * u - c1 * u with c1 = 1 + s"""
        c1 = 1.0 + self.stab
        return (u * u) * u - c1 * u

    def _tables(self, dt):
        """(D1, D2), the operand order of the engine's tables (h2d_dinv)"""
        mu = self._mu
        d1 = 1.0 / (1.0 + dt * (self.eps ** 2 * mu * mu + self.stab * mu))
        return d1, -(dt * mu) * d1

    def _step_imex(self, u, dt):
        if self._hartley is None:
            self._hartley = hartley_matrix(self.nx)
            lam = periodic_laplacian_eigenvalues(self.nx, self.dx)
            self._mu = lam[:, None] + lam[None, :]
        T = self._hartley
        d1, d2 = self._tables(dt)
        return T @ (((T @ u) @ T) * d1 + ((T @ self._w(u)) @ T) * d2) @ T

    def step(self, u_start: VectorCahnHilliard2D, t_start: float, t_stop: float) -> VectorCahnHilliard2D:
        u = np.asarray(u_start.get_values(), dtype=np.float64)
        ret = VectorCahnHilliard2D(self.nx, self.ny)
        ret.set_values(self._step_imex(u, t_stop - t_start))
        return ret

    def device_stepper(self):
        """description of Phi for the HIP engine (mgrit_hip_level_cahnhilliard2d)"""
        return {"kind": "cahnhilliard2d", "n": self.nx * self.nx, "nx": self.nx, "inv_dx2": 1.0 / self.dx ** 2,
                "eps2": self.eps ** 2, "stab": self.stab}

    def initial_guess(self):
        initial = VectorCahnHilliard2D(self.nx, self.ny)
        X, Y = self.x[:, None] / self.L, self.x[None, :] / self.L
        initial.set_values(self.mean + self.amplitude * (np.cos(4 * np.pi * X) * np.cos(2 * np.pi * Y) +
                                                         0.5 * np.sin(2 * np.pi * X) * np.sin(6 * np.pi * Y)))
        return initial
