"""Spatial coarsening for Heat2D by a factor of two per axis on grids that include the boundary (fine nx = 2*coarse nx - 1,
fine ny = 2*coarse ny - 1): the rim by injection, the interior by 9-point full weighting, bilinear interpolation. The
reference ships no 2-D transfer class (its interface, core/grid_transfer.py:31-55, is open); the arithmetic, operand by
operand, is DESIGN.md 3.10. HIP kernels via ``device_transfer()`` (MGRIT_HIP_TRANSFER_HEAT2D)."""
import numpy as np

from pymgrit_amd.core.grid_transfer import GridTransfer
from pymgrit_amd.heat.heat_2d import VectorHeat2D

TRANSFER_HEAT2D = 4  # MGRIT_HIP_TRANSFER_HEAT2D


class GridTransferHeat2D(GridTransfer):
    def __init__(self):
        super().__init__()

    def restriction(self, u: VectorHeat2D) -> VectorHeat2D:
        f = np.asarray(u.get_values())
        if f.ndim != 2 or f.shape[0] % 2 == 0 or f.shape[1] % 2 == 0 or min(f.shape) < 5:
            raise Exception(f"GridTransferHeat2D restricts odd fine grids of at least 5 x 5 points (2*nc - 1 per axis), "
                            f"not {f.shape}")
        c = f[::2, ::2].copy()     # the rim by injection
        # ((((4 f[i][j] + 2 (((f[i-1][j] + f[i+1][j]) + f[i][j-1]) + f[i][j+1])) + f[i-1][j-1]) + f[i-1][j+1]) + f[i+1][j-1])
        # + f[i+1][j+1], over 16: numpy evaluates left to right
        c[1:-1, 1:-1] = (4 * f[2:-2:2, 2:-2:2] + 2 * (f[1:-3:2, 2:-2:2] + f[3:-1:2, 2:-2:2] + f[2:-2:2, 1:-3:2] + f[2:-2:2, 3:-1:2]) +
                         f[1:-3:2, 1:-3:2] + f[1:-3:2, 3:-1:2] + f[3:-1:2, 1:-3:2] + f[3:-1:2, 3:-1:2]) / 16
        out = VectorHeat2D(*c.shape)
        out.set_values(c)
        return out

    def interpolation(self, u: VectorHeat2D) -> VectorHeat2D:
        c = np.asarray(u.get_values())
        if c.ndim != 2 or min(c.shape) < 3:
            raise Exception(f"GridTransferHeat2D interpolates coarse grids of at least 3 x 3 points, not {c.shape}")
        f = np.zeros((2 * c.shape[0] - 1, 2 * c.shape[1] - 1))
        f[::2, ::2] = c
        f[1::2, ::2] = (c[:-1, :] + c[1:, :]) / 2
        f[::2, 1::2] = (c[:, :-1] + c[:, 1:]) / 2
        f[1::2, 1::2] = (c[:-1, :-1] + c[1:, :-1] + c[:-1, 1:] + c[1:, 1:]) / 4
        out = VectorHeat2D(*f.shape)
        out.set_values(f)
        return out

    def device_transfer(self) -> int:
        return TRANSFER_HEAT2D
