"""Spatial coarsening for the periodic Burgers grid by a factor of two per axis (fine nx = 2*coarse nx): the arithmetic of
GridTransferAllenCahn, operand by operand (9-point full weighting, bilinear interpolation, periodic wrap-around),
applied to each of the two velocity planes of a state on its own, returning VectorBurgers2D. HIP kernels via ``device_transfer()``
(MGRIT_HIP_TRANSFER_PERIODIC2D, which joins two Burgers levels as it joins two Allen-Cahn levels; the kernels take the planes of a
row). L and nu are properties of the problem and stay fixed while dx doubles."""
from pymgrit_amd.burgers.burgers import VectorBurgers2D
from pymgrit_amd.core.grid_transfer_periodic2d import GridTransferPeriodic2D


class GridTransferBurgers(GridTransferPeriodic2D):
    VECTOR, PLANES = VectorBurgers2D, 2
