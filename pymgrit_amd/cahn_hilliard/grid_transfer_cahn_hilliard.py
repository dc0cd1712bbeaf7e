"""Spatial coarsening for the periodic Cahn-Hilliard grid by a factor of two per axis (fine nx = 2*coarse nx): the arithmetic of
GridTransferAllenCahn, operand by operand (9-point full weighting, bilinear interpolation, periodic wrap-around),
returning VectorCahnHilliard2D. HIP kernels via ``device_transfer()`` (MGRIT_HIP_TRANSFER_PERIODIC2D, which joins two Cahn-Hilliard
levels as it joins two Allen-Cahn levels). eps is a property of the equation and stays fixed while dx doubles, so the coarse level
resolves the interface worse: such hierarchies converge, but slowly."""
from pymgrit_amd.cahn_hilliard.cahn_hilliard import VectorCahnHilliard2D
from pymgrit_amd.core.grid_transfer_periodic2d import PLANE, GridTransferPeriodic2D


class GridTransferCahnHilliard(GridTransferPeriodic2D):
    VECTOR, PLANES, NAME = VectorCahnHilliard2D, 1, PLANE
