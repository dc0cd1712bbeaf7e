"""Spatial coarsening for the periodic Gray-Scott grid by a factor of two per axis (fine nx = 2*coarse nx): the arithmetic of
GridTransferAllenCahn, operand by operand (9-point full weighting, bilinear interpolation, periodic wrap-around),
applied to each of the two planes of a state on its own -- plane c of the result is the transfer of plane c of the argument and of
nothing else --, returning VectorGrayScott2D. HIP kernels via ``device_transfer()`` (MGRIT_HIP_TRANSFER_PERIODIC2D, which joins two
Gray-Scott levels as it joins two Allen-Cahn levels; the kernels take the planes of a row). L, du, dv, a and b are properties of the
problem and stay fixed while dx doubles."""
from pymgrit_amd.core.grid_transfer_periodic2d import GridTransferPeriodic2D
from pymgrit_amd.gray_scott.gray_scott import VectorGrayScott2D


class GridTransferGrayScott(GridTransferPeriodic2D):
    VECTOR, PLANES = VectorGrayScott2D, 2
