"""Spatial coarsening for the periodic Ginzburg-Landau grid by a factor of two per axis (fine nx = 2*coarse nx): the arithmetic of
GridTransferAllenCahn, operand by operand (9-point full weighting, bilinear interpolation, periodic wrap-around),
applied to the real and the imaginary plane of a state each on its own, returning VectorGinzburgLandau2D. HIP kernels via
``device_transfer()`` (MGRIT_HIP_TRANSFER_PERIODIC2D, which joins two Ginzburg-Landau levels as it joins two Allen-Cahn levels; the
kernels take the planes of a row). L, b and c are properties of the problem and stay fixed while dx doubles."""
from pymgrit_amd.allen_cahn.grid_transfer_allen_cahn import TRANSFER_PERIODIC2D, GridTransferAllenCahn
from pymgrit_amd.core.grid_transfer import GridTransfer
from pymgrit_amd.ginzburg_landau.ginzburg_landau import VectorGinzburgLandau2D
from pymgrit_amd.gray_scott.grid_transfer_gray_scott import per_plane


class GridTransferGinzburgLandau(GridTransfer):
    def __init__(self):
        super().__init__()
        self._periodic = GridTransferAllenCahn()

    def restriction(self, u: VectorGinzburgLandau2D) -> VectorGinzburgLandau2D:
        return per_plane(self._periodic.restriction, u, "GridTransferGinzburgLandau restricts", VectorGinzburgLandau2D, even=True)

    def interpolation(self, u: VectorGinzburgLandau2D) -> VectorGinzburgLandau2D:
        return per_plane(self._periodic.interpolation, u, "GridTransferGinzburgLandau interpolates", VectorGinzburgLandau2D)

    def device_transfer(self) -> int:
        return TRANSFER_PERIODIC2D
