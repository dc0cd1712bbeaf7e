"""pymgrit_amd -- MI355X-native MGRIT relaxation engine behind PyMGRIT's plugin API.

Same public names as the reference package for everything on the hot path (``Mgrit``, ``AtMgrit``, ``Application``, ``Vector``,
``GridTransfer``, ``GridTransferCopy``, ``simple_setup_problem``, ``Dahlquist``, ``Heat1D``, ``Heat1DBDF1``, ``Heat1DBDF2``,
``Heat2D``, ``Advection1D``, ``AllenCahn``), the Gray-Scott system of the reference's PETSc examples in numpy with its IMEX step on the
device (``GrayScott``), the 2-D Burgers equation of its Firedrake examples in numpy with its IMEX step on the device (``Burgers2D``), the Cahn-Hilliard equation with its stabilised IMEX step on the device (``CahnHilliard``), the incompressible Navier-Stokes equations in vorticity form with their IMEX step on the device (``NavierStokes2D``), the complex Ginzburg-Landau equation with its coupled-plane IMEX step on the device (``GinzburgLandau2D``), plus the spatial-coarsening transfers that run as HIP kernels (``GridTransferHeat``,
``GridTransferAdvection``, ``GridTransferHeat2D``, ``GridTransferAllenCahn``, ``GridTransferCahnHilliard``, ``GridTransferNavierStokes``, and for the states of two planes ``GridTransferGrayScott``, ``GridTransferBurgers``, ``GridTransferGinzburgLandau``).
"""
from pymgrit_amd.core.application import Application
from pymgrit_amd.core.vector import Vector
from pymgrit_amd.core.grid_transfer import GridTransfer
from pymgrit_amd.core.grid_transfer_copy import GridTransferCopy
from pymgrit_amd.core.simple_setup_problem import simple_setup_problem
from pymgrit_amd.core.mgrit import Mgrit
from pymgrit_amd.core.at_mgrit import AtMgrit

from pymgrit_amd.dahlquist.dahlquist import Dahlquist
from pymgrit_amd.heat.heat_1d import Heat1D
from pymgrit_amd.heat.heat_1d_2pts_bdf1 import Heat1DBDF1
from pymgrit_amd.heat.heat_1d_2pts_bdf2 import Heat1DBDF2
from pymgrit_amd.heat.heat_2d import Heat2D
from pymgrit_amd.heat.vector_heat_1d_2pts import VectorHeat1D2Pts
from pymgrit_amd.heat.grid_transfer_heat import GridTransferHeat
from pymgrit_amd.heat.grid_transfer_heat_2d import GridTransferHeat2D
from pymgrit_amd.allen_cahn.allen_cahn import AllenCahn, VectorAllenCahn2D
from pymgrit_amd.allen_cahn.grid_transfer_allen_cahn import GridTransferAllenCahn
from pymgrit_amd.gray_scott.gray_scott import GrayScott, VectorGrayScott2D
from pymgrit_amd.gray_scott.grid_transfer_gray_scott import GridTransferGrayScott
from pymgrit_amd.cahn_hilliard.cahn_hilliard import CahnHilliard, VectorCahnHilliard2D
from pymgrit_amd.cahn_hilliard.grid_transfer_cahn_hilliard import GridTransferCahnHilliard
from pymgrit_amd.burgers.burgers import Burgers2D, VectorBurgers2D
from pymgrit_amd.burgers.grid_transfer_burgers import GridTransferBurgers
from pymgrit_amd.navier_stokes.navier_stokes import NavierStokes2D, VectorNavierStokes2D
from pymgrit_amd.navier_stokes.grid_transfer_navier_stokes import GridTransferNavierStokes
from pymgrit_amd.ginzburg_landau.ginzburg_landau import GinzburgLandau2D, VectorGinzburgLandau2D
from pymgrit_amd.ginzburg_landau.grid_transfer_ginzburg_landau import GridTransferGinzburgLandau
from pymgrit_amd.advection.advection_1d import Advection1D
from pymgrit_amd.advection.grid_transfer_advection import GridTransferAdvection



def elementwise(f):
    """Declare a forcing time factor tau(t) elementwise: called with an array of times it returns, entry by entry, exactly what
    it returns for each time alone (no dependence on position, length, other entries or earlier calls). The device path then
    evaluates it once per level instead of once per time point (core/backend_hip._time_factor)."""
    f.elementwise = True
    return f


__all__ = ["elementwise", "Application", "Vector", "GridTransfer", "GridTransferCopy", "simple_setup_problem", "Mgrit", "AtMgrit", "Dahlquist",
           "Heat1D", "Heat1DBDF1", "Heat1DBDF2", "Heat2D", "GridTransferHeat", "Advection1D", "GridTransferAdvection", "AllenCahn", "VectorAllenCahn2D", "VectorHeat1D2Pts",
           "GridTransferHeat2D", "GridTransferAllenCahn", "GrayScott", "VectorGrayScott2D",
           "CahnHilliard", "VectorCahnHilliard2D", "GridTransferCahnHilliard", "VectorBurgers2D", "Burgers2D",
           "NavierStokes2D", "VectorNavierStokes2D", "GridTransferNavierStokes", "GridTransferGrayScott", "GridTransferBurgers",
           "GinzburgLandau2D", "VectorGinzburgLandau2D", "GridTransferGinzburgLandau"]
