"""Host-side mirror of the reference's ``ClimateMachine.Mesh`` (``src/Numerics/Mesh``):
the data producers of the DG hot path.  Not a GPU workload (one-time, host)."""
from . import brickmesh, elements, filters, grids, interpolation, topologies
from .grids import DiscontinuousSpectralElementGrid
from .topologies import (BrickTopology, CubedShellTopology, StackedBrickTopology,
                         StackedCubedSphereTopology, equiangular_cubed_sphere_unwarp,
                         equiangular_cubed_sphere_warp)
from .interpolation import (InterpolationBrick, InterpolationCubedSphere,
                            accumulate_interpolated_data, dimensions,
                            interpolate_local, project_cubed_sphere)
# (``mesh.dss`` is the function, the reference's ``dss!``; the module's other names are re-exported here)
from .dss import DSS, CmdgDssDesc, dss, dss_apply, group_dss

__all__ = [
    "brickmesh", "elements", "filters", "grids", "interpolation", "topologies",
    "DiscontinuousSpectralElementGrid", "BrickTopology", "StackedBrickTopology",
    "CubedShellTopology", "StackedCubedSphereTopology",
    "equiangular_cubed_sphere_warp", "equiangular_cubed_sphere_unwarp",
    "InterpolationBrick", "InterpolationCubedSphere", "interpolate_local",
    "project_cubed_sphere", "accumulate_interpolated_data", "dimensions",
    "DSS", "dss", "dss_apply", "group_dss", "CmdgDssDesc",
]
