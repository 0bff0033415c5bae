"""Grids, laws and fields shared by tests/test_esdg_linear_host.py and tests/test_gpu_esdg_imex.py: the
baroclinic-wave model of esdg_cases.case_c on taller stacks, a flat stacked brick, random fields and
the step size the reference takes."""
import numpy as np

from cmdg_loader import cm
from esdg_cases import ReferencePerturbation

M = cm.mesh
E = cm.esdg
A = cm.atmos

# the size of each state of a perturbation around the atmosphere's rest state
STATE_SCALE = np.array([1e-3, 1.0, 1.0, 1.0, 1e2])


def _model(orientation, problem, ps):
    return E.DryAtmosModel(orientation, problem,
                           ref_state=E.DryReferenceState(A.DecayingTemperatureProfile(ps, 290.0, 220.0, 8e3)),
                           sources=(E.Coriolis(), E.Gravity()), param_set=ps)


def sphere(N=3, nvert=4, nhorz=2, problem=None):
    """esdg_cases.case_c (2 x 2 per panel, spherical orientation, DryReferenceState, Coriolis + Gravity)
    with ``nvert`` levels to 30 km: at four the column probe has two units per probe group and an
    element with neighbours on both sides."""
    ps = A.PlanetParameters()
    Rrange = np.linspace(ps.planet_radius, ps.planet_radius + 30e3, nvert + 1)
    topl = M.StackedCubedSphereTopology(nhorz, Rrange, boundary=(1, 2))
    grid = M.DiscontinuousSpectralElementGrid(topl, N, meshwarp=E.cubedshellwarp)
    return _model(E.SphericalOrientation(), problem or ReferencePerturbation(), ps), grid


def brick(N=3, nvert=4):
    """2 x 2 x ``nvert`` stacked brick, 200 km x 200 km x 30 km (the step of cfl = 3 in the
    vertical stays explicit-stable in the horizontal), laterally periodic, walls (tags 1, 2) at
    the bottom and the top; flat orientation, the same reference state and sources."""
    ps = A.PlanetParameters()
    rng = [np.linspace(0.0, 200e3, 3), np.linspace(0.0, 200e3, 3), np.linspace(0.0, 30e3, nvert + 1)]
    topl = M.StackedBrickTopology(rng, periodicity=(True, True, False), boundary=((0, 0), (0, 0), (1, 2)))
    grid = M.DiscontinuousSpectralElementGrid(topl, N)
    return _model(E.FlatOrientation(), ReferencePerturbation(), ps), grid


CASES = {"sphere": sphere, "brick": brick}


def random_state(grid, seed, scale=STATE_SCALE):
    """Node-wise random (rho, rho u, rho e) of the size of a perturbation: discontinuous at every face,
    with momentum normal to the walls, so that the penalty and the reflection both act."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((grid.nelem, 5, grid.Np)) * scale[None, :, None]


def reference_dt(grid, ps, cfl=3):
    """``dt = cfl dx / soundspeed_air(330 K)`` with ``dx = min_node_distance(grid)``
    (baroclinic_wave.jl:273-279), from the host grid."""
    import esdg_linear_restatement as LR
    dx = float(LR.min_neighbor_distance(grid, LR.EVERY).min())
    return cfl * dx / np.sqrt(ps.cp_d / ps.cv_d * ps.R_d * 330.0)


def per_state_max_rel(a, b):
    """max|a_s - b_s| / max|b_s| of each of the five columns."""
    a, b = np.asarray(a), np.asarray(b)
    num = np.max(np.abs(a - b), axis=(0, 2))
    den = np.maximum(np.max(np.abs(b), axis=(0, 2)), np.finfo(np.float64).tiny)
    return np.asarray(num / den, dtype=np.float64)
