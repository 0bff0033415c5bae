"""The two set-ups of the reference's interpolation test (test/Numerics/Mesh/interpolation.jl)
and the fields the interpolation tests put on them.  Shared by tests/test_interpolation_host.py
and tests/test_gpu_interpolation.py."""
import numpy as np

from cmdg_loader import cm

M = cm.mesh
I = cm.mesh.interpolation
_x1, _x2, _x3 = 12, 13, 14          # vgeo columns of the node coordinates (grids.py)

PLANET_RADIUS = cm.atmos.PlanetParameters().planet_radius
BRICK_MAX = (2000.0, 400.0, 2000.0)
BRICK_TOL = 1e-9                    # interpolation.jl:432 and :435 (Float64, N = 5 and (5, 6))
SPHERE_TOL = 2e-7                   # interpolation.jl:441 and :444


def brick_case(N, rank=0, size=1, ne=(20, 4, 20), spacing=10.0):
    """run_brick_interpolation_test (interpolation.jl:90-231): [0,2000] x [0,400] x [0,2000],
    Ne = (20, 4, 20), periodic in x and y, 10 m output spacing."""
    rng = [np.linspace(0.0, BRICK_MAX[d], ne[d] + 1) for d in range(3)]
    topl = M.StackedBrickTopology(rng, periodicity=(True, True, False), rank=rank, size=size)
    grid = M.DiscontinuousSpectralElementGrid(topl, N)
    xbnd = np.array([[0.0, 0.0, 0.0], list(BRICK_MAX)])
    xg = [np.arange(int(round(BRICK_MAX[d] / spacing)) + 1) * spacing for d in range(3)]
    return grid, I.InterpolationBrick(grid, xbnd, *xg)


def sphere_case(N, rank=0, size=1, nhor=6, nvert=4, res=1.0, nrad=21):
    """run_cubed_sphere_interpolation_test (interpolation.jl:237-423): nhor = 6, 4 levels over
    30 km, 1 x 1 degree x 21 radii."""
    a = PLANET_RADIUS
    vert_range = np.linspace(a, a + 30e3, nvert + 1)
    topl = M.StackedCubedSphereTopology(nhor, vert_range, rank=rank, size=size)
    grid = M.DiscontinuousSpectralElementGrid(topl, N, meshwarp=M.equiangular_cubed_sphere_warp)
    lat = -90.0 + res * np.arange(int(round(180.0 / res)) + 1)
    lon = -180.0 + res * np.arange(int(round(360.0 / res)) + 1)
    rad = vert_range[0] + ((vert_range[-1] - vert_range[0]) / (nrad - 1)) * np.arange(nrad)
    return grid, I.InterpolationCubedSphere(grid, vert_range, nhor, lat, lon, rad)


def node_coordinates(grid):
    """(nelem, Np) arrays x1, x2, x3."""
    return grid.vgeo[:, _x1, :], grid.vgeo[:, _x2, :], grid.vgeo[:, _x3, :]


def fcn(x, y, z):
    return np.sin(x) * np.cos(y) * np.cos(z)        # interpolation.jl:37


def reference_state(grid, scale, nstate):
    """``Q.data .= sin.(x1 ./ xmax) .* cos.(x2 ./ ymax) .* cos.(x3 ./ zmax)`` in every state."""
    x1, x2, x3 = node_coordinates(grid)
    f = fcn(x1 / scale[0], x2 / scale[1], x3 / scale[2])
    return np.ascontiguousarray(np.repeat(f[:, None, :], nstate, axis=1))


def brick_expected(intrp, nstate):
    """fex of interpolation.jl:206-212 as (nstate, n3, n2, n1)."""
    f = fcn(intrp.x1g[None, None, :] / BRICK_MAX[0], intrp.x2g[None, :, None] / BRICK_MAX[1],
            intrp.x3g[:, None, None] / BRICK_MAX[2])
    return np.repeat(f[None], nstate, axis=0)


def sphere_expected(intrp, nstate, projected=True):
    """fex of interpolation.jl:376-405 as (nstate, n_rad, n_lat, n_long): the sample function in
    every state, columns 2-4 then projected as if they held one Cartesian vector."""
    a = PLANET_RADIUS
    lat, lon, rad = intrp.lat_grd[None, :, None], intrp.long_grd[None, None, :], intrp.rad_grd[:, None, None]
    x1 = rad * I.cosd(lat) * I.cosd(lon)
    x2 = rad * I.cosd(lat) * I.sind(lon)
    x3 = rad * I.sind(lat) * np.ones_like(lon)
    f = fcn(x1 / a, x2 / a, x3 / a)
    fex = np.repeat(f[None], nstate, axis=0)
    if projected:
        fex[1] = -f * I.sind(lon) + f * I.cosd(lon)
        fex[2] = -f * I.sind(lat) * I.cosd(lon) - f * I.sind(lat) * I.sind(lon) + f * I.cosd(lat)
        fex[3] = f * I.cosd(lat) * I.cosd(lon) + f * I.cosd(lat) * I.sind(lon) + f * I.sind(lat)
    return fex


def random_state(grid, nstate, seed):
    """A seeded random state, discontinuous across elements."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((grid.nelem, nstate, grid.Np))
