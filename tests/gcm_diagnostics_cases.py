"""Set-ups and states of the AtmosGCMDefault diagnostics tests (test infrastructure): the brick cut out
of the reference's own test mesh, the small Held-Suarez sphere with its output grid, the noisy states of
the bit-for-bit comparisons and the solid-body rotation.  Shared by tests/test_gcm_diagnostics_host.py and
tests/test_gpu_gcm_diagnostics.py."""
import functools

import numpy as np

from cmdg_loader import cm
from dgfv_atmos_cases import counter_hash
from helpers import held_suarez_setup

M = cm.mesh
A = cm.atmos
I = cm.mesh.interpolation
XMAX = 2500.0                       # diagnostic_fields_test.jl:147-149
SIDE = XMAX / 13                    # an element of its horizontal mesh (Δh = 50, N = 4)
OMEGA = 5e-6                        # solid-body rotation rate: 32 m/s at the equator
X = (M.grids._x1, M.grids._x2, M.grids._x3)


def brick(n=3, N=4, rank=0, size=1):
    """n x n x n elements of side 2500 / 13 m, every side a boundary (walls), the dry law with a flat
    orientation on it."""
    rng = [np.linspace(0.0, n * SIDE, n + 1)] * 3
    topl = M.StackedBrickTopology(rng, boundary=((1, 1), (1, 1), (1, 2)), periodicity=(False,) * 3,
                                  connectivity="full", rank=rank, size=size)
    grid = M.DiscontinuousSpectralElementGrid(topl, N)
    ps = A.PlanetParameters()
    law = A.DryAtmosModel(A.CourantTestSetup(ps), orientation=A.ORIENT_FLAT, ref_state=None, viscosity=0.0,
                          dynamic_viscosity=True, sources=A.SRC_GRAVITY,
                          boundary_conditions=(A.BC_ATMOS_DEFAULT, A.BC_ATMOS_DEFAULT), param_set=ps)
    return law, grid


@functools.lru_cache(maxsize=None)
def sphere(rank=0, size=1):
    """held_suarez_setup(3, 2, 4) and a 15 x 15 degree x 10 km output grid."""
    law, grid, _, _ = held_suarez_setup(n_horz=3, n_vert=2, N=4, rank=rank, size=size)
    a = law.ps.planet_radius
    vert_range = np.linspace(a, a + 30e3, 3)
    lat = -90.0 + 15.0 * np.arange(13)
    lon = -180.0 + 15.0 * np.arange(25)
    rad = a + 10e3 * np.arange(4)
    return law, grid, I.InterpolationCubedSphere(grid, vert_range, 3, lat, lon, rad)


def coordinates(grid):
    return [grid.vgeo[:, c] for c in X]


def fcn0(x, y, z):
    return np.sin(np.pi * x / XMAX) * np.cos(np.pi * y / XMAX) * np.cos(np.pi * z / XMAX)


def fcn_grad(x, y, z):
    """fcnx, fcny, fcnz of diagnostic_fields_test.jl:199-207."""
    sx, cx = np.sin(np.pi * x / XMAX), np.cos(np.pi * x / XMAX)
    sy, cy = np.sin(np.pi * y / XMAX), np.cos(np.pi * y / XMAX)
    sz, cz = np.sin(np.pi * z / XMAX), np.cos(np.pi * z / XMAX)
    return [cx * cy * cz * np.pi / XMAX, -sx * sy * cz * np.pi / XMAX, -sx * cy * sz * np.pi / XMAX]


def reference_field(grid):
    """ρ = 1 + 5 f, ρu = ρv = ρw = ρ f (:209-215) and a ρe that plays no part: ``Q (nelem, 5, Np)``."""
    f = fcn0(*coordinates(grid))
    Q = np.zeros((grid.nelem, 5, grid.Np))
    Q[:, 0] = 1.0 + f * 5.0
    for c in range(3):
        Q[:, 1 + c] = Q[:, 0] * f
    Q[:, 4] = 1.0
    return Q


def exact_gradients(grid):
    """The nine analytic gradients ``[3 c + m]`` and the analytic curl of (f, f, f) on the real elements."""
    g = [a[:grid.nreal] for a in fcn_grad(*coordinates(grid))]
    return [g[m] for _ in range(3) for m in range(3)], [g[1] - g[2], g[2] - g[0], g[0] - g[1]]


def _hash(grid, ncol, salt=0):
    """counter hash of (global element, column, node) in [-1, 1): the same on every partition."""
    gid = np.asarray(grid.topology.globalelems, dtype=np.int64)[:grid.nelem]
    counter = ((gid[:, None, None] + salt) * ncol + np.arange(ncol)[None, :, None]) * grid.Np \
        + np.arange(grid.Np)[None, None, :]
    return counter_hash(counter)


def noisy_state(law, grid, base=None):
    """A physical state with per-node noise, so that no symmetry hides an index error: ``base`` (default:
    air at rest at 280 K on the brick, the law's own initial state on the sphere) with density and energy
    times ``1 + 1e-3 h`` and a momentum of ``5 ρ h`` per component."""
    aux = law.init_state_auxiliary(grid)
    if base is None:
        if law.orientation == A.ORIENT_SPHERICAL:
            base = law.init_state_prognostic(grid, aux, 0.0)
        else:
            ps = law.ps
            base = np.zeros((grid.nelem, 5, grid.Np))
            base[:, 0] = 1.1
            base[:, 4] = base[:, 0] * (ps.cv_d * (280.0 - ps.T_0) + aux[:, law.off_phi])
    h = _hash(grid, 5)
    Q = base.copy()
    Q[:, 0] *= 1 + 1e-3 * h[:, 0]
    Q[:, 4] *= 1 + 1e-3 * h[:, 4]
    for d in range(3):
        Q[:, 1 + d] += Q[:, 0] * 5.0 * h[:, 1 + d]
    return Q, aux


def element_offsets(grid, amplitude):
    """One random offset per (global element, component), ``(nelem, 3, 1)``: makes a velocity
    discontinuous across every face."""
    gid = np.asarray(grid.topology.globalelems, dtype=np.int64)[:grid.nelem]
    return amplitude * counter_hash((gid[:, None] + 7919) * 3 + np.arange(3)[None, :])[:, :, None]


def solid_body_state(law, grid):
    """Solid-body rotation about the polar axis: ρ and the reference energy of HeldSuarezSetup, ρu = ρ ω × x,
    ρe = ρe_ref + ρ |u|^2 / 2."""
    aux = law.init_state_auxiliary(grid)
    x = aux[:, 0:3]
    rho = aux[:, law.off_ref]
    u = np.stack([-OMEGA * x[:, 1], OMEGA * x[:, 0], 0.0 * x[:, 2]], axis=1)
    Q = np.zeros((grid.nelem, 5, grid.Np))
    Q[:, 0] = rho
    Q[:, 1:4] = rho[:, None] * u
    Q[:, 4] = aux[:, law.off_ref + 3] + rho * (0.5 * (u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1] + u[:, 2] * u[:, 2]))
    return Q, aux


def solid_body_expected(law, intrp):
    """The known answer on the output grid, ``name -> (nlevel, nlat, nlong)``: u = ω r cos(lat), v = w = 0,
    vort = vort2 = 2 ω sin(lat), and ρ, T, p of the hydrostatic reference state at the level's height."""
    ps = law.ps
    lat = np.deg2rad(intrp.lat_grd)[None, :, None]
    r = intrp.rad_grd[:, None, None]
    one = np.ones((intrp.n_rad, intrp.n_lat, intrp.n_long))
    T, p = law.ref_state(intrp.rad_grd - ps.planet_radius)
    rho = p / (ps.R_d * T)
    vort = 2 * OMEGA * np.sin(lat) * one
    return dict(u=OMEGA * r * np.cos(lat) * one, v=0 * one, w=0 * one, vort=vort, vort2=vort,
                rho=rho[:, None, None] * one, temp=T[:, None, None] * one, pres=p[:, None, None] * one)


# The deviation of the NumPy restatement (the reference's arithmetic) from solid_body_expected on
# sphere(): the order-4 representation of the warped geometry on 30-degree elements, measured on the CPU
# (tests/test_gcm_diagnostics_host.py recomputes it and holds it to these figures).  The device is
# allowed four times each.
#   u 1.887e-4 m/s (of 32.0), v 1.220e-4, w 1.220e-4, vort 3.748e-9 1/s (of 1e-5), vort2 1.700e-8,
#   rho 5.964e-4 kg/m^3 (of 1.217), temp 0.1901 K (of 290), pres 21.22 Pa (of 101325)
SOLID_BODY_DEVIATION = dict(u=1.89e-4, v=1.23e-4, w=1.23e-4, vort=3.75e-9, vort2=1.71e-8, rho=5.97e-4, temp=0.191,
                            pres=21.3)
