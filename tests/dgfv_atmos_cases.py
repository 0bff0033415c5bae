"""Set-ups for the dry atmosphere law on a DGFVModel (test infrastructure): the brick and the shell of
``test/Numerics/DGMethods/Euler/fvm_balance.jl``, the y-invariant slice of ``fvm_isentropicvortex.jl``
(``dims = 2``), and the noisy state the one-evaluation comparisons use.  Shared by
tests/test_dgfv_atmos_host.py and tests/test_gpu_dgfv_atmos.py."""
import numpy as np

from cmdg_loader import cm

M = cm.mesh
A = cm.atmos
WALLS = (A.BC_ATMOS_DEFAULT, A.BC_ATMOS_DEFAULT)


def counter_hash(counter):
    """Uniform numbers in [-1, 1) as a function of an integer counter alone (the splitmix64
    finaliser): the same value for the same (global element, state, node), whoever asks."""
    x = np.asarray(counter, dtype=np.uint64) + np.uint64(0x9E3779B97F4A7C15)
    with np.errstate(over="ignore"):
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    x = x ^ (x >> np.uint64(31))
    return (x >> np.uint64(11)).astype(np.float64) / 2.0 ** 52 - 1.0


def balanced_state(law, aux, coord, t):
    """``initialcondition!`` of fvm_balance.jl:203-207: the reference state at rest."""
    rho = aux[:, law.off_ref, :]
    zero = 0.0 * rho
    return rho, [zero, zero, zero], aux[:, law.off_ref + 3, :]


class NoisyDryAtmosModel(A.DryAtmosModel):
    """The law's own initial state times ``1 + amplitude h`` in density and energy, with a momentum
    of ``rho speed h`` per component; ``h`` the counter hash of (global element, state, node)."""
    amplitude, speed = 1e-3, 5.0

    def init_state_prognostic(self, grid, aux, t):
        Q = super().init_state_prognostic(grid, aux, t)
        gid = np.asarray(grid.topology.globalelems, dtype=np.int64)[:Q.shape[0]]
        counter = (gid[:, None, None] * 5 + np.arange(5)[None, :, None]) * grid.Np + np.arange(grid.Np)[None, None, :]
        h = counter_hash(counter)
        Q[:, 0] *= 1 + self.amplitude * h[:, 0]
        Q[:, 4] *= 1 + self.amplitude * h[:, 4]
        for d in range(3):
            Q[:, 1 + d] += Q[:, 0] * self.speed * h[:, 1 + d]
        return Q


def box_grid(n_horz, n_vert, periodic_stack=False, width=20e3, height=10e3, rank=0, size=1):
    h = np.linspace(0.0, width, n_horz + 1)
    topl = M.StackedBrickTopology([h, h, np.linspace(0.0, height, n_vert + 1)], boundary=((0, 0), (0, 0), (1, 2)),
                                  periodicity=(True, True, periodic_stack), connectivity="full", rank=rank, size=size)
    return M.DiscontinuousSpectralElementGrid(topl, (4, 0))


def balance_box(n_horz=2, n_vert=32, periodic_stack=False, sources=A.SRC_GRAVITY, noisy=False, rank=0, size=1):
    """fvm_balance.jl, ``:box``: 20 km x 20 km x 10 km, periodic in the horizontal, isothermal 300 K
    reference state that is not subtracted, Gravity."""
    ps = A.PlanetParameters()
    cls = NoisyDryAtmosModel if noisy else A.DryAtmosModel
    law = cls(balanced_state, orientation=A.ORIENT_FLAT, ref_state=A.IsothermalProfile(ps, 300.0), subtract_off=False,
              viscosity=0.0, dynamic_viscosity=True, sources=sources,
              boundary_conditions=() if periodic_stack else WALLS, param_set=ps)
    return law, box_grid(n_horz, n_vert, periodic_stack, rank=rank, size=size)


def balance_sphere(n_horz=2, n_vert=32, height=10e3, rank=0, size=1):
    """fvm_balance.jl, ``:sphere``: Gravity and Coriolis on a shell of ``height``."""
    ps = A.PlanetParameters()
    a = ps.planet_radius
    topl = M.StackedCubedSphereTopology(n_horz, np.linspace(a, a + height, n_vert + 1), boundary=(1, 2), rank=rank,
                                        size=size)
    grid = M.DiscontinuousSpectralElementGrid(topl, (4, 0), meshwarp=M.equiangular_cubed_sphere_warp)
    law = A.DryAtmosModel(balanced_state, orientation=A.ORIENT_SPHERICAL, ref_state=A.IsothermalProfile(ps, 300.0),
                          subtract_off=False, viscosity=0.0, dynamic_viscosity=True,
                          sources=A.SRC_GRAVITY | A.SRC_CORIOLIS, boundary_conditions=WALLS, param_set=ps)
    return law, grid


def balance_dt(law, height=10e3, n_vert=32, timeend=100.0, cfl=0.2):
    """fvm_balance.jl:138-143."""
    ps = law.ps
    dt = cfl * (height / n_vert) / np.sqrt(ps.cp_d / ps.cv_d * ps.R_d * 300.0)
    nsteps = int(np.ceil(timeend / dt))
    return timeend / nsteps, nsteps


def vortex_box(n_horz=2, n_vert=6, noisy=True):
    """The vortex law (NoOrientation, NoReferenceState, no source) on a fully periodic brick of the
    vortex's domain."""
    ps = A.PlanetParameters()
    setup = A.IsentropicVortexSetup(ps)
    L = setup.domain_halflength
    h = np.linspace(-L, L, n_horz + 1)
    topl = M.StackedBrickTopology([h, h, np.linspace(-L, L, n_vert + 1)], periodicity=(True, True, True),
                                  connectivity="full")
    cls = NoisyDryAtmosModel if noisy else A.DryAtmosModel
    law = cls(setup, orientation=A.ORIENT_NONE, ref_state=None, viscosity=0.0, dynamic_viscosity=True, sources=0,
              boundary_conditions=(), param_set=ps)
    return law, M.DiscontinuousSpectralElementGrid(topl, (4, 0))
