"""Shared pieces of the NTracers checks (CPU oracle and device).

The oracle's dry atmosphere law is frozen without tracers, so a tracer tendency has no oracle of
its own.  The oracle's AdvectionDiffusion law does (the reference stores numbers for it), it reads a
nodal velocity and a nodal diffusion tensor from its auxiliary state, its Rusanov speed is
``|n . u|`` -- the tracer's own (tracers.jl:162-178) -- and its second-order flux is
``-D grad(state)`` with central fluxes.  On a periodic grid, for tracer ``k``

    T_atmos[rho chi_k] == T_advdiff(state = rho chi_k, u = rho u / rho nodal, no diffusion)
                        + T_advdiff(state = rho chi_k / rho, no advection, D = rho delta_k D_t I nodal)

with ``D_t = nu inv_Pr_turb`` (constant kinematic viscosity), both sides under Rusanov or both under
the central flux: term by term ``rho chi u`` (tendencies_tracers.jl:7-11) and
``((-D_t) delta_chi') .* grad chi rho`` (:17-22).  ``crosslaw_expected`` evaluates the right-hand
side through ``make_dg(law, grid, direction, diffusion_direction, nf)``, an operator whose call is
``dg(tendency, Q, t, alpha, beta)`` on numpy arrays (the oracle on the host).

The grids and the smooth states (a few elements per wavelength, all three velocity components) of
tests/test_tracers_host.py and tests/test_gpu_tracers.py are built here too."""
import numpy as np

from helpers import cm

M, A, BL = cm.mesh, cm.atmos, cm.balancelaws
NU = 75.0          # constant kinematic viscosity of the viscous cases, m^2 / s


# ---- grids -------------------------------------------------------------------------------------
def periodic_brick(Ne=2, N=4, L=1000.0):
    x = np.linspace(0.0, L, Ne + 1)
    topl = M.StackedBrickTopology([x] * 3, periodicity=(True,) * 3, connectivity="full")
    return M.DiscontinuousSpectralElementGrid(topl, N)


def walled_box(ne=(3, 3, 2), N=4, L=(1500.0, 1500.0, 1000.0), rank=0, size=1):
    """Walls on all six sides, boundary tags 1 and 2 in every direction."""
    rng = [np.linspace(0.0, L[d], ne[d] + 1) for d in range(3)]
    topl = M.StackedBrickTopology(rng, periodicity=(False,) * 3, boundary=((1, 2),) * 3, connectivity="full",
                                  rank=rank, size=size)
    return M.DiscontinuousSpectralElementGrid(topl, N)


def sphere(n_horz=2, n_vert=2, N=4, rank=0, size=1):
    ps = A.PlanetParameters()
    R = np.linspace(ps.planet_radius, ps.planet_radius + 30e3, n_vert + 1)
    topl = M.StackedCubedSphereTopology(n_horz, R, boundary=(1, 2), rank=rank, size=size)
    return M.DiscontinuousSpectralElementGrid(topl, N, meshwarp=M.equiangular_cubed_sphere_warp)


# ---- smooth states -------------------------------------------------------------------------------
class SmoothBox:
    """A smooth state of one wavelength per box length: density, three velocity components,
    temperature and ``ntr`` different mixing ratios (or ``mixing``: constants)."""

    def __init__(self, ps, L, mixing=None):
        self.ps, self.L, self.mixing = ps, L, mixing

    def __call__(self, law, aux, coord, t):
        ps = self.ps
        X = [2 * np.pi * coord[d] / self.L[d] for d in range(3)]
        rho = 1.1 * (1 + 0.05 * np.sin(X[0]) * np.cos(X[1]) + 0.03 * np.sin(X[2] + X[0]))
        u = [20 * np.sin(X[1] + 0.3) * np.cos(X[2]), 15 * np.cos(X[0]) * np.sin(X[2] + 0.5),
             10 * np.sin(X[0] + X[1])]
        T = 290 + 8 * np.cos(X[0]) * np.cos(X[1]) * np.sin(X[2] + 0.2)
        e_pot = aux[:, law.off_phi, :] if law.orientation != A.ORIENT_NONE else 0.0
        rhoe = rho * (ps.cv_d * (T - ps.T_0) + (u[0] * u[0] + u[1] * u[1] + u[2] * u[2]) / 2 + e_pot)
        out = (rho, [rho * u[0], rho * u[1], rho * u[2]], rhoe)
        if not law.ntracers:
            return out
        if self.mixing is not None:
            return out + ([c * rho for c in self.mixing],)
        chi = [1.0 + 0.5 * np.sin(X[0] + 0.4 * (k + 1)) * np.cos(X[1] - 0.7 * k) + 0.3 * np.cos(X[2] * (1 + (k % 2)) + k)
               for k in range(law.ntracers)]
        return out + ([rho * c for c in chi],)


class SmoothSphere:
    """The Held-Suarez state with a smooth wind of three Cartesian components and a temperature
    anomaly (tests/hs_crosslaw.py), and ``ntr`` mixing ratios."""

    def __init__(self, ps, mixing=None):
        self.ps, self.mixing, self.hs = ps, mixing, A.HeldSuarezSetup(ps)

    def __call__(self, law, aux, coord, t):
        ps = self.ps
        rho = aux[:, law.off_ref + 0, :].copy()
        r = np.sqrt(coord[0] ** 2 + coord[1] ** 2 + coord[2] ** 2)
        lam, phi = np.arctan2(coord[1], coord[0]), np.arcsin(coord[2] / r)
        u = [30 * np.sin(2 * lam) * np.cos(phi), 20 * np.cos(3 * phi) * np.cos(lam), 10 * np.sin(lam + phi)]
        rhoe = (aux[:, law.off_ref + 3, :] + rho * 0.5 * (u[0] ** 2 + u[1] ** 2 + u[2] ** 2)
                + rho * ps.cv_d * 2.0 * np.sin(3 * lam) * np.cos(phi) ** 2)
        out = (rho, [rho * u[0], rho * u[1], rho * u[2]], rhoe)
        if not law.ntracers:
            return out
        if self.mixing is not None:
            return out + ([c * rho for c in self.mixing],)
        return out + ([rho * (1 + 0.5 * np.sin((k + 1) * lam) * np.cos(phi + k)) for k in range(law.ntracers)],)


# ---- models ------------------------------------------------------------------------------------
def plain_model(delta=None, viscosity=NU, mixing=None, L=(1000.0,) * 3):
    """``DryAtmos<false, false, false>``: no orientation, no reference state, no sources."""
    ps = A.PlanetParameters()
    return A.DryAtmosModel(SmoothBox(ps, L, mixing), orientation=A.ORIENT_NONE, ref_state=None,
                           viscosity=viscosity, dynamic_viscosity=False, sources=0, boundary_conditions=(),
                           param_set=ps, tracers=None if delta is None else A.NTracers(delta))


def box_model(delta=None, viscosity=NU, smagorinsky=False, mixing=None, L=(1500.0, 1500.0, 1000.0)):
    """``DryAtmos<true, true, false[, SMAG]>`` in the walled box: flat orientation, hydrostatic
    reference state, gravity, ``AtmosBC()`` on both tags."""
    ps = A.PlanetParameters()
    return A.DryAtmosModel(SmoothBox(ps, L, mixing), orientation=A.ORIENT_FLAT,
                           ref_state=A.DryAdiabaticProfile(ps, 300.0, 0.0),
                           viscosity=0.0 if smagorinsky else viscosity, dynamic_viscosity=False,
                           smagorinsky=ps.C_smag if smagorinsky else None, sources=A.SRC_GRAVITY,
                           boundary_conditions=(A.BC_ATMOS_DEFAULT, A.BC_ATMOS_DEFAULT), param_set=ps,
                           tracers=None if delta is None else A.NTracers(delta))


def sphere_model(delta=None, viscosity=0.0, hyperdiffusion=True, mixing=None):
    """``DryAtmos<true, true, HYPER>`` on the sphere: the Held-Suarez configuration."""
    ps = A.PlanetParameters()
    return A.DryAtmosModel(SmoothSphere(ps, mixing), orientation=A.ORIENT_SPHERICAL,
                           ref_state=A.DecayingTemperatureProfile(ps, 290.0, 220.0, 8e3),
                           viscosity=viscosity, dynamic_viscosity=False,
                           hyperdiffusion_timescale=8 * 3600.0 if hyperdiffusion else None,
                           sources=A.SRC_GRAVITY | A.SRC_CORIOLIS | A.SRC_HELD_SUAREZ,
                           boundary_conditions=(A.BC_ATMOS_DEFAULT, A.BC_ATMOS_DEFAULT), param_set=ps,
                           tracers=None if delta is None else A.NTracers(delta))


def initial_state(law, grid):
    aux = law.init_state_auxiliary(grid)
    return law.init_state_prognostic(grid, aux, 0.0), aux


def scaled_linf(a, b):
    """max |a - b| / max |b|: the device-vs-oracle parity measure (1e-12 is the bar)."""
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


# ---- the cross-law right-hand side ---------------------------------------------------------------
class _Nodal:
    """A host-only 'problem' of the advection-diffusion law: nodal velocity ``u`` (3 fields) and
    nodal isotropic diffusion tensor ``D I``."""
    problem_id = 6

    def __init__(self, u=None, D=None):
        self.u, self.D = u, D

    def dparam(self):
        return np.zeros(32)

    def init_velocity_diffusion(self, law, aux, coord):
        if law.advection:
            for d in range(3):
                aux[:, law.off_u + d, :] = self.u[d]
        if law.diffusion:
            for d in range(3):
                aux[:, law.off_D + 4 * d, :] = self.D          # column-major 3 x 3

    def initial_condition(self, coord, t):
        return 0.0 * coord[0]


def advdiff_tendency(make_dg, grid, state, u=None, D=None, direction=0, diffusion_direction=None, nf=0):
    """Tendency of the one-state AdvectionDiffusion law with nodal coefficients, real elements."""
    law = BL.AdvectionDiffusion(3, _Nodal(u, D), (), advection=u is not None, diffusion=D is not None)
    dd = direction if diffusion_direction is None else diffusion_direction
    dg = make_dg(law, grid, direction, dd, nf)
    q = np.zeros((grid.nelem, 1, grid.Np))
    q[:, 0, :] = state
    t = np.zeros_like(q)
    dg(t, q, 0.0, 1.0, 0.0)
    return t[:grid.nreal, 0, :]


def crosslaw_expected(make_dg, grid, law, Q, k, direction=0, diffusion_direction=None, nf=0):
    """The right-hand side of the identity for tracer ``k`` of ``law`` (constant kinematic viscosity)."""
    assert law.C_smag is None and not law.dynamic_viscosity
    rho, rhochi = Q[:, 0, :], Q[:, 5 + k, :]
    u = [Q[:, 1 + d, :] / rho for d in range(3)]
    expect = advdiff_tendency(make_dg, grid, rhochi, u=u, direction=direction, nf=nf)
    D_t = law.viscosity * law.ps.inv_Pr_turb
    if D_t != 0:
        D = rho * (law.tracers.delta_chi[k] * D_t)
        expect = expect + advdiff_tendency(make_dg, grid, rhochi / rho, D=D, direction=direction,
                                           diffusion_direction=diffusion_direction, nf=nf)
    return expect


# ---- the acoustic wave with its tracer (acousticwave_1d_imex.jl:47,116-123,308) -----------------------
def acoustic_setup(n_horz, n_vert, N=5, tracer=True):
    """``imex_cases.acoustic_setup`` with the reference's passive tracer carried: ``rho chi = 1``,
    ``delta_chi = 1``."""
    from imex_cases import AcousticWaveSetup
    ps = A.PlanetParameters()
    a = ps.planet_radius
    topl = M.StackedCubedSphereTopology(n_horz, np.linspace(a, a + 10e3, n_vert + 1), boundary=(1, 2))
    grid = M.DiscontinuousSpectralElementGrid(topl, N, meshwarp=M.equiangular_cubed_sphere_warp)
    base = AcousticWaveSetup(ps)

    def init(law, aux, coord, t):
        rho, rhou, rhoe = base(law, aux, coord, t)
        return (rho, rhou, rhoe, [1.0 + 0.0 * rho]) if law.ntracers else (rho, rhou, rhoe)

    law = A.DryAtmosModel(init, orientation=A.ORIENT_SPHERICAL, ref_state=A.IsothermalProfile(ps, 300.0),
                          viscosity=0.0, dynamic_viscosity=True, sources=A.SRC_GRAVITY,
                          boundary_conditions=(A.BC_ATMOS_DEFAULT, A.BC_ATMOS_DEFAULT), param_set=ps,
                          discrete_hydrostatic_balance=True, tracers=A.NTracers((1.0,)) if tracer else None)
    return law, grid
