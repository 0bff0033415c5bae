"""Host-side description of the dry ``AtmosModel`` configurations carried by libcmdg
(device functor: ``csrc/physics_atmos.h``).

Reference: ``src/Atmos/Model/AtmosModel.jl`` (vars_state :397-511, gradient argument
:625-690, wavespeed :808-828), ``tendencies_{mass,momentum,energy}.jl``,
``atmos_tendencies.jl``, ``energy.jl``, ``moisture.jl:47-62`` (DryModel auxiliary
``theta_v, air_T`` refreshed every RHS), ``ref_state.jl``, ``boundaryconditions.jl`` +
``bc_momentum.jl`` + ``bc_energy.jl`` (default ``AtmosBC``: Impenetrable(FreeSlip),
Insulating), ``src/Common/Orientations/Orientations.jl``,
``src/Common/TurbulenceClosures/TurbulenceClosures.jl:300-420`` (constant viscosity) and
``:846-912`` (DryBiharmonic), ``experiments/AtmosGCM/heldsuarez.jl`` (initial condition
:47-104, forcing :106-172, configuration :174-218),
``test/Numerics/DGMethods/Euler/isentropicvortex*.jl``.

Thermodynamics.jl 0.3.2 and CLIMAParameters.jl 0.1.11 are registered packages that are
not vendored in the reference tree; the dry closed forms and planet constants below
restate their published definitions and are pinned at this boundary by the isentropic
vortex golden value (``isentropicvortex.jl:105``).

State layout: prognostic ``rho, rho*u(3), rho*e``; auxiliary ``coord(3) [, Phi, grad
Phi(3)] [, ref rho, p, T, rho*e, rho*q_tot, rho*q_liq, rho*q_ice] [, Delta] , theta_v,
air_T``; gradient ``u(3), h_tot [, u_h(3), h_tot]``; gradient flux ``grad h_tot(3),
S(6)``; gradient-laplacian ``u_h(3), h_tot``; hyperdiffusive ``nu grad^3 u_h (9), nu
grad^3 h_tot (3)``.

With ``tracers=NTracers(delta_chi)`` (``src/Atmos/Model/tracers.jl``, ``tendencies_tracers.jl``,
``bc_tracer.jl``) the ``NT`` tracers follow every other component: prognostic ``rho*chi[NT]``,
auxiliary ``delta_chi[NT]`` after ``theta_v, air_T``, gradient ``chi[NT]`` last, gradient flux
``grad chi`` (3 x NT, three consecutive columns per tracer) last.
"""
import numpy as np

from .balancelaws import (PHYSICS_ATMOS_LINEAR_ACOUSTIC, PHYSICS_ATMOS_LINEAR_AG, PHYSICS_DRY_ATMOS,
                          PHYSICS_MOIST_ATMOS, PHYSICS_MOIST_LINEAR_AG)
from .mesh import grids as G

__all__ = ["PlanetParameters", "DryAtmosModel", "NTracers", "IsentropicVortexSetup", "HeldSuarezSetup",
           "DecayingTemperatureProfile", "DryAdiabaticProfile", "RisingBubbleSetup",
           "CourantTestSetup", "MMSSetup", "IsothermalProfile", "AtmosAcousticGravityLinearModel",
           "IsentropicVortexReferenceState", "AtmosAcousticLinearModel", "HBFVReconstruction",
           "prognostic_to_primitive", "primitive_to_prognostic", "construct_face_auxiliary_state",
           "fvm_balance", "vert_fvm_auxiliary_field_gradient"]


class PlanetParameters:
    """CLIMAParameters.jl 0.1.11 ``Planet`` / ``SubgridScale`` values used by the dry model."""
    gas_constant = 8.3144598
    molmass_dryair = 28.97e-3
    kappa_d = 2 / 7
    T_0 = 273.16
    grav = 9.81
    planet_radius = 6.371e6
    Omega = 7.2921159e-5
    MSLP = 1.01325e5
    day = 86400.0
    inv_Pr_turb = 3.0
    C_smag = 0.21

    @property
    def R_d(self):
        return self.gas_constant / self.molmass_dryair

    @property
    def cp_d(self):
        return self.R_d / self.kappa_d

    @property
    def cv_d(self):
        return self.cp_d - self.R_d


class DecayingTemperatureProfile:
    """``DecayingTemperatureProfile(T_virt_surf, T_min_ref, H_t)`` of
    Thermodynamics.TemperatureProfiles: returns ``(T_virt, p)`` at altitude ``z``."""

    def __init__(self, ps, T_virt_surf=290.0, T_min_ref=220.0, H_t=8e3):
        self.ps, self.Ts, self.Tm, self.Ht = ps, T_virt_surf, T_min_ref, H_t

    def __call__(self, z):
        ps = self.ps
        H_sfc = ps.R_d * self.Ts / ps.grav
        zp = z / self.Ht
        th = np.tanh(zp)
        dTv = self.Ts - self.Tm
        Tv = self.Ts - dTv * th
        dTvp = dTv / self.Ts
        p = -self.Ht * (zp + dTvp * (np.log(1 - dTvp * th) - np.log(1 + th) + zp))
        p = p / (H_sfc * (1 - dTvp ** 2))
        p = ps.MSLP * np.exp(p)
        return Tv, p


class IsothermalProfile:
    """``IsothermalProfile(param_set, T)`` of Thermodynamics.TemperatureProfiles (not vendored):
    ``T_virt = T`` and ``p = MSLP exp(-g z / (R_d T))`` at altitude ``z``."""

    def __init__(self, ps, T=300.0):
        self.ps, self.T = ps, float(T)

    def __call__(self, z):
        ps = self.ps
        Tv = self.T + 0.0 * z
        p = ps.MSLP * np.exp(-z * ps.grav / (ps.R_d * self.T))
        return Tv, p


class DryAdiabaticProfile:
    """``DryAdiabaticProfile(T_surface, T_min_ref)`` of Thermodynamics.TemperatureProfiles
    (Thermodynamics.jl 0.3.2, not vendored): ``T = max(T_surface - Gamma z, T_min)`` with
    ``Gamma = g / cp_d``, ``p = MSLP (T / T_surface)^(g / (R_d Gamma))`` and an isothermal
    decay above the height where ``T_min`` is reached."""

    def __init__(self, ps, T_surface=300.0, T_min_ref=0.0):
        self.ps, self.T_surface, self.T_min_ref = ps, T_surface, T_min_ref

    def __call__(self, z):
        ps = self.ps
        Gamma = ps.grav / ps.cp_d
        T = np.maximum(self.T_surface - Gamma * z, self.T_min_ref)
        p = ps.MSLP * (T / self.T_surface) ** (ps.grav / (ps.R_d * Gamma))
        if self.T_min_ref > 0:
            z_top = (self.T_surface - self.T_min_ref) / Gamma
            H_min = ps.R_d * self.T_min_ref / ps.grav
            p = np.where(T == self.T_min_ref, p * np.exp(-(z - z_top) / H_min), p)
        return T, p


class RisingBubbleSetup:
    """``init_risingbubble!`` of experiments/TestCase/risingbubble.jl:22-91 (dry)."""

    def __init__(self, ps, theta_ref=300.0, xc=5000.0, zc=2000.0, rc=2000.0, theta_amplitude=2.0):
        self.ps, self.theta_ref = ps, theta_ref
        self.xc, self.zc, self.rc, self.amp = xc, zc, rc, theta_amplitude

    def __call__(self, law, aux, coord, t):
        ps = self.ps
        x, z = coord[0], coord[2]
        r = np.sqrt((x - self.xc) ** 2 + (z - self.zc) ** 2)
        dtheta = np.where(r <= self.rc, self.amp * (1.0 - r / self.rc), 0.0)
        theta = self.theta_ref + dtheta
        pi_exner = 1.0 - ps.grav / (ps.cp_d * theta) * z
        rho = ps.MSLP / (ps.R_d * theta) * pi_exner ** (ps.cv_d / ps.R_d)
        T = theta * pi_exner
        e_int = ps.cv_d * (T - ps.T_0)
        e_pot = aux[:, law.off_phi, :]
        rhoe = rho * (0.0 + e_pot + e_int)
        zero = 0.0 * rho
        return rho, [zero, zero, zero], rhoe


class IsentropicVortexSetup:
    """``IsentropicVortexSetup`` (isentropicvortex_setup.jl:3-60).  ``plane``: the two coordinate
    directions the vortex turns and travels in, ``(0, 1)`` as in the reference's three-dimensional
    runs; ``(0, 2)`` puts the plane of a ``dims = 2`` run (horizontal, vertical) into the y-invariant
    slice of a three-dimensional grid."""

    def __init__(self, ps, plane=(0, 1)):
        self.ps = ps
        self.plane = tuple(plane)
        self.p_inf, self.T_inf = 1e5, 300.0
        self.rho_inf = self.p_inf / (ps.R_d * self.T_inf)
        self.translation_speed, self.translation_angle = 150.0, np.pi / 4
        self.vortex_speed, self.vortex_radius = 50.0, 1 / 200
        self.domain_halflength = 1 / 20

    def __call__(self, law, aux, coord, t):
        ps = self.ps
        a = self.translation_angle
        i, j = self.plane
        uinf = np.zeros(3)
        uinf[i], uinf[j] = self.translation_speed * np.cos(a), self.translation_speed * np.sin(a)
        L, R = self.domain_halflength, self.vortex_radius
        x = [coord[d] - uinf[d] * t for d in range(3)]
        x = [xd - np.floor((xd + L) / (2 * L)) * 2 * L for xd in x]
        r = np.sqrt(x[i] ** 2 + x[j] ** 2)
        du = [0 * x[i], 0 * x[i], 0 * x[i]]
        du[i] = -self.vortex_speed * x[j] / R * np.exp(-(r / R) ** 2 / 2)
        du[j] = self.vortex_speed * x[i] / R * np.exp(-(r / R) ** 2 / 2)
        u = [uinf[d] + du[d] for d in range(3)]
        T = self.T_inf * (1 - ps.kappa_d * self.vortex_speed ** 2 / 2 * self.rho_inf / self.p_inf
                          * np.exp(-(r / R) ** 2))
        p = self.p_inf * (T / self.T_inf) ** (1.0 / ps.kappa_d)
        rho = p / (ps.R_d * T)
        e_kin = (u[0] * u[0] + u[1] * u[1] + u[2] * u[2]) / 2
        rhoe = rho * (e_kin + 0.0 + ps.cv_d * (T - ps.T_0))
        return rho, [rho * u[0], rho * u[1], rho * u[2]], rhoe


class IsentropicVortexReferenceState:
    """``IsentropicVortexReferenceState(setup)`` (isentropicvortex_setup.jl:64-100): the constant
    far field ``rho_inf, p_inf, T_inf, rho_inf cv_d (T_inf - T_0)`` in the reference-state columns.
    It is not a ``HydrostaticState``: the full law carries it and subtracts nothing
    (tendencies_momentum.jl), so ``DryAtmosModel`` turns ``subtract_off`` off for it; its user is the
    linear model (``AtmosAcousticLinearModel``)."""

    def __init__(self, setup):
        self.setup = setup

    def fill(self, ps, aux, off_ref):
        s = self.setup
        aux[:, off_ref + 0, :] = s.rho_inf
        aux[:, off_ref + 1, :] = s.p_inf
        aux[:, off_ref + 2, :] = s.T_inf
        aux[:, off_ref + 3, :] = s.rho_inf * (ps.cv_d * (s.T_inf - ps.T_0))   # internal_energy(T_inf)


class MMSSetup:
    """``mms3_init_state!`` of test/Numerics/DGMethods/compressible_Navier_Stokes/
    mms_bc_atmos.jl:88-97: the manufactured solution (generating script mms_solution.jl:10-25)
    ``rho = c g + 3, rho u = rho (c g, c g, c h), rho e = c g + 100`` with ``c = cos(pi t)``,
    ``g = sin(pi x) cos(pi y) cos(pi z)``, ``h = sin(pi x) cos(pi y) sin(pi z)``."""

    def __init__(self, ps):
        self.ps = ps

    def __call__(self, law, aux, coord, t):
        x, y, z = coord
        c = np.cos(np.pi * t)
        g = np.sin(np.pi * x) * np.cos(np.pi * y) * np.cos(np.pi * z)
        h = np.sin(np.pi * x) * np.cos(np.pi * y) * np.sin(np.pi * z)
        rho = g * c + 3
        return rho, [rho * g * c, rho * g * c, rho * h * c], g * c + 100


class CourantTestSetup:
    """``initialcondition!`` of test/Numerics/DGMethods/courant.jl:31-60: isothermal air at
    ``T_inf``, ``p_inf`` moving with ``u = 150 x (1, 1, 0)``; the potential energy passed to
    ``total_energy`` is zero there."""

    def __init__(self, ps, p_inf=1e5, T_inf=300.0, translation_speed=150.0):
        self.ps, self.p_inf, self.T_inf, self.speed = ps, p_inf, T_inf, translation_speed

    def __call__(self, law, aux, coord, t):
        ps = self.ps
        u = [self.speed * coord[0], self.speed * coord[0], 0.0 * coord[0]]
        T = self.T_inf
        p = self.p_inf * (T / self.T_inf) ** (1.0 / ps.kappa_d)
        rho = p / (ps.R_d * T) + 0.0 * coord[0]
        e_kin = (u[0] * u[0] + u[1] * u[1] + u[2] * u[2]) / 2
        rhoe = rho * (e_kin + 0.0 + ps.cv_d * (T - ps.T_0))
        return rho, [rho * u[0], rho * u[1], rho * u[2]], rhoe


class HeldSuarezSetup:
    """``init_heldsuarez!`` (experiments/AtmosGCM/heldsuarez.jl:47-104).  On a model with tracers it
    adds the experiment's dummy initialisation ``rho chi[k] = k`` (:99-100, ``k`` counted from one);
    ``HeldSuarezSetup.tracers(n)`` is the model to go with it, ``delta_chi[k] = k`` (:184-186)."""

    @staticmethod
    def tracers(number_of_tracers):
        return NTracers([float(k) for k in range(1, int(number_of_tracers) + 1)]) if number_of_tracers else None

    def __init__(self, ps):
        self.ps = ps

    def __call__(self, law, aux, coord, t):
        ps = self.ps
        a = ps.planet_radius
        z_t, lam_c, phi_c, d_0, V_p = 15e3, np.pi / 9, 2 * np.pi / 9, a / 6, 10.0
        nrm = np.sqrt(coord[0] ** 2 + coord[1] ** 2 + coord[2] ** 2)
        phi = np.arcsin(coord[2] / nrm)
        lam = np.arctan2(coord[1], coord[0])
        z = aux[:, law.off_phi, :] / ps.grav
        F_z = 1 - 3 * (z / z_t) ** 2 + 2 * (z / z_t) ** 3
        F_z = np.where(z > z_t, 0.0, F_z)
        arg = np.sin(phi) * np.sin(phi_c) + np.cos(phi) * np.cos(phi_c) * np.cos(lam - lam_c)
        d = a * np.arccos(np.clip(arg, -1.0, 1.0))
        c3 = np.cos(np.pi * d / 2 / d_0) ** 3
        s1 = np.sin(np.pi * d / 2 / d_0)
        ok = (0 < d) & (d < d_0) & (d != a * np.pi)
        with np.errstate(divide="ignore", invalid="ignore"):
            up = (-16 * V_p / 3 / np.sqrt(3) * F_z * c3 * s1
                  * (-np.sin(phi_c) * np.cos(phi) + np.cos(phi_c) * np.sin(phi) * np.cos(lam - lam_c))
                  / np.sin(d / a))
            vp = (16 * V_p / 3 / np.sqrt(3) * F_z * c3 * s1 * np.cos(phi_c) * np.sin(lam - lam_c)
                  / np.sin(d / a))
        up = np.where(ok, up, 0.0)
        vp = np.where(ok, vp, 0.0)
        wp = 0.0 * up
        sl, cl = np.sin(phi), np.cos(phi)
        so, co = np.sin(lam), np.cos(lam)
        u = [-so * up - sl * co * vp + cl * co * wp,
             co * up - sl * so * vp + cl * so * wp,
             cl * vp + sl * wp]
        e_kin = 0.5 * (u[0] * u[0] + u[1] * u[1] + u[2] * u[2])
        rho = aux[:, law.off_ref + 0, :]
        rhoe = aux[:, law.off_ref + 3, :] + rho * e_kin
        if getattr(law, "ntracers", 0):
            return rho, [rho * u[0], rho * u[1], rho * u[2]], rhoe, [k + 0.0 * rho for k in range(1, law.ntracers + 1)]
        return rho, [rho * u[0], rho * u[1], rho * u[2]], rhoe


ORIENT_NONE, ORIENT_FLAT, ORIENT_SPHERICAL = 0, 1, 2
SRC_GRAVITY, SRC_CORIOLIS, SRC_HELD_SUAREZ, SRC_MMS = 1, 2, 4, 8
# AtmosBC() default (Impenetrable(FreeSlip), Insulating); InitStateBC (bc_initstate.jl) with the
# manufactured solution of MMSSetup
BC_NONE, BC_ATMOS_DEFAULT, BC_INIT_STATE_MMS = 0, 1, 2


MAX_TRACERS = 8


class NTracers:
    """``NTracers{N, FT}(delta_chi)`` (src/Atmos/Model/tracers.jl:111-125): ``N = len(delta_chi)``
    passive tracers ``rho chi[k]``, advected with ``u`` and diffused with ``delta_chi[k] D_t``, the
    turbulence closure's diffusivity scaled per tracer; ``ImpermeableTracer`` on every boundary."""

    def __init__(self, delta_chi):
        self.delta_chi = tuple(float(x) for x in np.atleast_1d(np.asarray(delta_chi, dtype=np.float64)))
        if not 1 <= len(self.delta_chi) <= MAX_TRACERS:
            raise ValueError("NTracers: 1 to %d tracers (got %d); no tracers is tracers=None"
                             % (MAX_TRACERS, len(self.delta_chi)))

    def __len__(self):
        return len(self.delta_chi)


class DryAtmosModel:
    """Dry compressible ``AtmosModel``: ``TotalEnergyModel``, ``DryModel``, constant
    viscosity or ``SmagorinskyLilly(C_smag)``, optional hydrostatic reference state,
    ``DryBiharmonic`` hyperdiffusion, sources ``Gravity / Coriolis / HeldSuarezForcing``."""
    physics_id = PHYSICS_DRY_ATMOS

    def __init__(self, init_state, orientation=ORIENT_SPHERICAL, ref_state=None,
                 subtract_off=True, viscosity=0.0, dynamic_viscosity=False,
                 hyperdiffusion_timescale=None, sources=0, boundary_conditions=(),
                 param_set=None, smagorinsky=None, discrete_hydrostatic_balance=False,
                 with_divergence=False, zero_enthalpy=False, tracers=None):
        if tracers is not None and not isinstance(tracers, NTracers):
            tracers = NTracers(tracers)
        self.tracers = tracers
        self.ntracers = nt = 0 if tracers is None else len(tracers)
        if nt and (int(sources) & SRC_MMS or BC_INIT_STATE_MMS in tuple(boundary_conditions)):
            raise ValueError("DryAtmosModel: MMSSource / InitStateBC are not defined for a model with tracers")
        # ConstantViscosity(..., WithDivergence()) (TurbulenceClosures.jl:290-370) and the
        # total_specific_enthalpy == 0 override of mms_bc_atmos.jl:50-51
        self.with_divergence, self.zero_enthalpy = bool(with_divergence), bool(zero_enthalpy)
        # ref_state.jl:150-175: rho_ref = -k . grad(p_ref) / (k . grad Phi) with the DG gradient of
        # the reference pressure.  Needs the operator (device or oracle); off = analytic density
        self.discrete_hydrostatic_balance = bool(discrete_hydrostatic_balance)
        self.C_smag = smagorinsky
        if smagorinsky is not None:
            assert hyperdiffusion_timescale is None and orientation != ORIENT_NONE
        self.ps = param_set or PlanetParameters()
        self.init_state = init_state
        self.orientation = orientation
        self.ref_state = ref_state
        # only a HydrostaticState is subtracted (tendencies_momentum.jl)
        self.subtract_off = bool(subtract_off) and not isinstance(ref_state, IsentropicVortexReferenceState)
        if orientation == ORIENT_NONE and ref_state is not None and self.subtract_off:
            raise ValueError("DryAtmosModel: a hydrostatic reference state needs an orientation")
        self.viscosity, self.dynamic_viscosity = float(viscosity), bool(dynamic_viscosity)
        self.tau_hyper = hyperdiffusion_timescale
        self.sources = int(sources)
        self.boundary_conditions = tuple(boundary_conditions)
        has_or = orientation != ORIENT_NONE
        has_ref = ref_state is not None
        has_hyp = hyperdiffusion_timescale is not None
        o = 3
        self.off_phi = o
        o += 4 if has_or else 0
        self.off_ref = o
        o += 7 if has_ref else 0
        has_smag = self.C_smag is not None
        self.off_turb = o                      # turbulence.Delta (AtmosModel.jl:494-511 order)
        o += 1 if has_smag else 0
        self.off_delta = o
        o += 1 if has_hyp else 0
        self.off_moist = o
        o += 2
        self.off_tracers = o                   # tracers.delta_chi[NT]
        o += nt
        self.ns, self.naux = 5 + nt, o
        self.ngrad = 4 + (1 if has_smag else 0) + (4 if has_hyp else 0) + nt
        self.ngradflux = 9 + (1 if has_smag else 0) + 3 * nt
        self.ngradlap = 4 if has_hyp else 0
        self.nhyper = 12 if has_hyp else 0

    def descriptor(self):
        ps = self.ps
        ip = np.zeros(16, dtype=np.int32)
        ip[0] = self.orientation
        ip[1] = 1 if self.ref_state is not None else 0
        ip[2] = int(self.subtract_off)
        ip[3] = 0 if self.dynamic_viscosity else 1
        ip[4] = 1 if self.tau_hyper is not None else 0
        ip[5] = self.sources
        ip[6] = len(self.boundary_conditions)
        for i, bc in enumerate(self.boundary_conditions):
            ip[7 + i] = bc
        ip[14] = 1 if self.C_smag is not None else 0
        ip[15] = int(self.with_divergence) | (int(self.zero_enthalpy) << 1)
        dp = np.zeros(32)
        dp[0] = self.viscosity
        dp[1] = self.tau_hyper if self.tau_hyper is not None else 0.0
        dp[2:13] = [ps.R_d, ps.cp_d, ps.cv_d, ps.T_0, ps.grav, ps.Omega, ps.MSLP, ps.day,
                    ps.planet_radius, ps.inv_Pr_turb, ps.kappa_d]
        dp[13] = self.C_smag if self.C_smag is not None else 0.0
        if self.ntracers:       # NT in bits 8..15 of iparam[15], delta_chi[k] in dparam[16 + k]
            ip[15] |= self.ntracers << 8
            dp[16:16 + self.ntracers] = self.tracers.delta_chi
        return ip, dp

    def state_names(self):
        return (["ρ", "ρu[1]", "ρu[2]", "ρu[3]", "energy.ρe"]
                + ["tracers.ρχ[%d]" % (k + 1) for k in range(self.ntracers)])

    # -- init_state_auxiliary! (AtmosModel.jl:880-940) -------------------------------------
    def init_state_auxiliary(self, grid):
        ps = self.ps
        vg = grid.vgeo
        aux = np.zeros((grid.nelem, self.naux, grid.Np))
        x = [vg[:, c, :] for c in (G._x1, G._x2, G._x3)]
        for d in range(3):
            aux[:, d, :] = x[d]
        if self.orientation != ORIENT_NONE:
            if self.orientation == ORIENT_SPHERICAL:     # Orientations.jl:140-150
                phi = ps.grav * (np.sqrt(x[0] ** 2 + x[1] ** 2 + x[2] ** 2) - ps.planet_radius)
            else:                                         # FlatOrientation
                phi = ps.grav * x[2]
            aux[:, self.off_phi, :] = phi
            # auxiliary_field_gradient!: element-local strong gradient
            # (dgsem_auxiliary_field_gradient!, DGModel_kernels.jl:3097-3232)
            if _vertical_fvm(grid):
                # polynomialorder = (N_h, 0): the horizontal DG part, then the vertical finite-volume
                # difference incrementing (SpaceDiscretization.jl:413-481)
                gphi = G.auxiliary_field_gradient(grid, phi, 1)
                gphi += vert_fvm_auxiliary_field_gradient(grid, phi)
                aux[:, self.off_phi + 1:self.off_phi + 4, :] = gphi
            else:
                aux[:, self.off_phi + 1:self.off_phi + 4, :] = G.auxiliary_field_gradient(grid, phi)
        if isinstance(self.ref_state, IsentropicVortexReferenceState):
            self.ref_state.fill(ps, aux, self.off_ref)
        elif self.ref_state is not None:
            # ref_state_init_p_rho! and ref_state_finalize_init! (ref_state.jl:70-140).  The
            # reference additionally re-derives rho from a DG gradient of p (discrete
            # hydrostatic balance, :150-175); the synthetic state here keeps the analytic
            # rho = p / (R_d T_v) -- documented in DESIGN.md.
            z = aux[:, self.off_phi, :] / ps.grav
            Tv, p = self.ref_state(z)
            rho = p / (Tv * ps.R_d)
            if _vertical_fvm(grid):
                # atmos_init_aux! step 2 of a finite-volume vertical (ref_state.jl:160-166):
                # p_i - p_{i+1} = g (rho_{i+1} dz_{i+1} + rho_i dz_i) / 2 up every stack
                rho, p = fvm_balance(grid, rho, p, ps)
            T = p / (ps.R_d * rho)
            o = self.off_ref
            aux[:, o + 0, :] = rho
            aux[:, o + 1, :] = p
            aux[:, o + 2, :] = T
            aux[:, o + 3, :] = rho * (0.0 + aux[:, self.off_phi, :] + ps.cv_d * (T - ps.T_0))
        if self.C_smag is not None:
            # init_aux_turbulence!: Delta = lengthscale(geom) = 2 / (cbrt(det(invJ)) max(N))
            # (TurbulenceClosures.jl:431-438, Geometry.jl:121-122)
            m = [[vg[:, c, :] for c in row] for row in (
                (G._xi1x1, G._xi1x2, G._xi1x3), (G._xi2x1, G._xi2x2, G._xi2x3),
                (G._xi3x1, G._xi3x2, G._xi3x3))]
            det = (m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1])
                   - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0])
                   + m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]))
            aux[:, self.off_turb, :] = 2 / (np.cbrt(det) * max(max(1, n) for n in grid.N))
        if self.tau_hyper is not None:
            # lengthscale_horizontal (Geometry.jl:129-151): with invJ[i, j] = d xi_i / d x_j taken
            # from the xi-x columns of vgeo (LocalGeometry, Geometry.jl:78-85),
            #   Delta_1 = |invJ \ e_1| 2 / N_1,  Delta_2 = |invJ \ e_2| 2 / N_2.
            # (Not the stored x-xi columns: in this snapshot Metrics.jl:617-667 fills them with
            # adj * adj' / det, which is not the inverse, and nothing on this path reads them.
            # tests/test_hyperdiffusion_cross_law.py would see the difference.)
            N = grid.N
            invJ = np.stack([np.stack([vg[:, c] for c in row], axis=-1) for row in (
                (G._xi1x1, G._xi1x2, G._xi1x3), (G._xi2x1, G._xi2x2, G._xi2x3),
                (G._xi3x1, G._xi3x2, G._xi3x3))], axis=-2)          # (nelem, Np, 3, 3)
            J = np.linalg.inv(invJ)
            c1 = np.sqrt((J[..., :, 0] ** 2).sum(axis=-1))
            c2 = np.sqrt((J[..., :, 1] ** 2).sum(axis=-1))
            aux[:, self.off_delta, :] = (c1 * 2 / N[0] + c2 * 2 / N[1]) / 2
        for k in range(self.ntracers):       # atmos_init_aux!(::NTracers) (tracers.jl:133-140)
            aux[:, self.off_tracers + k, :] = self.tracers.delta_chi[k]
        return aux

    def rebalance_reference_state(self, grid, aux, gradp):
        """``ref_state_init_density_from_pressure!`` + ``ref_state_finalize_init!``
        (ref_state.jl:83-135) on the real elements: the density that balances the DG gradient
        of the reference pressure, then T and rho e consistent with (rho, p)."""
        ps, nr = self.ps, grid.nreal
        gP = aux[:nr, self.off_phi + 1:self.off_phi + 4, :]
        k = gP / ps.grav
        num = -(k[:, 0] * gradp[:nr, 0] + k[:, 1] * gradp[:nr, 1] + k[:, 2] * gradp[:nr, 2])
        den = k[:, 0] * gP[:, 0] + k[:, 1] * gP[:, 1] + k[:, 2] * gP[:, 2]
        rho = num / den
        o = self.off_ref
        p = aux[:nr, o + 1, :]
        T = p / (ps.R_d * rho)
        aux[:nr, o + 0, :] = rho
        aux[:nr, o + 2, :] = T
        aux[:nr, o + 3, :] = rho * (0.0 + aux[:nr, self.off_phi, :] + ps.cv_d * (T - ps.T_0))

    def init_state_prognostic(self, grid, aux, t):
        Q = np.zeros((grid.nelem, self.ns, grid.Np))
        coord = [aux[:, d, :] for d in range(3)]
        out = self.init_state(self, aux, coord, t)
        if len(out) != (4 if self.ntracers else 3):
            raise ValueError("DryAtmosModel: init_state of a model with %d tracers returns (rho, rhou, rhoe%s)"
                             % (self.ntracers, ", [rho chi[k]]" if self.ntracers else ""))
        rho, rhou, rhoe = out[:3]
        Q[:, 0, :] = rho
        for d in range(3):
            Q[:, 1 + d, :] = rhou[d]
        Q[:, 4, :] = rhoe
        if self.ntracers:
            if len(out[3]) != self.ntracers:
                raise ValueError("DryAtmosModel: init_state returned %d tracer fields for %d tracers"
                                 % (len(out[3]), self.ntracers))
            for k in range(self.ntracers):
                Q[:, 5 + k, :] = out[3][k]
        return Q


# ---- DGFVModel on the dry law: a finite-volume vertical, polynomialorder = (N_h, 0) ---------------
def _vertical_fvm(grid):
    return grid.dim == 3 and grid.N[2] == 0


def _stack_view(grid, a):
    """(nelem, ..., Np) as (nstack, nvertelem, ..., Np): elements are numbered up their stacks."""
    nv = int(grid.topology.stacksize)
    assert a.shape[0] % nv == 0
    return a.reshape((a.shape[0] // nv, nv) + a.shape[1:])


def vert_fvm_auxiliary_field_gradient(grid, a):
    """``vert_fvm_auxiliary_field_gradient!`` (DGFVModel_kernels.jl:946-1063) of a field ``a``
    (nelem, Np): the difference of the cells above and below over ``dz_top / 2 + dz + dz_bottom / 2``,
    one-sided through linear extrapolation at a boundary face, rotated back to Cartesian with the
    vertical metric terms.  Returns (nelem, 3, Np), to be added to the horizontal DG part."""
    vg = grid.vgeo
    nv = int(grid.topology.stacksize)
    periodic = bool(grid.topology.periodicstack)
    s, dzh = _stack_view(grid, a), _stack_view(grid, vg[:, G._JcV, :])
    top, bot = np.roll(s, -1, axis=1), np.roll(s, 1, axis=1)
    dzh_top, dzh_bot = np.roll(dzh, -1, axis=1), np.roll(dzh, 1, axis=1)
    if not periodic:
        assert nv >= 2
        bot[:, 0] = 2 * s[:, 0] - top[:, 0]
        dzh_bot[:, 0] = dzh_top[:, 0]
        top[:, -1] = 2 * s[:, -1] - bot[:, -1]
        dzh_top[:, -1] = dzh_bot[:, -1]
    dz = dzh_top + 2 * dzh + dzh_bot
    grad_v = ((top - bot) / dz).reshape(a.shape)
    out = np.zeros((a.shape[0], 3, a.shape[1]))
    for d, c in enumerate((G._xi3x1, G._xi3x2, G._xi3x3)):
        out[:, d, :] = vg[:, c, :] * vg[:, G._JcV, :] * grad_v
    return out


def fvm_balance(grid, rho, p, ps):
    """``fvm_balance!(fvm_balance_init!, ...)`` (DGFVModel_kernels.jl:1079-1149, ref_state.jl:265-285):
    walking each stack from its bottom cell, ``rho_i = rho_{i-1} (R_d T_{i-1} - g dz_{i-1} / 2) /
    (R_d T_i + g dz_i / 2)`` and ``p_i = R_d rho_i T_i`` with the virtual temperatures ``T = p /
    (R_d rho)`` of the state it is handed.  Returns the balanced ``(rho, p)``, (nelem, Np)."""
    nv = int(grid.topology.stacksize)
    r, q = _stack_view(grid, rho.copy()), _stack_view(grid, p.copy())
    dz = 2 * _stack_view(grid, grid.vgeo[:, G._JcV, :])
    R_d, grav = ps.R_d, ps.grav
    for i in range(1, nv):
        T_virt = q[:, i - 1] / (R_d * r[:, i - 1])
        top_T_virt = q[:, i] / (R_d * r[:, i])
        r[:, i] = r[:, i - 1] * (R_d * T_virt - grav * dz[:, i - 1] / 2) / (R_d * top_T_virt + grav * dz[:, i] / 2)
        q[:, i] = R_d * r[:, i] * top_T_virt
    return r.reshape(rho.shape), q.reshape(p.shape)


def prognostic_to_primitive(law, Q, aux):
    """``prognostic_to_primitive!`` of the ``DryModel`` (prog_prim_conversion.jl:67-78): ``Q``
    (..., 5, Np) to the primitives ``rho, u (3), p`` with the full pressure of the dry phase."""
    ps = law.ps
    rho = Q[..., 0, :]
    e_pot = aux[..., law.off_phi, :] if law.orientation != ORIENT_NONE else 0.0
    rhoe_kin = (Q[..., 1, :] ** 2 + Q[..., 2, :] ** 2 + Q[..., 3, :] ** 2) / rho / 2
    e_int = (Q[..., 4, :] - rhoe_kin - rho * e_pot) / rho
    T = ps.T_0 + e_int / ps.cv_d
    prim = np.empty_like(Q)
    prim[..., 0, :] = rho
    for d in range(3):
        prim[..., 1 + d, :] = Q[..., 1 + d, :] / rho
    prim[..., 4, :] = ps.R_d * rho * T
    return prim


def primitive_to_prognostic(law, prim, aux):
    """``primitive_to_prognostic!`` (prog_prim_conversion.jl:114-131): ``PhaseDry_rho_p``, ``T = p /
    (rho R_d)``, ``rho e = rho (cv_d (T - T_0) + |u|^2 / 2 + Phi)`` with ``Phi`` of ``aux``."""
    ps = law.ps
    rho, p = prim[..., 0, :], prim[..., 4, :]
    T = p / (ps.R_d * rho)
    e_kin = (prim[..., 1, :] ** 2 + prim[..., 2, :] ** 2 + prim[..., 3, :] ** 2) / 2
    e_pot = aux[..., law.off_phi, :] if law.orientation != ORIENT_NONE else 0.0
    Q = np.empty_like(prim)
    Q[..., 0, :] = rho
    for d in range(3):
        Q[..., 1 + d, :] = rho * prim[..., 1 + d, :]
    Q[..., 4, :] = rho * (ps.cv_d * (T - ps.T_0) + e_kin + e_pot)
    return Q


def construct_face_auxiliary_state(law, aux_cell, dz):
    """``construct_face_auxiliary_state!`` (prog_prim_conversion.jl:187-202): the copy, with ``Phi +
    g dz / 2`` under an orientation; ``dz`` is signed (negative towards the bottom face)."""
    aux_face = aux_cell.copy()
    if law.orientation != ORIENT_NONE:
        aux_face[..., law.off_phi, :] = aux_cell[..., law.off_phi, :] + law.ps.grav * dz / 2
    return aux_face


class HBFVReconstruction:
    """``HBFVReconstruction(atmos, reconstruction)`` (src/Atmos/Model/reconstructions.jl:15-73): the
    hydrostatic reference pressures of the stencil, built outward from the centre cell with ``rho g
    dz / 2`` of the cell weights, are taken off ``p`` before ``reconstruction`` (an ``FVConstant`` or
    ``FVLinear``) and ``p_ref +- rho g dz / 2`` of the centre cell is put back on the two face values.
    ``DGFVModel`` hands it to the library as ``reconstruction | FV_HYDROSTATIC``.  Called with primitive
    cell states ``(2 w + 1, 5, ...)`` and weights ``(2 w + 1, ...)`` it evaluates on the host like the inner object."""

    def __init__(self, model, reconstruction):
        self.model, self.reconstruction = model, reconstruction
        self.reconstruction_id = int(reconstruction.reconstruction_id) | 0x100
        self.width, self.limiter = reconstruction.width, reconstruction.limiter

    def __call__(self, cell_states, cell_weights):
        c = np.array(cell_states, dtype=np.float64)
        w = np.asarray(cell_weights, dtype=np.float64)
        D = c.shape[0]
        W = (D - 1) // 2
        grav = self.model.ps.grav
        half = c[:, 0] * grav * w / 2
        p_ref = c[W, 4].copy()
        c[W, 4] -= p_ref
        p_minus, p_plus = p_ref.copy(), p_ref.copy()
        for i in range(1, W + 1):
            p_minus = p_minus + (half[W - i + 1] + half[W - i])
            c[W - i, 4] -= p_minus
            p_plus = p_plus - (half[W + i - 1] + half[W + i])
            c[W + i, 4] -= p_plus
        bot, top = self.reconstruction(c, w)
        bot[4] += p_ref + half[W]
        top[4] += p_ref - half[W]
        return bot, top


class AtmosAcousticGravityLinearModel:
    """``AtmosAcousticGravityLinearModel(atmos)`` (src/Atmos/Model/linear.jl:249-345,
    linear_tendencies.jl) of a dry ``DryAtmosModel``: prognostic ``rho, rho u, rho e`` (the first
    five states of the full model), first-order fluxes ``rho u``, ``p_lin I`` and
    ``((rho e_ref + p_ref) / rho_ref) rho u`` with ``p_lin = rho R_d T_0 + R_d / cv_d (rho e -
    rho Phi)``, source ``-rho grad Phi`` (vertical and every direction), Rusanov wavespeed
    ``soundspeed(ref.T)``, ``AtmosBC()`` on every boundary.  It reads the full model's auxiliary
    state: build it as ``DGModel(linear, grid, direction=VerticalDirection,
    state_auxiliary=dg.state_auxiliary)``.  Device functor: csrc/physics_atmos_linear.h.

    Of a ``moist.MoistAtmosModel`` (``EquilMoist``, linear.jl:57-72) it carries the sixth state
    Of a model with tracers it carries none (AtmosModel.jl:399-406, linear.jl:104-112): five states,
    the leading ones of the full model, on the full model's wider auxiliary array; ``AdditiveRungeKutta``
    with the column solver steps such a pair, the tracers explicitly.

    ``rho q_tot`` (no flux, no source), ``p_lin`` gains ``- rho q_tot e_int_v0``, the auxiliary state
    is the moist model's 19 columns and the physics id is ``PHYSICS_MOIST_LINEAR_AG``."""
    physics_id = PHYSICS_ATMOS_LINEAR_AG

    def __init__(self, atmos):
        if atmos.physics_id == PHYSICS_MOIST_ATMOS:
            if atmos.no_orientation or atmos.ref_state is None:
                raise ValueError("AtmosAcousticGravityLinearModel needs a moist model with an "
                                 "orientation and a reference state (this one has no_orientation)")
            self.atmos = atmos
            self.ps = atmos.ps
            self.physics_id = PHYSICS_MOIST_LINEAR_AG
            self.off_phi, self.off_ref = atmos.off_phi, atmos.off_ref
            self.ns, self.naux = 6, atmos.naux
            self.ngrad = self.ngradflux = self.ngradlap = self.nhyper = 0
            return
        if atmos.ref_state is None:
            raise ValueError("AtmosAcousticGravityLinearModel needs a model with a reference state")
        if atmos.orientation == ORIENT_NONE:
            raise ValueError("AtmosAcousticGravityLinearModel needs a model with an orientation")
        self.atmos = atmos
        self.ps = atmos.ps
        self.off_phi, self.off_ref = atmos.off_phi, atmos.off_ref
        self.ns, self.naux = 5, atmos.naux
        self.ngrad = self.ngradflux = self.ngradlap = self.nhyper = 0

    def descriptor(self):
        return self.atmos.descriptor()

    def state_names(self):
        return self.atmos.state_names()[:self.ns]

    def init_state_auxiliary(self, grid):
        raise ValueError("AtmosAcousticGravityLinearModel shares the full model's auxiliary state: "
                         "pass state_auxiliary=dg.state_auxiliary")

    def init_state_prognostic(self, grid, aux, t):
        return np.zeros((grid.nelem, self.ns, grid.Np))


class AtmosAcousticLinearModel(AtmosAcousticGravityLinearModel):
    """``AtmosAcousticLinearModel(atmos)`` (src/Atmos/Model/linear.jl:214-245,
    linear_tendencies.jl:55-60) of a dry ``DryAtmosModel`` with ``ORIENT_NONE`` and a reference state
    (the isentropic vortex's): the acoustic-gravity model's fluxes with ``e_pot = 0`` -- ``rho u``,
    ``p_lin I`` with ``p_lin = rho R_d T_0 + R_d / cv_d rho e`` and ``((rho e_ref + p_ref) / rho_ref)
    rho u`` -- and no source.  It reads the full model's auxiliary state (reference state at
    ``off_ref = 3``) and works in any direction.  Device functor: csrc/physics_atmos_linear.h with
    ``ORIENT = false``, N = 4."""
    physics_id = PHYSICS_ATMOS_LINEAR_ACOUSTIC

    def __init__(self, atmos):
        if getattr(atmos, "ntracers", 0):
            raise ValueError("AtmosAcousticLinearModel: a model with tracers is not served")
        if atmos.physics_id != PHYSICS_DRY_ATMOS:
            raise ValueError("AtmosAcousticLinearModel: only the dry model is implemented (the moist "
                             "acoustic law is not)")
        if atmos.ref_state is None:
            raise ValueError("AtmosAcousticLinearModel needs a model with a reference state")
        if atmos.orientation != ORIENT_NONE:
            raise ValueError("AtmosAcousticLinearModel is implemented for ORIENT_NONE (e_pot = 0); with an "
                             "orientation use AtmosAcousticGravityLinearModel")
        if atmos.tau_hyper is not None or atmos.C_smag is not None:
            raise ValueError("AtmosAcousticLinearModel: the full model's auxiliary layout must be "
                             "coordinates, reference state, moisture (no hyperdiffusion, no Smagorinsky)")
        self.atmos = atmos
        self.ps = atmos.ps
        self.off_phi, self.off_ref = atmos.off_phi, atmos.off_ref
        self.ns, self.naux = 5, atmos.naux
        self.ngrad = self.ngradflux = self.ngradlap = self.nhyper = 0
