"""Host-side mirror of the dry atmosphere of the reference's entropy-stable DG tests.

Reference: ``test/Numerics/ESDGMethods/DryAtmos/DryAtmos.jl`` -- ``DryAtmosModel`` ``:48-74``, the
orientations' geopotential ``:130-154``, ``DryReferenceState`` ``:170-196``, the entropy transforms
``:339-409``, the sources ``:542-561`` and ``:801-810``, the two-point flux types ``:485-539`` and
``:564-621``; ``EntropyConservative`` is ``src/Numerics/DGMethods/NumericalFluxes.jl:410-414``.  The
reference's compile-time settings are fixed as they stand there: ``total_energy = false`` and
``fluctuation_gravity = false``.  The device functor is ``csrc/physics_esdg_dryatmos.h``; the operator is
``dgmodel.ESDGModel``.

State ``rho, rho u[3], rho e``; auxiliary ``Phi, grad Phi[3]`` and, with a ``DryReferenceState``,
``ref_state.T, p, rho, rho e``.  Arrays are ``(nelem, nstate, Np)`` as everywhere in this package.
"""
import numpy as np

from .atmos import PlanetParameters
from .mesh.grids import _x1, _x2, _x3
from .mesh.topologies import equiangular_cubed_sphere_warp

PHYSICS_ESDG_DRY_ATMOS = 12
PHYSICS_ESDG_DRY_ATMOS_LINEAR_AG = 14

__all__ = ["DryAtmosModel", "FlatOrientation", "SphericalOrientation", "Coriolis", "Gravity",
           "DryReferenceState", "EntropyConservative", "CentralVolumeFlux", "KGVolumeFlux",
           "RusanovNumericalFlux", "EntropyConservativeWithPenalty", "MatrixFlux",
           "state_to_entropy_variables", "entropy_variables_to_state", "state_to_entropy", "pressure",
           "totalenergy", "soundspeed", "gamma", "DryAtmosAcousticGravityLinearModel", "BaroclinicWave",
           "cubedshellwarp", "sphr_to_cart_vec"]

# ``cubedshellwarp`` of DryAtmos.jl:827-860 is ``cubed_sphere_warp(EquiangularCubedSphere(), ...)``
# (Topologies.jl:1253-1298) restated: the same ``tan(pi xi / 4)`` map, the same face branches in the
# same order, ``R = max(|a|, |b|, |c|)`` by default.
cubedshellwarp = equiangular_cubed_sphere_warp


class FlatOrientation:
    orientation_id = 0


class SphericalOrientation:
    orientation_id = 1


class Coriolis:
    source_id = 1


class Gravity:
    source_id = 2


class DryReferenceState:
    """``DryReferenceState(temperature_profile)``: the profile maps an altitude to ``(T, p)``
    (``atmos.DecayingTemperatureProfile`` and its kin)."""

    def __init__(self, temperature_profile):
        self.temperature_profile = temperature_profile


# ---- two-point fluxes (ids of include/cmdg.h CMDG_ESDG_FLUX_*) -----------------------------------
class _Flux:
    Mcut, low_mach, kinetic_energy_preserving = 0.0, False, False


class EntropyConservative(_Flux):
    flux_id, volume, surface = 1, True, True


class CentralVolumeFlux(_Flux):
    flux_id, volume, surface = 2, True, False


class KGVolumeFlux(_Flux):
    flux_id, volume, surface = 3, True, False


class RusanovNumericalFlux(_Flux):
    flux_id, volume, surface = 4, False, True


class EntropyConservativeWithPenalty(_Flux):
    flux_id, volume, surface = 5, False, True


class MatrixFlux(_Flux):
    """``MatrixFlux(Mcut = 0, low_mach = false, kinetic_energy_preserving = false)``."""
    flux_id, volume, surface = 6, False, True

    def __init__(self, Mcut=0.0, low_mach=False, kinetic_energy_preserving=False):
        self.Mcut, self.low_mach = float(Mcut), bool(low_mach)
        self.kinetic_energy_preserving = bool(kinetic_energy_preserving)


# ---- pointwise functions, dtype-generic (DryAtmos.jl:245-280, :339-409) ----------------------------
def gamma(ps=None, dtype=np.float64):
    ps = ps or PlanetParameters()
    return dtype(ps.cp_d) / dtype(ps.cv_d)


def pressure(rho, rhou, rhoe, g):
    return (g - 1) * (rhoe - (rhou[0] * rhou[0] + rhou[1] * rhou[1] + rhou[2] * rhou[2]) / (2 * rho))


def totalenergy(rho, rhou, p, g):
    return p / (g - 1) + (rhou[0] * rhou[0] + rhou[1] * rhou[1] + rhou[2] * rhou[2]) / (2 * rho)


def soundspeed(rho, p, g):
    return np.sqrt(g * p / rho)


def state_to_entropy_variables(Q, g=None):
    """``state_to_entropy_variables!``: ``Q (..., 5, Np)`` -> ``(..., 6, Np)``."""
    Q = np.asarray(Q)
    g = gamma(dtype=Q.dtype.type) if g is None else g
    rho, rhou, rhoe = Q[..., 0, :], [Q[..., 1 + d, :] for d in range(3)], Q[..., 4, :]
    p = pressure(rho, rhou, rhoe, g)
    s = np.log(p / rho ** g)
    b = rho / (2 * p)
    u = [m / rho for m in rhou]
    ent = [(g - s) / (g - 1) - (u[0] * u[0] + u[1] * u[1] + u[2] * u[2]) * b]
    ent += [2 * b * u[d] for d in range(3)]
    ent += [-2 * b, 2 * rho * b]
    return np.stack(ent, axis=-2)


def entropy_variables_to_state(ent, g=None):
    """``entropy_variables_to_state!``: ``(..., 6, Np)`` -> state ``(..., 5, Np)`` and ``Phi (..., Np)``."""
    ent = np.asarray(ent)
    g = gamma(dtype=ent.dtype.type) if g is None else g
    b = -ent[..., 4, :] / 2
    rho = ent[..., 5, :] / (2 * b)
    rhou = [rho * ent[..., 1 + d, :] / (2 * b) for d in range(3)]
    p = rho / (2 * b)
    s = np.log(p / rho ** g)
    uu = rhou[0] * rhou[0] + rhou[1] * rhou[1] + rhou[2] * rhou[2]
    Phi = uu / (2 * rho ** 2) - ((g - s) / (g - 1) - ent[..., 0, :]) / (2 * b)
    rhoe = p / (g - 1) + uu / (2 * rho) + rho * Phi
    return np.stack([rho] + rhou + [rhoe], axis=-2), Phi


def state_to_entropy(Q, g=None):
    """``state_to_entropy``: ``eta = -rho s / (gamma - 1)``, ``(..., Np)``."""
    Q = np.asarray(Q)
    g = gamma(dtype=Q.dtype.type) if g is None else g
    rho = Q[..., 0, :]
    p = pressure(rho, [Q[..., 1 + d, :] for d in range(3)], Q[..., 4, :], g)
    return -rho * np.log(p / rho ** g) / (g - 1)


class DryAtmosModel:
    """``DryAtmosModel{dim}(orientation, problem; ref_state, sources)``.  ``problem`` supplies
    ``init_state_prognostic(coord, aux)`` on the host: ``coord`` is the list of the three coordinate
    arrays ``(nelem, Np)``, ``aux`` the auxiliary array, the result ``(nelem, 5, Np)``."""
    physics_id = PHYSICS_ESDG_DRY_ATMOS
    ns, ngrad, ngradflux, ngradlap, nhyper = 5, 0, 0, 0, 0
    nentropy = 6

    def __init__(self, orientation, problem, ref_state=None, sources=(), param_set=None):
        self.orientation, self.problem, self.ref_state = orientation, problem, ref_state
        self.sources = tuple(sources)
        if len(self.sources) > 2:
            raise ValueError("DryAtmosModel: at most two sources (Coriolis, Gravity)")
        self.param_set = param_set or PlanetParameters()
        self.naux = 4 + (4 if ref_state is not None else 0)

    @property
    def gamma(self):
        return gamma(self.param_set)

    def descriptor(self):
        ps = self.param_set
        ip = np.zeros(16, dtype=np.int32)
        ip[0] = self.orientation.orientation_id
        ip[1] = int(self.ref_state is not None)
        ip[2] = len(self.sources)
        for i, s in enumerate(self.sources):
            ip[3 + i] = s.source_id
        dp = np.zeros(32)
        dp[2:13] = [ps.R_d, ps.cp_d, ps.cv_d, ps.T_0, ps.grav, ps.Omega, ps.MSLP, ps.day,
                    ps.planet_radius, ps.inv_Pr_turb, ps.kappa_d]
        return ip, dp

    def init_state_auxiliary(self, grid):
        """``nodal_init_state_auxiliary!``: orientation, then reference state (:100-196)."""
        ps = self.param_set
        x = [grid.vgeo[:, c, :] for c in (_x1, _x2, _x3)]
        aux = np.zeros((grid.nelem, self.naux, grid.Np))
        if self.orientation.orientation_id == 0:
            aux[:, 0, :] = ps.grav * x[2]
            aux[:, 3, :] = ps.grav
            z = x[2]
        else:
            r = np.sqrt(x[0] ** 2 + x[1] ** 2 + x[2] ** 2)
            aux[:, 0, :] = ps.grav * r
            for d in range(3):
                aux[:, 1 + d, :] = ps.grav * x[d] / r
            z = r - ps.planet_radius
        if self.ref_state is not None:
            T, p = self.ref_state.temperature_profile(z)
            rho = p / (ps.R_d * T)
            zero = np.zeros_like(rho)
            aux[:, 4, :], aux[:, 5, :], aux[:, 6, :] = T, p, rho
            aux[:, 7, :] = totalenergy(rho, [zero, zero, zero], p, self.gamma)
        return aux

    def init_state_prognostic(self, grid, aux, t=0.0):
        coord = [grid.vgeo[:, c, :] for c in (_x1, _x2, _x3)]
        return np.ascontiguousarray(self.problem.init_state_prognostic(coord, aux), dtype=np.float64)


class DryAtmosAcousticGravityLinearModel:
    """``DryAtmosAcousticGravityLinearModel(atmos)`` (test/Numerics/ESDGMethods/DryAtmos/linear.jl) of
    a ``DryAtmosModel`` with a reference state: prognostic ``rho, rho u, rho e``, first-order fluxes
    ``rho u``, ``pL I`` with ``pL = (gamma - 1) rho e`` and ``((ref.rho e + ref.p) / ref.rho) rho u``,
    source ``rho u -= rho grad Phi``, ``rho e -= rho u . grad Phi`` (vertical and every direction), Rusanov
    wavespeed ``soundspeed(ref.rho, ref.p)``, the full model's wall on tags 1 and 2.  It reads the full
    model's auxiliary state: build it as ``DGModel(linear, grid, RusanovNumericalFlux,
    direction=VerticalDirection, state_auxiliary=esdg_model.state_auxiliary)``.  Device functor:
    csrc/physics_esdg_dryatmos_linear.h."""
    physics_id = PHYSICS_ESDG_DRY_ATMOS_LINEAR_AG
    ns, ngrad, ngradflux, ngradlap, nhyper = 5, 0, 0, 0, 0

    def __init__(self, atmos):
        if atmos.ref_state is None:
            raise ValueError("DryAtmosAcousticGravityLinearModel needs a model with a reference state")
        self.atmos = atmos
        self.param_set = atmos.param_set
        self.naux = atmos.naux

    def descriptor(self):
        return self.atmos.descriptor()

    def init_state_auxiliary(self, grid):
        raise ValueError("DryAtmosAcousticGravityLinearModel shares the full model's auxiliary state: "
                         "pass state_auxiliary=esdg_model.state_auxiliary")

    def init_state_prognostic(self, grid, aux, t=0.0):
        return np.zeros((grid.nelem, self.ns, grid.Np))


def sphr_to_cart_vec(vec, lat, lon):
    """``sphr_to_cart_vec`` of baroclinic_wave.jl:38-48."""
    slat, clat = np.sin(lat), np.cos(lat)
    slon, clon = np.sin(lon), np.cos(lon)
    return [-slon * vec[0] - slat * clon * vec[1] + clat * clon * vec[2],
            clon * vec[0] - slat * slon * vec[1] + clat * slon * vec[2],
            clat * vec[1] + slat * vec[2]]


class BaroclinicWave:
    """``BaroclinicWave()`` of test/Numerics/ESDGMethods/DryAtmos/baroclinic_wave.jl:50-178: the
    deep-atmosphere baroclinic wave (``q_0 = 0``), the reference's expressions in their order, on
    the host."""

    def __init__(self, param_set=None):
        self.param_set = param_set or PlanetParameters()

    def base_state(self, coord):
        """``(lam, phi, z, T_v, p, u_ref)`` at the nodes."""
        ps = self.param_set
        _grav, _R_d, _Omega, _a, _p_0 = ps.grav, ps.R_d, ps.Omega, ps.planet_radius, ps.MSLP
        k, T_E, T_P = 3.0, 310.0, 240.0
        T_0 = 0.5 * (T_E + T_P)
        Gamma = 0.005
        A = 1 / Gamma
        B = (T_0 - T_P) / T_0 / T_P
        Cc = 0.5 * (k + 2) * (T_E - T_P) / T_E / T_P
        b = 2.0
        H = _R_d * T_0 / _grav
        x1, x2, x3 = coord
        nrm = np.sqrt(x1 * x1 + x2 * x2 + x3 * x3)
        lam = np.arctan2(x2, x1)
        phi = np.arcsin(x3 / nrm)
        z = nrm - _a
        g = 1.0        # deep atmosphere
        zbH = z / b / H
        tau_z_1 = np.exp(Gamma * z / T_0)
        tau_z_2 = 1 - 2 * (zbH * zbH)
        tau_z_3 = np.exp(-(zbH * zbH))
        tau_1 = 1 / T_0 * tau_z_1 + B * tau_z_2 * tau_z_3
        tau_2 = Cc * tau_z_2 * tau_z_3
        tau_int_1 = A * (tau_z_1 - 1) + B * z * tau_z_3
        tau_int_2 = Cc * z * tau_z_3
        cz = np.cos(phi) * (1 + g * z / _a)
        I_T = cz ** k - k / (k + 2) * cz ** (k + 2)
        T_v = 1 / (tau_1 - tau_2 * I_T)
        p = _p_0 * np.exp(-_grav / _R_d * (tau_int_1 - tau_int_2 * I_T))
        U = _grav * k / _a * tau_int_2 * T_v * (cz ** (k - 1) - cz ** (k + 1))
        oc = _Omega * (_a + g * z) * np.cos(phi)
        u_ref = -oc + np.sqrt(oc * oc + (_a + g * z) * np.cos(phi) * U)
        return lam, phi, z, T_v, p, u_ref

    def perturbation(self, lam, phi, z):
        """``(u', v', d)``: zero unless ``0 < d < d_0``."""
        _a = self.param_set.planet_radius
        z_t, lam_c, phi_c, d_0, V_p = 15e3, np.pi / 9, 2 * np.pi / 9, _a / 6, 1.0
        zz = z / z_t
        F_z = np.where(z > z_t, 0.0, 1 - 3 * (zz * zz) + 2 * (zz * zz * zz))
        d = _a * np.arccos(np.sin(phi) * np.sin(phi_c) + np.cos(phi) * np.cos(phi_c) * np.cos(lam - lam_c))
        c1 = np.cos(np.pi * d / 2 / d_0)
        c3 = c1 * c1 * c1
        s1 = np.sin(np.pi * d / 2 / d_0)
        inside = (0 < d) & (d < d_0) & (d != _a * np.pi)
        with np.errstate(divide="ignore", invalid="ignore"):
            up = (-16 * V_p / 3 / np.sqrt(3.0) * F_z * c3 * s1
                  * (-np.sin(phi_c) * np.cos(phi) + np.cos(phi_c) * np.sin(phi) * np.cos(lam - lam_c))
                  / np.sin(d / _a))
            vp = 16 * V_p / 3 / np.sqrt(3.0) * F_z * c3 * s1 * np.cos(phi_c) * np.sin(lam - lam_c) / np.sin(d / _a)
        return np.where(inside, up, 0.0), np.where(inside, vp, 0.0), d

    def init_state_prognostic(self, coord, aux):
        ps = self.param_set
        lam, phi, z, T_v, p, u_ref = self.base_state(coord)
        up, vp, _ = self.perturbation(lam, phi, z)
        zero = np.zeros_like(z)
        u_cart = sphr_to_cart_vec([u_ref + up, zero + vp, zero + zero], phi, lam)
        T = T_v
        rho = p / (ps.R_d * T)
        e_kin = 0.5 * (u_cart[0] * u_cart[0] + u_cart[1] * u_cart[1] + u_cart[2] * u_cart[2])
        e_int = ps.cv_d * T
        return np.stack([rho] + [rho * u for u in u_cart] + [rho * (e_int + e_kin)], axis=1)
