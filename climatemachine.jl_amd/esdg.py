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

PHYSICS_ESDG_DRY_ATMOS = 12

__all__ = ["DryAtmosModel", "FlatOrientation", "SphericalOrientation", "Coriolis", "Gravity",
           "DryReferenceState", "EntropyConservative", "CentralVolumeFlux", "KGVolumeFlux",
           "RusanovNumericalFlux", "EntropyConservativeWithPenalty", "MatrixFlux",
           "state_to_entropy_variables", "entropy_variables_to_state", "state_to_entropy", "pressure",
           "totalenergy", "soundspeed", "gamma"]


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
