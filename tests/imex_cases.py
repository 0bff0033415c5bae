"""Grids, laws and fields shared by the IMEX tests (tests/test_gpu_imex.py,
tests/test_gpu_imex_oracle.py, tests/test_imex_oracle.py): the acoustic-wave case of
acousticwave_1d_imex.jl, the small Held-Suarez-like sphere, a flat stacked brick, reference
states and smooth perturbations."""
import numpy as np

VERTICAL, HORIZONTAL, EVERY = 2, 1, 0
# acousticwave_1d_imex.jl:65, expected_result[Float64]
ACOUSTIC_GOLDEN = 9.5073452847149594e+13


class AcousticWaveSetup:
    """``AcousticWaveSetup{Float64}()`` (acousticwave_1d_imex.jl:284-317): domain height 10 km,
    T_ref 300 K, alpha 3, gamma 100, nv 1; the passive tracer is not carried (see the golden test)."""

    def __init__(self, ps, domain_height=10e3, T_ref=300.0, alpha=3.0, gamma=100.0, nv=1):
        self.ps, self.H, self.T_ref, self.alpha, self.gamma, self.nv = ps, domain_height, T_ref, alpha, gamma, nv

    def __call__(self, law, aux, coord, t):
        ps = self.ps
        x, y, z3 = coord
        lam = np.arctan2(y, x)
        phi = np.arcsin(z3 / np.sqrt(x * x + y * y + z3 * z3))
        z = aux[:, law.off_phi, :] / ps.grav
        beta = np.minimum(1.0, self.alpha * np.arccos(np.cos(phi) * np.cos(lam)))
        f = (1 + np.cos(np.pi * beta)) / 2
        g = np.sin(self.nv * np.pi * z / self.H)
        p = aux[:, law.off_ref + 1, :] + self.gamma * f * g
        rho = p / (ps.R_d * self.T_ref)                       # PhaseDry_pT
        e_int = ps.cv_d * (self.T_ref - ps.T_0)
        e_pot = aux[:, law.off_phi, :]
        zero = 0.0 * rho
        return rho, [zero, zero, zero], rho * (e_int + e_pot)


def acoustic_setup(cm, n_horz=10, n_vert=5, N=5):
    M, A = cm.mesh, cm.atmos
    ps = A.PlanetParameters()
    a = ps.planet_radius
    topl = M.StackedCubedSphereTopology(n_horz, np.linspace(a, a + 10e3, n_vert + 1), boundary=(1, 2))
    grid = M.DiscontinuousSpectralElementGrid(topl, N, meshwarp=M.equiangular_cubed_sphere_warp)
    law = A.DryAtmosModel(AcousticWaveSetup(ps), orientation=A.ORIENT_SPHERICAL,
                          ref_state=A.IsothermalProfile(ps, 300.0), viscosity=0.0,
                          dynamic_viscosity=True, sources=A.SRC_GRAVITY,
                          boundary_conditions=(A.BC_ATMOS_DEFAULT, A.BC_ATMOS_DEFAULT), param_set=ps,
                          discrete_hydrostatic_balance=True)
    return law, grid


def make_pair(cm, law, grid):
    dg = cm.dgmodel.DGModel(law, grid, direction=0)
    lin = cm.dgmodel.DGModel(cm.atmos.AtmosAcousticGravityLinearModel(law), grid, direction=VERTICAL,
                             state_auxiliary=dg.state_auxiliary)
    return dg, lin


def small_sphere(cm, N=4, hyper=False, smag=False, nvert=3):
    """2 x 2 x 6 x nvert stacked cubed sphere, 30 km deep, the full law with viscosity 0, Gravity,
    a reference state; ``hyper``: DryBiharmonic(8 h) (NAUX 17), ``smag``: SmagorinskyLilly (NAUX
    17, the extra column in another place)."""
    M, A = cm.mesh, cm.atmos
    ps = A.PlanetParameters()
    a = ps.planet_radius
    topl = M.StackedCubedSphereTopology(2, np.linspace(a, a + 30e3, nvert + 1), boundary=(1, 2))
    grid = M.DiscontinuousSpectralElementGrid(topl, N, meshwarp=M.equiangular_cubed_sphere_warp)
    law = A.DryAtmosModel(A.HeldSuarezSetup(ps), orientation=A.ORIENT_SPHERICAL,
                          ref_state=A.DecayingTemperatureProfile(ps, 290.0, 220.0, 8e3), viscosity=0.0,
                          hyperdiffusion_timescale=8 * 3600.0 if hyper else None,
                          smagorinsky=ps.C_smag if smag else None,
                          sources=A.SRC_GRAVITY, boundary_conditions=(A.BC_ATMOS_DEFAULT, A.BC_ATMOS_DEFAULT),
                          param_set=ps)
    return law, grid


def flat_brick(cm, N=4, nx=3, ny=2, nvert=4, hyper=False, smag=False, periodic=False):
    """nx x ny x nvert stacked brick (1 km x 1 km x 2.5 km elements, walls on every side unless
    ``periodic``), FlatOrientation, the full law with viscosity 0, Gravity and a dry-adiabatic
    reference state; ``periodic`` makes the stacks vertically periodic as well."""
    M, A = cm.mesh, cm.atmos
    ps = A.PlanetParameters()
    rng = [np.linspace(0.0, 1e3 * nx, nx + 1), np.linspace(0.0, 1e3 * ny, ny + 1),
           np.linspace(0.0, 2.5e3 * nvert, nvert + 1)]
    per = (True, True, True) if periodic else (False, False, False)
    bnd = ((0, 0), (0, 0), (0, 0)) if periodic else ((1, 2), (1, 2), (1, 2))
    topl = M.StackedBrickTopology(rng, periodicity=per, boundary=bnd)
    grid = M.DiscontinuousSpectralElementGrid(topl, N)
    setup = A.RisingBubbleSetup(ps, xc=500.0 * nx, zc=500.0 * nvert, rc=400.0 * nx)
    law = A.DryAtmosModel(setup, orientation=A.ORIENT_FLAT,
                          ref_state=A.DryAdiabaticProfile(ps, 300.0, 0.0), viscosity=0.0,
                          hyperdiffusion_timescale=8 * 3600.0 if hyper else None,
                          smagorinsky=ps.C_smag if smag else None,
                          sources=A.SRC_GRAVITY, boundary_conditions=(A.BC_ATMOS_DEFAULT, A.BC_ATMOS_DEFAULT),
                          param_set=ps)
    return law, grid


def ref_state(law, aux):
    """Q0 = the reference state at rest."""
    Q0 = np.zeros((aux.shape[0], 5, aux.shape[2]))
    Q0[:, 0] = aux[:, law.off_ref]
    Q0[:, 4] = aux[:, law.off_ref + 3]
    return Q0


def smooth_perturbation(grid, aux, seed=3):
    rng = np.random.default_rng(seed)
    x = [aux[:, d, :] / 6.4e6 for d in range(3)]
    r = np.sqrt(x[0] ** 2 + x[1] ** 2 + x[2] ** 2)
    zeta = (r * 6.4e6 - 6.371e6) / 30e3               # 0 at the bottom wall, 1 at the top
    out = np.zeros((aux.shape[0], 5, aux.shape[2]))
    for s in range(5):
        c = rng.uniform(0.5, 1.5, 6)
        out[:, s] = (np.sin(c[0] * 3 * x[0] + c[1]) * np.cos(c[2] * 2 * x[1] + c[3])
                     * np.sin(c[4] * 4 * zeta + c[5]))
    # rho u tangential at the bottom and top walls: the radial part fades out there
    rhat = [xd / r for xd in x]
    un = sum(out[:, 1 + d] * rhat[d] for d in range(3))
    fade = np.sin(np.pi * np.clip(zeta, 0.0, 1.0))
    for d in range(3):
        out[:, 1 + d] += (fade - 1.0) * un * rhat[d]
    return out


def column_nodes(grid, nvert, column):
    """(element, node) of every matrix row of one column, rows ordered (state, k, v) -> n."""
    Nq, Nqv = grid.N[0] + 1, grid.N[2] + 1
    nqh2 = Nq * Nq
    h, ij = divmod(column, nqh2)
    rows = []
    for v in range(nvert):
        for k in range(Nqv):
            for s in range(5):
                rows.append((h * nvert + v, s, ij + nqh2 * k))
    return rows


def band_to_dense(band, p, q):
    P, n = band.shape
    A = np.zeros((n, n))
    for col in range(n):
        for d in range(P):
            row = col + d - q
            if 0 <= row < n:
                A[row, col] = band[d, col]
    return A


def wall_perturbation(law, aux, normal=False, seed=3):
    """A smooth perturbation of (rho, rho u, rho e) of unit size on any oriented grid: products of
    sines of the scaled coordinates and of the height.  Without ``normal`` the momentum's
    vertical part fades to zero at the bottom and top walls (tangential there); with it the
    vertical momentum stays, so the free-slip reflection of the wall faces is exercised."""
    rng = np.random.default_rng(seed)
    x = [aux[:, d, :] / max(np.abs(aux[:, d, :]).max(), 1.0) for d in range(3)]
    g = law.ps.grav
    z = aux[:, law.off_phi, :] / g
    zeta = (z - z.min()) / (z.max() - z.min())
    k = [aux[:, law.off_phi + 1 + d, :] / g for d in range(3)]
    out = np.zeros((aux.shape[0], 5, aux.shape[2]))
    for s in range(5):
        c = rng.uniform(0.5, 1.5, 6)
        out[:, s] = (np.sin(c[0] * 3 * x[0] + c[1]) * np.cos(c[2] * 2 * x[1] + c[3])
                     * np.sin(c[4] * 4 * zeta + c[5]))
    if not normal:
        un = sum(out[:, 1 + d] * k[d] for d in range(3))
        fade = np.sin(np.pi * np.clip(zeta, 0.0, 1.0))
        for d in range(3):
            out[:, 1 + d] += (fade - 1.0) * un * k[d]
    return out


# the size of each state of a perturbation around the atmosphere's rest state
STATE_SCALE = np.array([1e-3, 1.0, 1.0, 1.0, 1e2])


# rho, rho u (one vector state: in VerticalDirection on a flat grid its horizontal components
# are zero up to rounding), rho e
STATES = ((0,), (1, 2, 3), (4,))


def per_state_rel(a, b, states=STATES):
    """max over the states of max|a_s - b_s| / max|b_s|: every state against its own max-norm
    (``a``, ``b``: ``(nelem, 5, Np)``), so that rho e does not hide rho and rho u."""
    return max(per_state_errors(a, b, states))


def per_state_errors(a, b, states=STATES):
    out = []
    for s in states:
        s = list(s)
        out.append(float(np.abs(a[:, s] - b[:, s]).max() / max(np.abs(b[:, s]).max(), 1e-300)))
    return out


def oracle_pair(O, law, grid, state_auxiliary=None, nf_first=0, lin_nf=0, lin_direction=VERTICAL,
                full_direction=EVERY, diffusion_direction=None):
    """The oracle full model and its linear model on the same auxiliary array."""
    from cmdg_loader import cm
    full = O.OracleDGModel(law, grid, nf_first=nf_first, direction=full_direction,
                           diffusion_direction=diffusion_direction, state_auxiliary=state_auxiliary)
    lin = O.OracleDGModel(cm.atmos.AtmosAcousticGravityLinearModel(law), grid, nf_first=lin_nf,
                          direction=lin_direction, state_auxiliary=full.state_auxiliary)
    return full, lin
