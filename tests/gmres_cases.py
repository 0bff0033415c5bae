"""Grids, laws and drivers shared by the GMRES tests (tests/test_gmres_host.py,
tests/test_gpu_gmres.py, tests/test_gpu_gmres_steppers.py): the isentropic vortex of
isentropicvortex_imex.jl / isentropicvortex_mrigark_implicit.jl (dims = 2, run as the z-invariant
slice of a one-element-deep periodic extrusion, DESIGN.md "dim = 2": mass-weighted norms carry the
factor sqrt(Lz), an unweighted dot scales every GMRES norm alike), its no-orientation acoustic
linear model, and the oracle twin of that model.

The oracle has no no-orientation linear law.  The same numbers come from its acoustic-gravity law on
a twin model with ``ORIENT_FLAT`` and ``grav = 0``: then Phi = 0, grad Phi = 0 and the source is 0,
and the reference-state columns hold the same values (so the same ``h_ref``)."""
import json
import math
import os

import numpy as np

GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden",
                                   "isentropicvortex_implicit_values.json")))
EVERY, HORIZONTAL, VERTICAL = 0, 1, 2

# Differences measured on the MI355X, each a per-state relative Linf (every state against its own
# max-norm) unless said otherwise; the tests assert a fixed multiple of them.
MEASURED = {
    # The device solve against the restatement on the oracle operator, 2 x 2 x 1 brick, rtol = 1e-8,
    # (acoustic Courant, M) = (1, 10), (4, 10), (1, 3), (4, 3): 33, 110, 36 and 129 iterations on both
    # sides; the solution differs by 3.5e-16, 6.9e-16, 3.5e-16, 9.5e-16.  The two sides differ in the
    # summation order of fp64 dots over 2 500 terms.  Asserted: 10 x.
    "solve": 9.5e-16,
    # ... and the residual norm |g0[j+1]| of the last iteration, relative: 2.3e-10, 6.5e-11, 2.4e-10,
    # 6.5e-9.  It is rtol = 1e-8 of |r0|, so a rounding of a few eps |r0| in the recurrence is a few
    # 1e-8 of it.  Asserted: 10 x.
    "residual_norm": 6.6e-9,
    # Three ARK2GKC steps through GMRES against the restatement chain, the increment: 5.0e-13 (split
    # off), 1.5e-11 (split on: the explicit tendency is a difference of two evaluations).  Asserted: 10 x.
    "ark": 1.5e-11,
    # GMRES (M = 30, rtol = 1e-12) against the column LU on the small Held-Suarez sphere at vertical
    # acoustic Courant 2.  One solve: 2.0e-14 after 1 110 iterations for a model state as right-hand
    # side, 3.3e-11 after 750 for white noise.  ARK2GKC after 1 and 3 steps, the increment: at most
    # 1.8e-11 (split off, 810 to 1 050 iterations per solve) and 1.6e-10 (split on, 330 to 570).
    # Asserted: 100 x, at most 1e-8.
    "lu_solve": {"state": 2.0e-14, "random": 3.3e-11}, "lu_ark": 1.6e-10,
}


def soundspeed(ps, T):
    return math.sqrt(ps.cp_d / ps.cv_d * ps.R_d * T)


def vortex_law(cm, ref=True, twin=False):
    """The dry law of the two reference tests (NoOrientation, IsentropicVortexReferenceState,
    ConstantDynamicViscosity(0), no sources), or the oracle twin of its reference state."""
    A = cm.atmos
    if twin:
        class NoGravity(A.PlanetParameters):
            grav = 0.0
        ps = NoGravity()
    else:
        ps = A.PlanetParameters()
    setup = A.IsentropicVortexSetup(ps)
    return A.DryAtmosModel(setup, orientation=A.ORIENT_FLAT if twin else A.ORIENT_NONE,
                           ref_state=A.IsentropicVortexReferenceState(setup) if ref else None,
                           viscosity=0.0, dynamic_viscosity=True, sources=0, boundary_conditions=(),
                           param_set=ps)


def vortex_grid(cm, numelems, N=4):
    """Periodic brick of ``numelems`` (x, y) elements over the vortex's domain, one element deep."""
    M = cm.mesh
    L = cm.atmos.IsentropicVortexSetup(cm.atmos.PlanetParameters()).domain_halflength
    Lz = min(2 * L / n for n in numelems)
    rng = [np.linspace(-L, L, n + 1) for n in numelems] + [np.array([0.0, Lz])]
    topl = M.BrickTopology(rng, periodicity=(True,) * 3, connectivity="face")
    return M.DiscontinuousSpectralElementGrid(topl, N), Lz


def vortex_setup(cm, level=1, mri=False, N=4):
    """-> (law, grid, dt, nsteps, timeend, sqrt(Lz)) of level ``level`` of isentropicvortex_imex.jl
    (``mri``: of isentropicvortex_mrigark_implicit.jl, dt a fifth)."""
    law = vortex_law(cm)
    setup = law.init_state
    n = 2 ** (level - 1) * 5
    grid, Lz = vortex_grid(cm, (n, n), N)
    timeend = 2 * setup.domain_halflength / setup.translation_speed
    elementsize = 2 * setup.domain_halflength / n
    dt = elementsize / soundspeed(law.ps, setup.T_inf) / N ** 2
    if mri:
        dt = dt / 5
    nsteps = int(math.ceil(timeend / dt))
    return law, grid, timeend / nsteps, nsteps, timeend, math.sqrt(Lz)


def small_brick(cm, N=4):
    """The 2 x 2 x 1 periodic brick of the solve tests (elements of the level-1 size)."""
    M = cm.mesh
    h = 0.02
    rng = [np.linspace(0.0, 2 * h, 3), np.linspace(0.0, 2 * h, 3), np.array([0.0, h])]
    topl = M.BrickTopology(rng, periodicity=(True,) * 3, connectivity="face")
    return M.DiscontinuousSpectralElementGrid(topl, N), h


def oracle_acoustic(cm, O, grid, nf=0, direction=EVERY):
    """The oracle's acoustic linear operator: its acoustic-gravity law on the twin model."""
    twin = vortex_law(cm, twin=True)
    aux = twin.init_state_auxiliary(grid)
    return O.OracleDGModel(cm.atmos.AtmosAcousticGravityLinearModel(twin), grid, nf_first=nf,
                           direction=direction, state_auxiliary=aux)


def device_pair(cm, law, grid, nf=0, direction=EVERY):
    """The device's full model and its no-orientation acoustic linear model on one auxiliary state."""
    dg = cm.dgmodel.DGModel(law, grid, direction=EVERY)
    lin = cm.dgmodel.DGModel(cm.atmos.AtmosAcousticLinearModel(law), grid, direction=direction,
                             numerical_flux_first_order=nf, state_auxiliary=dg.state_auxiliary)
    return dg, lin


STATE_SCALE = np.array([1e-3, 1.0, 1.0, 1.0, 1e2])


def random_state(grid, seed, like=None):
    """A random (nelem, 5, Np) state of the size of a perturbation of the vortex's far field."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((grid.nelem, 5, grid.Np)) * STATE_SCALE[None, :, None]


def solve_schedule(t0, dt, timeend):
    """The (t, step) pairs of ``solve!(...; timeend, adjustfinalstep = true)`` (ODESolvers.jl:49-158)."""
    out, t = [], t0
    while t < timeend:
        if t + dt > timeend:
            out.append((t, timeend - t))
            t = timeend
        else:
            out.append((t, dt))
            t += dt
    return out
