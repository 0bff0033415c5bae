"""Moving, discontinuous states for the dry law's Roe / HLLC / LMARS fluxes, and the host-side
census of what every face-node pair of a grid does with them (test infrastructure).

The state is built from primitives, so it is admissible by construction: around a background
``(rho0, T0)`` -- the hydrostatic reference state the law carries, or the isentropic vortex's far
field -- ``rho = rho0 (1 + a xi)``, ``T = T0 (1 + a xi')``, ``u = Mach c(T) N(0, 1)`` per component
and node, ``rho e = rho (cv_d (T - T_0) + |u|^2 / 2 + Phi)``.  The noise is drawn per node, so
every face sees a jump.

The auxiliary state is roughened as well (``roughen``): the reference pressure and the
geopotential are continuous functions of position, so on any grid the two sides of a face carry
the same ``p_ref`` and ``Phi``, and a flux that read the wrong side's would go unnoticed.  Per node
noise, keyed by the global element number so that a rank's ghost elements get their owner's
values, makes the two sides differ; both models take the auxiliary state as data."""
import numpy as np

import atmos_nf_restatement as R
from helpers import isentropic_vortex_setup
from test_hydrostatic_balance import balanced_setup

SEED = 7
HARD = dict(a=0.1, mach=1.0)        # every branch of the three fluxes, supersonic wall nodes
MILD = dict(a=0.01, mach=0.05)      # survives LSRK steps


def soundspeed(ps, T):
    return np.sqrt(ps.cp_d / ps.cv_d * ps.R_d * T)


def conserved(ps, rho, T, u, Phi):
    """``(k, 5)`` prognostic state of primitives ``rho (k,)``, ``T (k,)``, ``u (k, 3)``, ``Phi (k,)``."""
    Q = np.empty(rho.shape + (5,))
    Q[..., 0] = rho
    Q[..., 1:4] = rho[..., None] * u
    Q[..., 4] = rho * (ps.cv_d * (T - ps.T_0) + (u * u).sum(axis=-1) / 2 + Phi)
    return Q


class NoisyState:
    """An ``init_state`` for ``DryAtmosModel``: the recipe above on every node of the grid it is
    asked for (the same numbers for the same grid, whoever asks)."""

    def __init__(self, ps, a, mach, background=None, seed=SEED):
        self.ps, self.a, self.mach, self.background, self.seed = ps, a, mach, background, seed

    def __call__(self, law, aux, coord, t):
        ps, rng = self.ps, np.random.default_rng(self.seed)
        shape = coord[0].shape
        Phi = aux[:, law.off_phi, :] if law.orientation != 0 else np.zeros(shape)
        if self.background is None:
            rho0 = aux[:, law.off_ref, :]
            T0 = ps.T_0 + (aux[:, law.off_ref + 3, :] / rho0 - Phi) / ps.cv_d
        else:
            rho0, T0 = (np.full(shape, v) for v in self.background)
        rho = rho0 * (1 + self.a * rng.uniform(-1, 1, shape))
        T = T0 * (1 + self.a * rng.uniform(-1, 1, shape))
        u = self.mach * soundspeed(ps, T)[..., None] * rng.standard_normal(shape + (3,))
        Q = conserved(ps, rho, T, u, Phi)
        return Q[..., 0], [Q[..., 1], Q[..., 2], Q[..., 3]], Q[..., 4]


ROUGH_P_REF = 1e-3      # relative, some 80 Pa
ROUGH_PHI = 50.0        # J / kg, some 5 m of height


def roughen(law, grid, aux):
    """Per-node noise on ``p_ref`` and ``Phi`` of every element of ``grid``, ghosts included, in
    place; a function of the global element number and the node alone."""
    for e, g in enumerate(grid.topology.globalelems):
        xi = np.random.default_rng([SEED, int(g)]).uniform(-1, 1, (2, grid.Np))
        aux[e, law.off_ref + 1] *= 1 + ROUGH_P_REF * xi[0]
        aux[e, law.off_phi] += ROUGH_PHI * xi[1]
    return aux


def walled_setup(config, subtract_off, a, mach, rank=0, size=1, rough_init=False):
    """``balanced_setup(config, "decaying")`` (LES box: 27 elements, GCM shell: 162) with walls at
    the bottom and the top.  With ``subtract_off`` the analytic reference density is kept
    (``balance=False``), so that ``p_ref`` and ``rho_ref`` do not cancel discretely.  With
    ``rough_init`` the law's ``init_state_auxiliary`` returns the roughened state (for models that
    build their own; needs ``balance=False``)."""
    law, grid = balanced_setup(config, "decaying", balance=not subtract_off, rank=rank, size=size)
    law.subtract_off = bool(subtract_off)
    law.init_state = NoisyState(law.ps, a, mach)
    if rough_init:
        assert not law.discrete_hydrostatic_balance
        smooth = law.init_state_auxiliary
        law.init_state_auxiliary = lambda g: roughen(law, g, smooth(g))
    return law, grid


def vortex_setup(a, mach):
    """The plain variant: ``isentropic_vortex_setup()`` at level 1 (25 elements, periodic, no
    orientation, no reference state) with the noise around the vortex's far field."""
    law, grid = isentropic_vortex_setup()[:2]
    s = law.init_state
    law.init_state = NoisyState(law.ps, a, mach, background=(s.rho_inf, s.T_inf))
    return law, grid


def face_pairs(law, grid, Q, aux):
    """Every face-node pair of the real elements as the interface kernel sees it:
    ``(n, QM, auxM, QP, auxP, wall)`` with the free-slip ghost state (momentum reflected with
    ``2 (rho u . n) n``, bc_momentum.jl:25-52) on boundary faces."""
    nr, Np = grid.nreal, grid.Np
    vM = np.asarray(grid.vmapM)[:nr] - 1
    vP = np.asarray(grid.vmapP)[:nr] - 1
    n = np.asarray(grid.sgeo)[:nr, :, :, 0:3].reshape(-1, 3)
    wall = np.broadcast_to(np.asarray(grid.elemtobndy)[:nr, :, None] != 0, vM.shape).reshape(-1)
    eM, iM, eP, iP = (vM // Np).ravel(), (vM % Np).ravel(), (vP // Np).ravel(), (vP % Np).ravel()
    QM, QP = Q[eM, :, iM].copy(), Q[eP, :, iP].copy()
    auxM, auxP = aux[eM, :, iM].copy(), aux[eP, :, iP].copy()
    dn = (QM[wall, 1:4] * n[wall]).sum(axis=1)
    QP[wall] = QM[wall]
    QP[wall, 1:4] -= 2 * dn[:, None] * n[wall]
    auxP[wall] = auxM[wall]
    return n, QM, auxM, QP, auxP, wall


ROE_PATTERNS = ((-1, -1, -1), (-1, -1, 1), (-1, 1, 1), (1, 1, 1))


def census(law, grid, Q, aux):
    """What the restatement says every face-node pair does: counts over the interior pairs of
    the four HLLC branches, the two LMARS directions and the four Roe sign patterns, the
    smallest tie margin there, and the largest ``|u . n| / c`` on a wall."""
    n, QM, auxM, QP, auxP, wall = face_pairs(law, grid, Q, aux)
    info = R.numerical_flux(R.HLLC, R.Switches.of(law), n, QM, auxM, QP, auxP)[1]
    inner = ~wall
    rough = [0.0, 0.0]       # largest jump of Phi and of p_ref across an interior face
    if law.orientation != 0 and law.ref_state is not None:
        rough = [float(np.abs(auxP[inner, c] - auxM[inner, c]).max())
                 for c in (law.off_phi, law.off_ref + 1)]
    signs = info["roe_signs"][inner]
    return dict(
        interior=int(inner.sum()), wall=int(wall.sum()),
        hllc=[int((info["hllc"][inner] == b).sum()) for b in range(4)],
        lmars=[int(info["lmars_up"][inner].sum()), int((~info["lmars_up"][inner]).sum())],
        roe=[int((signs == np.array(p)).all(axis=1).sum()) for p in ROE_PATTERNS],
        tie=float(info["tie"][inner].min()),
        wall_mach=float(info["un_over_c"][wall].max()) if wall.any() else 0.0, rough=rough)


def assert_hard_census(c, walls=True):
    """The conditions a HARD state must meet before anything is launched."""
    assert min(c["hllc"]) >= 50, c
    assert min(c["lmars"]) >= 1, c
    assert min(c["roe"]) >= 1, c
    assert c["tie"] >= 1e-6, c
    if walls:
        assert c["wall"] > 0 and c["wall_mach"] > 1, c
        assert c["rough"][0] > ROUGH_PHI and c["rough"][1] > 50.0, c     # the sides differ
