"""DGFVModel on the dry atmosphere law on the device (cmdg_create_dgfv with CMDG_PHYSICS_DRY_ATMOS;
csrc/fv.h with the hooks of csrc/physics_atmos.h) against the NumPy restatement of
tests/dgfv_atmos_restatement.py, the reference's stored errors of fvm_isentropicvortex.jl
(tests/golden/dgfv_atmos_reference_values.json) and the bound of fvm_balance.jl."""
import json
import os

import numpy as np
import pytest

from cmdg_loader import cm
import dgfv_atmos_cases as CASES
import dgfv_atmos_restatement as RA
import dgfv_restatement as R
from helpers import rel_linf

pytestmark = pytest.mark.gpu
A = cm.atmos
F = cm.fvreconstructions
M = cm.mesh
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "dgfv_atmos_reference_values.json")))
RUSANOV, ROE = 0, 2
EVERY, VERTICAL = 0, 2
TOL = 1e-12                   # HIP against a restatement, relative Linf


def _recons(name, law):
    """The library's reconstruction object and the restatement's."""
    inner = {"constant": (F.FVConstant(), R.Recon(False)),
             "linear1-vanleer": (F.FVLinear(1, F.VanLeer()), R.Recon(True, 1, R.van_leer)),
             "linear2-nolimiter": (F.FVLinear(2, F.NoLimiter()), R.Recon(True, 2, R.no_limiter))}
    if name.startswith("hb-"):
        dev, ref = inner[name[3:]]
        return A.HBFVReconstruction(law, dev), RA.HBRecon(ref, law.ps.grav)
    return inner[name]


def _setup(model, periodic, n_vert=6):
    if model == "vortex":
        assert periodic
        return CASES.vortex_box(2, n_vert)
    return CASES.balance_box(2, n_vert, periodic_stack=periodic, noisy=True)


# (law, reconstruction, first-order flux, direction, periodic stack, cells).  Every value of every
# axis at least once; the formerly dead paths by name:
#   conversions            every case (the box law converts with Phi, the vortex law without);
#   face auxiliary state   the box law, whose Phi moves to the faces -- with a reconstruction that is
#                          not constant the two sides of a face then differ in their energy;
#   HB wrapper             hb-*: around the linear and the constant reconstruction, on walls (one-cell
#                          stencils at the ends) and periodic;
#   source                 Vertical direction on the box law (Gravity); on the periodic stack the top
#                          cell receives it twice;
#   32 cells               the 71 400 B stack, launched with the raised LDS limit.
ONE_EVALUATION = [
    ("box", "constant", RUSANOV, EVERY, False, 6),
    ("box", "linear1-vanleer", ROE, EVERY, False, 6),
    ("box", "linear2-nolimiter", RUSANOV, VERTICAL, False, 6),
    ("box", "hb-linear1-vanleer", ROE, EVERY, False, 6),
    ("box", "hb-linear1-vanleer", ROE, VERTICAL, False, 6),
    ("box", "hb-constant", RUSANOV, VERTICAL, False, 6),
    ("box", "linear1-vanleer", ROE, VERTICAL, True, 6),
    ("box", "hb-linear2-nolimiter", RUSANOV, EVERY, True, 6),
    ("vortex", "constant", ROE, EVERY, True, 6),
    ("vortex", "linear1-vanleer", RUSANOV, VERTICAL, True, 6),
    ("vortex", "hb-linear1-vanleer", ROE, EVERY, True, 6),
    ("box", "hb-linear1-vanleer", ROE, EVERY, False, 32),
]


@pytest.mark.parametrize("model,recon,flux,direction,periodic,n_vert", ONE_EVALUATION)
def test_one_evaluation(torch, oracle, model, recon, flux, direction, periodic, n_vert):
    """Tendency of the noisy state (reference state times 1 + 1e-3 h, moving) against the restatement,
    (alpha, beta) = (1, 0) and (0.5, 2): relative Linf per state column below 1e-12."""
    law, grid = _setup(model, periodic, n_vert)
    dev, ref = _recons(recon, law)
    dg = cm.dgmodel.DGFVModel(law, grid, dev, numerical_flux_first_order=flux, direction=direction)
    rs = RA.DGFVAtmosRestatement(law, grid, ref, nf_first=flux, direction=direction)
    Q = dg.init_ode_state(0.0)
    Qh = Q.cpu().numpy().copy()
    assert np.abs(Qh[:, 1:4]).min() > 0
    T0 = np.random.default_rng(11).standard_normal(Qh.shape)
    for alpha, beta in ((1.0, 0.0), (0.5, 2.0)):
        T = torch.from_numpy(T0.copy()).to(Q.device)
        Th = T0.copy()
        dg(T, Q, 0.3, alpha, beta)
        rs(Th, Qh, 0.3, alpha, beta)
        Td = T.cpu().numpy()
        errs = [rel_linf(Td[:grid.nreal, s], Th[:grid.nreal, s]) for s in range(5)]
        print("%s %s flux %d dir %d periodic %d nv %d (%.1f, %.1f): %s"
              % (model, recon, flux, direction, periodic, n_vert, alpha, beta, " ".join("%.2e" % e for e in errs)))
        assert np.isfinite(Td).all() and max(errs) < TOL
    dg.close()


def test_three_ranks_equal_one(torch, oracle):
    """Three ranks of one process (group_rhs) on the 2 x 2 x 6 box equal the single rank bit for bit."""
    kw = dict(numerical_flux_first_order=ROE, direction=EVERY)
    law, grid = CASES.balance_box(2, 6, noisy=True)
    one = cm.dgmodel.DGFVModel(law, grid, A.HBFVReconstruction(law, F.FVLinear()), **kw)
    Q1 = one.init_ode_state(0.0)
    T1 = one.create_state()
    one(T1, Q1, 0.1)
    full = T1.cpu().numpy()
    by_global = {int(g): full[i] for i, g in enumerate(grid.topology.globalelems[:grid.nreal])}
    parts = [CASES.balance_box(2, 6, noisy=True, rank=r, size=3) for r in range(3)]
    assert sum(p[1].nreal for p in parts) == grid.nreal
    dgs = [cm.dgmodel.DGFVModel(p[0], p[1], A.HBFVReconstruction(p[0], F.FVLinear()), **kw) for p in parts]
    Qs, Ts = [], []
    for d, (_, g) in zip(dgs, parts):
        q = d.init_ode_state(0.0)
        q[g.nreal:] = float("nan")                  # ghosts must come from the exchange
        Qs.append(q)
        Ts.append(d.create_state())
    torch.cuda.synchronize()
    cm.dgmodel.connect_local(dgs)
    cm.dgmodel.group_rhs(dgs, Ts, Qs, 0.1, 1.0, 0.0)
    for (_, g), T in zip(parts, Ts):
        Tn = T.cpu().numpy()
        want = np.stack([by_global[int(ge)] for ge in g.topology.globalelems[:g.nreal]])
        assert np.array_equal(Tn[:g.nreal], want)
    for d in dgs + [one]:
        d.close()


# ---- fvm_isentropicvortex.jl (dims = 2) through the y-invariant slice --------------------------------
def vortex_dim2_setup(level, N=4):
    """fvm_isentropicvortex.jl:123-190: 5 * 2^(level - 1) elements across and N times as many cells
    up, fully periodic, as a three-dimensional grid of one periodic element across y with the
    vortex's plane mapped to (x, z) (DESIGN "dim = 2", helpers.pseudo1d_dim2_setup): mass-weighted
    norms carry the factor sqrt(Ly)."""
    ps = A.PlanetParameters()
    setup = A.IsentropicVortexSetup(ps, plane=(0, 2))
    L = setup.domain_halflength
    ne = 2 ** (level - 1) * 5
    Ly = 2 * L / ne
    topl = M.StackedBrickTopology([np.linspace(-L, L, ne + 1), np.array([0.0, Ly]), np.linspace(-L, L, ne * N + 1)],
                                  periodicity=(True, True, True), connectivity="full")
    grid = M.DiscontinuousSpectralElementGrid(topl, (N, 0))
    law = A.DryAtmosModel(setup, orientation=A.ORIENT_NONE, ref_state=None, viscosity=0.0, dynamic_viscosity=True,
                          sources=0, boundary_conditions=(), param_set=ps)
    timeend = 2 * L / 10 / setup.translation_speed
    elementsize = min(2 * L / ne, 2 * L / (ne * N))
    dt = elementsize / np.sqrt(ps.cp_d / ps.cv_d * ps.R_d * setup.T_inf) / N ** 2
    nsteps = int(np.ceil(timeend / dt))
    return law, grid, timeend / nsteps, nsteps, timeend, np.sqrt(Ly)


@pytest.mark.parametrize("recon", ["FVConstant", "FVLinear"])
@pytest.mark.parametrize("level", [1, 2])
def test_golden_isentropic_vortex(torch, level, recon):
    """Levels 1 and 2 (5 x 20 and 10 x 40 elements), Roe: the reference's stored errors within its own
    ``isapprox`` (rtol sqrt(eps))."""
    law, grid, dt, nsteps, timeend, sq = vortex_dim2_setup(level)
    dg = cm.dgmodel.DGFVModel(law, grid, F.FVConstant() if recon == "FVConstant" else F.FVLinear(),
                              numerical_flux_first_order=ROE)
    Q = dg.init_ode_state(0.0)
    cm.odesolvers.LSRK54CarpenterKennedy(dg, Q, dt=dt).dostep(Q, nsteps=nsteps)
    dg.synchronize()
    aux = dg.state_auxiliary.cpu().numpy()
    Qe = torch.from_numpy(law.init_state_prognostic(grid, aux, timeend)).to(Q.device)
    err = dg.euclidean_distance(Q, Qe) / sq
    want = GOLD["errors"][recon][str(level)]
    print("level %d %s: %.16e (reference %.16e)" % (level, recon, err, want))
    dg.close()
    assert abs(err - want) <= GOLD["rtol"] * max(abs(err), abs(want))


# ---- fvm_balance.jl ----------------------------------------------------------------------------
@pytest.mark.parametrize("domain", ["box", "sphere"])
def test_hydrostatic_balance(torch, domain):
    """HB(FVLinear()), Roe, isothermal 300 K, reference state not subtracted, 100 s at CFL 0.2 on
    2 x 2 columns (2 elements per cube edge) of 32 cells: norm(Q - Q0) / norm(Q0) below the
    reference's 6e-12."""
    law, grid = CASES.balance_box(2, 32) if domain == "box" else CASES.balance_sphere(2, 32)
    dt, nsteps = CASES.balance_dt(law)
    dg = cm.dgmodel.DGFVModel(law, grid, A.HBFVReconstruction(law, F.FVLinear()), numerical_flux_first_order=ROE)
    Q = dg.init_ode_state(0.0)
    Q0 = Q.clone()
    cm.odesolvers.LSRK54CarpenterKennedy(dg, Q, dt=dt).dostep(Q, nsteps=nsteps)
    dg.synchronize()
    err = dg.euclidean_distance(Q, Q0) / dg.norm(Q0)
    print("%s: %d steps of %.6f s: norm(Q - Q0) / norm(Q0) = %.3e" % (domain, nsteps, dt, err))
    dg.close()
    assert err < GOLD["balance_bound"]


# ---- refusals ------------------------------------------------------------------------------------------
def test_refusals(torch):
    """Status and message of every refusal this law adds to cmdg_create_dgfv."""
    E = cm._lib.CmdgError
    BL = cm.balancelaws
    law, grid = CASES.balance_box(2, 6)
    # the hydrostatic wrapper on a law without a pressure primitive
    adv = BL.AdvectionDiffusion(3, BL.Pseudo1D(np.ones(3) / np.sqrt(3), 1.0, 1 / 100, -1 / 2, 1 / 10), (),
                                diffusion=False)
    with pytest.raises(E, match=r"\(-1\).*CMDG_FV_HYDROSTATIC.*pressure primitive"):
        cm.dgmodel.DGFVModel(adv, CASES.vortex_box(2, 3)[1], A.HBFVReconstruction(law, F.FVLinear()))
    # the dry law at another horizontal order
    x = np.linspace(0.0, 20e3, 3)
    topl = M.StackedBrickTopology([x, x, np.linspace(0.0, 10e3, 7)], boundary=((0, 0), (0, 0), (1, 2)),
                                  periodicity=(True, True, False), connectivity="full")
    with pytest.raises(E, match=r"\(-5\).*polynomial order is not compiled in.*N_h = 4"):
        cm.dgmodel.DGFVModel(law, M.DiscontinuousSpectralElementGrid(topl, (2, 0)), F.FVConstant())
    # closures outside the compiled set
    common = dict(orientation=A.ORIENT_FLAT, ref_state=A.IsothermalProfile(law.ps, 300.0), sources=A.SRC_GRAVITY,
                  boundary_conditions=CASES.WALLS, param_set=law.ps)
    with pytest.raises(E, match=r"\(-5\).*SmagorinskyLilly is not compiled in.*N_h = 4"):
        cm.dgmodel.DGFVModel(A.DryAtmosModel(CASES.balanced_state, smagorinsky=0.21, **common), grid, F.FVConstant())
    with pytest.raises(E, match=r"\(-5\).*hyperdiffusive.*N_h = 4"):
        cm.dgmodel.DGFVModel(A.DryAtmosModel(CASES.balanced_state, hyperdiffusion_timescale=3600.0, **common), grid,
                             F.FVConstant())
    # an orientation without a reference state
    with pytest.raises(E, match=r"\(-5\).*combination is not compiled in"):
        cm.dgmodel.DGFVModel(A.DryAtmosModel(CASES.balanced_state, orientation=A.ORIENT_FLAT, sources=A.SRC_GRAVITY,
                                             boundary_conditions=CASES.WALLS), grid, F.FVConstant())
    # 75 cells of 5 states at N_h = 4 are 8 * 25 * 830 = 166 000 B: more than a work-group may own
    with pytest.raises(E, match=r"\(-5\).*160 KiB"):
        cm.dgmodel.DGFVModel(*CASES.balance_box(2, 75), F.FVConstant())
    # ... and 74 cells (163 800 B) are served
    tall_law, tall_grid = CASES.balance_box(2, 74)
    dg = cm.dgmodel.DGFVModel(tall_law, tall_grid, A.HBFVReconstruction(tall_law, F.FVLinear()),
                              numerical_flux_first_order=ROE)
    Q = dg.init_ode_state(0.0)
    T = dg.create_state()
    dg(T, Q, 0.0)
    dg.synchronize()
    assert np.isfinite(T.cpu().numpy()).all()
    dg.close()
