"""Host side of the DGFVModel: the (N_h, 0) grid (``computegeometry_fvm``, Grids.jl:812-1010), the
finite-volume reconstructions (FVReconstructions.jl) and the NumPy restatement of the operator
(tests/dgfv_restatement.py) against the reference's stored errors
(tests/golden/dgfv_reference_values.json, fvm_advection_diffusion.jl:372-406)."""
import json
import os

import numpy as np
import pytest

from cmdg_loader import cm
import dgfv_restatement as R

M = cm.mesh
BL = cm.balancelaws
G = cm.mesh.grids
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "dgfv_reference_values.json")))
RTOL = GOLD["rtol"]


def gold_advdiff(level, recon):
    for r in GOLD["fvm_advection_diffusion"]["rows"]:
        if r["key"] == ["3", str(level), "Float64", recon + "()"]:
            return r["value"]
    raise KeyError((level, recon))


def fvm_advection_diffusion_setup(level=1, field=0, periodic_vertical=False, rank=0, size=1, N=4):
    """fvm_advection_diffusion.jl:118-209, dim = 3: ``field`` 0 / 1 / 2 is the horizontal, vertical
    or diagonal equation of the reference's decoupled three-equation law, run as its own
    single-equation law."""
    n = (np.array([1, 1, 0]) / np.sqrt(2), np.array([0, 0, 1.0]), np.ones(3) / np.sqrt(3))[field]
    Ne = 2 ** (level - 1) * 4
    Lh, Lv = N / 4, 1 / 4
    rng = [np.linspace(-Lh, Lh, Ne + 1)] * 2 + [np.linspace(-Lv, Lv, Ne + 1)]
    topl = M.StackedBrickTopology(rng, boundary=((1, 2),) * 3, periodicity=(False, False, periodic_vertical),
                                  connectivity="full", rank=rank, size=size)
    grid = M.DiscontinuousSpectralElementGrid(topl, (N, 0))
    law = BL.AdvectionDiffusion(3, BL.Pseudo1D(n, 1.0, 1 / 100, -1 / 2, 1 / 10),
                                (BL.InhomogeneousBC(0), BL.InhomogeneousBC(1)))
    dt = (1.0 / 4) * Lh / (Ne * N ** 2)
    return law, grid, dt


def gold_advection(level, recon):
    for r in GOLD["fvm_advection"]["rows"]:
        if r["key"] == ["3", str(level), "Float64", recon + "()"]:
            return r["value"]
    raise KeyError((level, recon))


def gold_periodic(level, recon, equation):
    for r in GOLD["fvm_advection_diffusion_periodic"]["rows"]:
        if r["key"] == ["2", "4", recon + "()", str(level), "Float64", str(equation)]:
            return r["value"]
    raise KeyError((level, recon, equation))


def fvm_advection_setup(level=1, N=4):
    """fvm_advection.jl:262-300, dim = 3: the sine wave along (1, 1, 1) / sqrt 3, N Ne cells in the
    vertical, inflow data on every boundary; 64 steps to t = 1/4 at level 1."""
    Ne = 2 ** (level - 1) * 4
    rng = [np.linspace(-1, 1, Ne + 1)] * 2 + [np.linspace(-1, 1, N * Ne + 1)]
    topl = M.StackedBrickTopology(rng, boundary=((1, 1),) * 3, periodicity=(False,) * 3, connectivity="full")
    grid = M.DiscontinuousSpectralElementGrid(topl, (N, 0))
    law = BL.AdvectionDiffusion(3, BL.SineAdvection(np.ones(3) / np.sqrt(3), 1.0), (BL.InhomogeneousBC(0),),
                                diffusion=False)
    dt = (1.0 / 4) / (Ne * N ** 2)
    nsteps = int(np.ceil(0.25 / dt))
    return law, grid, 0.25 / nsteps, nsteps


def l2_error(grid, Q, Qe):
    Mw = grid.vgeo[:grid.nreal, G._M, :]
    return float(np.sqrt(np.sum(Mw * (Q[:grid.nreal, 0] - Qe[:grid.nreal, 0]) ** 2)))


# ---- (a) grid identities -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def grids():
    z = np.array([0.0, 0.1, 0.35, 0.5, 1.0])
    x = np.linspace(0.0, 2.0, 3)
    out = {}
    for per in (False, True):
        topl = M.StackedBrickTopology([x, x, z], boundary=((1, 2),) * 3, periodicity=(False, False, per),
                                      connectivity="full")
        out[per] = (M.DiscontinuousSpectralElementGrid(topl, (3, 0)),
                    M.DiscontinuousSpectralElementGrid(topl, (3, 1)), z)
    return out


def test_grid_identities(grids):
    g, g1, z = grids[False]
    nv = len(z) - 1
    assert g.Nq == (4, 4, 1) and g.Np == 16 and g.Nfp == (4, 4, 16)
    assert np.array_equal(g.xi[2], [0.0]) and np.array_equal(g.omega[2], [2.0]) and np.array_equal(g.D[2], [[0.0]])
    vol = 2.0 * 2.0 * 1.0
    assert abs(g.vgeo[:, G._M, :].sum() - vol) <= 1e-14 * vol
    h = np.tile(np.diff(z), g.nelem // nv)
    assert np.allclose(2 * g.vgeo[:, G._JcV, :], h[:, None], rtol=1e-14, atol=0)
    # M equals the two nodes of the N_v = 1 grid summed; MI its reciprocal
    M1 = g1.vgeo[:, G._M, :].reshape(g.nelem, 2, 16)
    assert np.array_equal(g.vgeo[:, G._M, :], M1[:, 0] + M1[:, 1])
    assert np.array_equal(g.vgeo[:, G._MI, :], 1.0 / g.vgeo[:, G._M, :])
    # vertical faces: sM is the horizontal mass; vMI is MI at the face node on every face
    for f in (4, 5):
        assert np.allclose(g.sgeo[:, f, :16, G._sM], g.vgeo[:, G._MH, :], rtol=1e-14, atol=0)
        assert np.array_equal(g.sgeo[:, f, :16, G._n3], np.full((g.nelem, 16), -1.0 if f == 4 else 1.0))
    fm = G._fmask(list(g.Nq))
    for f in range(6):
        nfp = g.Nfp[f // 2]
        assert np.array_equal(g.sgeo[:, f, :nfp, G._vMI], g.vgeo[:, G._MI, :][:, fm[f]])
    # xi3x3 = 2 / h (mass-weighted average of a constant), the cell centre in x3
    assert np.allclose(g.vgeo[:, G._xi3x3, :], (2 / h)[:, None], rtol=1e-13)
    zc = np.tile((z[1:] + z[:-1]) / 2, g.nelem // nv)
    assert np.allclose(g.vgeo[:, G._x3, :], zc[:, None], rtol=1e-14)
    assert abs(G.min_node_distance(g, 2) - np.diff(z).min()) <= 1e-15


def test_grid_vertical_neighbours(grids):
    for per in (False, True):
        g, _, z = grids[per]
        nv, Np = len(z) - 1, g.Np
        e = np.arange(g.nelem)
        eV = e % nv
        for f, step in ((4, -1), (5, 1)):
            eP = (g.vmapP[:, f, :Np] - 1) // Np
            nP = (g.vmapP[:, f, :Np] - 1) % Np
            edge = (eV == 0) if f == 4 else (eV == nv - 1)
            want = np.where(edge, e + (nv - 1) * (1 if f == 4 else -1) if per else e, e + step)
            bnd = g.elemtobndy[:, f] != 0
            assert np.array_equal(bnd, edge & (not per))
            # (on a boundary face every kernel takes the minus node itself, DGModel_kernels.jl:686-692,
            # whatever the topology's self-connection put into vmap+)
            inner = ~bnd
            assert np.array_equal(eP[inner], np.broadcast_to(want[inner, None], eP[inner].shape))
            assert np.array_equal(nP[inner], np.broadcast_to(np.arange(Np)[None, :], nP[inner].shape))


def test_order_ge1_grids_unchanged():
    """Grids with every order >= 1 do not go through the FV path."""
    x = np.linspace(0, 1, 3)
    topl = M.StackedBrickTopology([x, x, x], boundary=((1, 2),) * 3, periodicity=(False,) * 3, connectivity="full")
    g = M.DiscontinuousSpectralElementGrid(topl, (2, 1))
    vg, sg = G.computegeometry(topl.elemtocoord, g.D, g.xi, g.omega)
    assert np.array_equal(g.vgeo, vg) and np.array_equal(g.sgeo, sg, equal_nan=True)
    with pytest.raises(ValueError):
        M.DiscontinuousSpectralElementGrid(topl, (0, 1))


# ---- (b) reconstructions -------------------------------------------------------------------------
def test_fvlinear_hand_computed():
    F = cm.fvreconstructions
    c = [np.array([1.0]), np.array([2.0]), np.array([4.0])]
    w = [np.array([1.0]), np.array([2.0]), np.array([1.0])]
    # d_top = (4 - 2) / 3 = 2/3, d_bot = (2 - 1) / 3 = 1/3; Van Leer 2 ab / (a + b) = 4/9
    bot, top = F.FVLinear()(c, w)
    assert abs(top[0] - (2 + 8 / 9)) < 1e-15 and abs(bot[0] - (2 - 8 / 9)) < 1e-15
    # no limiter: the mean slope 1/2
    bot, top = F.FVLinear(limiter=F.NoLimiter())(c, w)
    assert abs(top[0] - 3.0) < 1e-15 and abs(bot[0] - 1.0) < 1e-15
    # Van Leer's zero branch: a local extremum is not steepened
    bot, top = F.FVLinear()([np.array([1.0]), np.array([3.0]), np.array([2.0])], w)
    assert bot[0] == 3.0 and top[0] == 3.0
    # the restatement's own functor agrees
    rb, rt = R.Recon(True)(c, w)
    assert abs(rt[0] - (2 + 8 / 9)) < 1e-15 and abs(rb[0] - (2 - 8 / 9)) < 1e-15
    assert F.width(F.FVConstant()) == 0 and F.width(F.FVLinear(3)) == 3
    with pytest.raises(ValueError):
        F.FVLinear(width=0)


def test_fvlinear_width3_is_width1():
    F = cm.fvreconstructions
    rng = np.random.default_rng(3)
    c = [rng.standard_normal(5) for _ in range(7)]
    w = [rng.uniform(0.5, 2.0, 5) for _ in range(7)]
    b1, t1 = F.FVLinear(1)(c[2:5], w[2:5])
    b3, t3 = F.FVLinear(3)(c, w)
    assert np.array_equal(b1, b3) and np.array_equal(t1, t3)
    b, t = F.FVLinear(2)(c[3:4], w[3:4])
    assert np.array_equal(b, c[3]) and np.array_equal(t, c[3])
    b, t = F.FVConstant()(c[3:4])
    assert np.array_equal(b, c[3]) and np.array_equal(t, c[3])


# ---- (c) the restatement against the reference's stored errors ----------------------------------
RECONS = {"FVConstant": lambda: R.Recon(False), "FVLinear": lambda: R.Recon(True, 1),
          "FVLinear3": lambda: R.Recon(True, 3)}


@pytest.mark.parametrize("recon", ["FVConstant", "FVLinear", "FVLinear3"])
@pytest.mark.parametrize("field", [0, 1, 2])
def test_restatement_fvm_advection_diffusion_level1(recon, field):
    """fvm_advection_diffusion.jl, dim 3, level 1, EveryDirection: 256 steps to t = 1."""
    law, grid, dt = fvm_advection_diffusion_setup(1, field)
    dg = R.DGFVRestatement(law, grid, RECONS[recon](), nf_first=0, direction=R.EVERY)
    Q = law.init_state_prognostic(grid, dg.state_auxiliary, 0.0)
    assert round(1 / dt) == 256
    R.lsrk54_steps(dg, Q, dt, 256)
    err = l2_error(grid, Q, law.init_state_prognostic(grid, dg.state_auxiliary, 1.0))
    want = gold_advdiff(1, "FVLinear" if recon != "FVConstant" else recon)[field]
    print("field %d %s: %.16e (reference %.16e)" % (field, recon, err, want))
    assert abs(err - want) <= RTOL * abs(want)


@pytest.mark.parametrize("recon", ["FVConstant", "FVLinear"])
def test_restatement_fvm_advection_level1(recon):
    """fvm_advection.jl, dim 3, level 1: 4 x 4 x 16 cells, 64 steps to t = 1/4."""
    law, grid, dt, nsteps = fvm_advection_setup(1)
    assert nsteps == 64 and grid.topology.stacksize == 16
    dg = R.DGFVRestatement(law, grid, RECONS[recon](), nf_first=0, direction=R.EVERY)
    Q = law.init_state_prognostic(grid, dg.state_auxiliary, 0.0)
    R.lsrk54_steps(dg, Q, dt, nsteps)
    err = l2_error(grid, Q, law.init_state_prognostic(grid, dg.state_auxiliary, 0.25))
    want = gold_advection(1, recon)
    print("fvm_advection %s: %.16e (reference %.16e)" % (recon, err, want))
    assert abs(err - want) <= RTOL * abs(want)


@pytest.mark.parametrize("direction,field", [(R.HORIZONTAL, 0), (R.VERTICAL, 1)])
def test_restatement_single_direction_runs(direction, field):
    """The Horizontal- and Vertical-direction runs against fields 1 and 2 (:452-466)."""
    law, grid, dt = fvm_advection_diffusion_setup(1, field)
    dg = R.DGFVRestatement(law, grid, R.Recon(True, 1), nf_first=0, direction=direction)
    Q = law.init_state_prognostic(grid, dg.state_auxiliary, 0.0)
    R.lsrk54_steps(dg, Q, dt, 256)
    err = l2_error(grid, Q, law.init_state_prognostic(grid, dg.state_auxiliary, 1.0))
    want = gold_advdiff(1, "FVLinear")[field]
    print("direction %d: %.16e (reference %.16e)" % (direction, err, want))
    assert abs(err - want) <= RTOL * abs(want)


def test_restatement_periodic_conservation():
    """On the periodic stack the vertical operator conserves the integral: 20 steps change the
    mass-weighted sum by at most 10 eps |sum|."""
    law, grid, dt = fvm_advection_diffusion_setup(1, 1, periodic_vertical=True)
    dg = R.DGFVRestatement(law, grid, R.Recon(True, 1), nf_first=0, direction=R.VERTICAL)
    Q = law.init_state_prognostic(grid, dg.state_auxiliary, 0.0)
    Mw = grid.vgeo[:grid.nreal, G._M, :]
    import math
    s0 = math.fsum((Mw * Q[:grid.nreal, 0]).ravel())
    R.lsrk54_steps(dg, Q, dt, 20)
    s1 = math.fsum((Mw * Q[:grid.nreal, 0]).ravel())
    assert abs(s1 - s0) <= 10 * np.finfo(float).eps * abs(s0)
