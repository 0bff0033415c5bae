"""Host side of the DGFVModel on the dry atmosphere law: the one-time set-up of a finite-volume vertical
(``vert_fvm_auxiliary_field_gradient!``, ``fvm_balance!``), the primitive-variable hooks and
``HBFVReconstruction`` (climatemachine.jl_amd/atmos.py), by their defining properties and against
the independent restatement of tests/dgfv_atmos_restatement.py."""
import numpy as np
import pytest

from cmdg_loader import cm
import dgfv_atmos_cases as CASES
import dgfv_atmos_restatement as RA
import dgfv_restatement as R

A = cm.atmos
G = cm.mesh.grids
F = cm.fvreconstructions
EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def box():
    law, grid = CASES.balance_box(2, 8)
    return law, grid, law.init_state_auxiliary(grid)


@pytest.fixture(scope="module")
def sphere():
    law, grid = CASES.balance_sphere(2, 8)
    return law, grid, law.init_state_auxiliary(grid)


def _stacked(grid, a):
    nv = int(grid.topology.stacksize)
    return a.reshape((a.shape[0] // nv, nv) + a.shape[1:])


# Every level of the recursion is local: rho_i comes from (rho, p) of the level below in twelve
# rounded operations (two virtual temperatures at a product and a quotient each, R_d T twice,
# g dz / 2 twice -- the halving is exact --, a difference, a sum, a product, a quotient) and p_i in two
# more, each on a quantity no larger than p_surface (R_d rho T is a pressure).  With the four
# roundings of the residual itself that is at most 18 half-ulps: 9 eps p_surface.  Nothing
# accumulates up the stack, because level i + 1 starts from the stored (rho_i, p_i).
BALANCE_ULPS = 9


@pytest.mark.parametrize("which", ["box", "sphere"])
def test_fvm_balance(which, box, sphere):
    """p_i - p_{i+1} = g (rho_{i+1} dz_{i+1} + rho_i dz_i) / 2 on every node of a 2 x 2 x 8 box and
    of a 2-per-edge, 8-cell shell."""
    law, grid, aux = box if which == "box" else sphere
    g = law.ps.grav
    rho, p = _stacked(grid, aux[:, law.off_ref]), _stacked(grid, aux[:, law.off_ref + 1])
    dz = 2 * _stacked(grid, grid.vgeo[:, G._JcV, :])
    res = (p[:, :-1] - p[:, 1:]) - g * (rho[:, 1:] * dz[:, 1:] + rho[:, :-1] * dz[:, :-1]) / 2
    worst = float(np.abs(res).max())
    print("%s: worst residual %.3e Pa = %.2f eps p_surface" % (which, worst, worst / (EPS * p.max())))
    assert worst <= BALANCE_ULPS * EPS * p.max()
    # T and rho e are consistent with the balanced (rho, p) (ref_state_finalize_init!)
    ps = law.ps
    T = aux[:, law.off_ref + 1] / (ps.R_d * aux[:, law.off_ref])
    assert np.array_equal(aux[:, law.off_ref + 2], T)
    # ... and the recursion moved rho off the analytic profile by a discretisation error, not more
    Tv, p_exact = law.ref_state(aux[:, law.off_phi] / g)
    assert 0 < np.abs(aux[:, law.off_ref] - p_exact / (ps.R_d * Tv)).max() < 1e-3


def test_fv_gradient_of_geopotential(box):
    """FV gradient of Phi = g z on the box: (0, 0, g) to rounding.  The bound has four parts.  The
    difference of two potentials carries half an ulp of each, over the 2 dz it is divided by.  The
    quotient, the products and the sum add a few ulps of g.  The grid's metric terms are data here:
    the rotation back to Cartesian multiplies by xi3x * JcV, which the grid holds as (0, 0, 1) only to
    its own accuracy.  And the horizontal DG part differentiates a field that is constant across the
    element: rounding of size eps Phi |D|_inf |xi1x|."""
    law, grid, aux = box
    g = law.ps.grav
    gphi = aux[:, law.off_phi + 1:law.off_phi + 4, :]
    vg = grid.vgeo
    dz = 2 * vg[:, G._JcV, :].min()
    phi_max = np.abs(aux[:, law.off_phi]).max()
    rot = np.stack([vg[:, c, :] * vg[:, G._JcV, :] for c in (G._xi3x1, G._xi3x2, G._xi3x3)], axis=1)
    metric = np.abs(rot - np.array([0.0, 0.0, 1.0])[None, :, None]).max()
    horizontal = EPS * phi_max * np.abs(grid.D[0]).sum(axis=1).max() * np.abs(vg[:, G._xi1x1, :]).max()
    tol = EPS * phi_max / (2 * dz) + 4 * EPS * g + g * metric + 2 * horizontal
    err = np.abs(gphi - np.array([0.0, 0.0, g])[None, :, None]).max()
    print("grad Phi: worst error %.3e, bound %.3e" % (err, tol))
    assert err <= tol


def test_order_one_grids_keep_their_path():
    """A grid with a polynomial vertical takes the element-local DG gradient and the analytic density."""
    law, _ = CASES.balance_box(2, 2)
    x = np.linspace(0.0, 20e3, 3)
    topl = cm.mesh.StackedBrickTopology([x, x, np.linspace(0.0, 10e3, 3)], boundary=((0, 0), (0, 0), (1, 2)),
                                        periodicity=(True, True, False), connectivity="full")
    grid = cm.mesh.DiscontinuousSpectralElementGrid(topl, (4, 1))
    aux = law.init_state_auxiliary(grid)
    phi = aux[:, law.off_phi]
    assert np.array_equal(aux[:, law.off_phi + 1:law.off_phi + 4], G.auxiliary_field_gradient(grid, phi))
    Tv, p = law.ref_state(phi / law.ps.grav)
    assert np.array_equal(aux[:, law.off_ref], p / (Tv * law.ps.R_d))


def test_conversion_round_trip(box):
    """prognostic -> primitive -> prognostic is the identity to 1e-14 relative on seeded states, with
    and without an orientation."""
    law, grid, aux = box
    noisy, _ = CASES.balance_box(2, 8, noisy=True)
    Q = noisy.init_state_prognostic(grid, aux, 0.0)
    vlaw, vgrid = CASES.vortex_box(2, 4)
    vaux = vlaw.init_state_auxiliary(vgrid)
    for m, q, a in ((law, Q, aux), (vlaw, vlaw.init_state_prognostic(vgrid, vaux, 0.0), vaux)):
        prim = A.prognostic_to_primitive(m, q, a)
        back = A.primitive_to_prognostic(m, prim, a)
        scale = np.abs(q).max(axis=(0, 2))[None, :, None]
        err = float((np.abs(back - q) / scale).max())
        print("round trip: %.2e" % err)
        assert err <= 1e-14
        assert np.all(prim[:, 4] > 0) and np.array_equal(prim[:, 0], q[:, 0])
        # the face auxiliary state moves Phi alone, by g dz / 2
        dzs = 7.0
        face = A.construct_face_auxiliary_state(m, a, -dzs)
        if m.orientation != A.ORIENT_NONE:
            assert np.array_equal(face[:, m.off_phi], a[:, m.off_phi] + m.ps.grav * -dzs / 2)
            face[:, m.off_phi] = a[:, m.off_phi]
        assert np.array_equal(face, a)


# With (rho, p) balanced, the stencil's neighbours minus their reference pressures are rounding
# noise of size eps p: the slopes vanish to that size and each face value is p_ref -+ rho g dz / 2
# plus that noise.  p_top(i) - p_bot(i + 1) is then the balance residual (9 eps p_surface above)
# plus two reconstructions' noise of at most 4 eps p each.
HB_ULPS = BALANCE_ULPS + 8


@pytest.mark.parametrize("inner", ["constant", "linear", "linear3-nolimiter"])
def test_hb_reconstruction_of_a_balanced_column(box, inner):
    """HBFVReconstruction of a discretely balanced column: p_top(i) = p_bot(i + 1) to rounding, with
    density and velocity untouched by the wrapper -- the property that keeps the balanced state at rest."""
    law, grid, aux = box
    recon = {"constant": F.FVConstant(), "linear": F.FVLinear(),
             "linear3-nolimiter": F.FVLinear(3, F.NoLimiter())}[inner]
    hb = A.HBFVReconstruction(law, recon)
    assert hb.reconstruction_id == recon.reconstruction_id | cm._lib.FV_HYDROSTATIC and hb.width == recon.width
    Q = law.init_state_prognostic(grid, aux, 0.0)
    prim = _stacked(grid, A.prognostic_to_primitive(law, Q, aux))        # (stacks, nv, 5, Np)
    dz = 2 * _stacked(grid, grid.vgeo[:, G._JcV, :])
    nv, W = prim.shape[1], recon.width
    faces = []
    for k in range(nv):
        hw = min(W, k, nv - 1 - k)
        cells = np.stack([np.moveaxis(prim[:, j], 1, 0) for j in range(k - hw, k + hw + 1)])   # (D, 5, stacks, Np)
        wts = np.stack([dz[:, j] for j in range(k - hw, k + hw + 1)])
        if hw == 0:
            bot, top = A.HBFVReconstruction(law, F.FVConstant())(cells, wts)
        else:
            bot, top = hb(cells, wts)
        plain_bot, plain_top = (F.FVConstant() if hw == 0 else recon)(cells, wts)
        assert np.array_equal(bot[:4], plain_bot[:4]) and np.array_equal(top[:4], plain_top[:4])
        faces.append((bot, top))
    p_surface = prim[:, 0, 4].max()
    worst = max(float(np.abs(faces[k][1][4] - faces[k + 1][0][4]).max()) for k in range(nv - 1))
    print("%s: worst face-pressure jump %.3e Pa = %.2f eps p_surface" % (inner, worst, worst / (EPS * p_surface)))
    assert worst <= HB_ULPS * EPS * p_surface


def test_host_functions_against_the_restatement(box, sphere):
    """The library's host set-up and the restatement, written apart from each other, agree bit for bit."""
    for law, grid, aux in (box, sphere):
        ps = law.ps
        phi = aux[:, law.off_phi]
        assert np.array_equal(A.vert_fvm_auxiliary_field_gradient(grid, phi), RA.fv_field_gradient(grid, phi))
        Tv, p = law.ref_state(phi / ps.grav)
        rho = p / (Tv * ps.R_d)
        got, want = A.fvm_balance(grid, rho, p, ps), RA.fvm_balance(grid, rho, p, ps.R_d, ps.grav)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert np.array_equal(got[0], aux[:, law.off_ref]) and np.array_equal(got[1], aux[:, law.off_ref + 1])
    law, grid, aux = box
    noisy, _ = CASES.balance_box(2, 8, noisy=True)
    Q = noisy.init_state_prognostic(grid, aux, 0.0)
    L = RA.DryLaw(law, 0)
    prim = L.prognostic_to_primitive(Q, aux)
    assert np.abs(prim - A.prognostic_to_primitive(law, Q, aux)).max() <= 4 * EPS * np.abs(prim).max()
    s = _stacked(grid, prim)
    w = 2 * _stacked(grid, grid.vgeo[:, G._JcV, :])[:, :, None, :]
    cells, wts = [s[:, k] for k in (2, 3, 4)], [w[:, k] for k in (2, 3, 4)]
    bot, top = A.HBFVReconstruction(law, F.FVLinear())(np.stack([np.moveaxis(c, 1, 0) for c in cells]),
                                                       np.stack([x[:, 0] for x in wts]))
    rbot, rtop = RA.HBRecon(R.Recon(True, 1, R.van_leer), ps.grav)(cells, wts)
    assert np.array_equal(np.moveaxis(bot, 0, 1), rbot) and np.array_equal(np.moveaxis(top, 0, 1), rtop)


def test_one_evaluation_cases_feel_every_hook(oracle):
    """The case the device is compared on at 1e-12 (tests/test_gpu_dgfv_atmos.py: box law, HB(FVLinear),
    Roe, Vertical, walls, noisy state) moves by far more than that when any one of the four formerly
    dead paths is taken out of the restatement: the conversions, the face auxiliary state, the
    hydrostatic wrapper, the source.  On the periodic stack the top cell's source counts twice."""
    law, grid = CASES.balance_box(2, 6, noisy=True)
    hb = RA.HBRecon(R.Recon(True, 1, R.van_leer), law.ps.grav)

    def tendency(recon=hb, periodic=False, **patch):
        lw, gr = (law, grid) if not periodic else CASES.balance_box(2, 6, periodic_stack=True, noisy=True)
        rs = RA.DGFVAtmosRestatement(lw, gr, recon, nf_first=2, direction=RA.VERTICAL)
        for name, f in patch.items():
            setattr(rs.L, name, f)
        Q = lw.init_state_prognostic(gr, rs.state_auxiliary, 0.0)
        T = np.zeros_like(Q)
        rs(T, Q, 0.3)
        return T

    full = tendency()
    scale = np.abs(full).max(axis=(0, 2))[None, :, None]
    moved = lambda T: float((np.abs(T - full) / scale).max())
    changes = {
        "conversions": moved(tendency(prognostic_to_primitive=lambda Q, aux: Q.copy(),
                                      primitive_to_prognostic=lambda prim, aux: prim.copy(), recon=hb.inner)),
        "face auxiliary state": moved(tendency(face_auxiliary_state=lambda aux, dz: aux.copy())),
        "hydrostatic wrapper": moved(tendency(recon=hb.inner)),
        "source": moved(tendency(source=lambda Q, aux: np.zeros_like(Q))),
    }
    print(changes)
    assert min(changes.values()) > 1e-6
    # the periodic top cell: its tendency holds the source twice, every other cell once
    per = tendency(recon=hb.inner, periodic=True)
    per0 = tendency(recon=hb.inner, periodic=True, source=lambda Q, aux: np.zeros_like(Q))
    lw, gr = CASES.balance_box(2, 6, periodic_stack=True, noisy=True)
    aux = lw.init_state_auxiliary(gr)
    S = RA.DryLaw(lw, 2).source(lw.init_state_prognostic(gr, aux, 0.0), aux)
    times = _stacked(gr, per - per0)[:, :, 3] / _stacked(gr, S)[:, :, 3]
    assert np.allclose(times[:, :-1], 1.0, rtol=1e-9) and np.allclose(times[:, -1], 2.0, rtol=1e-9)
