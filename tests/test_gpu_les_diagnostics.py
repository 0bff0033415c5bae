"""The AtmosLESDefault diagnostics on the device (climatemachine.jl_amd/diagnostics.py, csrc/diagnostics.hip
and the laws' ``les_diagnostics``) against the reference's known answer (test/Diagnostics/sin_test.jl),
the NumPy restatement (les_diagnostics_restatement.py) and exact sums of the device's own terms."""
import math

import numpy as np
import pytest

import les_diagnostics_restatement as R
from helpers import bomex_setup, pseudo1d_setup

pytestmark = pytest.mark.gpu

# Largest difference of a column of D from the NumPy restatement, relative to the column's largest
# magnitude, measured on the first device run: 1.82e-16 in theta_dry, theta_vir and
# theta_liq_ice with either closure (the device's pow differs from NumPy's in the last bit); every
# other column is equal bit for bit.  Four times that, and never more than 1e-12.
NODAL_TOL = min(4 * 1.82e-16, 1e-12)


def _gpu(torch, a):
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    torch.cuda.synchronize()
    return t


def _moist(cm, closure, nx=3, nz=3, N=4, rank=0, size=1):
    law, grid = bomex_setup(nx=nx, ny=nx, nz=nz, N=N, L=1500.0, rank=rank, size=size)
    law.closure = int(closure)
    return law, grid


def _dry(cm, grid, smagorinsky=True, viscosity=0.0):
    """The dry LES law on the same box: FlatOrientation, a hydrostatic reference state, Gravity."""
    A = cm.atmos
    ps = cm.moist.MoistParameters()
    setup = A.RisingBubbleSetup(ps, xc=750.0, zc=1000.0, rc=500.0)
    return A.DryAtmosModel(setup, orientation=A.ORIENT_FLAT,
                           ref_state=A.DecayingTemperatureProfile(ps, 290.0, 220.0, ps.R_d * 290.0 / ps.grav),
                           smagorinsky=ps.C_smag if smagorinsky else None, viscosity=viscosity,
                           sources=A.SRC_GRAVITY, boundary_conditions=(A.BC_ATMOS_DEFAULT, A.BC_ATMOS_DEFAULT),
                           param_set=ps)


def _collected(cm, torch, law, grid, Qh):
    """Model, diagnostics object, device state, the profiles of one collection at (Q, 0)."""
    dg = cm.dgmodel.DGModel(law, grid)
    diag = cm.diagnostics.AtmosLESDefault(dg).init()
    Q = _gpu(torch, Qh)
    prof = diag.collect(Q, 0.0)
    return dg, diag, Q, prof


@pytest.fixture(scope="module")
def cloudy(cm, torch):
    """closure -> the cloudy BOMEX-profile state on 3 x 3 x 3, N = 4, collected once; shared, read-only."""
    out = {}
    for closure in (cm.moist.CLOSURE_CONSTANT, cm.moist.CLOSURE_SMAGORINSKY):
        law, grid = _moist(cm, closure)
        Qh = R.cloudy_state(law, grid, law.init_state_auxiliary(grid))
        dg, diag, Q, prof = _collected(cm, torch, law, grid, Qh)
        D = diag.nodal(Q, 0.0).cpu().numpy()
        aux = dg.state_auxiliary.cpu().numpy()
        gf = dg.state_gradient_flux.cpu().numpy().copy()
        out[closure] = dict(law=law, grid=grid, dg=dg, diag=diag, Q=Q, Qh=Qh, prof=prof, D=D, aux=aux, gf=gf,
                            raw={k: v.copy() for k, v in diag.raw.items()})
    yield out
    for c in out.values():
        c["dg"].close()


# ---- 1. the reference's known answer ---------------------------------------------------------------
@pytest.mark.parametrize("which", ["moist", "dry"])
def test_sine_state_known_answer(cm, torch, which):
    """sin_test.jl: u = 5 and cov_w_u = 0.5 on every level, with its thresholds."""
    law, grid = _moist(cm, cm.moist.CLOSURE_SMAGORINSKY, nz=2)
    if which == "dry":
        law = _dry(cm, grid)
    Qh = R.sine_state(law, grid, law.init_state_auxiliary(grid))
    dg, diag, Q, prof = _collected(cm, torch, law, grid, Qh)
    du, dc = prof["u"] - 5.0, prof["cov_w_u"] - 0.5
    print("%s: max |u - 5| = %.2e, max |cov_w_u - 0.5| = %.2e" % (which, np.abs(du).max(), np.abs(dc).max()))
    assert (du ** 2).sum() <= 1e-16
    assert np.sqrt((dc ** 2).mean()) <= 2e-15
    names = list(prof)
    assert names[:5] == ["z", "u", "v", "w", "avg_rho"]
    assert names[-1] == ("iwp" if which == "moist" else "cov_w_ei")
    assert len(prof["u"]) == 5 * 2 and np.array_equal(prof["z"], R.onetime(grid)[0])
    dg.close()


# ---- 2. the nodal pass --------------------------------------------------------------------------------
@pytest.mark.parametrize("closure", [0, 1])
def test_nodal_columns_match_the_restatement(cm, cloudy, closure):
    c = cloudy[closure]
    law, grid, nr = c["law"], c["grid"], c["grid"].nreal
    want = R.nodal(law, c["Qh"], c["aux"], c["gf"])
    qc = want[:nr, 7] + want[:nr, 8]
    assert np.all((qc == 0) | (qc > 1e-8)), "the state is too close to the saturation threshold"
    count = c["raw"]["cloud_levels"][:, 0]
    assert (count > 0).any() and (count == 0).any(), "saturated and unsaturated levels must both occur"
    names = R.NODAL + R.NODAL_MOIST
    for s, name in enumerate(names):
        got, ref = c["D"][:nr, s], want[:nr, s]
        rel = np.abs(got - ref).max() / max(np.abs(ref).max(), np.finfo(float).tiny)
        print("closure %d column %-14s rel. difference %.2e" % (closure, name, rel))
        if name == "has_condensate":
            assert np.array_equal(got, ref)
        else:
            assert rel <= NODAL_TOL, (name, rel)


# ---- 3. the sums against exact sums ---------------------------------------------------------------------
def _levelwise(grid, T):
    """terms (nelem, nv, Np) -> (L, nv, terms of the level)"""
    Nq, Nqk, nvert, nhorz = R._shape(grid)
    nv = T.shape[1]
    X = T[:grid.nreal].reshape(nhorz, nvert, nv, Nqk, Nq * Nq)
    return X.transpose(1, 3, 2, 0, 4).reshape(nvert * Nqk, nv, nhorz * Nq * Nq)


def _check_exact(terms_by_level, device, what):
    """|device - exact| <= ulp(exact) + n 2^-100 sum |term| per level and variable (the double-double
    bound; the second part only matters where the terms cancel).  Returns whether a plain np.sum of
    the same terms differs from the exact sum somewhere."""
    L, nv, n = terms_by_level.shape
    plain_differs = False
    for evk in range(L):
        for v in range(nv):
            t = terms_by_level[evk, v]
            exact = math.fsum(t)
            bound = np.spacing(abs(exact)) + n * 2.0 ** -100 * math.fsum(np.abs(t))
            assert abs(device[evk, v] - exact) <= bound, (what, evk, v, device[evk, v], exact, bound)
            plain_differs = plain_differs or float(np.sum(t)) != exact
    return plain_differs


def _check_sums(law, grids, Qs, Ds, raw, MH_z):
    """The raw sums of one collection against exact sums of the terms of (Q, D, MH, the device's own
    finished simple averages); the finished values against the host's finishing of the raw sums."""
    ns = raw["simple_sums"].shape[1]
    moist = R.is_moist(law)
    st = np.concatenate([_levelwise(g, R.simple_terms(law, g, Q, D)) for g, Q, D in zip(grids, Qs, Ds)], axis=2)
    ht = np.concatenate([_levelwise(g, R.ho_terms(law, g, Q, D, raw["simple_avgs"]))
                         for g, Q, D in zip(grids, Qs, Ds)], axis=2)
    differs = _check_exact(st[:, :ns], raw["simple_sums"], "simple")
    differs = _check_exact(ht, raw["ho_sums"], "higher order") or differs
    if moist:
        _check_exact(st[:, ns:ns + 2], raw["cloud_levels"][:, 2:4], "water path")
    assert differs, "a plain np.sum reproduces every exact sum: the case shows nothing"
    assert np.array_equal(raw["simple_avgs"], R.finish_simple(raw["simple_sums"].copy(), MH_z, ns))
    assert np.array_equal(raw["ho_avgs"], R.finish_ho(raw["ho_sums"], MH_z, raw["simple_avgs"][:, 3]))
    if moist:
        fin = raw["cloud_levels"][:, 2:4] / MH_z[:, None] / raw["simple_avgs"][:, 3:4]
        assert np.array_equal(raw["cloud_levels"][:, 4:6], fin)


def test_sums_are_exact_sums_of_the_device_terms(cm, cloudy):
    c = cloudy[1]
    _check_sums(c["law"], [c["grid"]], [c["Qh"]], [c["D"]], c["raw"], c["diag"].MH_z)


def test_sums_are_exact_at_another_order(cm, torch):
    """N = 6, the other order the library compiles the moist law for (it compiles no mixed pair for
    it: engine_moist.hip instantiates one order in every direction)."""
    law, grid = _moist(cm, cm.moist.CLOSURE_SMAGORINSKY, nx=3, nz=2, N=6)
    Qh = R.cloudy_state(law, grid, law.init_state_auxiliary(grid))
    dg, diag, Q, prof = _collected(cm, torch, law, grid, Qh)
    assert diag.nlevels == 7 * 2 and (diag.raw["cloud_levels"][:, 0] > 0).any()
    D = diag.nodal(Q, 0.0).cpu().numpy()
    _check_sums(law, [grid], [Qh], [D], diag.raw, diag.MH_z)
    dg.close()


# ---- 4. q_tot = 0 -------------------------------------------------------------------------------------
def test_moist_law_at_zero_water_equals_the_dry_law(cm, torch):
    MO = cm.moist
    _, grid = _moist(cm, MO.CLOSURE_CONSTANT, nz=2)
    dry = _dry(cm, grid, smagorinsky=False, viscosity=75.0)
    moist = MO.MoistAtmosModel(MO.DensityCurrentSetup(dry.ps), dry.ref_state, closure=MO.CLOSURE_CONSTANT,
                               coefficient=75.0, sources=cm.atmos.SRC_GRAVITY,
                               boundary_conditions=(cm.atmos.BC_ATMOS_DEFAULT, cm.atmos.BC_ATMOS_DEFAULT),
                               param_set=dry.ps)
    Qm = R.cloudy_state(moist, grid, moist.init_state_auxiliary(grid))
    assert np.all(Qm[:, 5] == 0.0)
    dgm, _, _, pm = _collected(cm, torch, moist, grid, Qm)
    dgd, _, _, pd = _collected(cm, torch, dry, grid, Qm[:, :5].copy())
    shared = R.SIMPLE + R.HO
    assert len(shared) == 24
    for name in shared:
        assert np.array_equal(pm[name], pd[name]), name
    assert np.abs(pm["w_ht_sgs"]).max() > 0 and np.abs(pm["cov_w_u"]).max() > 0
    dgm.close()
    dgd.close()


# ---- 5. ranks -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [2, 3])
def test_group_collect_over_local_ranks(cm, torch, size):
    DI = cm.diagnostics
    law, grid = _moist(cm, cm.moist.CLOSURE_SMAGORINSKY, nx=4, nz=2)
    Qh = R.cloudy_state(law, grid, law.init_state_auxiliary(grid))
    dg, diag, Q, single = _collected(cm, torch, law, grid, Qh)
    single_raw = {k: v.copy() for k, v in diag.raw.items()}
    dgs, grids, Qhs, Qs = [], [], [], []
    for r in range(size):
        lr, gr = _moist(cm, cm.moist.CLOSURE_SMAGORINSKY, nx=4, nz=2, rank=r, size=size)
        dgs.append(cm.dgmodel.DGModel(lr, gr))
        grids.append(gr)
        Qhs.append(R.cloudy_state(lr, gr, lr.init_state_auxiliary(gr)))
        Qs.append(_gpu(torch, Qhs[-1]))
    assert sum(g.nreal for g in grids) == grid.nreal
    cm.dgmodel.connect_local(dgs)
    prof, diags = DI.group_collect(dgs, Qs, 0.0)
    raw = {k: v.copy() for k, v in diags[0].raw.items()}
    Ds = [d.nodal(q, 0.0).cpu().numpy() for d, q in zip(diags, Qs)]
    _check_sums(law, grids, Qhs, Ds, raw, diags[0].MH_z)
    assert np.array_equal(prof["z"], single["z"])
    assert np.array_equal(raw["cloud_levels"][:, :2], single_raw["cloud_levels"][:, :2])
    assert np.array_equal(raw["cloud_scalars"][5:7], single_raw["cloud_scalars"][5:7])
    assert prof["cld_top"] == single["cld_top"] and prof["cld_base"] == single["cld_base"]
    assert prof["cld_cover"] == single["cld_cover"]
    # (MH_z: the same terms in another partition, each within an ulp of the exact sum)
    assert np.abs(diags[0].MH_z - diag.MH_z).max() <= 2 * np.spacing(diag.MH_z.max())
    again, _ = DI.group_collect(dgs, Qs, 0.0, diags=diags)
    for k, v in raw.items():
        assert np.array_equal(v, diags[0].raw[k]), k
    for k in prof:
        assert np.array_equal(prof[k], again[k], equal_nan=True), k
    with pytest.raises(cm._lib.CmdgError, match="cmdg_group_les"):
        diags[0].collect(Qs[0], 0.0, evaluate=False)
    for d in dgs + [dg]:
        d.close()


def test_rccl_communicator_of_one_rank_equals_the_plain_handle(cm, torch, cloudy):
    """The all-gather path of a handle with an RCCL communicator (one rank here): same bits."""
    c = cloudy[1]
    dg = cm.dgmodel.DGModel(c["law"], c["grid"])
    dg.comm_init_rccl(cm.dgmodel.rccl_unique_id(), 0, 1)
    diag = cm.diagnostics.AtmosLESDefault(dg).init()
    prof = diag.collect(c["Q"], 0.0)
    assert np.array_equal(diag.MH_z, c["diag"].MH_z)
    for k, v in c["raw"].items():
        assert np.array_equal(v, diag.raw[k], equal_nan=True), k
    for k in prof:
        assert np.array_equal(prof[k], c["prof"][k], equal_nan=True), k
    dg.close()


def test_two_collections_return_the_same_bits(cm, cloudy):
    c = cloudy[1]
    again = c["diag"].collect(c["Q"], 0.0)
    for k, v in c["raw"].items():
        assert np.array_equal(v, c["diag"].raw[k], equal_nan=True), k
    for k in again:
        assert np.array_equal(again[k], c["prof"][k], equal_nan=True), k


# ---- 6. cloud statistics and water paths ------------------------------------------------------------------
@pytest.mark.parametrize("closure", [0, 1])
def test_cloud_statistics_match_the_restatement(cm, cloudy, closure):
    c = cloudy[closure]
    law, grid, prof, raw = c["law"], c["grid"], c["prof"], c["raw"]
    want = R.collect(law, grid, c["Qh"], c["aux"], c["gf"], D=c["D"])
    assert np.array_equal(raw["cloud_levels"][:, 0], want["_raw"]["count"])
    assert np.all(raw["cloud_levels"][:, 1] == want["_raw"]["ncol"])
    assert np.array_equal(prof["cld_frac"], want["cld_frac"])
    assert 0 < prof["cld_cover"] < 1 and prof["cld_cover"] == want["cld_cover"]
    assert prof["cld_top"] == want["cld_top"] and prof["cld_base"] == want["cld_base"]
    assert prof["cld_base"] < prof["cld_top"]
    # the device's per-level values, finished on the host in the reference's order
    assert prof["lwp"] == R.water_path(raw["cloud_levels"][:, 4], grid) and prof["lwp"] > 0
    assert prof["iwp"] == R.water_path(raw["cloud_levels"][:, 5], grid)
    # ... and the restatement's plain sums agree to summation rounding (225 nodes a level)
    assert abs(prof["lwp"] - want["lwp"]) <= 1e-12 * want["lwp"]


# ---- 7. the callback, and what is refused --------------------------------------------------------------------
def test_callback_records_profiles_during_a_solve(cm, torch, tmp_path):
    law, grid = _moist(cm, cm.moist.CLOSURE_SMAGORINSKY, nz=2)
    dg = cm.dgmodel.DGModel(law, grid)
    Q = dg.init_ode_state(0.0)
    solver = cm.odesolvers.LSRK54CarpenterKennedy(dg, Q, dt=0.05)
    seen = []
    cb = cm.diagnostics.AtmosLESDefaultCallback(dg, sink=lambda t, p: seen.append(t))
    cm.odesolvers.solve(Q, solver, numberofsteps=4, callbacks=[(2, cb)])
    assert len(cb.records) == 2 and len(seen) == 2
    assert [t for t, _ in cb.records] == pytest.approx([0.1, 0.2])
    for _, p in cb.records:
        assert np.isfinite(p["avg_rho"]).all() and (p["avg_rho"] > 0).all()
    path = cb.save(str(tmp_path / "series.npz"))
    with np.load(path) as f:
        assert f["avg_rho"].shape == (2, 10) and f["time"].shape == (2,) and f["lwp"].shape == (2,)
    dg.close()


def test_refusals_say_why(cm, torch):
    DI = cm.diagnostics
    # a law without the hook
    law, grid, _ = pseudo1d_setup(Ne=2)
    dg = cm.dgmodel.DGModel(law, grid)
    with pytest.raises(cm._lib.CmdgError, match="defines no LES diagnostics"):
        DI.AtmosLESDefault(dg)
    dg.close()
    # a grid that is not stacked
    law, sgrid = _moist(cm, cm.moist.CLOSURE_SMAGORINSKY, nz=2)
    M = cm.mesh
    rng = [np.linspace(0.0, 1500.0, 3), np.linspace(0.0, 1500.0, 3), np.linspace(0.0, 3000.0, 3)]
    topl = M.BrickTopology(rng, periodicity=(True, True, False), boundary=((0, 0), (0, 0), (1, 2)))
    dg = cm.dgmodel.DGModel(law, M.DiscontinuousSpectralElementGrid(topl, 4))
    with pytest.raises(cm._lib.CmdgError, match="not stacked"):
        DI.AtmosLESDefault(dg)
    dg.close()
    # a state of the wrong size, and a collection before the one-time collection
    dg = cm.dgmodel.DGModel(law, sgrid)
    diag = DI.AtmosLESDefault(dg)
    with pytest.raises(ValueError, match="shape"):
        diag.collect(dg.create_state(5), 0.0)
    with pytest.raises(ValueError, match="init"):
        diag.collect(dg.create_state(), 0.0)
    res = cm._lib.CmdgLesResult()
    import ctypes as C
    assert dg.L.cmdg_les_collect(dg.handle, dg.create_state().data_ptr(), 0.0, C.byref(res)) != 0
    assert b"cmdg_les_init has not run" in dg.L.cmdg_last_error(dg.handle)
    dg.close()
