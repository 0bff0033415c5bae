"""The moist LES law on the device away from the warm branch: ice, mixed phase, the two kinks of the
liquid fraction, barely saturated air, a Newton start clamped at T_min.  ``-m gpu``.

(a) the saturation adjustment node by node against tests/golden/moist_phase_cases.npz (40-digit answers,
    tests/moist_phase_restatement.py; the fixture is read as data, mpmath is not needed here);
(b) the whole operator, LSRK steps and Courant numbers on a smooth state that crosses every regime
    (helpers.cold_cloudy_state) against the oracle;
(c) RoeNumericalFluxMoist on that state, with a potential and with water;
(d) the LES diagnostics: the nodal pass on that state against its NumPy restatement, and on the grid of
    (a) against the fixture.

Every law runs the adjustment with maxiter 40 and tolerance 1e-11 K.  Bounds of (a): the temperature to the
stopping tolerance, 1e-11 K; condensate to 1e-12 q_tot and theta_v to 1e-12 relative (the project's tolerance);
unsaturated air holds no condensate at all and its temperature is within 2 ulp of the all-vapour closed
form evaluated in double on the energy the kernel is handed.  Observed maxima: DESIGN.md section 5.
"""
import ctypes as C
import os

import numpy as np
import pytest

import les_diagnostics_restatement as LR
from helpers import (cold_cloudy_state, moist_converged_law, observe, periodic_brick_grid, phase_census,
                     rel_linf, rising_bubble_setup, tile_moist_phase_cases)
from test_gpu_les_diagnostics import NODAL_TOL
from test_roe_moist_oracle import FLUXES

pytestmark = pytest.mark.gpu
TOL = 1e-12
UNSATURATED, CLAMPED = 6, 7          # indices of the groups in the fixture (moist_phase_restatement.GROUPS)


def _gpu(torch, a):
    x = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return x


@pytest.fixture(scope="module")
def cases():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "moist_phase_cases.npz")
    with np.load(path) as f:
        return {n: f[n] for n in f.files}


# ---- (a), (d2): node by node against the fixture ---------------------------------------------------------
@pytest.fixture(scope="module", params=[4, 6])
def pointwise(request, cm, torch, cases):
    """The fixture's cases tiled over the smallest bubble grid (N = 4: 1000 nodes; N = 6: Np = 343, no
    multiple of the wave size), one evaluation, the refreshed auxiliary state and the nodal
    diagnostics; shared, read-only."""
    N = request.param
    law = moist_converged_law()
    _, grid = rising_bubble_setup(nx=2, ny=2, nz=2, N=N)
    dg = cm.dgmodel.DGModel(law, grid)
    Q, idx = tile_moist_phase_cases(grid, dg.state_auxiliary.cpu().numpy(), cases, seed=N)
    assert len(np.unique(idx)) == len(cases["rho"])                 # every case is somewhere
    Qg = _gpu(torch, Q)
    dg(dg.create_state(), Qg, 0.0, 1.0, 0.0)
    dg.synchronize()
    aux = dg.state_auxiliary.cpu().numpy()
    D = cm.diagnostics.AtmosLESDefault(dg).nodal(Qg, 0.0).cpu().numpy()
    yield dict(N=N, law=law, grid=grid, Q=Q, idx=idx, aux=aux, D=D)
    dg.close()


def test_adjustment_pointwise_matches_the_40_digit_root(pointwise, cases):
    p, idx = pointwise, pointwise["idx"]
    aux, Q, ps = p["aux"], p["Q"], p["law"].ps
    ref = {n: cases[n][idx] for n in ("T", "q_liq", "q_ice", "theta_v", "q_tot")}
    T, thv, ql, qi = (aux[:, 15 + i] for i in range(4))
    dT = np.abs(T - ref["T"])
    dql = np.abs(ql - ref["q_liq"]) / ref["q_tot"]
    dqi = np.abs(qi - ref["q_ice"]) / ref["q_tot"]
    dth = np.abs(thv / ref["theta_v"] - 1)
    tag = "moist phases N=%d " % p["N"]
    print("%s|dT| %.2e K  |dq_liq|/q_tot %.2e  |dq_ice|/q_tot %.2e  theta_v rel. %.2e" % (
        tag, dT.max(), dql.max(), dqi.max(), dth.max()))
    for g in range(int(cases["group"].max()) + 1):
        m = cases["group"][idx] == g
        print("   group %d: |dT| %.2e  |dq_liq| %.2e  |dq_ice| %.2e  theta_v %.2e" % (
            g, dT[m].max(), dql[m].max(), dqi[m].max(), dth[m].max()))
    assert np.isfinite(aux[:, 15:19]).all()
    assert observe(tag + "|T - T_ref| (K)", dT.max()) <= 1e-11
    assert observe(tag + "|q_liq - ref| / q_tot", dql.max()) <= 1e-12
    assert observe(tag + "|q_ice - ref| / q_tot", dqi.max()) <= 1e-12
    assert observe(tag + "theta_v rel.", dth.max()) <= 1e-12
    # unsaturated air: no condensate at all, and the all-vapour closed form
    un = cases["group"][idx] == UNSATURATED
    assert un.sum() >= 64 and not ql[un].any() and not qi[un].any()
    rho = Q[:, 0]
    rhoinv = 1 / rho
    kin = rhoinv * (Q[:, 1] * Q[:, 1] + Q[:, 2] * Q[:, 2] + Q[:, 3] * Q[:, 3]) / 2
    e_int = rhoinv * (Q[:, 4] - kin - rho * aux[:, 3])
    qt = Q[:, 5] / rho
    closed = ps.T_0 + (e_int - qt * (ps.LH_v0 - ps.R_v * ps.T_0)) / ps.cv_m(qt)
    ulps = np.abs(T - closed)[un] / np.spacing(closed[un])
    print("   unsaturated T: %.1f ulp from the closed form" % ulps.max())
    assert observe(tag + "unsaturated T (ulp of the closed form)", ulps.max()) <= 2


def test_diagnostics_pointwise_match_the_fixture(pointwise, cases):
    """pres, theta_dry, theta_vir, theta_liq_ice, q_vap (and temp, h_int, the condensate columns) of the
    nodal diagnostics pass from their definitions at 40 digits; ``has_condensate`` exact."""
    p, idx, D = pointwise, pointwise["idx"], pointwise["D"]
    tag = "moist phases N=%d diagnostics " % p["N"]
    q_tot = cases["q_tot"][idx]
    clamped = cases["group"][idx] == CLAMPED
    for col, name in ((1, "pres"), (2, "theta_dry"), (10, "theta_vir"), (11, "theta_liq_ice"), (9, "q_vap"),
                      (5, "h_int")):
        each = np.abs(D[:, col] / cases[name][idx] - 1)
        rel = each[~clamped].max() if name == "q_vap" else each.max()
        print("%s%-14s rel. %.2e" % (tag, name, rel))
        assert observe(tag + name + " rel.", rel) <= 1e-12, name
    # q_vap = q_tot - q_liq - q_ice is formed from the stored doubles.  In the clamped-start group all but
    # 1e-4 of the water is ice, so the rounding of q_ice to a double (half an ulp of q_tot at most, as for
    # q_liq and for the two subtractions) is worth more than 1e-12 of what is left: the bound there is
    # 1e-12 relative plus two ulp of q_tot.
    dqv = np.abs(D[:, 9] - cases["q_vap"][idx])[clamped]
    print("%sq_vap, clamped start: %.2f ulp of q_tot" % (tag, (dqv / np.spacing(q_tot[clamped])).max()))
    assert (dqv <= 1e-12 * cases["q_vap"][idx][clamped] + 2 * np.spacing(q_tot[clamped])).all()
    assert np.abs(D[:, 0] - cases["T"][idx]).max() <= 1e-11
    assert (np.abs(D[:, 7] - cases["q_liq"][idx]) <= 1e-12 * q_tot).all()
    assert (np.abs(D[:, 8] - cases["q_ice"][idx]) <= 1e-12 * q_tot).all()
    cond = (cases["q_liq"] + cases["q_ice"])[idx]
    sure = cond > 1e-8 * q_tot
    assert sure.sum() > 0.7 * sure.size and np.array_equal(D[:, 12][sure], np.ones(int(sure.sum())))
    assert not D[:, 12][cond == 0].any()


# ---- (b): the whole operator on a cold cloudy smooth state ---------------------------------------------
def _cold(cm, oracle, closure, N, **kw):
    law = moist_converged_law(closure)
    _, grid = rising_bubble_setup(**dict(dict(nx=3, ny=2, nz=3) if N == 4 else dict(nx=2, ny=2, nz=2), N=N))
    odg = oracle.OracleDGModel(law, grid, **kw)
    return law, grid, odg, cold_cloudy_state(law, grid, odg.state_auxiliary)


def _assert_every_regime(odg):
    census = phase_census(odg.state_auxiliary)
    print("oracle's refreshed state:", census)
    for regime in ("ice", "mixed", "warm", "unsaturated"):
        assert census[regime] >= 20, (regime, census)
    assert census["T_min"] < 225 and census["T_max"] > 290


def _assert_moisture_block(dg, odg, name):
    """temperature, theta_v, q_liq, q_ice as the device's nodal refresh left them, against the oracle's."""
    auxg = dg.state_auxiliary.cpu().numpy()
    for c in (15, 16, 17, 18):
        sc = max(np.abs(odg.state_auxiliary[:, c]).max(), 1e-300)
        assert observe(name, np.abs(auxg[:, c] - odg.state_auxiliary[:, c]).max() / sc) < TOL, c


@pytest.mark.parametrize("closure,N", [(0, 4), (1, 4), (2, 4), (1, 6)])
def test_cold_cloudy_operator_matches_oracle(cm, oracle, torch, closure, N):
    """Tendency, gradient flux and the refreshed moisture block of one evaluation, then two LSRK54 steps."""
    law, grid, odg, Q0 = _cold(cm, oracle, closure, N)
    dg = cm.dgmodel.DGModel(law, grid)
    tag = "moist phases cold closure %d N=%d " % (closure, N)
    T0 = np.random.default_rng(closure).standard_normal(Q0.shape)
    for alpha, beta in ((1.0, 0.0), (0.5, 2.0)):
        To = T0.copy()
        odg(To, Q0.copy(), 0.0, alpha, beta)
        Tg = _gpu(torch, T0)
        dg(Tg, _gpu(torch, Q0), 0.0, alpha, beta)
        Tn = Tg.cpu().numpy()
        for s in range(6):
            assert observe(tag + "tendency", rel_linf(Tn[:, s], To[:, s])) < TOL, s
        gfg = dg.state_gradient_flux.cpu().numpy()
        for s in range(law.ngradflux):
            sc = max(np.abs(odg.state_gradient_flux[:, s]).max(), 1e-300)
            assert observe(tag + "gradient flux", np.abs(gfg[:, s] - odg.state_gradient_flux[:, s]).max() / sc) < TOL, s
    _assert_every_regime(odg)
    _assert_moisture_block(dg, odg, tag + "aux")
    Qo, dQo = Q0.copy(), np.zeros_like(Q0)
    for i in range(2):
        oracle.lsrk54_step(odg, Qo, dQo, i * 0.02, 0.02)
    Q = _gpu(torch, Q0)
    dQ = torch.zeros_like(Q)
    dg.lsrk_run(Q, dQ, 0.0, 0.02, 2, oracle.RKA, oracle.RKB, oracle.RKC)
    dg.synchronize()
    Qn = Q.cpu().numpy()
    assert np.abs(Qo - Q0).max() > 0
    for s in range(6):
        assert observe(tag + "two LSRK steps", rel_linf(Qn[:, s], Qo[:, s])) < TOL, s
    dg.close()


def _oracle_courant_field(oracle, kind, odg, Q, dt, direction):
    """``oracle.courant`` before its maximum: the local Courant number of every node."""
    pw = oracle.min_neighbor_distance(odg.og, direction)
    oracle.lib().orc_local_courant(odg.ph.c, C.byref(odg.og.c), int(kind), oracle._p(pw), oracle._p(Q),
                                   oracle._p(odg.state_auxiliary), oracle._p(odg.state_gradient_flux),
                                   C.c_double(dt), C.c_double(0.0), int(direction))
    return pw


@pytest.mark.parametrize("jet", [False, True])
def test_cold_cloudy_courant_numbers_match_oracle(cm, oracle, torch, jet):
    """Kind 1 (nondiffusive) repeats the saturation adjustment inside the Courant kernel.  A Courant
    number is a maximum over the nodes, and on the state as it stands the sound speed puts it on a warm
    node at the bottom; ``jet`` adds a zonal jet of 70 m/s at mid-height, strongest where the
    supersaturation is, so that the maximum of kind 1 over every direction and over the horizontal ones
    sits on a mixed-phase node (asserted).  Without the jet this test cannot see an error in the ice
    branch; with it, it does (mutation check)."""
    law, grid, odg, Q0 = _cold(cm, oracle, 1, 4)
    if jet:
        Q0 = cold_cloudy_state(law, grid, odg.state_auxiliary, jet=70.0)
    dg = cm.dgmodel.DGModel(law, grid)
    odg(np.zeros_like(Q0), Q0.copy(), 0.0, 1.0, 0.0)                 # fills the gradient flux (eddy viscosity)
    _assert_every_regime(odg)
    Qg = _gpu(torch, Q0)
    dg(torch.zeros_like(Qg), Qg, 0.0, 1.0, 0.0)
    for kind in (0, 1, 2):
        for d in (0, 1, 2):
            o = oracle.courant(kind, odg, Q0, 0.3, 0.0, d)
            g = dg.courant(kind, Qg, 0.3, 0.0, d)
            assert o > 0 and observe("moist phases cold courant", abs(g - o) / abs(o)) <= 1e-11, (kind, d, g, o)
            if jet and kind == 1 and d != 2:            # (the vertical direction sees w alone)
                field = _oracle_courant_field(oracle, kind, odg, Q0, 0.3, d)
                e, n = np.unravel_index(np.argmax(field), field.shape)
                assert field[e, n] == o
                assert odg.state_auxiliary[e, 17, n] > 1e-6 and odg.state_auxiliary[e, 18, n] > 1e-6, (d, e, n)
    dg.close()


# ---- (c): RoeNumericalFluxMoist with a potential and with water --------------------------------------------
@pytest.mark.parametrize("nf,name", FLUXES)
def test_roe_moist_on_the_cold_cloudy_state(cm, oracle, torch, nf, name):
    """The grid of the moist isentropic vortex (periodic brick, 5 x 5 x 1, N = 4) stretched to 1500 m, under a
    law with FlatOrientation, Gravity and a reference state, so that Phi enters the energy column of the
    Roe matrix and the Roe-averaged PhaseEquil state is cloudy, mixed or icy from face to face."""
    MO = cm.moist
    law = moist_converged_law(MO.CLOSURE_CONSTANT, coefficient=0.0, kinematic=False, boundary_conditions=())
    grid = periodic_brick_grid()
    odg = oracle.OracleDGModel(law, grid, nf_first=nf, direction=0)
    dg = cm.dgmodel.DGModel(law, grid, numerical_flux_first_order=nf, direction=0)
    Q0 = cold_cloudy_state(law, grid, odg.state_auxiliary)
    assert np.ptp(odg.state_auxiliary[:, law.off_phi]) > 1e4
    To = np.zeros_like(Q0)
    odg(To, Q0.copy(), 0.0, 1.0, 0.0)
    _assert_every_regime(odg)
    Q = _gpu(torch, Q0)
    T = dg.create_state()
    torch.cuda.synchronize()
    dg(T, Q, 0.0, 1.0, 0.0)
    Tg = T.cpu().numpy()
    assert np.abs(To[:, 5]).max() > 0 and np.abs(Tg[:, 5]).max() > 0           # water moves
    for s in range(6):
        assert observe("moist phases cold " + name, rel_linf(Tg[:, s], To[:, s])) < 1e-11, (name, s)
    _assert_moisture_block(dg, odg, "moist phases cold " + name + " aux")
    dg.close()


# ---- (d1): the nodal diagnostics pass on the cold cloudy state ----------------------------------------------
@pytest.mark.parametrize("closure", [0, 1])
def test_cold_cloudy_nodal_diagnostics_match_the_restatement(cm, oracle, torch, closure):
    """The first run of the q_ice terms of ``les_diagnostics``: R_m, cp_m, theta_liq_ice with LH_s0."""
    law, grid, odg, Q0 = _cold(cm, oracle, closure, 4)
    dg = cm.dgmodel.DGModel(law, grid)
    Qg = _gpu(torch, Q0)
    dg(dg.create_state(), Qg, 0.0, 1.0, 0.0)
    dg.synchronize()
    D = cm.diagnostics.AtmosLESDefault(dg).nodal(Qg, 0.0).cpu().numpy()
    aux, gf = dg.state_auxiliary.cpu().numpy(), dg.state_gradient_flux.cpu().numpy()
    # the restatement takes T, q_liq and q_ice from the device's refresh: they are the oracle's
    odg(np.zeros_like(Q0), Q0.copy(), 0.0, 1.0, 0.0)
    _assert_moisture_block(dg, odg, "moist phases cold nodal aux")
    census = phase_census(aux)
    assert min(census[r] for r in ("ice", "mixed", "warm", "unsaturated")) >= 20, census
    want = LR.nodal(law, Q0, aux, gf)
    assert want[:, 8].max() > 1e-6                                            # q_ice
    for s, name in enumerate(LR.NODAL + LR.NODAL_MOIST):
        got, ref = D[:grid.nreal, s], want[:grid.nreal, s]
        rel = np.abs(got - ref).max() / max(np.abs(ref).max(), np.finfo(float).tiny)
        print("closure %d column %-14s rel. difference %.2e" % (closure, name, rel))
        if name == "has_condensate":
            assert np.array_equal(got, ref)
        else:
            assert observe("moist phases cold nodal " + name, rel) <= NODAL_TOL, (name, rel)
    dg.close()
