"""NTracers of the dry atmosphere law on the device (``-m gpu``).

The oracle's dry law is frozen without tracers.  What pins the tracer columns here:
the tracer-free handle for the five leading states; the oracle's AdvectionDiffusion law through the
cross-law identity of tests/tracers_crosslaw.py; ``rho chi = c rho`` against the mass tendency;
linearity in ``delta_chi``; conservation between impermeable walls; one rank against three.
Parity bar: 1e-12 scaled by the maximum of the compared field."""
import numpy as np
import pytest

from helpers import cm, observe
import tracers_crosslaw as TC

pytestmark = pytest.mark.gpu
A = cm.atmos
TOL = 1e-12
EVERY, HORIZONTAL, VERTICAL = 0, 1, 2
RUSANOV, CENTRAL = 0, 1


def _gpu(torch, a):
    x = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return x


def _dg(law, grid, nf=RUSANOV, d=EVERY, dd=None):
    return cm.dgmodel.DGModel(law, grid, numerical_flux_first_order=nf, direction=d, diffusion_direction=dd)


def _tendency(torch, law, grid, Q, nf=RUSANOV, d=EVERY, dd=None):
    dg = _dg(law, grid, nf, d, dd)
    Qg = _gpu(torch, Q)
    T = torch.full_like(Qg, float("nan"))
    dg(T, Qg, 0.0)
    dg.synchronize()
    out = T[:grid.nreal].cpu().numpy()
    dg.close()
    assert np.isfinite(out).all()
    return out


def _steps(torch, law, grid, Q, dt, nsteps, nf=RUSANOV, d=EVERY, dd=None):
    dg = _dg(law, grid, nf, d, dd)
    Qg = _gpu(torch, Q)
    dQ = torch.zeros_like(Qg)
    s = cm.odesolvers.LSRK54CarpenterKennedy(dg, Qg, dt=dt)
    dg.lsrk_run(Qg, dQ, 0.0, dt, nsteps, s.RKA, s.RKB, s.RKC)
    dg.synchronize()
    out = Qg[:grid.nreal].cpu().numpy()
    dg.close()
    assert np.isfinite(out).all()
    return out


def _leading(tag, wide, narrow):
    bits = True
    for s in range(5):
        err = TC.scaled_linf(wide[:, s], narrow[:, s])
        bits = bits and np.array_equal(wide[:, s], narrow[:, s])
        print("%s state %d: %.3e" % (tag, s, err))
        assert err <= TOL, (tag, s, err)
    print("%s: leading states bit-identical: %s" % (tag, bits))


# ---- 1. the leading states do not see the tracers ------------------------------------------------
LEADING = {
    "brick": (TC.periodic_brick, lambda delta: TC.plain_model(delta), (1.0, 3.0), (EVERY, None), 0.1),
    "sphere": (TC.sphere, lambda delta: TC.sphere_model(delta), (2.0,), (EVERY, HORIZONTAL), 2.0),
    "box_smagorinsky": (TC.walled_box, lambda delta: TC.box_model(delta, smagorinsky=True), (1.0, 3.0),
                        (EVERY, None), None),
}


@pytest.mark.parametrize("case", sorted(LEADING))
def test_leading_states_equal_the_tracer_free_handle(torch, case):
    """(a) periodic brick, <F,F,F>, nu != 0, NT = 2; (b) sphere, <T,T,T>, Rusanov, NT = 1; (c) walled
    box, SmagorinskyLilly, NT = 2.  (a) and (b) again after two LSRK54 steps of ``cmdg_lsrk_run``: the
    fused update, and on the sphere the gradient-argument hand-off."""
    mkgrid, mklaw, delta, (d, dd), dt = LEADING[case]
    grid = mkgrid()
    wide, narrow = mklaw(delta), mklaw(None)
    Q, _ = TC.initial_state(wide, grid)
    Tw = _tendency(torch, wide, grid, Q, d=d, dd=dd)
    Tn = _tendency(torch, narrow, grid, Q[:, :5].copy(), d=d, dd=dd)
    _leading(case + " tendency", Tw, Tn)
    assert all(np.abs(Tw[:, 5 + k]).max() > 0 for k in range(len(delta)))
    if dt is not None:
        Qw = _steps(torch, wide, grid, Q, dt, 2, d=d, dd=dd)
        Qn = _steps(torch, narrow, grid, Q[:, :5].copy(), dt, 2, d=d, dd=dd)
        _leading(case + " two LSRK54 steps", Qw, Qn)
        assert all(not np.array_equal(Qw[:, 5 + k], Q[:grid.nreal, 5 + k]) for k in range(len(delta)))


# ---- 2. the cross-law identity ---------------------------------------------------------------------
@pytest.mark.parametrize("d,dd", [(EVERY, None), (HORIZONTAL, None), (VERTICAL, None), (EVERY, HORIZONTAL)])
def test_tracer_tendency_equals_the_advection_diffusion_law(torch, oracle, d, dd):
    """Periodic brick, NT = 2, delta = (1, 3), different fields in the two tracers, Rusanov: the
    device's tracer tendency against the oracle's AdvectionDiffusion law (advection by rho u / rho plus
    diffusion of chi with rho delta D_t I), per tracer."""
    def make_dg(law, grid, di, ddi, nf):
        return oracle.OracleDGModel(law, grid, nf_first=nf, direction=di, diffusion_direction=ddi)

    grid = TC.periodic_brick()
    law = TC.plain_model((1.0, 3.0))
    Q, _ = TC.initial_state(law, grid)
    T = _tendency(torch, law, grid, Q, nf=RUSANOV, d=d, dd=dd)
    for k in range(2):
        expect = TC.crosslaw_expected(make_dg, grid, law, Q, k, direction=d, diffusion_direction=dd, nf=RUSANOV)
        err = TC.scaled_linf(T[:, 5 + k], expect)
        print("direction %s/%s tracer %d: %.3e (max |T| %.3e)" % (d, dd, k, err, np.abs(expect).max()))
        assert err <= TOL, (k, err)
    # the two tracers are told apart: the other one's field or delta is off by far more than the bar
    other = TC.crosslaw_expected(make_dg, grid, law, Q, 1, direction=d, diffusion_direction=dd, nf=RUSANOV)
    assert TC.scaled_linf(T[:, 5], other) > 1e-3


# ---- 3. a uniform mixing ratio follows the mass ----------------------------------------------------
@pytest.mark.parametrize("variant", ["hyperdiffusion_inviscid", "viscous"])
def test_uniform_mixing_ratio_on_the_sphere(torch, variant):
    """rho chi_k = c_k rho under the central first-order flux: T[rho chi_k] = c_k T[rho].  The
    sphere's orientation flips, the wall faces, and neither sources nor hyperdiffusion touch a tracer."""
    c = (0.25, 3.0)
    if variant == "viscous":
        law = TC.sphere_model((1.0, 3.0), viscosity=TC.NU, hyperdiffusion=False, mixing=c)
    else:
        law = TC.sphere_model((1.0, 3.0), viscosity=0.0, hyperdiffusion=True, mixing=c)
    grid = TC.sphere()
    Q, _ = TC.initial_state(law, grid)
    T = _tendency(torch, law, grid, Q, nf=CENTRAL, d=EVERY, dd=HORIZONTAL)
    assert np.abs(T[:, 0]).max() > 0
    for k in range(2):
        err = TC.scaled_linf(T[:, 5 + k], c[k] * T[:, 0])
        print("%s tracer %d: %.3e" % (variant, k, err))
        assert err <= TOL, (k, err)


# ---- 4. delta slots and linearity under a space-dependent D_t -----------------------------------
def test_delta_slots_and_linearity_smagorinsky(torch):
    grid = TC.walled_box()
    one = TC.box_model((1.0, 1.0), smagorinsky=True)        # only its state is used
    Q, _ = TC.initial_state(one, grid)
    Q[:, 6] = Q[:, 5]                                          # all tracers hold the same field
    T01 = _tendency(torch, TC.box_model((0.0, 1.0), smagorinsky=True), grid, Q)
    T13 = _tendency(torch, TC.box_model((1.0, 3.0), smagorinsky=True), grid, Q)
    A0 = T01[:, 5]
    assert np.array_equal(T01[:, 6], T13[:, 5])               # delta = 1 in slot 1 and in slot 0
    d1, d3 = T13[:, 5] - A0, T13[:, 6] - A0
    assert np.abs(d1).max() > 0
    err = float(np.abs(d3 - 3 * d1).max() / np.abs(d3).max())
    print("linearity in delta: %.3e; |diffusive part| / |tendency| = %.3e" % (err, np.abs(d1).max() / np.abs(A0).max()))
    assert err <= TOL


# ---- 5. impermeable walls: conservation ----------------------------------------------------------
def test_tracer_mass_is_conserved_between_walls(torch):
    """Walled box, <T,T,F>, nu != 0, Rusanov, 5 LSRK54 steps at Courant 0.5: rho chi_k is conserved as
    well as rho is (the same telescoping of face fluxes; 5e-14 is advection_sphere.jl:431's bound)."""
    grid = TC.walled_box()
    law = TC.box_model((1.0, 3.0))
    Q, _ = TC.initial_state(law, grid)
    dx = cm.mesh.grids.min_node_distance(grid)
    speed = np.sqrt((Q[:, 1:4] ** 2).sum(axis=1)).max() / Q[:, 0].min() + np.sqrt(1.4 * law.ps.R_d * 300.0)
    dt = 0.5 * dx / speed
    dg = _dg(law, grid)
    Qg = _gpu(torch, Q)
    before = [cm.reductions.weightedsum(dg, Qg, states=[s + 1]) for s in (0, 5, 6)]
    dQ = torch.zeros_like(Qg)
    s = cm.odesolvers.LSRK54CarpenterKennedy(dg, Qg, dt=dt)
    dg.lsrk_run(Qg, dQ, 0.0, dt, 5, s.RKA, s.RKB, s.RKC)
    dg.synchronize()
    after = [cm.reductions.weightedsum(dg, Qg, states=[s + 1]) for s in (0, 5, 6)]
    moved = float((Qg[:grid.nreal, 5].cpu().numpy() - Q[:grid.nreal, 5]).__abs__().max())
    dg.close()
    rel = [abs(a - b) / abs(b) for a, b in zip(after, before)]
    print("relative change of the integrals: rho %.3e, rho chi_1 %.3e, rho chi_2 %.3e (dt = %.3e)" % (*rel, dt))
    assert moved > 0
    bound = max(10 * rel[0], 5e-14)
    assert rel[1] <= bound and rel[2] <= bound, (rel, bound)


# ---- 6. three ranks of one process -------------------------------------------------------------------
def test_three_ranks_equal_one_on_the_sphere(torch):
    """The sphere with one tracer as three ranks through the group entries against one rank: the
    tendency (1e-12) and two LSRK54 steps (1e-11), the bars of tests/test_gpu_orders_partitioned.py."""
    law = TC.sphere_model((2.0,))
    grid = TC.sphere()
    Q, _ = TC.initial_state(law, grid)
    dt, kw = 2.0, dict(d=EVERY, dd=HORIZONTAL)
    T1 = _tendency(torch, law, grid, Q, **kw)
    Q1 = _steps(torch, law, grid, Q, dt, 2, **kw)
    pos = {int(g): i for i, g in enumerate(grid.topology.globalelems[:grid.nreal])}
    grids = [TC.sphere(rank=r, size=3) for r in range(3)]
    assert sum(g.nreal for g in grids) == grid.nreal
    for what in ("tendency", "steps"):
        dgs = [_dg(law, g, **kw) for g in grids]
        Qs = []
        for g in grids:
            q = _gpu(torch, TC.initial_state(law, g)[0])
            q[g.nreal:] = float("nan")                        # ghosts come from the exchange
            Qs.append(q)
        torch.cuda.synchronize()
        cm.dgmodel.connect_local(dgs)
        if what == "tendency":
            out = [torch.zeros_like(q) for q in Qs]
            torch.cuda.synchronize()
            cm.dgmodel.group_rhs(dgs, out, Qs, 0.0)
            ref, tol = T1, TOL
        else:
            dQs = [x.create_state() for x in dgs]
            torch.cuda.synchronize()
            s = cm.odesolvers.LSRK54CarpenterKennedy(dgs[0], Qs[0], dt=dt)
            cm.dgmodel.group_lsrk_run(dgs, Qs, dQs, 0.0, dt, 2, s.RKA, s.RKB, s.RKC)
            out, ref, tol = Qs, Q1, 1e-11
        for x in dgs:
            x.synchronize()
        for g, o in zip(grids, out):
            rows = np.array([pos[int(e)] for e in g.topology.globalelems[:g.nreal]])
            on = o[:g.nreal].cpu().numpy()
            assert np.isfinite(on).all()
            for st in range(law.ns):
                err = observe("tracers partitioned sphere %s state %d" % (what, st), TC.scaled_linf(on[:, st], ref[rows, st]))
                assert err <= tol, (what, st, err)
        for x in dgs:
            x.close()


def test_two_ranks_exchange_the_widened_gradient_flux(torch):
    """The walled box, nu != 0, two tracers: the gradient flux (9 + 6 columns) is live and exchanged.
    Two ranks through ``group_rhs`` against one rank, every state."""
    law = TC.box_model((1.0, 3.0))
    grid = TC.walled_box()
    T1 = _tendency(torch, law, grid, TC.initial_state(law, grid)[0])
    pos = {int(g): i for i, g in enumerate(grid.topology.globalelems[:grid.nreal])}
    grids = [TC.walled_box(rank=r, size=2) for r in range(2)]
    assert sum(g.nreal for g in grids) == grid.nreal and all(g.nelem > g.nreal for g in grids)
    dgs = [_dg(law, g) for g in grids]
    Qs = []
    for g in grids:
        q = _gpu(torch, TC.initial_state(law, g)[0])
        q[g.nreal:] = float("nan")
        Qs.append(q)
    out = [torch.zeros_like(q) for q in Qs]
    torch.cuda.synchronize()
    cm.dgmodel.connect_local(dgs)
    assert all(x.query("GRADFLUX_LIVE") == 1 for x in dgs)
    cm.dgmodel.group_rhs(dgs, out, Qs, 0.0)
    for x in dgs:
        x.synchronize()
    for g, o in zip(grids, out):
        rows = np.array([pos[int(e)] for e in g.topology.globalelems[:g.nreal]])
        on = o[:g.nreal].cpu().numpy()
        assert np.isfinite(on).all()
        for st in range(law.ns):
            assert TC.scaled_linf(on[:, st], T1[rows, st]) <= TOL, st
    for x in dgs:
        x.close()


@pytest.mark.parametrize("option", ["OPT_STEP_GRAPH", "OPT_ASYNC_RUN"])
def test_run_options_give_the_same_bits(torch, option):
    """The recorded step and the asynchronous run on the sphere with one tracer: the bits of the plain run."""
    law, grid = TC.sphere_model((2.0,)), TC.sphere()
    Q0 = TC.initial_state(law, grid)[0]
    res = []
    for on in (0, 1):
        dg = _dg(law, grid, d=EVERY, dd=HORIZONTAL)
        dg.set_option(getattr(cm._lib, option), on)
        Q = _gpu(torch, Q0)
        s = cm.odesolvers.LSRK54CarpenterKennedy(dg, Q, dt=2.0)
        s.dostep(Q, nsteps=3)
        dg.synchronize()
        res.append(Q[:grid.nreal].cpu().numpy())
        dg.set_option(getattr(cm._lib, option), 0)
        dg.close()
    assert np.isfinite(res[0]).all() and np.array_equal(res[0], res[1])
    assert not np.array_equal(res[0][:, 5], Q0[:grid.nreal, 5])


# ---- 8. filters on tracer columns ----------------------------------------------------------------
@pytest.mark.parametrize("kind", ["exponential", "tmar"])
def test_filters_on_tracer_columns(torch, kind):
    """ExponentialFilter / TMARFilter on the tracer columns of a seven-state array: the bits of the
    same filter on that column in a one-state handle; every other column untouched."""
    F = cm.mesh.filters
    grid = TC.walled_box()
    law = TC.box_model((1.0, 3.0))
    Q, _ = TC.initial_state(law, grid)
    rng = np.random.default_rng(7)
    Q[:, 5:] += 0.6 * rng.standard_normal(Q[:, 5:].shape)     # rough, and negative in places (TMAR)
    assert (Q[:, 5:] < 0).any()
    filt = F.ExponentialFilter(grid, 1, 8) if kind == "exponential" else F.TMARFilter()
    dg = _dg(law, grid)
    Qg = _gpu(torch, Q)
    F.apply(Qg, F.FilterIndices(6, 7), dg, filt)
    got = Qg.cpu().numpy()
    dg.close()
    one = cm.balancelaws.AdvectionDiffusion(3, TC._Nodal(u=[0.0] * 3), (), advection=True, diffusion=False)
    dg1 = _dg(one, grid)
    for k in (5, 6):
        q1 = _gpu(torch, Q[:, k:k + 1].copy())
        F.apply(q1, F.FilterIndices(1), dg1, filt)
        assert np.array_equal(got[:, k], q1.cpu().numpy()[:, 0]), k
        assert not np.array_equal(got[:grid.nreal, k], Q[:grid.nreal, k])
    dg1.close()
    assert np.array_equal(got[:, :5], Q[:, :5])


# ---- 4 of the issue's list: the state count comes from the handle -------------------------------------
def test_reductions_and_courant_take_the_widened_state(torch):
    grid = TC.walled_box()
    law, free = TC.box_model((1.0, 3.0)), TC.box_model(None)
    Q, _ = TC.initial_state(law, grid)
    dg, dg0 = _dg(law, grid), _dg(free, grid)
    Qg, Q0 = _gpu(torch, Q), _gpu(torch, Q[:, :5].copy())
    n = cm.reductions.norm(dg, Qg, dims=(1, 3))
    n0 = cm.reductions.norm(dg0, Q0, dims=(1, 3))
    assert n.shape == (7,) and np.array_equal(n[:5], n0)
    M = torch.from_numpy(np.ascontiguousarray(grid.vgeo[:grid.nreal, cm.mesh.grids._M, :])).cuda()
    for k in (5, 6):
        want = float(torch.sqrt((M * Qg[:grid.nreal, k] ** 2).sum()))
        assert abs(n[k] - want) <= 1e-13 * want
    for kind in (cm.dgmodel.ADVECTIVE_COURANT, cm.dgmodel.NONDIFFUSIVE_COURANT, cm.dgmodel.DIFFUSIVE_COURANT):
        assert dg.courant(kind, Qg, 0.1) == dg0.courant(kind, Q0, 0.1)           # courant.jl reads the dry quantities
    dg.close(), dg0.close()


# ---- 9. refusals -------------------------------------------------------------------------------------
def test_refusals_name_tracers(torch):
    Err = (cm._lib.CmdgError, ValueError)
    grid = TC.periodic_brick()
    law = TC.plain_model((1.0,))
    for nf in (cm.balancelaws.RoeNumericalFlux, cm.balancelaws.HLLCNumericalFlux, cm.balancelaws.LMARSNumericalFlux):
        with pytest.raises(Err, match="tracer"):
            _dg(law, grid, nf=nf)
    with pytest.raises(Err, match="tracer"):                      # MMSSource / InitStateBC
        A.DryAtmosModel(A.MMSSetup(law.ps), orientation=A.ORIENT_NONE, sources=A.SRC_MMS, tracers=A.NTracers((1.0,)))
    with pytest.raises(Err, match="tracer"):
        A.DryAtmosModel(A.MMSSetup(law.ps), orientation=A.ORIENT_NONE, boundary_conditions=(A.BC_INIT_STATE_MMS,),
                        tracers=A.NTracers((1.0,)))
    # ... and the library itself, whatever the host model lets through
    mms = TC.plain_model((1.0,))
    mms.sources = A.SRC_MMS
    with pytest.raises(Err, match="tracer"):
        _dg(mms, grid)
    # DGFVModel
    M = cm.mesh
    x = np.linspace(0.0, 1000.0, 3)
    fvgrid = M.DiscontinuousSpectralElementGrid(
        M.StackedBrickTopology([x] * 3, periodicity=(True,) * 3, connectivity="full"), (4, 0))
    with pytest.raises(Err, match="tracer"):
        cm.dgmodel.DGFVModel(law, fvgrid, cm.fvreconstructions.FVConstant())
    # the moist law; the acoustic linear model (its auxiliary layout has no tracer columns)
    with pytest.raises(Err, match="tracer"):
        cm.moist.MoistAtmosModel(None, None, tracers=A.NTracers((1.0,)))
    box = TC.box_model((1.0,))
    with pytest.raises(Err, match="tracer"):
        A.AtmosAcousticLinearModel(TC.plain_model((1.0,)))
    # three tracers are not compiled in: the message says where they come from
    with pytest.raises(Err, match="tracer"):
        _dg(TC.plain_model((1.0, 2.0, 3.0)), grid)
    # the default diagnostics groups
    bgrid = TC.walled_box()
    dg = _dg(box, bgrid)
    with pytest.raises(Err, match="tracer"):
        cm.diagnostics.AtmosLESDefault(dg)
    dg.close()
    sgrid = TC.sphere()
    sdg = _dg(TC.sphere_model((1.0,)), sgrid, d=EVERY, dd=HORIZONTAL)
    interpol = cm.mesh.InterpolationCubedSphere.__new__(cm.mesh.InterpolationCubedSphere)   # (never used)
    with pytest.raises(Err, match="tracer"):
        cm.diagnostics.AtmosGCMDefault(sdg, interpol)
    sdg.close()


def test_tracer_free_plugin_does_not_serve_a_tracer_descriptor(torch):
    """The plug-in of tests/test_gpu_plugins.py (orientation + hyperdiffusion, no reference state, no
    tracers) loaded: the same combination with one tracer is still refused, by name."""
    so = cm.plugins.build_dry_atmos(orient=True, ref_state=False, hyperdiffusion=True, N=4)
    cm.plugins.load(so)
    ps = A.PlanetParameters()
    kw = dict(orientation=A.ORIENT_SPHERICAL, ref_state=None, viscosity=0.0, dynamic_viscosity=False,
              hyperdiffusion_timescale=8 * 3600.0, sources=A.SRC_GRAVITY | A.SRC_CORIOLIS,
              boundary_conditions=(A.BC_ATMOS_DEFAULT, A.BC_ATMOS_DEFAULT), param_set=ps)
    grid = TC.sphere()
    free = _dg(A.DryAtmosModel(A.HeldSuarezSetup(ps), **kw), grid, d=EVERY, dd=HORIZONTAL)
    free.close()                                                 # the plug-in serves its own combination
    with pytest.raises(cm._lib.CmdgError, match="tracer"):
        _dg(A.DryAtmosModel(A.HeldSuarezSetup(ps), tracers=A.NTracers((1.0,)), **kw), grid, d=EVERY, dd=HORIZONTAL)


# ---- 7. IMEX: the linear model carries no tracers ---------------------------------------------------
def _pair(law, grid):
    dg = cm.dgmodel.DGModel(law, grid, direction=EVERY)
    lin = cm.dgmodel.DGModel(A.AtmosAcousticGravityLinearModel(law), grid, direction=VERTICAL,
                             state_auxiliary=dg.state_auxiliary)
    return dg, lin


def test_imex_band_of_a_tracer_pair_is_the_tracer_free_band(torch):
    """The band has the size and the entries of the tracer-free model: the linear model of a model with
    one tracer is the five-state law on a wider auxiliary array."""
    out = []
    for tracer in (True, False):
        law, grid = TC.acoustic_setup(2, 3, tracer=tracer)
        dg, lin = _pair(law, grid)
        assert lin.balance_law.ns == 5 and lin.balance_law.naux == law.naux
        lu = cm.systemsolvers.ColumnLU(lin, 7.5)
        lu.assemble(7.5)
        bands = [lu.export_band(c) for c in (0, 17, lu.ncol - 1)]
        lu.update(7.5)
        bands += [lu.export_band(c) for c in (0, 17, lu.ncol - 1)]          # ... and its LU factors
        out.append(((lu.n, lu.p, lu.q, lu.ncol, lu.band_bytes), bands))
        lu.close(), lin.close(), dg.close()
    assert out[0][0] == out[1][0]
    for a, b in zip(out[0][1], out[1][1]):
        assert np.array_equal(a, b)


def _ark_restated(torch, dg, lin, lu, Q, t, dt, split):
    """dostep!(..., ::LowStorageVariant) (AdditiveRungeKuttaMethod.jl:415-523, 565-690) on the device's
    own operators: the full operator on the wide arrays, the linear operator and the LU solve on
    narrow ones, the leading columns moved between them."""
    A_e, A_i, B, Cc = (np.array(x) for x in cm.odesolvers.ark2gkc_tableau())
    ns, nl = len(B), lin.balance_law.ns

    def full(q, tt):
        T = torch.zeros_like(q)
        dg(T, q, tt)
        dg.synchronize()
        return T

    def add_linear(T, q, tt, sign):
        """T[leading] += sign L(q[leading]): the linear operator increments a narrow copy."""
        qn, Tn = q[:, :nl].contiguous(), T[:, :nl].contiguous()
        lin(Tn, qn, tt, sign, 1.0)
        lin.synchronize()
        T[:, :nl] = Tn

    def explicit(q, tt):
        T = full(q, tt)
        if split:
            add_linear(T, q, tt, -1.0)
        return T

    Qs, R = [Q.clone()], [explicit(Q, t + Cc[0] * dt)]
    for i in range(1, ns):
        Qhat, Qst = Q.clone(), torch.full_like(Q, -0.0)
        for j in range(i):
            c = A_i[i, j] / A_i[i, i] if split else (A_i[i, j] - A_e[i, j]) / A_i[i, i]
            common = c * Qs[j]
            Qhat += common + (dt * A_e[i, j]) * R[j]
            Qst -= common
        alpha = dt * A_i[i, i]
        if lu.alpha != alpha:
            lu.update(alpha)
        b = Qhat[:, :nl].contiguous()
        x = torch.zeros_like(b)
        lu.solve(x, b)
        lin.synchronize()
        Qtt = Qhat.clone()                      # Q .= Qrhs, then the solve over the linear model's states
        Qtt[:, :nl] = x
        Qs.append(Qst + Qtt)
        R.append(explicit(Qs[i], t + Cc[i] * dt))
    if split:
        for i in range(ns):
            add_linear(R[i], Qs[i], t + Cc[i] * dt, 1.0)
    out = Q.clone()
    for i in range(ns):
        out += (B[i] * dt) * R[i]
    return out


@pytest.mark.parametrize("split", [False, True])
def test_imex_step_equals_its_restatement(torch, split):
    """One ARK2GKC step on the small acoustic grid with one tracer, then one at dt / 2 (the column
    matrices are refactored): all six states against the restatement on the device's own full operator,
    linear operator and LU solve; the leading five also against the tracer-free pair's steps."""
    from imex_cases import STATE_SCALE, wall_perturbation
    ode = cm.odesolvers
    law, grid = TC.acoustic_setup(2, 3)
    dg, lin = _pair(law, grid)
    nr = grid.nreal
    Q0 = dg.init_ode_state(0.0)
    aux = dg.state_auxiliary.cpu().numpy()
    pert = wall_perturbation(law, aux) * STATE_SCALE[None, :, None]
    Q0[:, :5] += _gpu(torch, pert)
    lam = np.arctan2(aux[:, 1], aux[:, 0])
    Q0[:, 5] = Q0[:, 0] * _gpu(torch, 1.0 + 0.3 * np.sin(2 * lam) * np.cos(aux[:, 2] / 6.4e6))
    dt = 40.0
    solver = ode.ARK2GiraldoKellyConstantinescu(dg, lin, ode.LinearBackwardEulerSolver(ode.ManyColumnLU()),
                                                Q0, dt=dt, split_explicit_implicit=split)
    lu = cm.systemsolvers.ColumnLU(lin, 1.0)
    Q, Qr, t = Q0.clone(), Q0.clone(), 0.0
    steps = []
    for h in (dt, dt / 2):
        solver.updatedt(h)
        solver.dostep(Q, 1)
        dg.synchronize()
        Qr = _ark_restated(torch, dg, lin, lu, Qr, t, h, split)
        t += h
        steps.append(Q[:nr].cpu().numpy())
        for s in range(6):
            err = TC.scaled_linf(steps[-1][:, s], Qr[:nr, s].cpu().numpy())
            print("split=%s dt=%g state %d vs restatement: %.3e" % (split, h, s, err))
            assert err <= TOL, (s, err)
        assert not np.array_equal(steps[-1][:, 5], Q0[:nr, 5].cpu().numpy())
    solver.close(), lu.close(), lin.close(), dg.close()
    # the tracer-free pair on the same leading data
    law0, grid0 = TC.acoustic_setup(2, 3, tracer=False)
    dg0, lin0 = _pair(law0, grid0)
    q = Q0[:, :5].contiguous()
    solver0 = ode.ARK2GiraldoKellyConstantinescu(dg0, lin0, ode.LinearBackwardEulerSolver(ode.ManyColumnLU()),
                                                 q, dt=dt, split_explicit_implicit=split)
    bits = True
    for h, wide in zip((dt, dt / 2), steps):
        solver0.updatedt(h)
        solver0.dostep(q, 1)
        dg0.synchronize()
        qn = q[:nr].cpu().numpy()
        for s in range(5):
            err = TC.scaled_linf(wide[:, s], qn[:, s])
            assert err <= TOL, (s, err)
        bits = bits and np.array_equal(wide[:, :5], qn)
    print("split=%s: leading states of the tracer pair bit-identical to the tracer-free pair: %s" % (split, bits))
    solver0.close(), lin0.close(), dg0.close()


@pytest.mark.parametrize("split", [False, True])
def test_acousticwave_golden_with_its_tracer(torch, split):
    """acousticwave_1d_imex.jl as tests/test_gpu_imex.py sets it up (N = 5, 10 x 5 elements, dt = 100 s,
    36 steps, the vertical exponential filter on every state each step), with the reference's tracer
    carried: rho chi = 1, delta_chi = 1.  norm(Q) over all six states against 9.5073452847149594e13
    (acousticwave_1d_imex.jl:65) at rtol = sqrt(eps), the reference's own ``isapprox``.

    What this is worth: the tracer is about 2.8e-10 of norm^2, far below sqrt(eps).  The number
    confirms that the run with a tracer is the reference's run; it does not pin the tracer.  The
    cross-law, mixing-ratio, linearity and conservation tests above do that."""
    import math
    from imex_cases import ACOUSTIC_GOLDEN
    from test_gpu_imex import run_acoustic
    law, grid = TC.acoustic_setup(10, 5)
    dg, lin, solver, Q = run_acoustic(cm, torch, split, law, grid, 100.0, 36)
    assert Q.shape[1] == 6
    got = math.sqrt(dg.norm2_local(Q))
    rel = abs(got - ACOUSTIC_GOLDEN) / ACOUSTIC_GOLDEN
    chi = Q[:grid.nreal, 5].cpu().numpy()
    print("acoustic wave with tracer, split=%s: norm(Q) = %.16e, relative error %.3e; rho chi in [%.6f, %.6f]"
          % (split, got, rel, chi.min(), chi.max()))
    assert np.isfinite(chi).all() and not np.all(chi == 1.0)
    assert rel <= math.sqrt(np.finfo(float).eps)
    solver.close(), lin.close(), dg.close()


def test_imex_pairs_that_stay_refused(torch):
    """GMRES pairs and MRI-GARK pairs of differing state counts: refused, by name."""
    ode = cm.odesolvers
    law, grid = TC.acoustic_setup(2, 3)
    dg, lin = _pair(law, grid)
    Q = dg.init_ode_state(0.0)
    with pytest.raises((cm._lib.CmdgError, ValueError), match="tracer"):
        ode.ARK2GiraldoKellyConstantinescu(
            dg, lin, ode.LinearBackwardEulerSolver(cm.systemsolvers.GeneralizedMinimalResidual(M=10)), Q, dt=1.0)
    with pytest.raises((cm._lib.CmdgError, ValueError), match="tracer"):
        cm.dgmodel.remainder_DGModel(dg, (lin,))
    lin.close(), dg.close()
