"""The AtmosGCMDefault diagnostics on the device (climatemachine.jl_amd/diagnostics.py; csrc/kernels.h
k_vector_gradients and k_gcm_nodal, csrc/physics_vorticity.h, csrc/interpolation.hip k_gcm_finish) against the
reference's known answer (test/Diagnostics/diagnostic_fields_test.jl), the NumPy restatement
(gcm_diagnostics_restatement.py), the step-by-step route through the public calls, and a solid-body
rotation on the sphere.

Solid-body rotation, measured on the CPU with the restatement (tests/test_gcm_diagnostics_host.py holds the
restatement to these figures; gcm_diagnostics_cases.SOLID_BODY_DEVIATION): u 1.887e-4 m/s (of 32.0), v and
w 1.220e-4, vort 3.748e-9 1/s (of 1e-5), vort2 1.700e-8, rho 5.964e-4 kg/m^3, temp 0.1901 K, pres 21.22 Pa.
The device is allowed four times each."""
import numpy as np
import pytest

import gcm_diagnostics_cases as GC
import gcm_diagnostics_restatement as R
from helpers import rel_linf
from test_gpu_les_diagnostics import NODAL_TOL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-8           # diagnostic_fields_test.jl:137
TENDENCY_TOL = 1e-12  # a device tendency against a restatement in another summation order


def _gpu(torch, a):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    torch.cuda.synchronize()
    return t


def _vort2(cm, torch, grid, u):
    """The tendency of a VorticityModel handle on ``grid`` whose auxiliary state is ``u``: (nreal, 3, Np)."""
    DI = cm.diagnostics
    vdg = cm.dgmodel.DGModel(DI.VorticityModel(), grid,
                             numerical_flux_first_order=cm.balancelaws.CentralNumericalFluxFirstOrder,
                             state_auxiliary=_gpu(torch, u))
    dQ = vdg.create_state()
    vdg(dQ, vdg.init_ode_state(0.0), 0.0)
    vdg.synchronize()
    out = dQ.cpu().numpy()[:grid.nreal]
    vdg.close()
    return out


@pytest.fixture(scope="module")
def brick(cm, torch):
    law, grid = GC.brick()
    dg = cm.dgmodel.DGModel(law, grid)
    yield law, grid, dg
    dg.close()


@pytest.fixture(scope="module")
def sphere(cm, torch):
    law, grid, it = GC.sphere()
    dg = cm.dgmodel.DGModel(law, grid, direction=0, diffusion_direction=1)
    yield law, grid, it, dg
    dg.close()


# ---- 1. the reference's known answer --------------------------------------------------------------------
def test_known_answer_on_the_device(cm, torch, brick):
    law, grid, dg = brick
    DI = cm.diagnostics
    Qh = GC.reference_field(grid)
    assert Qh[:, 0].min() >= 1.0
    vg = DI.VectorGradients(dg, _gpu(torch, Qh))
    vort = DI.Vorticity(dg, vg).data.cpu().numpy()
    vgrad = vg.data.cpu().numpy()
    assert list(vg.views) == R.VGRAD and vgrad.shape == (27, 9, 125)
    grads, curl = GC.exact_gradients(grid)
    errs = [np.abs(vgrad[:, q] - grads[q]).max() for q in range(9)]
    errs += [np.abs(vort[:, c] - curl[c]).max() for c in range(3)]
    vort2 = _vort2(cm, torch, grid, R.velocity(Qh))
    errs += [np.abs(vort2[:, c] - curl[c]).max() for c in range(3)]
    print("max errors (9 gradients, vort, vort2):", " ".join("%.2e" % e for e in errs))
    assert len(errs) == 15 and max(errs) < TOL, errs


# ---- 2. bits --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["brick", "sphere"])
def test_gradients_vorticity_and_nodal_pass_have_the_restatement_bits(cm, torch, brick, sphere, where):
    DI = cm.diagnostics
    law, grid, dg = brick if where == "brick" else (sphere[0], sphere[1], sphere[3])
    Qh, _ = GC.noisy_state(law, grid)
    aux = dg.state_auxiliary.cpu().numpy()
    Q = _gpu(torch, Qh)
    nr = grid.nreal
    want_g = R.vector_gradients(grid, Qh)
    want_o = R.vorticity(want_g)
    vg = DI.VectorGradients(dg, Q)
    assert np.array_equal(vg.data.cpu().numpy(), want_g)
    assert np.array_equal(vg["∂₂u₃"].cpu().numpy(), want_g[:, 7])
    vo = DI.Vorticity(dg, vg)
    assert np.array_equal(vo.data.cpu().numpy(), want_o)
    assert np.array_equal(vo["Ω₃"].cpu().numpy(), want_o[:, 2])
    # the fused nodal pass
    G, u = DI.gcm_nodal(dg, Q, 0.0)
    G, u = G.cpu().numpy(), u.cpu().numpy()
    assert G.shape == (grid.nelem, 14, grid.Np) and len(DI.GCM_NODAL_NAMES) == 14
    assert np.array_equal(u[:nr], R.velocity(Qh[:nr]))
    assert np.array_equal(G[:nr, :5], Qh[:nr])
    assert np.array_equal(G[:nr, 11:], want_o)
    th = R.thermo(law, Qh[:nr], aux[:nr])
    for s, name in enumerate(["temp", "pres", "θ_dry", "e_int", "h_tot", "h_int"]):
        got, ref = G[:nr, 5 + s], th[:, s]
        rel = np.abs(got - ref).max() / np.abs(ref).max()
        print("%s column %-6s rel. difference %.2e" % (where, name, rel))
        if name == "θ_dry":             # (the only one through pow)
            assert rel <= NODAL_TOL, (name, rel)
        else:
            assert np.array_equal(got, ref), name
    assert (th[:, 0] > 150).all() and (th[:, 0] < 400).all()


# ---- 3. the face terms of VorticityModel --------------------------------------------------------------
@pytest.mark.parametrize("where", ["brick", "sphere"])
def test_vorticity_model_tendency_with_a_discontinuous_velocity(cm, torch, where):
    """With a continuous u the central face terms cancel; an offset per element makes every interior face
    term matter (and the boundary faces, where plus = minus)."""
    if where == "brick":
        law, grid = GC.brick()
    else:
        law, grid, _ = GC.sphere()
    Qh, _ = GC.noisy_state(law, grid)
    u = R.velocity(Qh) + GC.element_offsets(grid, 3.0)
    want = R.vorticity_model_tendency(grid, u)
    smooth = R.vorticity_model_tendency(grid, R.velocity(Qh))
    assert np.abs(want - smooth).max() > 1e-2 * np.abs(want).max()      # the face terms are not small
    got = _vort2(cm, torch, grid, u)
    err = rel_linf(got, want)
    print("%s: VorticityModel tendency against the restatement, rel. L-inf %.2e" % (where, err))
    assert err <= TENDENCY_TOL, err


# ---- 4. the composition ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def collected(cm, torch, sphere):
    law, grid, it, dg = sphere
    Qh, _ = GC.noisy_state(law, grid)
    Q = _gpu(torch, Qh)
    diag = cm.diagnostics.AtmosGCMDefault(dg, it).init()
    out = diag.collect(Q, 0.0)
    yield diag, Q, Qh, out
    diag.close()


def test_collect_equals_the_route_through_the_public_calls(cm, torch, sphere, collected):
    law, grid, it, dg = sphere
    diag, Q, Qh, out = collected
    DI, I = cm.diagnostics, cm.mesh.interpolation
    assert list(out) == ["long", "lat", "level"] + R.NAMES
    nr = grid.nreal

    def interp(a):
        v = torch.zeros((a.shape[1], it.Npl), dtype=torch.float64, device=DEV)
        I.interpolate_local(it, a.contiguous(), v)
        return v

    G, u = DI.gcm_nodal(dg, Q, 0.0)
    istate = interp(Q[:, :5])
    ithermo = interp(G[:, 5:11])
    idyn = interp(DI.Vorticity(dg, DI.VectorGradients(dg, Q)).data)
    vdQ = _gpu(torch, _vort2(cm, torch, grid, u.cpu().numpy()))
    idyn_bl = interp(vdQ)
    I.project_cubed_sphere(it, istate, (2, 3, 4))
    I.project_cubed_sphere(it, idyn, (1, 2, 3))
    I.project_cubed_sphere(it, idyn_bl, (1, 2, 3))
    s, th, dy, bl = (a.cpu().numpy() for a in (istate, ithermo, idyn, idyn_bl))
    v = np.stack([s[1] / s[0], s[2] / s[0], s[3] / s[0], s[0], th[0], th[1], th[2], s[4] / s[0], th[3], th[4], th[5],
                  dy[2], bl[2]])
    fiv = torch.full((13,) + it.dims[::-1], float("nan"), dtype=torch.float64, device=DEV)
    I.accumulate_interpolated_data(it, _gpu(torch, v), fiv)
    want = fiv.cpu().numpy()
    assert not np.isnan(want).any()
    for i, name in enumerate(R.NAMES):
        assert out[name].shape == (4, 13, 25)
        assert np.array_equal(out[name], want[i]), name
    # ... and the whole thing is the restatement's, to the interpolation's own bound
    ref = R.collect(law, grid, it, Qh, dg.state_auxiliary.cpu().numpy())
    for name in R.NAMES:
        assert rel_linf(out[name], ref[name]) < 1e-10, name
    assert np.array_equal(out["long"], it.long_grd) and np.array_equal(out["lat"], it.lat_grd)
    assert out["level"][0] == 0.0 and np.allclose(out["level"], [0.0, 10e3, 20e3, 30e3], rtol=0, atol=1e-6)


def test_two_collections_return_the_same_bits(collected):
    diag, Q, _, out = collected
    again = diag.collect(Q, 0.0)
    views = diag.collect(Q, 0.0, copy=False)        # views of the group's pinned staging buffer
    for k in out:
        assert np.array_equal(out[k], again[k]), k
        assert np.array_equal(out[k], views[k]), k
    assert views["u"].base is not None and again["u"].base is None


# ---- 5. known answer on the sphere ------------------------------------------------------------------------
def test_solid_body_rotation_on_the_sphere(cm, torch, sphere):
    law, grid, it, dg = sphere
    Qh, _ = GC.solid_body_state(law, grid)
    diag = cm.diagnostics.AtmosGCMDefault(dg, it).init()
    out = diag.collect(_gpu(torch, Qh), 0.0)
    want = GC.solid_body_expected(law, it)
    for k, w in want.items():
        dev = float(np.abs(out[k] - w).max())
        print("%-6s deviation %.4e, allowed 4 x %.3e" % (k, dev, GC.SOLID_BODY_DEVIATION[k]))
        assert dev <= 4 * GC.SOLID_BODY_DEVIATION[k], (k, dev)
    diag.close()


# ---- 6. ranks ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [2, 3])
def test_group_collect_over_local_ranks(cm, torch, collected, size):
    DI = cm.diagnostics
    _, _, _, single = collected
    dgs, Qs, its = [], [], []
    for r in range(size):
        law, grid, it = GC.sphere(r, size)
        dgs.append(cm.dgmodel.DGModel(law, grid, direction=0, diffusion_direction=1))
        Qs.append(_gpu(torch, GC.noisy_state(law, grid)[0]))
        its.append(it)
    assert sum(d.grid.nreal for d in dgs) == 108 and all(d.grid.nelem > d.grid.nreal for d in dgs)
    cm.dgmodel.connect_local(dgs)
    out, diags = DI.group_collect_gcm(dgs, Qs, its, 0.0)
    for name in R.NAMES:
        if name == "vort2":     # the exterior faces read exchanged ghosts: another launch, another order
            err = rel_linf(out[name], single[name])
            print("%d ranks: vort2 against one rank, rel. L-inf %.2e" % (size, err))
            assert err <= TENDENCY_TOL, err
        else:
            assert np.array_equal(out[name], single[name]), name
    again, _ = DI.group_collect_gcm(dgs, Qs, its, 0.0, diags=diags)
    for name in R.NAMES:
        assert np.array_equal(out[name], again[name]), name
    for d in diags:
        d.close()
    for d in dgs:
        d.close()


# ---- 7. refusals ------------------------------------------------------------------------------------------
def test_refusals_say_why(cm, torch, brick, sphere):
    DI, I = cm.diagnostics, cm.mesh.interpolation
    law, grid, dg = brick
    # a brick interpolation
    n = 3 * GC.SIDE
    xg = [np.linspace(0.0, n, 4)] * 3
    ib = I.InterpolationBrick(grid, np.array([[0.0] * 3, [n] * 3]), *xg)
    with pytest.raises(ValueError, match="currently requires `InterpolationCubedSphere`"):
        DI.AtmosGCMDefault(dg, ib)
    # the moist law: VectorGradients is served, the nodal pass is not
    from helpers import bomex_setup
    mlaw, mgrid = bomex_setup(nx=2, ny=2, nz=2, N=4, L=1500.0)
    mdg = cm.dgmodel.DGModel(mlaw, mgrid)
    mQ = mdg.init_ode_state(0.0)
    assert DI.VectorGradients(mdg, mQ).data.shape == (mgrid.nreal, 9, mgrid.Np)
    with pytest.raises(cm._lib.CmdgError, match="moist columns are not built"):
        DI.gcm_nodal(mdg, mQ, 0.0)
    mdg.close()
    # an ocean law through VectorGradients
    from helpers import ocean_spindown_setup
    olaw, ogrid = ocean_spindown_setup(Nx=2, Ny=2, Nz=2)
    odg = cm.dgmodel.DGModel(olaw, ogrid)
    with pytest.raises(cm._lib.CmdgError, match="does not begin rho"):
        DI.VectorGradients(odg, odg.create_state())
    with pytest.raises(cm._lib.CmdgError, match="defines no GCM diagnostics"):
        DI.gcm_nodal(odg, odg.create_state(), 0.0)
    odg.close()
    # a DGFVModel handle
    import dgfv_atmos_cases as FC
    flaw, fgrid = FC.balance_box(n_horz=2, n_vert=4)
    fdg = cm.dgmodel.DGFVModel(flaw, fgrid, cm.fvreconstructions.FVConstant())
    with pytest.raises(cm._lib.CmdgError, match="vertical polynomial order 0"):
        DI.VectorGradients(fdg, fdg.create_state())
    fdg.close()
    # collect before init, and a Q of the wrong shape
    slaw, sgrid, it, sdg = sphere
    diag = DI.AtmosGCMDefault(sdg, it)
    with pytest.raises(ValueError, match="init"):
        diag.collect(sdg.create_state(), 0.0)
    diag.init()
    with pytest.raises(ValueError, match="shape"):
        diag.collect(sdg.create_state(4), 0.0)
    diag.close()
    # NULL arrays at the C entry
    assert dg.L.cmdg_vector_gradients(dg.handle, None, None) != 0
    assert b"NULL" in dg.L.cmdg_last_error(dg.handle)


# ---- 8. the callback -------------------------------------------------------------------------------------
def test_callback_records_the_grid_during_a_solve(cm, torch, sphere, tmp_path):
    law, grid, it, dg = sphere
    Q = dg.init_ode_state(0.0)
    solver = cm.odesolvers.LSRK54CarpenterKennedy(dg, Q, dt=1.0)
    seen = []
    cb = cm.diagnostics.AtmosGCMDefaultCallback(dg, it, sink=lambda t, p: seen.append(t))
    cm.odesolvers.solve(Q, solver, numberofsteps=4, callbacks=[(2, cb)])
    assert len(cb.records) == 2 and seen == pytest.approx([2.0, 4.0])
    for _, p in cb.records:
        assert list(p) == ["long", "lat", "level"] + R.NAMES
        assert np.isfinite(p["rho"]).all() and (p["rho"] > 0).all() and (p["temp"] > 150).all()
    path = cb.save(str(tmp_path / "series.npz"))
    with np.load(path) as f:
        assert list(f.keys()) == ["time", "long", "lat", "level"] + R.NAMES
        assert f["vort2"].shape == (2, 4, 13, 25) and f["time"].shape == (2,)
        assert f["level"][0] == 0.0 and f["level"].shape == (4,) and f["long"].shape == (25,)
    cb.diag.close()
