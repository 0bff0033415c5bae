"""Interpolation onto box and latitude-longitude grids on the device (csrc/interpolation.hip
through climatemachine.jl_amd/mesh/interpolation.py) against the NumPy restatement of the
reference's kernels (tests/interpolation_restatement.py), the reference's own accuracy rows,
the projection of a solid-body rotation, invariance under the partition, ordering behind a
deferred run, and the refusals."""
import ctypes as C
import functools

import numpy as np
import pytest

import interpolation_cases as IC
import interpolation_restatement as R
from helpers import observe, pseudo1d_setup, rel_linf

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# smaller output grids than the reference's for the parity sweep: same set-up code, same polar
# pile-up (all longitudes of the +-90 degree rows fall into one element each), seconds of NumPy
@functools.lru_cache(maxsize=None)
def small(kind, N, rank=0, size=1):
    if kind == "sphere":
        return IC.sphere_case(N, rank, size, nhor=3, nvert=2, res=3.0, nrad=7)
    return IC.brick_case(N, rank, size, ne=(5, 2, 4), spacing=40.0)


def _gpu(torch, a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=DEV)


def run_device(cm, torch, pairs, Qs, project=None, fill=float("nan")):
    """interpolate (+ project) every rank, scatter all ranks into one fiv; returns (vs, fiv)."""
    I = cm.mesh.interpolation
    nstate = Qs[0].shape[1]
    its = [it for _, it in pairs]
    vs = []
    for it, Q in zip(its, Qs):
        v = torch.full((nstate, it.Npl), fill, dtype=torch.float64, device=DEV)
        I.interpolate_local(it, _gpu(torch, Q), v)
        if project is not None:
            I.project_cubed_sphere(it, v, project)
        vs.append(v)
    fiv = torch.full((nstate,) + its[0].dims[::-1], fill, dtype=torch.float64, device=DEV)
    I.accumulate_interpolated_data(its, vs, fiv)
    torch.cuda.synchronize()
    return [v.cpu().numpy() for v in vs], fiv.cpu().numpy()


# ---- parity with the restatement --------------------------------------------------------
@pytest.mark.parametrize("nstate,size", [(5, 1), (6, 1), (5, 3), (6, 3)])
@pytest.mark.parametrize("N", [4, 5, (5, 6), 7])
@pytest.mark.parametrize("kind", ["brick", "sphere"])
def test_device_matches_the_restatement(cm, torch, kind, N, nstate, size):
    _parity(cm, torch, kind, N, nstate, size)


@pytest.mark.parametrize("kind,N,nstate", [("sphere", 7, 11), ("brick", 7, 9), ("sphere", (5, 6), 17)])
def test_device_matches_the_restatement_when_states_are_staged_in_chunks(cm, torch, kind, N, nstate):
    """More states than one LDS pass holds (32 kB: 8 states at N = 7, 16 at (5, 6)): the kernel
    re-stages behind a barrier, with a shorter last chunk (8 + 3, 8 + 1, 16 + 1).  The small
    sphere's polar elements own more than 128 points, so full, partly filled and (in their
    second wave) wholly idle groups all take the barriers."""
    it = small(kind, N)[1]
    per = np.diff(it.offset)
    assert int(np.prod(it.Nq)) * 8 * nstate > 32768
    assert per.max() > 128 and (per[per > 0] % 128 != 0).any()
    _parity(cm, torch, kind, N, nstate, 1)


def _parity(cm, torch, kind, N, nstate, size):
    pairs = [small(kind, N, r, size) for r in range(size)]
    Qs = [IC.random_state(grid, nstate, seed=11 + r) for r, (grid, _) in enumerate(pairs)]
    project = (2, 3, 4) if kind == "sphere" else None
    vs, fiv = run_device(cm, torch, pairs, Qs, project)
    want_v = []
    for (grid, it), Q in zip(pairs, Qs):
        v = R.interpolate_local(it, Q)
        if project:
            want_v.append(v.copy())
            R.project_cubed_sphere(it, v, project)
        want_v.append(v)
    if project:      # interpolate alone, then interpolate + project
        I = cm.mesh.interpolation
        it, Q = pairs[0][1], Qs[0]
        v0 = torch.zeros((nstate, it.Npl), dtype=torch.float64, device=DEV)
        I.interpolate_local(it, _gpu(torch, Q), v0)
        e0 = rel_linf(v0.cpu().numpy(), want_v[0])
        observe("interpolation_parity_interpolate", e0)
        assert e0 < 1e-12, e0
        want_v = want_v[1::2]
    want_fiv = np.full_like(fiv, np.nan)
    R.accumulate_interpolated_data([it for _, it in pairs], want_v, want_fiv)
    for v, w in zip(vs, want_v):
        e = rel_linf(v, w)
        observe("interpolation_parity_" + ("project" if project else "interpolate"), e)
        assert e < 1e-12, e
    assert not np.isnan(fiv).any()                       # every entry written
    e = rel_linf(fiv, want_fiv)
    observe("interpolation_parity_scatter", e)
    assert e < 1e-12, e
    if size == 1:                                        # the scatter itself moves values untouched
        mine = np.full_like(fiv, np.nan)
        R.accumulate_interpolated_data([pairs[0][1]], vs, mine)
        assert np.array_equal(mine, fiv)


# ---- the reference's accuracy rows, end to end on the device ------------------------------
@pytest.mark.parametrize("N", [5, (5, 6)])
def test_reference_accuracy_row_brick_on_device(cm, torch, N):
    """interpolation.jl:432 and :435: L-inf error below 1e-9."""
    grid, it = IC.brick_case(N)
    _, fiv = run_device(cm, torch, [(grid, it)], [IC.reference_state(grid, IC.BRICK_MAX, 6)])
    err = np.abs(fiv - IC.brick_expected(it, 6)).max()
    print("brick N = %s on the device: L-inf error %.3e" % (N, err))
    observe("interpolation_row_brick", err)
    assert err < IC.BRICK_TOL
    it.close()


@pytest.mark.parametrize("N", [5, (5, 6)])
def test_reference_accuracy_row_sphere_on_device(cm, torch, N):
    """interpolation.jl:441 and :444: L-inf error below 2e-7, columns 2-4 projected."""
    grid, it = IC.sphere_case(N)
    Q = IC.reference_state(grid, (IC.PLANET_RADIUS,) * 3, 5)
    _, fiv = run_device(cm, torch, [(grid, it)], [Q], project=(2, 3, 4))
    err = np.abs(fiv - IC.sphere_expected(it, 5)).max()
    print("sphere N = %s on the device: L-inf error %.3e" % (N, err))
    observe("interpolation_row_sphere", err)
    assert err < IC.SPHERE_TOL
    it.close()


def test_solid_body_rotation_projects_to_a_zonal_wind(cm, torch):
    """u = Omega x x in columns 2-4 gives (Omega r cos lat, 0, 0); bound: the sphere row's 2e-7
    relative to Omega r."""
    grid, it = IC.sphere_case(5)
    om = 7.292e-5
    x1, x2, x3 = IC.node_coordinates(grid)
    Q = np.zeros((grid.nelem, 5, grid.Np))
    Q[:, 0] = 1.0
    Q[:, 1], Q[:, 2] = -om * x2, om * x1                  # Omega = (0, 0, om)
    Q[:, 4] = 2.0
    _, fiv = run_device(cm, torch, [(grid, it)], [Q], project=(2, 3, 4))
    r = it.rad_grd[:, None, None]
    want = np.zeros_like(fiv)
    want[0], want[4] = 1.0, 2.0
    want[1] = om * r * cm.mesh.interpolation.cosd(it.lat_grd)[None, :, None] * np.ones(it.n_long)
    err = np.abs(fiv[1:4] - want[1:4]).max() / (om * it.rad_grd.max())
    observe("interpolation_solid_body", err)
    assert err < IC.SPHERE_TOL, err
    assert np.abs(fiv[[0, 4]] - want[[0, 4]]).max() < 1e-12  # constants are reproduced
    it.close()


# ---- rank invariance ----------------------------------------------------------------------
def _global_field(grid, nstate, continuous):
    """A state that depends on the node's position only (the same on every partition); the
    discontinuous variant adds a jump that depends on the element's centroid."""
    x1, x2, x3 = IC.node_coordinates(grid)
    s = max(np.abs(x1).max(), np.abs(x2).max(), np.abs(x3).max())
    f = np.sin(3 * x1 / s) + np.cos(2 * x2 / s) * (x3 / s)
    if not continuous:
        c = (x1.mean(axis=1) + 2 * x2.mean(axis=1) + 3 * x3.mean(axis=1)) / s
        f = f + np.round(7 * c)[:, None]
    return np.ascontiguousarray(np.stack([f * (k + 1) for k in range(nstate)], axis=1))


def test_sphere_is_invariant_under_the_partition_bit_for_bit(cm, torch):
    one = [small("sphere", 5)]
    three = [small("sphere", 5, r, 3) for r in range(3)]
    out = []
    for pairs in (one, three):
        Qs = [_global_field(grid, 5, continuous=False) for grid, _ in pairs]
        out.append(run_device(cm, torch, pairs, Qs, project=(2, 3, 4))[1])
    assert not np.isnan(out[0]).any()
    assert np.array_equal(out[0], out[1])


def test_brick_is_invariant_under_the_partition(cm, torch):
    one = [small("brick", 5)]
    three = [small("brick", 5, r, 3) for r in range(3)]
    for continuous in (False, True):
        out = []
        for pairs in (one, three):
            Qs = [_global_field(grid, 5, continuous) for grid, _ in pairs]
            out.append(run_device(cm, torch, pairs, Qs)[1])
        it = one[0][1]
        interior = np.zeros(out[0].shape[1:], dtype=bool)
        inside = (np.abs(it.xi1) < 1 - 1e-12) & (np.abs(it.xi2) < 1 - 1e-12) & (np.abs(it.xi3) < 1 - 1e-12)
        interior[it.i3[inside] - 1, it.i2[inside] - 1, it.i1[inside] - 1] = True
        assert interior.any() and not interior.all()
        assert np.array_equal(out[0][:, interior], out[1][:, interior])
        if continuous:
            e = rel_linf(out[1], out[0])
            observe("interpolation_brick_partition", e)
            assert e < 1e-12, e


# ---- ordering behind a deferred run ---------------------------------------------------------
def test_interpolation_waits_for_an_async_run(cm, torch):
    I, O = cm.mesh.interpolation, cm.odesolvers
    law, grid, dt = pseudo1d_setup(direction=0)
    xg = [np.linspace(-1.0, 1.0, 33)] * 3
    it = I.InterpolationBrick(grid, np.array([[-1.0] * 3, [1.0] * 3]), *xg)
    res = []
    for asyn in (0, 1):
        dg = cm.dgmodel.DGModel(law, grid, direction=0)
        dg.set_option(cm._lib.OPT_ASYNC_RUN, asyn)
        Q = dg.init_ode_state(0.0)
        v = torch.zeros((Q.shape[1], it.Npl), dtype=torch.float64, device=DEV)
        before = v.clone()
        I.interpolate_local(it, Q, before, dg=dg)
        s = O.LSRK54CarpenterKennedy(dg, Q, dt=dt)
        dg.lsrk_run(Q, s.dQ, 0.0, dt, 40, s.RKA, s.RKB, s.RKC)
        if not asyn:
            dg.synchronize()
        I.interpolate_local(it, Q, v, dg=dg)              # asyn: issued while the run may be queued
        res.append((v.cpu().numpy().copy(), before.cpu().numpy().copy()))
        dg.set_option(cm._lib.OPT_ASYNC_RUN, 0)
        dg.close()
    assert np.array_equal(res[0][0], res[1][0])
    assert not np.array_equal(res[0][0], res[0][1])       # the run changed the state
    it.close()


# ---- an object of index triples only --------------------------------------------------------
def test_object_without_xi_tables_scatters_the_gathered_ranks(cm, torch):
    """What a root does after gathering: one object from the concatenated index vectors of every
    rank (no offset, no xi), scattering the concatenated v; cmdg_interp_apply refuses it."""
    L = cm._lib.lib()
    I = cm.mesh.interpolation
    pairs = [small("sphere", 4, r, 3) for r in range(3)]
    Qs = [IC.random_state(grid, 5, seed=5 + r) for r, (grid, _) in enumerate(pairs)]
    vs, fiv = run_device(cm, torch, pairs, Qs)
    its = [it for _, it in pairs]
    idx = [np.ascontiguousarray(np.concatenate([getattr(it, k) for it in its])) for k in ("i1", "i2", "i3")]
    d = I.CmdgInterpDesc()
    d.npoints = len(idx[0])
    d.i1, d.i2, d.i3 = (a.ctypes.data for a in idx)
    d.n1, d.n2, d.n3 = its[0].dims
    h = C.c_void_p()
    assert L.cmdg_interp_create(None, C.byref(d), C.byref(h)) == 0, L.cmdg_last_error(None)
    v_all = _gpu(torch, np.concatenate(vs, axis=1))
    out = torch.full_like(_gpu(torch, fiv), float("nan"))
    hs, ps = (C.c_void_p * 1)(h.value), (C.c_void_p * 1)(v_all.data_ptr())
    assert L.cmdg_interp_scatter(None, hs, 1, ps, 5, out.data_ptr()) == 0
    assert np.array_equal(out.cpu().numpy(), fiv)
    assert L.cmdg_interp_apply(None, h, v_all.data_ptr(), 5, 1, v_all.data_ptr()) == -1
    assert "without offset" in L.cmdg_last_error(None).decode()
    assert L.cmdg_interp_destroy(None, h) == 0


# ---- refusals -----------------------------------------------------------------------------
def _create(cm, it, mutate):
    L = cm._lib.lib()
    d = it.descriptor()
    keep = mutate(d)
    h = C.c_void_p()
    r = L.cmdg_interp_create(None, C.byref(d), C.byref(h))
    return r, L.cmdg_last_error(None).decode(), h, keep


def test_refusals(cm, torch):
    L = cm._lib.lib()
    grid, it = small("sphere", 4)

    def bad_offset(d):
        off = it.offset.copy()
        off[-1] -= 1
        d.offset = off.ctypes.data
        return off

    def bad_xi(d):
        xi = it.xi2.copy()
        xi[it.Npl // 2] = 1.0 + 1e-6
        d.xi2 = xi.ctypes.data
        return xi

    def bad_index(d):
        i3 = it.i3.copy()
        i3[0] = it.dims[2] + 1
        d.i3 = i3.ctypes.data
        return i3

    for mutate, word in ((bad_offset, "offset"), (bad_xi, "xi2"), (bad_index, "i3")):
        r, msg, h, _ = _create(cm, it, mutate)
        assert r == -1 and word in msg and not h.value, (r, msg)
    # a column outside nstate: refused before any launch, v untouched
    v = torch.full((5, it.Npl), 3.0, dtype=torch.float64, device=DEV)
    with pytest.raises(cm._lib.CmdgError, match="column 6"):
        cm.mesh.interpolation.project_cubed_sphere(it, v, (2, 3, 6))
    with pytest.raises(cm._lib.CmdgError, match="column 0"):
        cm.mesh.interpolation.project_cubed_sphere(it, v, (0, 3, 4))
    torch.cuda.synchronize()
    assert bool((v == 3.0).all())
    cols = (C.c_int32 * 3)(2, 3, 6)
    assert L.cmdg_interp_project(None, it.device_object(DEV), v.data_ptr(), 5, cols) == -1
    # a brick has no latitudes to project at
    gb, ib = small("brick", 4)
    vb = torch.zeros((5, ib.Npl), dtype=torch.float64, device=DEV)
    with pytest.raises(cm._lib.CmdgError, match="brick"):
        cm.mesh.interpolation.project_cubed_sphere(ib, vb, (2, 3, 4))
