"""ESDGModel on the device (cmdg_create_esdg; csrc/esdg.h k_esdg_tendency, k_esdg_entropy) against
the NumPy restatement of the reference's kernels (tests/esdg_restatement.py) and the reference's own
operator identities (test/Numerics/ESDGMethods/DryAtmos/run_tests.jl:107-207).  Errors are relative
L-infinity per state, each tendency column normalised by its own maximum."""
import ctypes as C

import numpy as np
import pytest

from cmdg_loader import cm
import esdg_restatement as R
from esdg_cases import approx, case_a, case_b, case_c, per_state_rel_linf
from test_esdg_host import check_operator_identities

pytestmark = pytest.mark.gpu
E = cm.esdg
MATRIX_ON = dict(Mcut=0.1, low_mach=True, kinetic_energy_preserving=True)
VOLUME = {"ec": (E.EntropyConservative, R.EC), "central": (E.CentralVolumeFlux, R.CENTRAL),
          "kg": (E.KGVolumeFlux, R.KG)}
SURFACE = {"none": (None, R.NONE), "ec": (E.EntropyConservative, R.EC), "rusanov": (E.RusanovNumericalFlux, R.RUSANOV),
           "penalty": (E.EntropyConservativeWithPenalty, R.EC_PENALTY), "matrix": (E.MatrixFlux, R.MATRIX)}
ALPHA_BETA = ((1.0, 0.0), (1.0, 1.0), (0.5, 2.0))


def _models(law, grid, aux, vol, surf, matrix=None):
    vf = VOLUME[vol][0]() if vol else None
    sf = SURFACE[surf][0]
    sf = None if sf is None else (sf(**matrix) if matrix else sf())
    dg = cm.dgmodel.ESDGModel(law, grid, volume_numerical_flux_first_order=vf,
                              surface_numerical_flux_first_order=sf, state_auxiliary=aux)
    ref = R.ESDGRestatement(law, grid, VOLUME[vol][1] if vol else R.NONE, SURFACE[surf][1],
                            state_auxiliary=aux, matrix=matrix)
    return dg, ref


def _compare(torch, dg, ref, grid, Q, label, bound=1e-12, alpha_beta=ALPHA_BETA):
    Qh = Q.cpu().numpy().copy()
    T0 = np.random.default_rng(11).standard_normal(Qh.shape)
    for alpha, beta in alpha_beta:
        T = torch.from_numpy(T0.copy()).to(Q.device)
        Th = T0.copy()
        dg(T, Q, 0.0, alpha, beta)
        ref(Th, Qh, 0.0, alpha, beta)
        err = per_state_rel_linf(T.cpu().numpy()[:grid.nreal], Th[:grid.nreal])
        print("%s (%.1f, %.1f): per-state rel Linf %s" % (label, alpha, beta, " ".join("%.2e" % v for v in err)))
        assert np.all(err <= bound), (label, alpha, beta, err)


@pytest.mark.parametrize("N", [3, 4])
@pytest.mark.parametrize("surf", list(SURFACE))
@pytest.mark.parametrize("vol", list(VOLUME))
def test_one_evaluation_grid_a(torch, N, vol, surf):
    """Grid A, every volume flux x every surface flux (none included): <= 1e-12 per state."""
    law, grid, aux, _ = case_a(N)
    dg, ref = _models(law, grid, aux, vol, surf)
    _compare(torch, dg, ref, grid, dg.init_ode_state(0.0), "A N=%d %s+%s" % (N, vol, surf))
    dg.close()


@pytest.mark.parametrize("vol,surf,matrix", [("ec", "rusanov", None), ("kg", "matrix", MATRIX_ON)])
def test_one_evaluation_grid_b(torch, vol, surf, matrix):
    """Grid B (walls on all six sides, Gravity), N = 4: <= 1e-12 per state."""
    law, grid, aux, _ = case_b(4)
    dg, ref = _models(law, grid, aux, vol, surf, matrix)
    _compare(torch, dg, ref, grid, dg.init_ode_state(0.0), "B %s+%s" % (vol, surf))
    dg.close()


def test_one_evaluation_grid_c(torch):
    """Grid C (cubed sphere, the baroclinic-wave pairing KG + Rusanov, Coriolis + Gravity, reference
    state).  The pressure-gradient and gravity terms partly cancel, so the bound per state is
    max(1e-12, 4 x the restatement's own float64-versus-longdouble error on this case): the factor
    4 allows for one-ulp differences in division ordering."""
    law, grid = case_c(3)
    dg, ref = _models(law, grid, None, "kg", "rusanov")
    Q = dg.init_ode_state(0.0)
    Qh = Q.cpu().numpy()
    ld = np.longdouble
    refl = R.ESDGRestatement(law, grid, R.KG, R.RUSANOV, dtype=ld)
    T64, Tl = np.zeros_like(Qh), np.zeros(Qh.shape, dtype=ld)
    ref(T64, Qh.copy())
    refl(Tl, Qh.astype(ld))
    own = per_state_rel_linf(T64[:grid.nreal], Tl[:grid.nreal])
    bound = np.maximum(1e-12, 4 * own)
    print("C restatement float64 vs longdouble %s -> bound %s" % (" ".join("%.2e" % v for v in own),
                                                                 " ".join("%.2e" % v for v in bound)))
    _compare(torch, dg, ref, grid, Q, "C kg+rusanov", bound)
    dg.close()


@pytest.mark.parametrize("name,rho", [("uniform", lambda rng, shape: np.full(shape, 1.5)),
                                      ("1+1e-9u", lambda rng, shape: 1 + 1e-9 * rng.random(shape))])
def test_logave_series_branch(torch, name, rho):
    """Every density pair in the series branch of logave: u = 0 (uniform density) and 0 < u < eps."""
    law, grid, aux, _ = case_a(4, rho=rho)
    dg, ref = _models(law, grid, aux, "ec", "ec")
    _compare(torch, dg, ref, grid, dg.init_ode_state(0.0), "A logave " + name)
    dg.close()


def test_check_operators(torch):
    """The three check_operators identities on the device tendency, grid A, N = 4, the reference's
    tolerances; the global entropy sums through cmdg_esdg_entropy and the device dot."""
    law, grid, aux, _ = case_a(4)
    T, sums = {}, {}
    for name, vol, surf in (("volume", "ec", "none"), ("surface", None, "ec"), ("full", "ec", "ec")):
        dg, _ = _models(law, grid, aux, vol, surf)
        Q = dg.init_ode_state(0.0)
        Td = torch.zeros_like(Q)
        dg(Td, Q, 0.0)
        beta = dg.entropy_variables(Q)
        sums[name] = cm.dot(dg, beta[:, :5, :].contiguous(), Td)
        T[name] = Td.cpu().numpy()
        Qh, betah = Q.cpu().numpy(), beta.cpu().numpy()
        dg.close()
    vol_sum, surf_sum, full_sum = check_operator_identities(grid, Qh, betah, T)
    print("device dot: volume %.16e surface %.16e full %.3e" % (sums["volume"], sums["surface"], sums["full"]))
    assert approx(sums["volume"], -sums["surface"])
    assert abs(sums["full"]) <= np.sqrt(np.spacing(abs(sums["volume"])))
    assert approx(sums["volume"], vol_sum)


def test_time_stepping(torch):
    """Ten LSRK54CarpenterKennedy steps on grid A (N = 3, EntropyConservative + Rusanov, the random
    state) against the restatement's ten steps at 1e-11, with the reference's Courant-free dt = 1e-3.
    The warp angle is a quarter of the reference's: at 3 x 4 x 5 elements the full warp folds elements
    over (min M = -5.7e-4, esdg_cases.grid_a) and every run, the restatement's included, is NaN after
    two steps whatever the state; with a quarter of it min M = 5.2e-5 > 0, the metrics still vary
    from node to node, and the ten steps move the state by 0.7 (rho) to 2.2 (rho e)."""
    dt, nsteps = 1e-3, 10
    law, grid, aux, _ = case_a(3, warp_scale=0.25)
    assert grid.vgeo[:, 9, :].min() > 0
    dg, ref = _models(law, grid, aux, "ec", "rusanov")
    Q = dg.init_ode_state(0.0)
    Qh = Q.cpu().numpy().copy()
    cm.odesolvers.LSRK54CarpenterKennedy(dg, Q, dt=dt).dostep(Q, nsteps=nsteps)
    dg.synchronize()
    R.lsrk54_steps(ref, Qh, dt, nsteps)
    err = per_state_rel_linf(Q.cpu().numpy()[:grid.nreal], Qh[:grid.nreal])
    print("10 steps: per-state rel Linf %s" % " ".join("%.2e" % v for v in err))
    assert np.all(err <= 1e-11)
    dg.close()


def test_two_ranks(torch):
    """Two ranks of one process through connect_local against one rank, grid A with 4 x 3 x 2
    elements, auxiliary ghosts by global element id: an evaluation, then an incrementing one (a
    second exchange), <= 1e-12 per state."""
    Ne = (4, 3, 2)
    law, grid, aux, _ = case_a(3, Ne)
    one, _ = _models(law, grid, aux, "ec", "rusanov")
    Q1 = one.init_ode_state(0.0)
    T1 = torch.zeros_like(Q1)
    one(T1, Q1, 0.0)
    one(T1, Q1, 0.0, 0.5, 2.0)
    parts = [case_a(3, Ne, rank=r, size=2) for r in range(2)]
    dgs = [_models(p[0], p[1], p[2], "ec", "rusanov")[0] for p in parts]
    cm.dgmodel.connect_local(dgs)
    Qs = [d.init_ode_state(0.0) for d in dgs]
    Ts = [torch.zeros_like(q) for q in Qs]
    cm.dgmodel.group_rhs(dgs, Ts, Qs, 0.0)
    cm.dgmodel.group_rhs(dgs, Ts, Qs, 0.0, 0.5, 2.0)
    Tn = [t.cpu().numpy() for t in Ts]
    for full, got in ((T1.cpu().numpy(), Tn),):
        by_global = {int(gid): full[i] for i, gid in enumerate(grid.topology.globalelems[:grid.nreal])}
        for p, a in zip(parts, got):
            g = p[1]
            assert g.nelem > g.nreal
            want = np.stack([by_global[int(gid)] for gid in g.topology.globalelems[:g.nreal]])
            err = per_state_rel_linf(a[:g.nreal], want)
            assert np.all(err <= 1e-12), err
    for d in dgs + [one]:
        d.close()


def test_entropy_call(torch):
    """cmdg_esdg_entropy against the host transforms at 1e-14 relative per column, and the host
    round trip entropy_variables_to_state."""
    law, grid, aux, _ = case_a(3)
    dg, ref = _models(law, grid, aux, "ec", "ec")
    Q = dg.init_ode_state(0.0)
    Qh = Q.cpu().numpy()
    beta, eta = dg.entropy_variables(Q).cpu().numpy(), dg.entropy(Q).cpu().numpy()
    bh, eh = E.state_to_entropy_variables(Qh), E.state_to_entropy(Qh)[:, None, :]
    for got, want in ((beta, bh), (eta, eh), (beta, ref.entropy_variables(Qh)), (eta, ref.entropy(Qh))):
        err = np.max(np.abs(got - want), axis=(0, 2)) / np.max(np.abs(want), axis=(0, 2))
        print("entropy columns:", " ".join("%.2e" % v for v in err))
        assert np.all(err <= 1e-14)
    back, _ = E.entropy_variables_to_state(beta)
    assert approx(back, Qh).all()
    # a handle that is not an ESDGModel's refuses the call
    from helpers import pseudo1d_setup
    plaw, pgrid, _ = pseudo1d_setup(Ne=2)
    plain = cm.dgmodel.DGModel(plaw, pgrid)
    assert plain.L.cmdg_esdg_entropy(plain.handle, Q.data_ptr(), None, None) == -5
    assert b"not an ESDGModel handle" in plain.L.cmdg_last_error(plain.handle)
    plain.close()
    dg.close()


def test_refusals(torch):
    """Every refusal of cmdg_create_esdg and of the calls an ESDG handle does not serve: status and
    a message that names the cause."""
    L = cm._lib
    INVALID, UNSUPPORTED = -1, -5
    law, grid, aux, _ = case_a(3, Ne=(3, 3, 3))
    with pytest.raises(L.CmdgError, match=r"\(-1\).*use cmdg_create_esdg"):
        cm.dgmodel.DGModel(law, grid, state_auxiliary=aux)
    dg = cm.dgmodel.ESDGModel(law, grid, state_auxiliary=aux)
    lib = dg.L

    def create(desc_edit=None, **esdg_edit):
        d = type(dg._desc).from_buffer_copy(dg._desc)
        ed = type(dg._esdg_desc).from_buffer_copy(dg._esdg_desc)
        if desc_edit:
            desc_edit(d)
        for k, v in esdg_edit.items():
            setattr(ed, k, v)
        h = C.c_void_p()
        rc = lib.cmdg_create_esdg(C.byref(d), C.byref(ed), C.byref(h))
        assert not h.value
        return rc, lib.cmdg_last_error(None).decode()

    def expect(rc_msg, status, text):
        assert rc_msg[0] == status and text in rc_msg[1], rc_msg

    def other_law(d):
        d.physics_id = 2

    def order(n0, n1, n2):
        def edit(d):
            d.N[:] = [n0, n1, n2]
        return edit

    def dim2(d):
        d.dim = 2

    expect(create(other_law), UNSUPPORTED, "CMDG_PHYSICS_ESDG_DRY_ATMOS only")
    expect(create(order(2, 2, 2)), UNSUPPORTED, "polynomial orders 3 and 4")
    expect(create(order(5, 5, 5)), UNSUPPORTED, "polynomial orders 3 and 4")
    expect(create(order(3, 3, 4)), UNSUPPORTED, "mixed polynomial orders")
    expect(create(order(4, 3, 3)), UNSUPPORTED, "mixed polynomial orders")
    expect(create(dim2), UNSUPPORTED, "dim == 3")
    expect(create(volume_flux=7), INVALID, "unknown volume flux")
    expect(create(volume_flux=L.ESDG_FLUX_RUSANOV), INVALID, "unknown volume flux")
    expect(create(surface_flux=-1), INVALID, "unknown surface flux")
    expect(create(surface_flux=L.ESDG_FLUX_KG), INVALID, "unknown surface flux")

    fd, fh = cm.mesh.filters.CmdgFilterDesc(), C.c_void_p()
    assert lib.cmdg_filter_create(dg.handle, C.byref(fd), C.byref(fh)) == UNSUPPORTED
    assert b"ESDGModel handle applies no element filters" in lib.cmdg_last_error(dg.handle)
    hk = L.CmdgRhsHooks()
    assert lib.cmdg_set_rhs_hooks(dg.handle, C.byref(hk)) == UNSUPPORTED
    assert b"ESDGModel handle runs no update_auxiliary_state!" in lib.cmdg_last_error(dg.handle)
    lu = C.c_void_p()
    assert lib.cmdg_columnlu_create(dg.handle, 3, 1.0, C.byref(lu)) == UNSUPPORTED
    assert b"column LU is not available on an ESDGModel handle" in lib.cmdg_last_error(dg.handle)
    sd = L.CmdgStackIntegralDesc()
    sd.nout = 1
    Imat = np.eye(4)
    assert lib.cmdg_indefinite_stack_integral(dg.handle, None, 0, dg.state_auxiliary.data_ptr(), 4, 3,
                                              Imat.ctypes.data, C.byref(sd)) == UNSUPPORTED
    assert b"ESDGModel handle serves no column operators" in lib.cmdg_last_error(dg.handle)
    assert lib.cmdg_reverse_indefinite_stack_integral(dg.handle, dg.state_auxiliary.data_ptr(), 4, 3,
                                                      C.byref(sd)) == UNSUPPORTED
    # CMDG_OPT_STEP_GRAPH is accepted and ignored: the handle stays eager
    dg.set_option(L.OPT_STEP_GRAPH, 1)
    Q = dg.init_ode_state(0.0)
    cm.odesolvers.LSRK54CarpenterKennedy(dg, Q, dt=1e-3).dostep(Q, nsteps=3)
    dg.synchronize()
    assert dg.query("GRAPH_STEPS") == 0
    dg.close()
