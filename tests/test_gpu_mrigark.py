"""MRI-GARK stepping on the device (csrc/multirate.hip, cmdg_mrigark_step): the kernels against
NumPy bit for bit, whole steps against the NumPy restatement of the reference's dostep!s driving
oracle DG operators and the oracle column LU, the acousticwave_mrigark.jl goldens, refusals,
determinism and the bench-size Held-Suarez sphere."""
import ctypes as C
import math

import numpy as np
import pytest

from helpers import held_suarez_setup, observe
from imex_cases import (EVERY, HORIZONTAL, STATE_SCALE, VERTICAL, acoustic_setup, oracle_pair,
                        per_state_errors, small_sphere, wall_perturbation)
from mrigark_restatement import explicit_step, implicit_step

pytestmark = pytest.mark.gpu

# acousticwave_mrigark.jl:69-70, expected_result[Float64, explicit]
GOLDEN_EXPLICIT = 9.5073337869322578e+13
GOLDEN_IMPLICIT = 9.5073455070673781e+13
IMPLICIT = ("MRIGARKESDIRK24LSA", "MRIGARKESDIRK23LSA", "MRIGARKIRK21aSandu",
            "MRIGARKESDIRK34aSandu", "MRIGARKESDIRK46aSandu")


def _parr(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


@pytest.mark.parametrize("nR", [1, 2, 3, 4, 5, 6])
def test_low_level_kernels_match_numpy(cm, torch, nR):
    """cmdg_mri_lsrk_update and cmdg_mri_qhat against NumPy in the reference kernels' order, bit
    for bit on the real elements; the ghost elements are not touched."""
    law, grid = small_sphere(cm)
    dg = cm.dgmodel.DGModel(law, grid)
    rng = np.random.default_rng(nR)
    shape = (grid.nelem, law.ns, grid.Np)
    host = [rng.standard_normal(shape) for _ in range(3 + nR)]
    dev = [torch.from_numpy(h.copy()).to(dg.device) for h in host]
    dQ, Q, Qhat, R = dev[0], dev[1], dev[2], dev[3:]
    sc = (C.c_double * nR)(*rng.uniform(-2, 2, nR))
    rka, rkb_dt = -0.41789047449985195, 0.1496590219992291 * 7.3
    dg._torch_ready()
    cm._lib.check(dg.L.cmdg_mri_lsrk_update(dg.handle, dQ.data_ptr(), Q.data_ptr(), rka, rkb_dt, nR,
                                            C.cast(_parr(R), C.c_void_p), C.cast(sc, C.c_void_p)),
                  dg.handle)
    cm._lib.check(dg.L.cmdg_mri_qhat(dg.handle, Qhat.data_ptr(), Q.data_ptr(), nR,
                                     C.cast(_parr(R), C.c_void_p), C.cast(sc, C.c_void_p)), dg.handle)
    dg.synchronize()
    nr = grid.nreal
    dq = host[0][:nr].copy()
    for j in range(nR):
        dq = dq + sc[j] * host[3 + j][:nr]
    q = host[1][:nr] + rkb_dt * dq
    qh = q.copy()
    for j in range(nR):
        qh = qh + sc[j] * host[3 + j][:nr]
    got = [a.cpu().numpy() for a in (dQ, Q, Qhat)]
    assert np.array_equal(got[0][:nr], rka * dq)
    assert np.array_equal(got[1][:nr], q)
    assert np.array_equal(got[2][:nr], qh)
    for g, h in zip(got, host[:3]):
        assert np.array_equal(g[nr:], h[nr:])
    bad = (C.c_void_p * 7)(*([R[0].data_ptr()] * 7))
    r = dg.L.cmdg_mri_qhat(dg.handle, Qhat.data_ptr(), Q.data_ptr(), 7, C.cast(bad, C.c_void_p),
                           C.cast((C.c_double * 7)(), C.c_void_p))
    assert r != 0 and b"forcing arrays" in dg.L.cmdg_last_error(dg.handle)
    dg.close()


# -- whole steps against the restatement -------------------------------------------------------
def initial(cm, law, grid):
    full = cm.dgmodel.DGModel(law, grid, direction=EVERY)
    aux = full.state_auxiliary.cpu().numpy().copy()
    Q0 = law.init_state_prognostic(grid, aux, 0.0)
    Q0 = Q0 + 1e-2 * wall_perturbation(law, aux, normal=True) * STATE_SCALE[None, :, None]
    full.close()
    return np.ascontiguousarray(Q0, dtype=np.float64), aux


def fast_tableau(cm, fast):
    ode = cm.odesolvers
    s = (ode.LSRK54CarpenterKennedy if fast == "LSRK54" else ode.LSRK144NiegemannDiehlBusch)
    return s


def device_run(cm, torch, law, grid, Q0, name, fast, dt, fast_dt, nsteps, adjustable=True):
    """Device MRI-GARK steps from Q0; the state after every step.  Explicit schemes: slow = full
    minus linear, fast = the vertical linear law; decoupled-implicit: slow = the linear law with
    the column LU, fast = full minus linear."""
    ode, dgm = cm.odesolvers, cm.dgmodel
    full = dgm.DGModel(law, grid, direction=EVERY, diffusion_direction=HORIZONTAL)
    lin = dgm.DGModel(cm.atmos.AtmosAcousticGravityLinearModel(law), grid, direction=VERTICAL,
                      state_auxiliary=full.state_auxiliary)
    rem = dgm.remainder_DGModel(full, (lin,))
    Q = torch.from_numpy(Q0.copy()).to(full.device)
    make = getattr(ode, name)
    if ode.MRIGARK_TABLEAUS[name][0] == "explicit":
        solver = make(rem, fast_tableau(cm, fast)(lin, Q, dt=fast_dt), Q, dt=dt)
    else:
        solver = make(lin, ode.LinearBackwardEulerSolver(ode.ManyColumnLU(), isadjustable=adjustable),
                      fast_tableau(cm, fast)(rem, Q, dt=fast_dt), Q, dt=dt)
    out = []
    for _ in range(nsteps):
        solver.dostep(Q, 1)
        full.synchronize()
        out.append(Q.cpu().numpy().copy())
    assert float(np.abs(solver.fastsolver.dQ.cpu().numpy()[:grid.nreal]).max()) == 0.0
    solver.close()
    lin.close()
    full.close()
    return out


def restated_run(cm, oracle, law, grid, Q0, aux, name, fast, dt, fast_dt, nsteps):
    ode = cm.odesolvers
    full, lin = oracle_pair(oracle, law, grid, state_auxiliary=aux.copy(), diffusion_direction=HORIZONTAL)
    nr = grid.nreal
    rv = slice(0, nr)
    kind, mk = ode.MRIGARK_TABLEAUS[name]
    Gs, ghs = mk()
    Q = Q0.copy()
    dQ = np.zeros_like(Q)
    if fast == "LSRK54":
        from test_mrigark_host import lsrk54_tableau
        RK = lsrk54_tableau()
    else:
        RK = ode.LSRK144_COEFFICIENTS

    def rem(R, Qs, t, beta):
        full(R, Qs, t, 1.0, beta)
        lin(R, Qs, t, -1.0, 1.0)

    out = []
    t = 0.0
    if kind == "explicit":
        G, _, dc = ode.mrigark_explicit_coefficients(Gs, ghs)
        Rs = [np.zeros_like(Q) for _ in dc]
        for _ in range(nsteps):
            explicit_step(Q, t, dt, G.tolist(), dc.tolist(), lambda R, Qs, tt: rem(R, Qs, tt, 0.0),
                          lambda d, Qs, tt: lin(d, Qs, tt, 1.0, 1.0), dQ, RK, fast_dt, Rs, rv)
            t += dt
            out.append(Q.copy())
    else:
        G, _, dc = ode.mrigark_implicit_coefficients(Gs, ghs)
        Rs = [np.zeros_like(Q) for _ in dc]
        Qhat = np.zeros_like(Q)
        lu = oracle.OracleColumnLU(lin, grid.topology.stacksize, dt * G[0][1][1])

        def besolve(Qs, Qh, alpha, tt):
            if alpha != lu.alpha:
                lu.update(alpha)
            lu.solve(Qs, Qh)

        for _ in range(nsteps):
            implicit_step(Q, t, dt, G.tolist(), dc.tolist(), lambda R, Qs, tt: lin(R, Qs, tt, 1.0, 0.0),
                          besolve, lambda d, Qs, tt: rem(d, Qs, tt, 1.0), dQ, RK, fast_dt, Rs, Qhat, rv)
            t += dt
            out.append(Q.copy())
    return out


CASES = ([("MRIGARKERK33aSandu", f) for f in ("LSRK54", "LSRK144")]
         + [("MRIGARKERK45aSandu", f) for f in ("LSRK54", "LSRK144")]
         + [(n, "LSRK54") for n in IMPLICIT])


@pytest.mark.parametrize("hyper", [False, True])
@pytest.mark.parametrize("name,fast", CASES)
def test_step_matches_restatement(cm, torch, oracle, name, fast, hyper):
    """cmdg_mrigark_step against the restatement over oracle operators after 1 and 3 slow steps
    (30 s) on the small sphere, N = 4.  The fast dt (2.7 s for the vertical linear law, 7 s for
    the remainder) does not divide the stages, so every stage ends on a shortened fast step.  The
    increments Q_n - Q_0 are compared per state; the observed maximum is recorded."""
    law, grid = small_sphere(cm, N=4, hyper=hyper)
    Q0, aux = initial(cm, law, grid)
    explicit = cm.odesolvers.MRIGARK_TABLEAUS[name][0] == "explicit"
    dt, fast_dt = 30.0, (2.7 if explicit else 7.0)
    got = device_run(cm, torch, law, grid, Q0, name, fast, dt, fast_dt, 3)
    want = restated_run(cm, oracle, law, grid, Q0, aux, name, fast, dt, fast_dt, 3)
    nr = grid.nreal
    for n in (0, 2):
        errs = per_state_errors(got[n][:nr] - Q0[:nr], want[n][:nr] - Q0[:nr])
        same = np.array_equal(got[n][:nr], want[n][:nr])
        print("%s/%s hyper=%s step %d: bit-identical %s, increment error per state %s"
              % (name, fast, hyper, n + 1, same, ["%.2e" % e for e in errs]))
        observe("mrigark increment vs restatement (%s, %s, hyper=%s, %d steps)" % (name, fast, hyper, n + 1),
                max(errs))
        assert max(errs) <= 1e-10, errs
        assert np.all(np.isfinite(got[n][:nr]))


def test_step_is_deterministic(cm, torch):
    law, grid = small_sphere(cm, N=4, hyper=True)
    Q0, _ = initial(cm, law, grid)
    for name in ("MRIGARKERK45aSandu", "MRIGARKESDIRK24LSA"):
        fd = 2.7 if name == "MRIGARKERK45aSandu" else 7.0
        a = device_run(cm, torch, law, grid, Q0, name, "LSRK54", 30.0, fd, 2)
        b = device_run(cm, torch, law, grid, Q0, name, "LSRK54", 30.0, fd, 2)
        assert np.array_equal(a[-1][:grid.nreal], b[-1][:grid.nreal]), name


# -- the reference's goldens ---------------------------------------------------------------------
def mass_weighted_norm_with_tracer(cm, dg, grid, Q):
    """norm(Q) with the reference's tracer rho chi = 1 (as test_gpu_imex.py's golden does)."""
    M = grid.vgeo[:grid.nreal, cm.mesh.grids._M, :]
    return math.sqrt(dg.norm2_local(Q) + float(M.sum()))


@pytest.mark.parametrize("explicit", [True, False])
def test_acousticwave_mrigark_golden(cm, torch, explicit):
    """acousticwave_mrigark.jl in Float64: N = 5, 10 x 5 elements, 1 h, the order-18 vertical
    exponential filter after every slow step, adjustfinalstep = false.  Explicit: ERK45a on the
    remainder, LSRK54 on the vertical linear law at vmnd / c, slow dt 5 vmnd / c rounded to divide
    3600 s.  Implicit: ESDIRK24LSA on the linear law with a non-adjustable column LU at
    dt = 3600 / ceil(3600 / (200 vmnd / c)), LSRK54 on the remainder at min(min(hmnd, vmnd),
    hmnd / c).  norm(Q) within sqrt(eps) of the reference's."""
    ode, dgm, F = cm.odesolvers, cm.dgmodel, cm.mesh.filters
    law, grid = acoustic_setup(cm)
    ps = law.ps
    full = dgm.DGModel(law, grid, direction=EVERY)
    lin = dgm.DGModel(cm.atmos.AtmosAcousticGravityLinearModel(law), grid, direction=VERTICAL,
                      state_auxiliary=full.state_auxiliary)
    rem = dgm.remainder_DGModel(full, (lin,))
    hmnd = full.min_node_distance(HORIZONTAL)
    vmnd = full.min_node_distance(VERTICAL)
    c = math.sqrt(ps.cp_d / ps.cv_d * ps.R_d * 300.0)
    Q = full.init_ode_state(0.0)
    vdt = vmnd / c
    if explicit:
        rdt = 5 * vdt
        rdt = 3600 / math.ceil(3600 / rdt)
        nsteps = math.ceil(3600 / rdt)
        solver = ode.MRIGARKERK45aSandu(rem, ode.LSRK54CarpenterKennedy(lin, Q, dt=vdt), Q, dt=rdt)
    else:
        rdt = min(min(hmnd, vmnd) / 1.0, hmnd / c)
        vdt = 200 * vdt
        vdt = 3600 / math.ceil(3600 / vdt)
        nsteps = math.ceil(3600 / vdt)
        solver = ode.MRIGARKESDIRK24LSA(
            lin, ode.LinearBackwardEulerSolver(ode.ManyColumnLU(), isadjustable=False),
            ode.LSRK54CarpenterKennedy(rem, Q, dt=rdt), Q, dt=vdt)
    print("vmnd %.6f hmnd %.3f: %d slow steps" % (vmnd, hmnd, nsteps))
    filt = F.ExponentialFilter(grid, 0, 18)
    cbs = [(1, lambda s, q, t: F.apply(q, None, full, filt, direction=VERTICAL))]
    ode.solve(Q, solver, numberofsteps=nsteps, adjustfinalstep=False, callbacks=cbs)
    assert solver.steps == nsteps
    got = mass_weighted_norm_with_tracer(cm, full, grid, Q)
    want = GOLDEN_EXPLICIT if explicit else GOLDEN_IMPLICIT
    rel = abs(got - want) / want
    print("acoustic wave MRI-GARK explicit=%s: %d steps, norm(Q) = %.16e, relative error %.3e"
          % (explicit, nsteps, got, rel))
    observe("mrigark acousticwave golden relative error (explicit=%s)" % explicit, rel)
    assert rel <= math.sqrt(np.finfo(float).eps)
    solver.close()
    lin.close()
    full.close()


# -- refusals -----------------------------------------------------------------------------------
def test_refusals_name_the_member(cm, torch):
    ode, dgm, L_ = cm.odesolvers, cm.dgmodel, cm._lib
    law, grid = small_sphere(cm, N=4)
    full = dgm.DGModel(law, grid, direction=EVERY)
    lin = dgm.DGModel(cm.atmos.AtmosAcousticGravityLinearModel(law), grid, direction=VERTICAL,
                      state_auxiliary=full.state_auxiliary)
    rem = dgm.remainder_DGModel(full, (lin,))
    Q = full.init_ode_state(0.0)
    solver = ode.MRIGARKERK45aSandu(rem, ode.LSRK54CarpenterKennedy(lin, Q, dt=2.0), Q, dt=10.0)
    L = full.L
    d = solver._desc
    d.fast_dt = 2.0

    def call(slow=full.handle, sm=lin.handle, fast=lin.handle, fm=None, lu=None, desc=d,
             work=solver._work, dt=10.0):
        full._torch_ready()
        return L.cmdg_mrigark_step(slow, sm, fast, fm, lu, C.byref(desc), Q.data_ptr(),
                                   C.cast(work, C.c_void_p) if work is not None else None, 0.0, dt)

    def refused(match, **kw):
        r = call(**kw)
        assert r == -1, r                                         # CMDG_ERR_INVALID
        msg = L.cmdg_last_error(full.handle).decode()
        assert match in msg, msg
        return msg

    assert call() == 0
    # another grid: the fast member is named
    law2, grid2 = small_sphere(cm, N=4, nvert=2)
    full2 = dgm.DGModel(law2, grid2, direction=EVERY)
    other = dgm.DGModel(cm.atmos.AtmosAcousticGravityLinearModel(law2), grid2, direction=VERTICAL,
                        state_auxiliary=full2.state_auxiliary)
    msg = refused("another grid", fast=other.handle)
    assert msg.startswith("fast: "), msg
    refused("dt must be > 0", dt=0.0)
    refused("dt must be > 0", dt=-1.0)
    for field, value, match in (("nstages", 7, "slow stages"), ("fast_nstages", 15, "14"),
                                ("fast_dt", 0.0, "fast dt"), ("kind", 1, "column solver")):
        old = getattr(d, field)
        setattr(d, field, value)
        msg = refused(match)
        setattr(d, field, old)
    d.fast_dt = -1.0
    assert refused("fast dt").startswith("slow minus / fast: ")
    d.fast_dt = 2.0
    work = (C.c_void_p * 7)(*list(solver._work)[:5], None, None)
    refused("the fast dQ", work=work)
    refused("work array list", work=None)
    # host-side refusals
    with pytest.raises(TypeError, match="LowStorageRungeKutta2N"):
        ode.MRIGARKERK45aSandu(rem, ode.SSPRK33ShuOsher(lin, Q, dt=1.0), Q, dt=10.0)
    with pytest.raises(TypeError, match="nested"):
        ode.MRIGARKERK45aSandu(rem, solver, Q, dt=10.0)
    with pytest.raises(L_.CmdgError, match="exactly one"):
        dgm.remainder_DGModel(full, (lin, lin))
    with pytest.raises(L_.CmdgError, match="another grid"):
        dgm.remainder_DGModel(full, (other,))
    # isadjustable = false: a dt that needs another alpha is refused, the same dt runs
    imp = ode.MRIGARKESDIRK24LSA(lin, ode.LinearBackwardEulerSolver(ode.ManyColumnLU(), isadjustable=False),
                                 ode.LSRK54CarpenterKennedy(rem, Q, dt=5.0), Q, dt=20.0)
    imp.dostep(Q, 1)
    with pytest.raises(ValueError, match="isadjustable"):
        imp.updatedt(10.0)
    with pytest.raises(ValueError, match="isadjustable"):
        imp.dostep(Q, 1, dt=10.0)
    # ... and by the library itself
    dd = imp._desc
    r = L.cmdg_mrigark_step(lin.handle, None, full.handle, lin.handle, imp.lu.handle, C.byref(dd),
                            Q.data_ptr(), C.cast(imp._work, C.c_void_p), 0.0, 10.0)
    assert r == -1 and b"not adjustable" in L.cmdg_last_error(lin.handle)
    imp.close()
    # the ARK path honours the flag too
    ark = ode.ARK2GiraldoKellyConstantinescu(
        full, lin, ode.LinearBackwardEulerSolver(ode.ManyColumnLU(), isadjustable=False), Q, dt=20.0,
        split_explicit_implicit=True)
    with pytest.raises(ValueError, match="isadjustable"):
        ark.updatedt(10.0)
    with pytest.raises(ValueError, match="isadjustable"):
        ark.dostep(Q, 1, dt=10.0)
    ark.close()
    other.close()
    full2.close()
    lin.close()
    full.close()


# -- the bench sphere ---------------------------------------------------------------------------
BENCH = {"MRIGARKERK45aSandu": (20.0, 1.0), "MRIGARKESDIRK24LSA": (60.0, 20.0)}


@pytest.mark.parametrize("name", sorted(BENCH))
def test_heldsuarez_bench_size_mrigark(cm, torch, name):
    """Bench-size Held-Suarez (6 x 30 x 30 x 8, N = 4, full physics): 5 slow steps stay finite
    and weightedsum(rho) changes by <= 1e-12 relative.  (slow dt, fast dt as multiples of the
    vertical acoustic dt): ERK45a on the remainder over LSRK54 on the linear law, ESDIRK24LSA on
    the linear law over LSRK54 on the remainder."""
    ode, dgm = cm.odesolvers, cm.dgmodel
    law, grid, _, _ = held_suarez_setup(n_horz=30, n_vert=8)
    full = dgm.DGModel(law, grid, direction=EVERY, diffusion_direction=HORIZONTAL)
    lin = dgm.DGModel(cm.atmos.AtmosAcousticGravityLinearModel(law), grid, direction=VERTICAL,
                      state_auxiliary=full.state_auxiliary)
    rem = dgm.remainder_DGModel(full, (lin,))
    Q = full.init_ode_state(0.0)
    dt_v = full.calculate_dt(Q, 1.0, direction=VERTICAL)
    slow_f, fast_f = BENCH[name]
    if name == "MRIGARKERK45aSandu":
        solver = ode.MRIGARKERK45aSandu(rem, ode.LSRK54CarpenterKennedy(lin, Q, dt=fast_f * dt_v), Q,
                                        dt=slow_f * dt_v)
    else:
        solver = ode.MRIGARKESDIRK24LSA(lin, ode.LinearBackwardEulerSolver(ode.ManyColumnLU()),
                                        ode.LSRK54CarpenterKennedy(rem, Q, dt=fast_f * dt_v), Q,
                                        dt=slow_f * dt_v)
    m0 = cm.reductions.weightedsum(full, Q, states=[1])
    ode.solve(Q, solver, numberofsteps=5)
    m1 = cm.reductions.weightedsum(full, Q, states=[1])
    assert bool(torch.isfinite(Q[:grid.nreal]).all())
    print("%s: dt %.2f s, mass drift %.2e" % (name, slow_f * dt_v, abs(m1 - m0) / abs(m0)))
    assert abs(m1 - m0) <= 1e-12 * abs(m0)
    solver.close()
    lin.close()
    full.close()
