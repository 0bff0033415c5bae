"""IMEX stepping on the device: AtmosAcousticGravityLinearModel (csrc/physics_atmos_linear.h),
ManyColumnLU (csrc/columnlu.hip) and ARK2GiraldoKellyConstantinescu (csrc/steppers.hip) with
LinearBackwardEulerSolver(ManyColumnLU()) -- the Held-Suarez solver configuration of
experiments/AtmosGCM/heldsuarez.jl:234-240 and the parity pin of
test/Numerics/DGMethods/Euler/acousticwave_1d_imex.jl."""
import ctypes as C
import math

import numpy as np
import pytest

from helpers import held_suarez_setup
from imex_cases import (ACOUSTIC_GOLDEN, HORIZONTAL, VERTICAL, acoustic_setup, band_to_dense,
                        column_nodes, make_pair, ref_state, small_sphere, smooth_perturbation)

pytestmark = pytest.mark.gpu


def dense_column(cm, torch, lin, grid, nvert, column, alpha):
    """Dense I - alpha L of one column, one evaluation of the linear DG per unit vector."""
    rows = column_nodes(grid, nvert, column)
    n = len(rows)
    Q = lin.create_state()
    T = lin.create_state()
    A = np.zeros((n, n))
    for j, (e, s, node) in enumerate(rows):
        Q.zero_()
        Q[e, s, node] = 1.0
        lin(T, Q, float("nan"), 1.0, 0.0)
        Tn = T.cpu().numpy()
        for i, (e2, s2, node2) in enumerate(rows):
            A[i, j] = (1.0 if i == j else 0.0) + (-alpha) * Tn[e2, s2, node2]
    return A


def test_linear_counts_and_refusals(cm, torch):
    law, grid = small_sphere(cm)
    L = cm._lib.lib()
    ip, _ = law.descriptor()
    counts = (C.c_int32 * 6)()
    ipa = (C.c_int32 * 16)(*[int(v) for v in ip])
    assert L.cmdg_physics_counts(10, C.cast(ipa, C.c_void_p), C.cast(counts, C.c_void_p)) == 0
    assert tuple(counts) == (5, law.naux, 0, 0, 0, 0)
    dg, lin = make_pair(cm, law, grid)
    # a linear model needs a stacked, vertical-direction operator for the column solver
    every = cm.dgmodel.DGModel(cm.atmos.AtmosAcousticGravityLinearModel(law), grid, direction=0,
                               state_auxiliary=dg.state_auxiliary)
    with pytest.raises(cm._lib.CmdgError, match="VerticalDirection"):
        cm.systemsolvers.ColumnLU(every, 1.0)
    every.close()
    lin.close()
    dg.close()


def test_linear_law_is_the_jacobian_of_the_full_law(cm, torch):
    """Central difference of the full DryAtmosModel (VerticalDirection, no hyperdiffusion) at the
    reference state along a smooth perturbation against the linear DG applied to it.  The
    perturbation's momentum is tangential at the walls: there the Rusanov penalty |u.n| (QM - QP)
    of the free-slip reflection is O(eps |eps|) and would leave an O(eps) difference (1.9e-3 at
    eps = 1e-2 with a normal component), everywhere else it cancels in the central difference."""
    law, grid = small_sphere(cm)
    dgv = cm.dgmodel.DGModel(law, grid, direction=VERTICAL)
    lin = cm.dgmodel.DGModel(cm.atmos.AtmosAcousticGravityLinearModel(law), grid, direction=VERTICAL,
                             state_auxiliary=dgv.state_auxiliary)
    aux = dgv.state_auxiliary.cpu().numpy()
    Q0 = ref_state(law, aux)
    dl = smooth_perturbation(grid, aux)
    dev = dgv.device
    nr = grid.nreal
    T1, T2, TL = dgv.create_state(), dgv.create_state(), dgv.create_state()
    results = []
    for eps in (1e-2, 1e-3, 1e-4):
        scale = eps * np.array([1e-3, 1.0, 1.0, 1.0, 1e2])           # rho, rho u (m/s), rho e
        d = dl * scale[None, :, None]
        dgv(T1, torch.from_numpy(Q0 + d).to(dev), 0.0, 1.0, 0.0)
        dgv(T2, torch.from_numpy(Q0 - d).to(dev), 0.0, 1.0, 0.0)
        lin(TL, torch.from_numpy(d).to(dev), 0.0, 1.0, 0.0)
        fd = ((T1 - T2) / 2).cpu().numpy()[:nr]
        ld = TL.cpu().numpy()[:nr]
        per = [np.abs(fd[:, s] - ld[:, s]).max() / np.abs(ld[:, s]).max() for s in range(5)]
        results.append((eps, max(per)))
        print("eps %.0e: relative max-norm difference per state %s" % (eps, ["%.2e" % v for v in per]))
    assert min(r for _, r in results) <= 1e-6
    lin.close()
    dgv.close()


def test_band_equals_dense_operator(cm, torch):
    law, grid = small_sphere(cm)
    dg, lin = make_pair(cm, law, grid)
    nvert = grid.topology.stacksize
    alpha = 37.5
    lu = cm.systemsolvers.ColumnLU(lin, alpha)
    S = cm.systemsolvers
    assert lu.p == lu.q == S.lower_bandwidth(grid.N[2], 5, 1)
    assert lu.n == 5 * (grid.N[2] + 1) * nvert
    lu.assemble(alpha)
    for column in (0, 7, lu.ncol - 1):
        band = lu.export_band(column)
        A = dense_column(cm, torch, lin, grid, nvert, column, alpha)
        B = band_to_dense(band, lu.p, lu.q)
        err = np.abs(A - B).max() / np.abs(A).max()
        assert err <= 1e-14, err
        i, j = np.indices(A.shape)
        outside = np.abs(i - j) > lu.p
        assert np.all(A[outside] == 0.0)
        # band slots outside the matrix stay zero
        for col in range(lu.n):
            for d in range(lu.p + lu.q + 1):
                if not 0 <= col + d - lu.q < lu.n:
                    assert band[d, col] == 0.0
    lu.close()
    lin.close()
    dg.close()


def test_factor_solve_matches_numpy(cm, torch):
    law, grid = small_sphere(cm)
    dg, lin = make_pair(cm, law, grid)
    nvert = grid.topology.stacksize
    alpha = 80.0
    lu = cm.systemsolvers.ColumnLU(lin, alpha)
    rng = np.random.default_rng(11)
    b = rng.standard_normal((grid.nelem, 5, grid.Np))
    bt = torch.from_numpy(b).to(lin.device)
    x = lin.create_state()
    lu.solve(x, bt)
    xn = x.cpu().numpy()
    for column in (0, 13, lu.ncol // 2, lu.ncol - 1):
        A = dense_column(cm, torch, lin, grid, nvert, column, alpha)
        rows = column_nodes(grid, nvert, column)
        rhs = np.array([b[e, s, n] for e, s, n in rows])
        want = np.linalg.solve(A, rhs)
        got = np.array([xn[e, s, n] for e, s, n in rows])
        err = np.abs(got - want).max() / np.abs(want).max()
        assert err <= 1e-11, err
    lu.close()
    lin.close()
    dg.close()


def test_solve_residual_update_and_determinism(cm, torch):
    """On the acoustic-wave grid: residual through the linear DG, refactoring after update(alpha2)
    bit-identical to a fresh solver, repeated factor + solve bit-identical."""
    law, grid = acoustic_setup(cm)
    dg, lin = make_pair(cm, law, grid)
    alpha1, alpha2 = 29.289321881345254, 14.644660940672627
    # a right-hand side of the size the stepper solves: the initial state plus noise in every state
    rng = np.random.default_rng(5)
    Q0 = dg.init_ode_state(0.0).cpu().numpy()
    noise = rng.standard_normal(Q0.shape) * np.array([1e-3, 1.0, 1.0, 1.0, 1e2])[None, :, None]
    b = torch.from_numpy(Q0 + noise).to(lin.device)
    lu = cm.systemsolvers.ColumnLU(lin, alpha1)
    x = lin.create_state()
    lu.solve(x, b)
    T = lin.create_state()
    lin(T, x, float("nan"), 1.0, 0.0)
    nr = grid.nreal
    r = (x - alpha1 * T - b)[:nr]
    res = (torch.linalg.vector_norm(r) / torch.linalg.vector_norm(b[:nr])).item()
    print("relative residual of the column solve: %.3e" % res)
    assert res <= 1e-12
    lu.update(alpha2)
    assert lu.alpha == alpha2
    x2 = lin.create_state()
    lu.solve(x2, b)
    lu.close()
    fresh = cm.systemsolvers.ColumnLU(lin, alpha2)
    x3 = lin.create_state()
    fresh.solve(x3, b)
    assert torch.equal(x2[:nr], x3[:nr])
    fresh.update(alpha2)
    x4 = lin.create_state()
    fresh.solve(x4, b)
    assert torch.equal(x3[:nr], x4[:nr])
    assert fresh.band_bytes == fresh.ncol * fresh.n * (fresh.p + fresh.q + 1) * 8
    fresh.close()
    lin.close()
    dg.close()


def mass_weighted_norm_with_tracer(dg, grid, Q):
    """norm(Q) of the reference's Q, which also carries rho chi: the 5-state mass-weighted norm^2
    plus int 1 dV for the tracer (rho chi = 1 initially; see test_acousticwave_golden)."""
    from cmdg_loader import cm
    M = grid.vgeo[:grid.nreal, cm.mesh.grids._M, :]
    return math.sqrt(dg.norm2_local(Q) + float(M.sum()))


def run_acoustic(cm, torch, split, law, grid, dt, nsteps, filtered=True):
    F = cm.mesh.filters
    dg, lin = make_pair(cm, law, grid)
    Q = dg.init_ode_state(0.0)
    ode = cm.odesolvers
    solver = ode.ARK2GiraldoKellyConstantinescu(
        dg, lin, ode.LinearBackwardEulerSolver(ode.ManyColumnLU(), isadjustable=True), Q, dt=dt,
        t0=0.0, split_explicit_implicit=split)
    cbs = []
    if filtered:
        filt = F.ExponentialFilter(grid, 0, 18)
        cbs = [(1, lambda s, q, t: F.apply(q, None, dg, filt, direction=VERTICAL))]
    ode.solve(Q, solver, numberofsteps=nsteps, adjustfinalstep=False, callbacks=cbs)
    assert solver.steps == nsteps
    return dg, lin, solver, Q


@pytest.mark.parametrize("split", [False, True])
def test_acousticwave_golden(cm, torch, split):
    """acousticwave_1d_imex.jl in Float64: N = 5, 10 x 5 elements, dt_factor 445 -> dt = 100 s,
    36 steps, order-18 vertical exponential filter every step; norm(Q) against
    9.5073452847149594e+13 (acousticwave_1d_imex.jl:65) at rtol = sqrt(eps).  The dry law has no
    tracer: int 1 dV (the tracer's rho chi = 1) is added to the 5-state norm^2.  The tracer's part
    is ~2.8e-10 of norm^2 and drifts from 1 by O(1e-3) of that, so the substitution errs by
    <~1e-12."""
    law, grid = acoustic_setup(cm)
    ps = law.ps
    c = math.sqrt(ps.cp_d / ps.cv_d * ps.R_d * 300.0)
    dt = 445 * (10e3 / 5) / c / 5 ** 2
    dt = 60 * 60 / math.ceil(60 * 60 / dt)
    nsteps = math.ceil(3600 / dt)
    assert (dt, nsteps) == (100.0, 36)
    dg, lin, solver, Q = run_acoustic(cm, torch, split, law, grid, dt, nsteps)
    got = mass_weighted_norm_with_tracer(dg, grid, Q)
    rel = abs(got - ACOUSTIC_GOLDEN) / ACOUSTIC_GOLDEN
    print("acoustic wave IMEX split=%s: norm(Q) = %.16e, relative error %.3e" % (split, got, rel))
    assert rel <= math.sqrt(np.finfo(float).eps)
    solver.close()
    lin.close()
    dg.close()


@pytest.mark.parametrize("split", [False, True])
def test_temporal_convergence(cm, torch, split):
    """ARK2GKC is second order: errors at dt, dt/2, dt/4 against dt/16 (2 s, no filter).  dt =
    0.2 s keeps the vertical acoustic Courant number near 1: at larger dt the unresolved stiff
    vertical modes reduce the observed order (order reduction of the stiff part, not the method's
    order)."""
    law, grid = acoustic_setup(cm, n_horz=4, n_vert=5)
    T, dt0 = 2.0, 0.2
    runs = {}
    for k in (1, 2, 4, 16):
        dg, lin, solver, Q = run_acoustic(cm, torch, split, law, grid, dt0 / k, int(round(T * k / dt0)),
                                          filtered=False)
        runs[k] = Q.clone()
        solver.close()
        lin.close()
        if k != 16:
            dg.close()
    err = [dg.euclidean_distance(runs[k], runs[16]) for k in (1, 2, 4)]
    orders = [math.log2(err[i] / err[i + 1]) for i in range(2)]
    print("split=%s errors %s observed orders %s" % (split, err, orders))
    assert min(orders) >= 1.8
    dg.close()


def test_heldsuarez_bench_size_imex(cm, torch):
    """Bench-size Held-Suarez (6 x 30 x 30 x 8, N = 4): split IMEX steps at 10x the explicit
    vertical-acoustic dt stay finite, and the mass (weightedsum of rho) is kept to 1e-12."""
    law, grid, _, _ = held_suarez_setup(n_horz=30, n_vert=8)
    dg = cm.dgmodel.DGModel(law, grid, direction=0, diffusion_direction=HORIZONTAL)
    lin = cm.dgmodel.DGModel(cm.atmos.AtmosAcousticGravityLinearModel(law), grid, direction=VERTICAL,
                             state_auxiliary=dg.state_auxiliary)
    Q = dg.init_ode_state(0.0)
    dt_v = dg.calculate_dt(Q, 1.0, direction=VERTICAL)
    dt = 10 * dt_v
    ode = cm.odesolvers
    solver = ode.ARK2GiraldoKellyConstantinescu(
        dg, lin, ode.LinearBackwardEulerSolver(ode.ManyColumnLU()), Q, dt=dt, split_explicit_implicit=True)
    m0 = cm.reductions.weightedsum(dg, Q, states=[1])
    solver.dostep(Q, 1)
    dg.synchronize()
    assert torch.isfinite(Q[:grid.nreal]).all()
    solver.dostep(Q, 4)
    dg.synchronize()
    assert torch.isfinite(Q[:grid.nreal]).all()
    m5 = cm.reductions.weightedsum(dg, Q, states=[1])
    rel = abs(m5 - m0) / abs(m0)
    print("Held-Suarez IMEX dt = %.3f s (10 x vertical acoustic %.4f s): mass drift %.3e" % (dt, dt_v, rel))
    assert rel <= 1e-12
    solver.close()
    lin.close()
    dg.close()
