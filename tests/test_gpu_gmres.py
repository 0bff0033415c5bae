"""The device GMRES (csrc/gmres.hip, cmdg_gmres_*) and the no-orientation acoustic linear law
(csrc/physics_atmos_linear.h, ORIENT = false): solves against the NumPy restatement
(tests/gmres_restatement.py) driving the oracle's operator, the true residual, the column LU, early
exit and iteration limit, determinism, the law against the oracle twin, refusals.  The CPU reference
of the no-orientation law is the oracle's acoustic-gravity law on a flat, grav = 0 twin model
(tests/gmres_cases.py)."""
import ctypes as C
import math
import time
import warnings

import numpy as np
import pytest

from gmres_cases import (EVERY, HORIZONTAL, MEASURED, VERTICAL, device_pair, oracle_acoustic, random_state,
                         small_brick, soundspeed, vortex_law)
from gmres_restatement import GMRES, euler_operator
from helpers import observe
from imex_cases import per_state_errors, per_state_rel

pytestmark = pytest.mark.gpu

A_II = 1 - 1 / math.sqrt(2)             # ARK2GKC's implicit diagonal
RTOL = 1e-8
CASES = [(1.0, 10), (4.0, 10), (1.0, 3), (4.0, 3)]     # (acoustic Courant number, M)
MAX_ITERS = 400


def brick_case(cm, courant):
    law = vortex_law(cm)
    grid, h = small_brick(cm)
    dt = courant * cm.mesh.grids.min_node_distance(grid) / soundspeed(law.ps, law.init_state.T_inf)
    return law, grid, dt * A_II


@pytest.fixture(scope="module")
def restated(cm, oracle):
    """The restatement's solves of the four cases on the oracle operator, computed once."""
    out = {}
    for courant, M in CASES:
        law, grid, alpha = brick_case(cm, courant)
        olin = oracle_acoustic(cm, oracle, grid)
        guess, rhs = random_state(grid, 11), random_state(grid, 12)
        x = guess.copy()
        info = GMRES(x, M=M, rtol=RTOL, rv=slice(0, grid.nreal)).linearsolve(
            euler_operator(olin, alpha), x, rhs, max_iters=MAX_ITERS)
        out[(courant, M)] = (x, info)
    return out


def device_solve(cm, torch, courant, M, max_iters=MAX_ITERS, rtol=RTOL, atol=2.0 ** -52):
    law, grid, alpha = brick_case(cm, courant)
    dg, lin = device_pair(cm, law, grid)
    gm = cm.systemsolvers.GmresSolver(lin, alpha, cm.systemsolvers.GeneralizedMinimalResidual(
        None, M=M, rtol=rtol, atol=atol))
    x = torch.from_numpy(random_state(grid, 11)).to(lin.device)
    rhs = torch.from_numpy(random_state(grid, 12)).to(lin.device)
    info = gm.solve(x, rhs, max_iters=max_iters)
    # the true residual, with an operator evaluation of its own
    r = x.clone()
    lin(r, x, 0.0, -alpha, 1.0)
    lin.synchronize()
    nr = grid.nreal
    true_res = float(np.linalg.norm((rhs.cpu().numpy() - r.cpu().numpy())[:nr].ravel()))
    out = x.cpu().numpy().copy()
    gm.close(), lin.close(), dg.close()
    return out, info, true_res, nr


def test_restatement_margins(restated):
    """The iteration counts are compared only where the restatement's deciding residuals stay 1e-6
    (relative) away from the threshold; at least 3 of the 4 cases must."""
    safe = [k for k, (_, info) in restated.items() if info.margin() >= 1e-6]
    assert len(safe) >= 3, {k: i.margin() for k, (_, i) in restated.items()}


@pytest.mark.parametrize("courant,M", CASES)
def test_solve_matches_restatement_and_true_residual(cm, torch, restated, courant, M):
    """Solution, residual norm and iteration count against the restatement; the true residual
    |Qrhs - (Q - alpha L Q)| <= threshold (1 + 1e-3) when converged (the recurrence and the true
    residual differ by rounding, about 1e-13 of |r0|, far below 1e-3 of rtol = 1e-8)."""
    want, winfo = restated[(courant, M)]
    got, info, true_res, nr = device_solve(cm, torch, courant, M)
    err = per_state_rel(got[:nr], want[:nr])
    rerr = abs(info.residual_norm - winfo.residual_norm) / winfo.residual_norm
    print("courant %g M %d: iterations %d (restatement %d, margin %.1e), converged %s, solution "
          "error %.2e, residual norm %.6e (rel diff %.2e), threshold %.6e, true residual %.6e"
          % (courant, M, info.iterations, winfo.iterations, winfo.margin(), info.converged, err,
             info.residual_norm, rerr, info.threshold, true_res))
    observe("gmres solution vs restatement", err)
    observe("gmres residual norm vs restatement", rerr)
    assert info.converged == winfo.converged
    assert abs(info.threshold - winfo.threshold) <= 1e-12 * winfo.threshold
    if winfo.margin() >= 1e-6:
        assert info.iterations == winfo.iterations
    if M == 3:
        assert info.iterations > 3                        # restarts ran
    assert err <= 10 * MEASURED["solve"]
    assert rerr <= 10 * MEASURED["residual_norm"]
    if info.converged:
        assert true_res <= info.threshold * (1 + 1e-3)


def test_determinism(cm, torch):
    """The same solve twice: identical bits in Q and in info."""
    a, ia, _, _ = device_solve(cm, torch, 4.0, 3)
    b, ib, _, _ = device_solve(cm, torch, 4.0, 3)
    assert np.array_equal(a, b)
    assert ia == ib, (ia, ib)


def test_early_exit_leaves_the_guess_untouched(cm, torch):
    """Qrhs = A Q: rtol |r0| < atol, converged after 0 iterations, Q bitwise unchanged."""
    law, grid, alpha = brick_case(cm, 1.0)
    dg, lin = device_pair(cm, law, grid)
    gm = cm.systemsolvers.GmresSolver(lin, alpha, cm.systemsolvers.GeneralizedMinimalResidual(None, M=5))
    x = torch.from_numpy(random_state(grid, 11)).to(lin.device)
    rhs = x.clone()
    lin(rhs, x, 0.0, -alpha, 1.0)
    lin.synchronize()
    x0 = x.clone()
    info = gm.solve(x, rhs)
    assert info.converged and info.iterations == 0
    assert info.threshold < 2.0 ** -52
    assert torch.equal(x, x0)
    gm.close(), lin.close(), dg.close()


@pytest.mark.parametrize("M", [5, 2])
def test_iteration_limit_warns_and_fills_info(cm, torch, M):
    """max_iters = 2 on a case that needs more: unconverged after exactly 2 iterations (one full
    cycle when M = 2), info filled, one warning."""
    law, grid, alpha = brick_case(cm, 4.0)
    dg, lin = device_pair(cm, law, grid)
    gm = cm.systemsolvers.GmresSolver(lin, alpha, cm.systemsolvers.GeneralizedMinimalResidual(
        None, M=M, rtol=RTOL))
    x = torch.from_numpy(random_state(grid, 11)).to(lin.device)
    rhs = torch.from_numpy(random_state(grid, 12)).to(lin.device)
    with pytest.warns(RuntimeWarning, match="did not attain convergence after 2 iterations"):
        info = gm.solve(x, rhs, max_iters=2)
    assert not info.converged and info.iterations == 2
    assert info.threshold > 0 and info.residual_norm >= info.threshold
    assert np.isfinite(x.cpu().numpy()).all()
    with warnings.catch_warnings():
        warnings.simplefilter("error")                     # warns once
        gm.solve(x, rhs, max_iters=2)
    gm.close(), lin.close(), dg.close()


@pytest.mark.parametrize("rhs_kind", ["state", "random"])
def test_against_the_column_lu(cm, torch, rhs_kind):
    """Small Held-Suarez sphere, vertical acoustic-gravity model, alpha at vertical acoustic Courant
    2: GeneralizedMinimalResidual(M = 30, rtol = 1e-12) against cmdg_columnlu_solve on the same
    right-hand side (a model state, and white noise), the right-hand side as the initial guess.  The
    difference scales with the operator's condition number at that Courant number: the bound is
    100 x the measured value (gmres_cases.MEASURED), and no more than 1e-8.  GMRES(30) needs 1 110
    and 750 iterations here (0.1 s): the columns are solved as one global system in an unscaled norm."""
    from helpers import held_suarez_setup
    law, grid, _, _ = held_suarez_setup(n_horz=2, n_vert=3)
    dg = cm.dgmodel.DGModel(law, grid, direction=EVERY, diffusion_direction=HORIZONTAL)
    lin = cm.dgmodel.DGModel(cm.atmos.AtmosAcousticGravityLinearModel(law), grid, direction=VERTICAL,
                             state_auxiliary=dg.state_auxiliary)
    dt = 2.0 * cm.mesh.grids.min_node_distance(grid, VERTICAL) / soundspeed(law.ps, 290.0)
    alpha = dt * A_II
    if rhs_kind == "state":
        from imex_cases import STATE_SCALE, wall_perturbation
        aux = dg.state_auxiliary.cpu().numpy()
        rhs = dg.init_ode_state(0.0) + torch.from_numpy(
            1e-2 * wall_perturbation(law, aux, normal=True) * STATE_SCALE[None, :, None]).to(lin.device)
    else:
        rhs = torch.from_numpy(random_state(grid, 21)).to(lin.device)
    lu = cm.systemsolvers.ColumnLU(lin, alpha)
    want = lin.create_state()
    lu.solve(want, rhs)
    gm = cm.systemsolvers.GmresSolver(lin, alpha, cm.systemsolvers.GeneralizedMinimalResidual(
        None, M=30, rtol=1e-12))
    x = rhs.clone()
    t0 = time.time()
    info = gm.solve(x, rhs)
    wall = time.time() - t0
    nr = grid.nreal
    err = per_state_rel(x.cpu().numpy()[:nr], want.cpu().numpy()[:nr])
    print("GMRES vs column LU (%s rhs): %d iterations in %.2f s, converged %s, residual %.3e, threshold %.3e, "
          "per-state relative Linf %.3e" % (rhs_kind, info.iterations, wall, info.converged, info.residual_norm,
                                            info.threshold, err))
    observe("gmres vs column LU solve", err)
    assert info.converged
    assert err <= min(100 * MEASURED["lu_solve"][rhs_kind], 1e-8)
    gm.close(), lu.close(), lin.close(), dg.close()


@pytest.mark.parametrize("nf", [0, 1])
def test_acoustic_law_matches_the_oracle_twin(cm, torch, oracle, nf):
    """The no-orientation acoustic tendency on the 2 x 2 x 1 brick against the oracle twin (flat,
    grav = 0), per state, Rusanov and central, every direction: the same terms in the same order.
    Measured: bit-identical (the bound of tests/test_gpu_imex*.py would be 1e-12)."""
    law = vortex_law(cm)
    grid, _ = small_brick(cm)
    q = random_state(grid, 31)
    T0 = random_state(grid, 32)
    nr = grid.nreal
    worst = 0.0
    for direction in (EVERY, HORIZONTAL, VERTICAL):
        dg, lin = device_pair(cm, law, grid, nf=nf, direction=direction)
        olin = oracle_acoustic(cm, oracle, grid, nf=nf, direction=direction)
        for alpha, beta in ((1.0, 0.0), (-0.25, 1.0)):
            T = torch.from_numpy(T0.copy()).to(lin.device)
            lin(T, torch.from_numpy(q).to(lin.device), 0.0, alpha, beta)
            lin.synchronize()
            To = T0.copy()
            olin(To, q, 0.0, alpha, beta)
            errs = per_state_errors(T.cpu().numpy()[:nr], To[:nr])
            worst = max(worst, max(errs))
        lin.close(), dg.close()
    print("acoustic law vs oracle twin, nf %d: worst per-state error %.2e" % (nf, worst))
    assert worst == 0.0


def test_full_law_ignores_the_vortex_reference_state(cm, torch):
    """The full dry law with IsentropicVortexReferenceState equals the one with ref_state = None,
    bit for bit: only a HydrostaticState is subtracted."""
    grid, _ = small_brick(cm)
    outs = []
    for ref in (True, False):
        law = vortex_law(cm, ref=ref)
        dg = cm.dgmodel.DGModel(law, grid, direction=EVERY)
        Q = dg.init_ode_state(0.0) + torch.from_numpy(1e-3 * random_state(grid, 41)).to(dg.device)
        T = dg.create_state()
        dg(T, Q, 0.0)
        s = cm.odesolvers.LSRK54CarpenterKennedy(dg, Q, dt=1e-6)
        s.dostep(Q, nsteps=2)
        dg.synchronize()
        outs.append((T.cpu().numpy()[:grid.nreal].copy(), Q.cpu().numpy()[:grid.nreal].copy()))
        dg.close()
    assert np.isfinite(outs[0][0]).all() and np.abs(outs[0][0]).max() > 0
    assert np.array_equal(outs[0][0], outs[1][0])
    assert np.array_equal(outs[0][1], outs[1][1])


def _create(lin, M, rtol, atol=2.0 ** -52):
    h = C.c_void_p()
    lin._torch_ready()
    return lin.L.cmdg_gmres_create(lin.handle, M, rtol, atol, C.byref(h)), h


def test_refusals(cm, torch):
    law, grid, alpha = brick_case(cm, 1.0)
    dg, lin = device_pair(cm, law, grid)
    for M, rtol, what in ((0, 1e-8, "M must be 1 to 64"), (cm._lib.GMRES_MAX_M + 1, 1e-8, "M must be 1 to 64"),
                          (5, -1.0, "rtol and atol must be >= 0"), (5, float("nan"), "rtol and atol must be >= 0")):
        r, h = _create(lin, M, rtol)
        assert r == -1 and not h.value
        with pytest.raises(cm._lib.CmdgError, match=what):
            cm._lib.check(r, lin.handle)
    # a basis larger than free memory, through the size check cmdg_gmres_create makes
    gm = cm.systemsolvers.GmresSolver(lin, alpha, cm.systemsolvers.GeneralizedMinimalResidual(None, M=4))
    state_bytes = grid.nelem * 5 * grid.Np * 8
    M = cm._lib.GMRES_MAX_M
    assert gm.fits(M, 1 << 40) == (M + 1) * state_bytes
    assert gm.fits(M, (M + 1) * state_bytes + (64 << 20)) == (M + 1) * state_bytes
    with pytest.raises(cm._lib.CmdgError, match=r"Krylov basis needs .* GB \(M \+ 1 = 65 state arrays"):
        gm.fits(M, (M + 1) * state_bytes + (64 << 20) - 1)
    # a solve whose alpha was never set
    with pytest.raises(cm._lib.CmdgError, match="alpha is NaN"):
        gm.solve(lin.create_state(), lin.create_state(), alpha=float("nan"))
    gm.close()
    # the moist model
    with pytest.raises(ValueError, match="moist"):
        cm.atmos.AtmosAcousticLinearModel(
            type("Moist", (), {"physics_id": cm.balancelaws.PHYSICS_MOIST_ATMOS, "ps": law.ps})())
    # preconditioner_update_freq > 0
    with pytest.raises(ValueError, match="preconditioner_update_freq"):
        cm.odesolvers.LinearBackwardEulerSolver(cm.systemsolvers.GeneralizedMinimalResidual(None),
                                                preconditioner_update_freq=2)
    lin.close(), dg.close()


def test_a_handle_with_neighbours_is_refused(cm, torch):
    """The single-GPU multi-rank set-up of tests/test_gpu_halo_direct.py: rank 0 of 2."""
    from helpers import pseudo1d_setup
    law, grid, _ = pseudo1d_setup(direction=0, rank=0, size=2)
    dg = cm.dgmodel.DGModel(law, grid, direction=0)
    r, h = _create(dg, 5, 1e-8)
    assert r == -5 and not h.value
    with pytest.raises(cm._lib.CmdgError, match="halo neighbours .* follow-up"):
        cm._lib.check(r, dg.handle)
    dg.close()
