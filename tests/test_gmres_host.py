"""GMRES without a GPU: the NumPy restatement (tests/gmres_restatement.py) on dense systems, the
refusals of the Python classes, and the reference's IMEX isentropic-vortex errors of level 1
(isentropicvortex_imex.jl:49,54) from the restatement driving the oracle operators."""
import math

import numpy as np
import pytest

from cmdg_loader import cm
from gmres_cases import GOLD, oracle_acoustic, solve_schedule, vortex_law, vortex_setup
from gmres_restatement import GMRES, LinBESolver


def dense_system(n=30, seed=5):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((n, n))
    A += np.diag(np.abs(A).sum(axis=1) + 1.0)        # strictly diagonally dominant
    return A, rng.standard_normal(n), rng.standard_normal(n)


@pytest.mark.parametrize("M", [30, 5])
def test_restatement_solves_dense_systems_to_its_own_criterion(M):
    """n = 30 with M = 30 (one cycle) and M = 5 (restarts): converged, the true residual within the
    threshold rtol |r0| up to the rounding of the recurrence, the iterations counted."""
    A, b, x0 = dense_system()
    op = lambda out, q: out.__setitem__(Ellipsis, A @ q)
    g = GMRES(x0, M=M, rtol=1e-10)
    x = x0.copy()
    info = g.linearsolve(op, x, b)
    r0 = np.linalg.norm(b - A @ x0)
    assert info.converged and 0 < info.iterations <= 30 * (1 if M == 30 else 6)
    assert info.threshold == 1e-10 * r0
    assert info.residual_norm < info.threshold
    assert np.linalg.norm(b - A @ x) <= info.threshold * (1 + 1e-3)
    assert len(info.residuals) == info.iterations
    if M == 5:
        assert info.iterations > 5                      # the restart path ran


def test_restatement_returns_the_untouched_guess_when_already_converged():
    """rtol |r0| < atol: converged after 0 iterations, Q bitwise unchanged."""
    A, _, x0 = dense_system()
    op = lambda out, q: out.__setitem__(Ellipsis, A @ q)
    b = A @ x0 + 1e-9
    g = GMRES(x0, M=5, rtol=1e-10, atol=1e-12)
    x = x0.copy()
    info = g.linearsolve(op, x, b)
    assert info.converged and info.iterations == 0 and np.array_equal(x, x0)


def test_restatement_stops_at_max_iters():
    A, b, x0 = dense_system()
    op = lambda out, q: out.__setitem__(Ellipsis, A @ q)
    x = x0.copy()
    info = GMRES(x0, M=5, rtol=1e-12).linearsolve(op, x, b, max_iters=2)
    assert not info.converged and info.iterations == 2
    x = x0.copy()
    info = GMRES(x0, M=2, rtol=1e-12).linearsolve(op, x, b, max_iters=2)
    assert not info.converged and info.iterations == 2


def test_python_argument_refusals():
    ode, ss = cm.odesolvers, cm.systemsolvers
    g = ss.GeneralizedMinimalResidual(None)
    assert (g.M, g.rtol, g.atol) == (20, math.sqrt(2.0 ** -52), 2.0 ** -52)
    for bad in ({"M": 0}, {"M": cm._lib.GMRES_MAX_M + 1}, {"rtol": -1.0}, {"rtol": float("nan")},
                {"atol": -1e-3}):
        with pytest.raises(ValueError, match="M must be|rtol and atol"):
            ss.GeneralizedMinimalResidual(None, **bad)
    assert cm._lib.GMRES_MAX_M >= 50
    be = ode.LinearBackwardEulerSolver(g, isadjustable=False)
    assert be.solver is g and not be.isadjustable
    with pytest.raises(TypeError):
        ode.LinearBackwardEulerSolver(object())
    with pytest.raises(ValueError, match="preconditioner_update_freq"):
        ode.LinearBackwardEulerSolver(g, preconditioner_update_freq=1)
    assert "#define CMDG_GMRES_MAX_M %d" % cm._lib.GMRES_MAX_M in open(
        cm._lib.LIB_PATH.replace("libcmdg.so", "../include/cmdg.h")).read()


def test_acoustic_linear_model_refusals_and_layout():
    A = cm.atmos
    law = vortex_law(cm)
    assert (law.off_ref, law.naux, law.subtract_off) == (3, 12, False)
    lin = A.AtmosAcousticLinearModel(law)
    assert lin.physics_id == 13 == cm.balancelaws.PHYSICS_ATMOS_LINEAR_ACOUSTIC
    assert (lin.ns, lin.naux, lin.off_ref) == (5, 12, 3)
    with pytest.raises(ValueError, match="reference state"):
        A.AtmosAcousticLinearModel(vortex_law(cm, ref=False))
    with pytest.raises(ValueError, match="ORIENT_NONE"):
        A.AtmosAcousticLinearModel(vortex_law(cm, twin=True))
    moist = type("Moist", (), {"physics_id": cm.balancelaws.PHYSICS_MOIST_ATMOS, "ps": law.ps})()
    with pytest.raises(ValueError, match="moist"):
        A.AtmosAcousticLinearModel(moist)
    with pytest.raises(ValueError, match="needs an orientation"):
        A.DryAtmosModel(law.init_state, orientation=A.ORIENT_NONE,
                        ref_state=A.IsothermalProfile(law.ps, 300.0))


def test_vortex_reference_state_columns():
    """The reference-state columns of the no-orientation model and of the oracle twin hold the
    reference's constants (isentropicvortex_setup.jl:84-100)."""
    from gmres_cases import small_brick
    grid, _ = small_brick(cm)
    for twin, off in ((False, 3), (True, 7)):
        law = vortex_law(cm, twin=twin)
        s, ps = law.init_state, law.ps
        aux = law.init_state_auxiliary(grid)
        assert law.off_ref == off
        want = (s.rho_inf, s.p_inf, s.T_inf, s.rho_inf * (ps.cv_d * (s.T_inf - ps.T_0)))
        for c, w in enumerate(want):
            assert np.all(aux[:, off + c, :] == w)
        if twin:
            assert np.all(aux[:, 3:7, :] == 0.0)


@pytest.mark.parametrize("split", [False, True])
def test_imex_vortex_level1_golden_on_the_oracle(oracle, split):
    """isentropicvortex_imex.jl level 1 (5 x 5 elements, N = 4, 186 steps of ARK2GKC,
    paperversion = true, GeneralizedMinimalResidual(M = 10, rtol = 1e-10)): the restatement of GMRES
    and of the ARK step (oracle.ark_step) on the oracle's operators reproduces the reference's error
    at its own rtol.  The full law runs without a reference state (it subtracts none, so the results
    are the same); the linear operator is the acoustic-gravity law on the flat, grav = 0 twin."""
    law, grid, dt, nsteps, timeend, scale = vortex_setup(cm, level=1)
    assert nsteps == 186 and grid.nreal == 25
    full = oracle.OracleDGModel(vortex_law(cm, ref=False), grid, nf_first=0, direction=0)
    lin = oracle_acoustic(cm, oracle, grid)
    Q = full.law.init_state_prognostic(grid, full.state_auxiliary, 0.0)
    tableau = cm.odesolvers.ark2gkc_tableau(paperversion=True)
    gm = GMRES(Q, M=10, rtol=1e-10, rv=slice(0, grid.nreal))
    be = LinBESolver(lin, gm, dt * tableau[1][1][1])
    # solve! steps until the running sum of the time reaches timeend: after the 186 steps it may
    # fall short of it by rounding, and a last step of that size follows (as in the reference)
    sched = solve_schedule(0.0, dt, timeend)
    assert len(sched) in (nsteps, nsteps + 1) and sched[nsteps - 1][1] > 0.99 * dt
    assert len(sched) == nsteps or sched[-1][1] < 1e-12 * dt
    for t, step in sched:
        oracle.ark_step(full, lin, be, Q, t, step, tableau, split)
    assert all(i.converged for i in be.infos) and len(be.infos) == 2 * len(sched)
    Qe = full.law.init_state_prognostic(grid, full.state_auxiliary, timeend)
    err = math.sqrt(oracle.weighted_norm2_local(grid, Q, Qe)) / scale
    exp = GOLD["isentropicvortex_imex"]["split_true" if split else "split_false"][0]
    print("split=%s: error %.16e, golden %.16e, rel %.2e, iterations per solve %.1f"
          % (split, err, exp, abs(err - exp) / exp, np.mean([i.iterations for i in be.infos])))
    assert abs(err - exp) <= GOLD["rtol"] * exp, (err, exp)
