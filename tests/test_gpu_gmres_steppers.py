"""ARK2GKC and decoupled-implicit MRI-GARK driving GMRES on the device (cmdg_ark_step_gmres,
cmdg_mrigark_step_gmres): the ARK step against the CPU restatement chain (oracle.ark_step on the
oracle operators with tests/gmres_restatement.py as its solver), the reference's isentropic-vortex
errors (isentropicvortex_imex.jl, isentropicvortex_mrigark_implicit.jl, dims = 2 as the z-invariant
slice of a one-element-deep extrusion), and ARK2GKC with GMRES against ARK2GKC with the column LU.
The CPU reference of the no-orientation linear law is the oracle's acoustic-gravity law on a flat,
grav = 0 twin model (tests/gmres_cases.py)."""
import ctypes as C
import time

import numpy as np
import pytest

from gmres_cases import (EVERY, GOLD, HORIZONTAL, MEASURED, VERTICAL, device_pair, oracle_acoustic, small_brick, soundspeed,
                         vortex_law, vortex_setup)
from gmres_restatement import GMRES, LinBESolver
from helpers import observe
from imex_cases import per_state_errors

pytestmark = pytest.mark.gpu


def gmres_be(cm, M, rtol, isadjustable=True):
    ode = cm.odesolvers
    return ode.LinearBackwardEulerSolver(ode.GeneralizedMinimalResidual(None, M=M, rtol=rtol),
                                         isadjustable=isadjustable)


@pytest.mark.parametrize("split", [False, True])
def test_ark_step_matches_the_restatement_chain(cm, torch, oracle, split):
    """Three ARK2GKC steps (paperversion) at acoustic Courant 1 on the 2 x 2 x 1 periodic brick,
    GeneralizedMinimalResidual(M = 10, rtol = 1e-10): the increment per state against
    oracle.ark_step with the NumPy GMRES on the oracle operators.  Qtt starts from Qhat on both
    sides (stage_update!, AdditiveRungeKuttaMethod.jl:603): the iteration counts agree."""
    law = vortex_law(cm)
    grid, _ = small_brick(cm)
    dt = cm.mesh.grids.min_node_distance(grid) / soundspeed(law.ps, law.init_state.T_inf)
    ode = cm.odesolvers
    dg, lin = device_pair(cm, law, grid)
    Q = dg.init_ode_state(0.0)
    Q0 = Q.cpu().numpy().copy()
    solver = ode.ARK2GiraldoKellyConstantinescu(dg, lin, gmres_be(cm, 10, 1e-10), Q, dt=dt,
                                                split_explicit_implicit=split, paperversion=True)
    its = []
    for _ in range(3):
        solver.dostep(Q, 1)
        its += [i.iterations for i in solver.solve_info]
        assert len(solver.solve_info) == 2 and all(i.converged for i in solver.solve_info)
    dg.synchronize()
    got = Q.cpu().numpy().copy()
    solver.close(), lin.close(), dg.close()

    full = oracle.OracleDGModel(vortex_law(cm, ref=False), grid, nf_first=0, direction=EVERY)
    olin = oracle_acoustic(cm, oracle, grid)
    tableau = ode.ark2gkc_tableau(paperversion=True)
    Qo = Q0.copy()
    nr = grid.nreal
    be = LinBESolver(olin, GMRES(Qo, M=10, rtol=1e-10, rv=slice(0, nr)), dt * tableau[1][1][1])
    t = 0.0
    for _ in range(3):
        oracle.ark_step(full, olin, be, Qo, t, dt, tableau, split)
        t += dt
    errs = per_state_errors(got[:nr] - Q0[:nr], Qo[:nr] - Q0[:nr])
    margin = min(i.margin() for i in be.infos)
    print("split=%s: increment error per state %s; iterations %s (restatement %s, margin %.1e)"
          % (split, ["%.2e" % e for e in errs], its, [i.iterations for i in be.infos], margin))
    observe("ark gmres increment vs restatement (split=%s)" % split, max(errs))
    if margin >= 1e-6:
        assert its == [i.iterations for i in be.infos]
    assert max(errs) <= 10 * MEASURED["ark"]


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("level", [1, 2])
def test_imex_vortex_goldens(cm, torch, level, split):
    """isentropicvortex_imex.jl levels 1 and 2 (186 steps on 25 elements, 371 on 100; solve! adds a
    last step of rounding size when the running sum of the time falls short of timeend, as the
    reference does): ARK2GKC, paperversion, GeneralizedMinimalResidual(M = 10, rtol = 1e-10), at the
    reference's own rtol."""
    law, grid, dt, nsteps, timeend, scale = vortex_setup(cm, level=level)
    assert nsteps == (186, 371)[level - 1]
    ode = cm.odesolvers
    dg, lin = device_pair(cm, law, grid)
    Q = dg.init_ode_state(0.0)
    solver = ode.ARK2GiraldoKellyConstantinescu(dg, lin, gmres_be(cm, 10, 1e-10), Q, dt=dt, t0=0.0,
                                                split_explicit_implicit=split, paperversion=True)
    t0 = time.time()
    tend = ode.solve(Q, solver, timeend=timeend)
    wall = time.time() - t0
    assert tend == timeend and solver.steps in (nsteps, nsteps + 1)
    err = dg.euclidean_distance(Q, dg.init_ode_state(timeend)) / scale
    exp = GOLD["isentropicvortex_imex"]["split_true" if split else "split_false"][level - 1]
    print("level %d split=%s: error %.16e, golden %.16e, rel %.2e, %d steps in %.2f s"
          % (level, split, err, exp, abs(err - exp) / exp, solver.steps, wall))
    observe("imex vortex golden (gmres)", abs(err - exp) / exp)
    assert abs(err - exp) <= GOLD["rtol"] * exp, (err, exp)
    solver.close(), lin.close(), dg.close()


@pytest.mark.parametrize("name", ["MRIGARKIRK21aSandu", "MRIGARKESDIRK34aSandu"])
def test_mrigark_implicit_vortex_goldens(cm, torch, name):
    """isentropicvortex_mrigark_implicit.jl level 1: 926 slow steps, the acoustic linear model
    solved by GeneralizedMinimalResidual(M = 50, rtol = 1e-10), LSRK54 on the remainder with the
    fast dt = dt, at the reference's own rtol."""
    law, grid, dt, nsteps, timeend, scale = vortex_setup(cm, level=1, mri=True)
    assert nsteps == 926
    ode = cm.odesolvers
    dg, slow = device_pair(cm, law, grid)
    fast = cm.dgmodel.remainder_DGModel(dg, (slow,))
    Q = dg.init_ode_state(0.0)
    solver = getattr(ode, name)(slow, gmres_be(cm, 50, 1e-10), ode.LSRK54CarpenterKennedy(fast, Q, dt=dt), Q,
                                dt=dt, t0=0.0)
    t0 = time.time()
    tend = ode.solve(Q, solver, timeend=timeend)
    wall = time.time() - t0
    assert tend == timeend and solver.steps in (nsteps, nsteps + 1)
    assert solver.solve_info and all(i.converged for i in solver.solve_info)
    err = dg.euclidean_distance(Q, dg.init_ode_state(timeend)) / scale
    exp = GOLD["isentropicvortex_mrigark_implicit"][name][0]
    print("%s: error %.16e, golden %.16e, rel %.2e, %d steps in %.2f s, last step's iterations %s"
          % (name, err, exp, abs(err - exp) / exp, solver.steps, wall,
             [i.iterations for i in solver.solve_info]))
    observe("mrigark implicit vortex golden (gmres)", abs(err - exp) / exp)
    assert abs(err - exp) <= GOLD["rtol"] * exp, (err, exp)
    solver.close(), slow.close(), dg.close()


def sphere_ark(cm, torch, be, nsteps, split, dt, Q0):
    from helpers import held_suarez_setup
    law, grid, _, _ = held_suarez_setup(n_horz=2, n_vert=3)
    dg = cm.dgmodel.DGModel(law, grid, direction=EVERY, diffusion_direction=HORIZONTAL)
    lin = cm.dgmodel.DGModel(cm.atmos.AtmosAcousticGravityLinearModel(law), grid, direction=VERTICAL,
                             state_auxiliary=dg.state_auxiliary)
    Q = dg.init_ode_state(0.0) if Q0 is None else torch.from_numpy(Q0.copy()).to(dg.device)
    start = Q.cpu().numpy().copy()
    if dt is None:
        dt = 2.0 * cm.mesh.grids.min_node_distance(grid, VERTICAL) / soundspeed(law.ps, 290.0)
    solver = cm.odesolvers.ARK2GiraldoKellyConstantinescu(dg, lin, be, Q, dt=dt, split_explicit_implicit=split)
    out, its = [], []
    for _ in range(nsteps):
        solver.dostep(Q, 1)
        dg.synchronize()
        out.append(Q.cpu().numpy()[:grid.nreal].copy())
        its += [i.iterations for i in getattr(solver, "solve_info", [])]
    solver.close(), lin.close(), dg.close()
    return out, start, dt, its


@pytest.mark.parametrize("split", [False, True])
def test_ark_gmres_against_ark_column_lu(cm, torch, split):
    """Small Held-Suarez sphere, vertical acoustic-gravity model, dt at vertical acoustic Courant 2:
    ARK2GKC with GeneralizedMinimalResidual(M = 30, rtol = 1e-12) against ARK2GKC with
    ManyColumnLU after 1 and 3 steps, the increment per state."""
    ode = cm.odesolvers
    want, Q0, dt, _ = sphere_ark(cm, torch, ode.LinearBackwardEulerSolver(ode.ManyColumnLU()), 3, split, None, None)
    got, _, _, its = sphere_ark(cm, torch, gmres_be(cm, 30, 1e-12), 3, split, dt, Q0)
    nr = want[0].shape[0]
    for n in (0, 2):
        errs = per_state_errors(got[n] - Q0[:nr], want[n] - Q0[:nr])
        print("split=%s, %d steps: increment error per state %s, iterations %s"
              % (split, n + 1, ["%.2e" % e for e in errs], its[:2 * (n + 1)]))
        observe("ark gmres vs ark column LU", max(errs))
        assert max(errs) <= min(100 * MEASURED["lu_ark"], 1e-8)


def test_non_adjustable_solver_refuses_another_alpha(cm, torch):
    """isadjustable = False: a dt that needs another alpha is refused, as for the column LU
    (@assert lin.isadjustable), by the ARK and the MRI-GARK stepper; the same dt runs."""
    law = vortex_law(cm)
    grid, _ = small_brick(cm)
    ode = cm.odesolvers
    dg, lin = device_pair(cm, law, grid)
    Q = dg.init_ode_state(0.0)
    dt = cm.mesh.grids.min_node_distance(grid) / soundspeed(law.ps, law.init_state.T_inf)
    ark = ode.ARK2GiraldoKellyConstantinescu(dg, lin, gmres_be(cm, 10, 1e-8, isadjustable=False), Q, dt=dt)
    ark.dostep(Q, 1)
    with pytest.raises(ValueError, match="isadjustable"):
        ark.updatedt(dt / 2)
    with pytest.raises(ValueError, match="isadjustable"):
        ark.dostep(Q, 1, dt=dt / 2)
    ark.close()
    rem = cm.dgmodel.remainder_DGModel(dg, (lin,))
    mri = ode.MRIGARKIRK21aSandu(lin, gmres_be(cm, 10, 1e-8, isadjustable=False),
                                 ode.LSRK54CarpenterKennedy(rem, Q, dt=dt), Q, dt=dt)
    mri.dostep(Q, 1)
    with pytest.raises(ValueError, match="isadjustable"):
        mri.dostep(Q, 1, dt=dt / 2)
    # ... and by the library itself
    mri._desc.fast_dt = dt
    rc = dg.L.cmdg_mrigark_step_gmres(mri._slow[0], mri._slow[1], mri._fast[0], mri._fast[1], mri.lu.handle,
                                      C.byref(mri._desc), Q.data_ptr(), C.cast(mri._work, C.c_void_p), 0.0,
                                      dt / 2)
    assert rc == -1
    with pytest.raises(cm._lib.CmdgError, match="not adjustable"):
        cm._lib.check(rc, lin.handle)
    with pytest.raises(TypeError, match="not a remainder"):
        ode.MRIGARKIRK21aSandu(rem, gmres_be(cm, 10, 1e-8), ode.LSRK54CarpenterKennedy(rem, Q, dt=dt), Q, dt=dt)
    mri.close(), lin.close(), dg.close()
