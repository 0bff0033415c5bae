"""IMEX stepping of an ESDGModel on the device against the NumPy restatement
(tests/esdg_linear_restatement.py): the linear law DryAtmosAcousticGravityLinearModel through the DG
pass kernels (csrc/physics_esdg_dryatmos_linear.h), the column LU on it, cmdg_ark_step with an ESDG
handle as the full operator, the Courant numbers of the ESDG law, and what the create path refuses.
Grids: esdg_imex_cases.sphere (the baroclinic-wave model, 2 x 2 per panel x 4 levels) and
esdg_imex_cases.brick (2 x 2 x 4, flat, walls at the bottom and the top).  Errors are per state, each
against its own max-norm."""
import ctypes as C

import numpy as np
import pytest

from cmdg_loader import cm
import esdg_linear_restatement as LR
import esdg_restatement as R
from esdg_imex_cases import CASES, per_state_max_rel, random_state, reference_dt, sphere

pytestmark = pytest.mark.gpu
E = cm.esdg
ode = cm.odesolvers
EVERY, HORIZONTAL, VERTICAL = 0, 1, 2
ALPHA_BETA = ((1.0, 0.0), (1.0, 1.0), (0.5, 2.0))
INVALID, UNSUPPORTED = -1, -5


def device_full(law, grid):
    return cm.dgmodel.ESDGModel(law, grid, volume_numerical_flux_first_order=E.KGVolumeFlux(),
                                surface_numerical_flux_first_order=E.RusanovNumericalFlux())


def device_linear(law, grid, full, direction=VERTICAL, nf=0):
    return cm.dgmodel.DGModel(E.DryAtmosAcousticGravityLinearModel(law), grid, numerical_flux_first_order=nf,
                              direction=direction, state_auxiliary=full.state_auxiliary)


def restated_pair(law, grid, aux, direction=VERTICAL, nf=LR.RUSANOV, dtype=np.float64):
    ps = law.param_set
    lin = LR.DGRestatement(LR.LinearLaw(ps.cp_d, ps.cv_d, dtype), grid, aux, direction, nf, dtype)
    full = R.ESDGRestatement(law, grid, R.KG, R.RUSANOV, state_auxiliary=aux, dtype=dtype)
    return full, lin


@pytest.mark.parametrize("case", ["sphere", "brick"])
@pytest.mark.parametrize("N", [3, 4])
def test_linear_tendency_matches_restatement(torch, case, N):
    """Vertical, horizontal and every-direction operators, Rusanov and central fluxes, three (alpha, beta)
    pairs, on node-wise random fields (jumps at every face, momentum into the walls): <= 1e-12 per state."""
    law, grid = CASES[case](N)
    full = device_full(law, grid)
    aux = full.state_auxiliary.cpu().numpy().copy()
    d, T0 = random_state(grid, 1), random_state(grid, 9)
    nr, dev = grid.nreal, full.device
    worst = 0.0
    for direction in (VERTICAL, HORIZONTAL, EVERY):
        for nf in (0, 1):
            lin = device_linear(law, grid, full, direction, nf)
            _, rlin = restated_pair(law, grid, aux, direction, nf)
            for alpha, beta in ALPHA_BETA:
                T = torch.from_numpy(T0.copy()).to(dev)
                lin(T, torch.from_numpy(d).to(dev), 0.0, alpha, beta)
                Tr = T0.copy()
                rlin(Tr, d, 0.0, alpha, beta)
                err = per_state_max_rel(T.cpu().numpy()[:nr], Tr[:nr])
                worst = max(worst, err.max())
                assert np.all(err <= 1e-12), (direction, nf, alpha, beta, err)
            lin.close()
    print("%s N=%d: worst per-state error %.2e" % (case, N, worst))
    full.close()


@pytest.mark.parametrize("case", ["sphere", "brick"])
@pytest.mark.parametrize("N", [3, 4])
def test_band_solve_matches_restatement(torch, case, N):
    """``(I - alpha L)^-1 b`` by the device column LU (four levels: two probed elements of a stack in one
    probing pass, an element with neighbours on both sides) against the restatement's dense solve of the
    matrix it probed from the restated operator: <= 1e-12 of the solution's max-norm, per state."""
    law, grid = CASES[case](N)
    full = device_full(law, grid)
    lin = device_linear(law, grid, full)
    aux = full.state_auxiliary.cpu().numpy().copy()
    _, rlin = restated_pair(law, grid, aux)
    alpha = reference_dt(grid, law.param_set) * float(LR.ark2gkc_tableau()[1][1, 1])
    lu = cm.systemsolvers.ColumnLU(lin, alpha)
    assert (lu.n, lu.p) == (5 * (N + 1) * 4, 5 * (N + 1) - 1)
    b = random_state(grid, 3)
    x = lin.create_state()
    lu.solve(x, torch.from_numpy(b).to(lin.device))
    lin.synchronize()
    want = LR.ColumnSolver(rlin, grid.topology.stacksize, alpha).solve(np.zeros_like(b), b)
    err = per_state_max_rel(x.cpu().numpy()[:grid.nreal], want[:grid.nreal])
    print("%s N=%d band solve: per-state error %s" % (case, N, err))
    assert np.all(err <= 1e-12), err
    lu.close()
    lin.close()
    full.close()


def device_steps(torch, law, grid, Q0, dt, nsteps, split, adjustable=False):
    full = device_full(law, grid)
    lin = device_linear(law, grid, full)
    Q = torch.from_numpy(Q0.copy()).to(full.device)
    solver = ode.ARK2GiraldoKellyConstantinescu(
        full, lin, ode.LinearBackwardEulerSolver(ode.ManyColumnLU(), isadjustable=adjustable), Q, dt=dt, t0=0.0,
        split_explicit_implicit=split)
    ode.solve(Q, solver, numberofsteps=nsteps, adjustfinalstep=False)
    out = Q.cpu().numpy().copy()
    norm_ratio = full.norm(Q) / full.norm(torch.from_numpy(Q0.copy()).to(full.device))
    solver.close()
    lin.close()
    full.close()
    return out, norm_ratio


def restated_steps(law, grid, aux, Q0, dt, nsteps, split, dtype=np.float64):
    full, lin = restated_pair(law, grid, aux, dtype=dtype)
    tab = LR.ark2gkc_tableau(dtype)
    solver = LR.ColumnSolver(lin, grid.topology.stacksize, dtype(dt) * tab[1][1, 1])
    Q = Q0.astype(dtype)
    for n in range(nsteps):
        LR.ark_step(full, lin, solver, Q, n * dt, dt, tab, split)
    return Q


@pytest.mark.parametrize("case", ["sphere", "brick"])
@pytest.mark.parametrize("split", [False, True])
def test_one_ark2_step(torch, case, split):
    """One ARK2GiraldoKellyConstantinescu step, the ESDGModel (KG + Rusanov) as the full operator, the
    vertical linear model solved by the column LU, ``dt = 3 dx / soundspeed_air(330 K)``: the increment
    per state <= 1e-10 of its max-norm, with ``split_explicit_implicit`` false and true."""
    law, grid = CASES[case](3)
    aux = law.init_state_auxiliary(grid)
    Q0 = law.init_state_prognostic(grid, aux)
    dt = reference_dt(grid, law.param_set)
    got, _ = device_steps(torch, law, grid, Q0, dt, 1, split)
    want = restated_steps(law, grid, aux, Q0, dt, 1, split)
    nr = grid.nreal
    err = per_state_max_rel(got[:nr] - Q0[:nr], want[:nr] - Q0[:nr])
    print("%s split=%s dt=%.3f: increment error per state %s" % (case, split, dt, err))
    assert np.all(err <= 1e-10), err


def test_ten_ark2_steps(torch):
    """Ten steps on the sphere.  The bound per state is max(1e-10, 4 x the restatement's own
    float64-versus-longdouble difference on the same ten steps), the rule of
    test_gpu_esdg.py::test_one_evaluation_grid_c.  The restatement's own difference measures 1.3e-15
    (rho, rho e) to 6.4e-14 (rho u), so the bound is 1e-10 for every state; the device's difference from
    the float64 restatement measured 0 on the MI355X."""
    law, grid = sphere(3)
    aux = law.init_state_auxiliary(grid)
    Q0 = law.init_state_prognostic(grid, aux)
    dt = reference_dt(grid, law.param_set)
    nr = grid.nreal
    got, _ = device_steps(torch, law, grid, Q0, dt, 10, False)
    want = restated_steps(law, grid, aux, Q0, dt, 10, False)
    wantl = restated_steps(law, grid, aux, Q0, dt, 10, False, dtype=np.longdouble)
    own = per_state_max_rel(want[:nr], wantl[:nr])
    bound = np.maximum(1e-10, 4 * own)
    err = per_state_max_rel(got[:nr], want[:nr])
    print("ten steps: restatement float64 vs longdouble %s -> bound %s; device error %s" % (own, bound, err))
    assert np.isfinite(got).all()
    assert np.all(err <= bound), (err, bound)


def test_not_adjustable_solver(torch):
    """``LinearBackwardEulerSolver(ManyColumnLU(); isadjustable = false)``: a step of another size is
    refused, and two fresh runs of two steps are bit-identical (the full handle's and the linear
    handle's streams are ordered by events)."""
    law, grid = sphere(3)
    aux = law.init_state_auxiliary(grid)
    Q0 = law.init_state_prognostic(grid, aux)
    dt = reference_dt(grid, law.param_set)
    a, _ = device_steps(torch, law, grid, Q0, dt, 2, False)
    b, _ = device_steps(torch, law, grid, Q0, dt, 2, False)
    assert np.array_equal(a[:grid.nreal], b[:grid.nreal])
    full = device_full(law, grid)
    lin = device_linear(law, grid, full)
    Q = torch.from_numpy(Q0.copy()).to(full.device)
    solver = ode.ARK2GiraldoKellyConstantinescu(
        full, lin, ode.LinearBackwardEulerSolver(ode.ManyColumnLU(), isadjustable=False), Q, dt=dt, t0=0.0,
        split_explicit_implicit=False)
    with pytest.raises(ValueError, match="isadjustable = false"):
        solver.dostep(Q, 1, dt=dt / 2)
    with pytest.raises(ValueError, match="isadjustable = false"):
        solver.updatedt(dt / 2)
    solver.dostep(Q, 1)
    full.synchronize()
    assert np.isfinite(Q.cpu().numpy()).all()
    solver.close()
    lin.close()
    full.close()


@pytest.mark.parametrize("case", ["sphere", "brick"])
def test_courant_numbers(torch, case):
    """``advective_courant`` and ``nondiffusive_courant`` of DryAtmos.jl:758-793 through ``ESDGModel.courant``,
    in the three directions, against a NumPy evaluation over the same nodes.  Both sides take the same
    products, quotients and square roots in the same order, each correctly rounded and none contracted,
    so the maxima are exactly equal (they were on the MI355X, all twelve); that is what is asserted.
    The diffusive kind is refused: the law has none."""
    law, grid = CASES[case](3)
    full = device_full(law, grid)
    aux = full.state_auxiliary.cpu().numpy().copy()
    Q = full.init_ode_state(0.0)
    Qh = Q.cpu().numpy()
    ps = law.param_set
    dt = reference_dt(grid, ps)
    for direction in (EVERY, HORIZONTAL, VERTICAL):
        for kind in (cm.dgmodel.ADVECTIVE_COURANT, cm.dgmodel.NONDIFFUSIVE_COURANT):
            got = full.courant(kind, Q, dt, 0.0, direction)
            want = LR.courant(kind, grid, Qh, aux, dt, direction, ps.cp_d, ps.cv_d, ps.grav)
            print("%s courant kind %d direction %d: device %.17g host %.17g rel %.1e"
                  % (case, kind, direction, got, want, abs(got - want) / want))
            assert want > 0 and got == want, (kind, direction, got, want)
    with pytest.raises(cm._lib.CmdgError, match="advective and the nondiffusive"):
        full.courant(cm.dgmodel.DIFFUSIVE_COURANT, Q, dt, 0.0, EVERY)
    full.close()


def _desc(physics_id, N, iparam):
    d = cm._lib.CmdgDesc()
    d.dim = 3
    d.N[0], d.N[1], d.N[2] = N
    d.physics_id = physics_id
    for i, v in enumerate(iparam):
        d.iparam[i] = v
    return d


def _create_refused(d):
    L = cm._lib.lib()
    h = C.c_void_p(0xdead)
    rc = L.cmdg_create(C.byref(d), C.byref(h))
    assert h.value is None
    return rc, L.cmdg_last_error(None).decode()


def test_refusals(torch):
    law, grid = sphere(3, nvert=2)
    lin_id = E.PHYSICS_ESDG_DRY_ATMOS_LINEAR_AG
    # the linear law through cmdg_create_esdg
    aux = law.init_state_auxiliary(grid)
    with pytest.raises(cm._lib.CmdgError, match="two-point fluxes are defined for CMDG_PHYSICS_ESDG_DRY_ATMOS only"):
        cm.dgmodel.ESDGModel(E.DryAtmosAcousticGravityLinearModel(law), grid, state_auxiliary=aux)
    # without a reference state: the host class and the library
    bare = E.DryAtmosModel(E.SphericalOrientation(), E.BaroclinicWave())
    with pytest.raises(ValueError, match="needs a model with a reference state"):
        E.DryAtmosAcousticGravityLinearModel(bare)
    rc, err = _create_refused(_desc(lin_id, (3, 3, 3), (1, 0)))
    assert rc == UNSUPPORTED and err.startswith("DryAtmosAcousticGravityLinearModel needs a model with a reference state")
    # an order outside the compiled set
    rc, err = _create_refused(_desc(lin_id, (5, 5, 5), (1, 1)))
    assert rc == UNSUPPORTED
    assert err.startswith("DryAtmosAcousticGravityLinearModel: polynomial order not compiled in (have N = 3, 4)")
    # the column LU on an ESDG handle
    full = device_full(law, grid)
    with pytest.raises(cm._lib.CmdgError, match="not available on an ESDGModel handle"):
        cm.systemsolvers.ColumnLU(full, 10.0)
    full.close()


def test_baroclinic_wave_stays_bounded(torch):
    """``BaroclinicWave()`` on a 2 x 2 per panel x 2 level sphere, twenty IMEX steps at cfl = 3:
    ``norm(Q) / norm(Q0)`` on the restatement and on the device.

    Measured on the restatement first: the ratio is 1 + 1.03e-2 after the twenty steps (683 s), growing
    by about 5e-4 a step from the first.  That is the grid's, not the split's: the restated ESDG operator
    alone, stepped explicitly (LSRK54, dt / 16) over the same time, gives 1 + 0.99e-2 -- two cubic elements
    over 30 km do not hold the analytic state in discrete balance.  So the 1e-6 first proposed cannot
    hold at this size; the bound is 2e-2, twice the restatement's measured drift, which a blow-up of the
    split (norms growing by factors) still fails at once, and the device must reproduce the restatement's
    ratio to 1e-10."""
    law, grid = sphere(3, nvert=2, problem=E.BaroclinicWave())
    aux = law.init_state_auxiliary(grid)
    Q0 = law.init_state_prognostic(grid, aux)
    dt = reference_dt(grid, law.param_set)
    got, ratio = device_steps(torch, law, grid, Q0, dt, 20, False)
    want = restated_steps(law, grid, aux, Q0, dt, 20, False)
    Mw = grid.vgeo[:grid.nreal, 9, :][:, None, :]
    norm = lambda Q: float(np.sqrt((Mw * Q[:grid.nreal] ** 2).sum()))
    rratio = norm(want) / norm(Q0)
    print("norm(Q)/norm(Q0) - 1: restatement %.4e device %.4e" % (rratio - 1, ratio - 1))
    assert abs(rratio - 1) <= 2e-2
    assert abs(ratio - 1) <= 2e-2
    assert abs(ratio - rratio) <= 1e-10
