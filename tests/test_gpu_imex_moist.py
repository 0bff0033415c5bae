"""IMEX stepping of the moist LES law: AtmosAcousticGravityLinearModel of a MoistAtmosModel
(EquilMoist, physics id 11, six states), its column LU and the ARK2GKC step.

The oracle has no moist linear law.  It is composed from the dry oracle linear law, which is
exact up to the rounding of p_lin:  with P(x) = L_dry(x, 0, 0, 0, 0)[0] the jump penalty of the
numerical flux on a state without flux (zero with the central flux, Rusanov's c [x] / 2 otherwise),
  L_moist(Q)[0:5] = L_dry(rho, rho u, rho e - e_int_v0 rho q_tot), then [4] += e_int_v0 P(rho q_tot)
  L_moist(Q)[5] = P(rho q_tot).
rho q_tot has no flux and no source, so its tendency is the penalty alone; and the Rusanov penalty
of rho e is on the jump of rho e, not of the shifted rho e - e_int_v0 rho q_tot p_lin sees, which
the energy term corrects (with a central flux, or a state without jumps, the correction is 0)."""
import ctypes as C
import math

import numpy as np
import pytest

from helpers import observe
from imex_cases import EVERY, HORIZONTAL, VERTICAL, band_to_dense, per_state_errors, wall_perturbation

pytestmark = pytest.mark.gpu

STATES6 = ((0,), (1, 2, 3), (4,), (5,))
SCALE6 = np.array([1e-3, 1.0, 1.0, 1.0, 1e2, 1e-4])


class MoistRestSetup:
    """The reference state at rest with an unsaturated total water q0 exp(-z / 2 km)."""

    def __init__(self, q0=2e-3):
        self.q0 = q0

    def __call__(self, law, aux, coord, t):
        rho = aux[:, law.off_ref, :]
        zero = 0.0 * rho
        return rho, [zero, zero, zero], aux[:, law.off_ref + 3, :].copy(), rho * self.q0 * np.exp(-coord[2] / 2e3)


def moist_brick(cm, N=4, nx=2, ny=2, nvert=3, dx=5e3, dz=1e3, q0=2e-3, **kw):
    """nx x ny x nvert stacked brick with walls on every side, the moist law with constant
    viscosity 0, Gravity only and the BOMEX reference state."""
    M, MO, A = cm.mesh, cm.moist, cm.atmos
    ps = MO.MoistParameters()
    rng = [np.linspace(0.0, dx * nx, nx + 1), np.linspace(0.0, dx * ny, ny + 1),
           np.linspace(0.0, dz * nvert, nvert + 1)]
    topl = M.StackedBrickTopology(rng, periodicity=(False, False, False), boundary=((1, 2), (1, 2), (1, 2)))
    grid = M.DiscontinuousSpectralElementGrid(topl, N)
    ref = A.DecayingTemperatureProfile(ps, 290.0, 220.0, ps.R_d * 290.0 / ps.grav)
    law = MO.MoistAtmosModel(MoistRestSetup(q0), ref, closure=MO.CLOSURE_CONSTANT, coefficient=0.0,
                             sources=A.SRC_GRAVITY, param_set=ps, **kw)
    return law, grid


def perturbation6(law, aux, seed, normal=True, moist=True):
    out = np.zeros((aux.shape[0], 6, aux.shape[2]))
    out[:, :5] = wall_perturbation(law, aux, normal=normal, seed=seed)
    if moist:
        out[:, 5] = wall_perturbation(law, aux, normal=normal, seed=seed + 100)[:, 0]
    return out * SCALE6[None, :, None]


def device_full(cm, law, grid, direction=EVERY):
    return cm.dgmodel.DGModel(law, grid, direction=direction)


def device_linear(cm, law, grid, aux, direction=VERTICAL, nf=0):
    return cm.dgmodel.DGModel(cm.atmos.AtmosAcousticGravityLinearModel(law), grid, direction=direction,
                              numerical_flux_first_order=nf, state_auxiliary=aux)


def dry_twin_aux(law, aux19):
    """The moist law's dry twin (the DryAtmosModel its first 15 auxiliary columns come from) and
    an auxiliary array of the twin's layout holding those 15 shared columns."""
    dry = law._dry
    aux = np.zeros((aux19.shape[0], dry.naux, aux19.shape[2]))
    aux[:, :15] = aux19[:, :15]
    return dry, aux


class ComposedMoistLinear:
    """The moist linear law from the dry oracle one (module docstring)."""

    def __init__(self, O, cm, law, grid, aux19, nf=0, direction=VERTICAL):
        dry, aux = dry_twin_aux(law, aux19)
        self.lin = O.OracleDGModel(cm.atmos.AtmosAcousticGravityLinearModel(dry), grid, nf_first=nf,
                                   direction=direction, state_auxiliary=aux)
        self.grid = grid
        ps = law.ps
        self.e_int_v0 = ps.LH_v0 - ps.R_v * ps.T_0

    def __call__(self, dQ, Q, t, alpha=1.0, beta=0.0):
        Qd = np.ascontiguousarray(Q[:, :5]).copy()
        Qd[:, 4] = Q[:, 4] - self.e_int_v0 * Q[:, 5]
        Td = np.ascontiguousarray(dQ[:, :5]).copy()
        self.lin(Td, Qd, t, alpha, beta)
        Qq = np.zeros_like(Qd)
        Qq[:, 0] = Q[:, 5]
        Tq = np.zeros_like(Td)
        self.lin(Tq, Qq, t, 1.0, 0.0)
        pen = Tq[:, 0].copy()
        Tq[:] = 0.0
        Tq[:, 0] = dQ[:, 5]
        self.lin(Tq, Qq, t, alpha, beta)
        Td[:, 4] += alpha * (self.e_int_v0 * pen)
        dQ[:, :5] = Td
        dQ[:, 5] = Tq[:, 0]


def oracle_column_lu6(O, lin, nvert, alpha):
    """oracle.OracleColumnLU probing six states."""

    class ColumnLU6(O.OracleColumnLU):
        def assemble(self, alpha):
            f = lambda dQ, Q: self.lin(dQ, Q, float("nan"), 1.0, 0.0)
            self.band, self.p, self.q = O.probe_band(f, self.grid, self.nvert, alpha, ns=6)
            self.alpha = alpha

    return ColumnLU6(lin, nvert, alpha)


def aux_of(cm, law, grid):
    full = device_full(cm, law, grid)
    aux = full.state_auxiliary.cpu().numpy().copy()
    return full, aux


# ---- 1. counts and refusals ----------------------------------------------------------------------

def test_moist_linear_counts_and_refusals(cm, torch):
    law, grid = moist_brick(cm)
    L = cm._lib.lib()
    ip, _ = law.descriptor()
    counts = (C.c_int32 * 6)()
    ipa = (C.c_int32 * 16)(*[int(v) for v in ip])
    assert L.cmdg_physics_counts(11, C.cast(ipa, C.c_void_p), C.cast(counts, C.c_void_p)) == 0
    assert tuple(counts) == (6, 19, 0, 0, 0, 0)
    full, _ = aux_of(cm, law, grid)
    lin = device_linear(cm, law, grid, full.state_auxiliary)
    assert lin.create_state().shape[1] == 6
    lu = cm.systemsolvers.ColumnLU(lin, 10.0)
    Nqv = grid.N[2] + 1
    assert lu.p == lu.q == 6 * Nqv - 1 and lu.n == 6 * Nqv * grid.topology.stacksize
    lu.close()
    # a Roe flux of the moist law on the linear law
    with pytest.raises(cm._lib.CmdgError, match="RoeNumericalFluxMoist"):
        device_linear(cm, law, grid, full.state_auxiliary, nf=cm.balancelaws.RoeNumericalFluxMoist)
    # a model without orientation: the library refuses the descriptor the host mirror refuses too
    mirror = cm.atmos.AtmosAcousticGravityLinearModel(law)
    ip4, dp = law.descriptor()
    ip4 = ip4.copy()
    ip4[4] = 1
    mirror.descriptor = lambda: (ip4, dp)
    with pytest.raises(cm._lib.CmdgError, match="no_orientation"):
        cm.dgmodel.DGModel(mirror, grid, direction=VERTICAL, state_auxiliary=full.state_auxiliary)
    # N = 5 is not compiled for the moist law (nor for its linear law)
    law5, grid5 = moist_brick(cm, N=5, nvert=2)
    with pytest.raises(cm._lib.CmdgError, match="N = 4, 6"):
        device_linear(cm, law5, grid5, law5.init_state_auxiliary(grid5))
    # a dry full model with the moist linear model in one ARK step
    dry = device_full(cm, law._dry, grid)
    Q = full.init_ode_state(0.0)
    ode = cm.odesolvers
    solver = ode.ARK2GiraldoKellyConstantinescu(dry, lin, ode.LinearBackwardEulerSolver(ode.ManyColumnLU()),
                                                Q, dt=1.0)
    with pytest.raises(cm._lib.CmdgError, match="5 states, the linear model 6"):
        solver.dostep(Q, 1)
    for h in (dry.handle, lin.handle):     # the refusal is on both members of the step
        assert b"5 states, the linear model 6" in L.cmdg_last_error(h)
    solver.close()
    dry.close()
    lin.close()
    full.close()


# ---- 2. dry limit, bit for bit -----------------------------------------------------------------

@pytest.mark.parametrize("nf", [0, 1])
def test_dry_limit_is_the_dry_linear_law_bitwise(cm, torch, nf):
    """rho q_tot = 0 (state and reference state): states 0-4 of the moist linear tendency equal
    the dry linear law's on the same 15 auxiliary columns, bit for bit; state 5 is exactly 0."""
    law, grid = moist_brick(cm, N=4, q0=0.0)
    full, aux = aux_of(cm, law, grid)
    dry, aux_dry = dry_twin_aux(law, aux)
    dev = full.device
    Q = perturbation6(law, aux, seed=5, moist=False)
    Q[:, 0] += aux[:, law.off_ref]
    Q[:, 4] += aux[:, law.off_ref + 3]
    Qt = torch.from_numpy(Q).to(dev)
    Qd = torch.from_numpy(np.ascontiguousarray(Q[:, :5])).to(dev)
    nr = grid.nreal
    for direction in (VERTICAL, EVERY, HORIZONTAL):
        lin = device_linear(cm, law, grid, full.state_auxiliary, direction, nf)
        dlin = cm.dgmodel.DGModel(cm.atmos.AtmosAcousticGravityLinearModel(dry), grid, direction=direction,
                                  numerical_flux_first_order=nf, state_auxiliary=aux_dry)
        T, Td = lin.create_state(), dlin.create_state()
        lin(T, Qt, 0.0, 1.0, 0.0)
        dlin(Td, Qd, 0.0, 1.0, 0.0)
        t, td = T.cpu().numpy()[:nr], Td.cpu().numpy()[:nr]
        assert np.array_equal(t[:, :5], td), (direction, np.abs(t[:, :5] - td).max())
        assert np.all(t[:, 5] == 0.0)
        assert np.abs(td).max() > 0
        dlin.close()
        lin.close()
    full.close()


# ---- 3. moisture coupling ----------------------------------------------------------------------

@pytest.mark.parametrize("N", [4, 6])
def test_moist_linear_tendency_matches_composed_oracle(cm, torch, oracle, N):
    """rho q_tot != 0: the device tendency against the composed oracle law, every direction,
    Rusanov and central, three (alpha, beta) pairs: <= 1e-12 per state of its max-norm (the
    composition rounds p_lin differently; 1.5e-13 is observed on the momentum at N = 6)."""
    law, grid = moist_brick(cm, N=N, nx=2, ny=1, nvert=3)
    full, aux = aux_of(cm, law, grid)
    dev = full.device
    d = perturbation6(law, aux, seed=3)
    d[:, 5] += 10 * aux[:, law.off_ref] * SCALE6[5]
    T0 = perturbation6(law, aux, seed=9)
    nr = grid.nreal
    worst = 0.0
    for direction in (VERTICAL, EVERY, HORIZONTAL):
        for nf in (0, 1):
            lin = device_linear(cm, law, grid, full.state_auxiliary, direction, nf)
            olin = ComposedMoistLinear(oracle, cm, law, grid, aux, nf, direction)
            for alpha, beta in ((1.0, 0.0), (1.0, 1.0), (0.5, 2.0)):
                T = torch.from_numpy(T0.copy()).to(dev)
                lin(T, torch.from_numpy(d).to(dev), 0.0, alpha, beta)
                To = T0.copy()
                olin(To, d, 0.0, alpha, beta)
                errs = per_state_errors(T.cpu().numpy()[:nr], To[:nr], STATES6)
                worst = max(worst, max(errs))
                assert max(errs) <= 1e-12, (direction, nf, alpha, beta, errs)
            lin.close()
    print("N=%d: worst per-state error %.2e" % (N, worst))
    observe("moist linear tendency vs composed oracle (N=%d)" % N, worst)
    full.close()


# ---- 4. Jacobian -------------------------------------------------------------------------------

def test_moist_linear_law_is_the_jacobian_of_the_full_law(cm, torch):
    """Central difference of the full moist law (VerticalDirection, constant viscosity 0, Gravity)
    at the dry reference state at rest along a perturbation of (rho, rho u, rho e), momentum
    tangential at the walls, against the moist linear DG applied to it."""
    law, grid = moist_brick(cm, N=4, q0=0.0)
    dgv = device_full(cm, law, grid, direction=VERTICAL)
    lin = device_linear(cm, law, grid, dgv.state_auxiliary)
    aux = dgv.state_auxiliary.cpu().numpy()
    Q0 = law.init_state_prognostic(grid, aux, 0.0)
    assert np.all(Q0[:, 5] == 0)
    dl = perturbation6(law, aux, seed=3, normal=False, moist=False) / SCALE6[None, :, None]
    dev = dgv.device
    nr = grid.nreal
    T1, T2, TL = dgv.create_state(), dgv.create_state(), dgv.create_state()
    results = []
    for eps in (1e-2, 1e-3, 1e-4):
        d = dl * (eps * SCALE6)[None, :, None]
        dgv(T1, torch.from_numpy(Q0 + d).to(dev), 0.0, 1.0, 0.0)
        dgv(T2, torch.from_numpy(Q0 - d).to(dev), 0.0, 1.0, 0.0)
        lin(TL, torch.from_numpy(d).to(dev), 0.0, 1.0, 0.0)
        fd = ((T1 - T2) / 2).cpu().numpy()[:nr]
        ld = TL.cpu().numpy()[:nr]
        # momentum as one vector state: its horizontal components are rounding in VerticalDirection
        per = per_state_errors(fd[:, :5], ld[:, :5])
        assert np.abs(ld[:, 5]).max() == 0.0 and np.abs(fd[:, 5]).max() <= 1e-12
        results.append((eps, max(per)))
        print("eps %.0e: relative max-norm difference per state %s" % (eps, ["%.2e" % v for v in per]))
    assert min(r for _, r in results) <= 1e-6
    lin.close()
    dgv.close()


# ---- 5. band -----------------------------------------------------------------------------------

def column_nodes6(grid, nvert, column):
    Nq, Nqv = grid.N[0] + 1, grid.N[2] + 1
    nqh2 = Nq * Nq
    h, ij = divmod(column, nqh2)
    return [(h * nvert + v, s, ij + nqh2 * k) for v in range(nvert) for k in range(Nqv) for s in range(6)]


def dense_column6(lin, grid, nvert, column, alpha):
    rows = column_nodes6(grid, nvert, column)
    n = len(rows)
    Q, T = lin.create_state(), lin.create_state()
    A = np.zeros((n, n))
    for j, (e, s, node) in enumerate(rows):
        Q.zero_()
        Q[e, s, node] = 1.0
        lin(T, Q, float("nan"), 1.0, 0.0)
        Tn = T.cpu().numpy()
        for i, (e2, s2, node2) in enumerate(rows):
            A[i, j] = (1.0 if i == j else 0.0) + (-alpha) * Tn[e2, s2, node2]
    return A


@pytest.mark.parametrize("nf", [0, 1])
def test_moist_band_equals_dense_operator(cm, torch, nf):
    """The assembled band against the dense I - alpha L probed from the device operator: <= 1e-14,
    exact zeros outside the band.  Central flux: every rho q_tot row is a unit row; Rusanov: a
    rho q_tot row couples rho q_tot only (the jump penalty)."""
    law, grid = moist_brick(cm, N=4, nx=2, ny=1, nvert=3)
    full, _ = aux_of(cm, law, grid)
    lin = device_linear(cm, law, grid, full.state_auxiliary, nf=nf)
    nvert = grid.topology.stacksize
    alpha = 37.5
    lu = cm.systemsolvers.ColumnLU(lin, alpha)
    assert lu.p == lu.q == cm.systemsolvers.lower_bandwidth(grid.N[2], 6, 1) == 29
    lu.assemble(alpha)
    for column in (0, 7, lu.ncol - 1):
        band = lu.export_band(column)
        A = dense_column6(lin, grid, nvert, column, alpha)
        B = band_to_dense(band, lu.p, lu.q)
        err = np.abs(A - B).max() / np.abs(A).max()
        assert err <= 1e-14, err
        i, j = np.indices(A.shape)
        assert np.all(A[np.abs(i - j) > lu.p] == 0.0)
        qrows = np.arange(5, lu.n, 6)
        if nf == 1:
            assert np.array_equal(B[qrows], np.eye(lu.n)[qrows])
        else:
            others = np.ones(lu.n, bool)
            others[qrows] = False
            assert np.all(B[np.ix_(qrows, np.nonzero(others)[0])] == 0.0)
            assert np.all(np.diag(B)[qrows] != 0.0)
    lu.close()
    lin.close()
    full.close()


# ---- 6. factor and solve, bit for bit ----------------------------------------------------------

def device_bands(lu, columns):
    return np.stack([lu.export_band(c).T for c in columns], axis=2)


@pytest.mark.parametrize("N", [4, 6])
@pytest.mark.parametrize("nvert", [1, 2, 3, 7])
def test_moist_band_factor_solve_match_oracle(cm, torch, oracle, N, nvert):
    """The device band against the oracle's probing of the composed law (<= 1e-12 of the column's
    max), and the device solve against the oracle's factor and solve of that band (<= 1e-11 per
    state).  The device's own band through oracle.band_lu / band_forward / band_back: the factors
    and the solve are bit-identical, which pins the kernels independently of the law."""
    law, grid = moist_brick(cm, N=N, nx=2, ny=1, nvert=nvert)
    full, aux = aux_of(cm, law, grid)
    lin = device_linear(cm, law, grid, full.state_auxiliary)
    olin = ComposedMoistLinear(oracle, cm, law, grid, aux)
    alpha = 10.0
    lu = cm.systemsolvers.ColumnLU(lin, alpha)
    columns = [0, lu.ncol // 2 + 3, lu.ncol - 1]
    lu.assemble(alpha)
    got = device_bands(lu, columns)
    want, p, q = oracle.probe_band(lambda dQ, Q: olin(dQ, Q, float("nan"), 1.0, 0.0), grid, nvert,
                                   alpha, ns=6)
    want = want[:, :, columns]
    assert (lu.p, lu.q) == (p, q)
    for i in range(len(columns)):
        err = np.abs(got[:, :, i] - want[:, :, i]).max() / np.abs(want[:, :, i]).max()
        assert err <= 1e-12, (columns[i], err)
    lu.update(alpha)
    factored = device_bands(lu, columns)
    assert np.array_equal(factored, oracle.band_lu(got.copy(), p, q))
    rng = np.random.default_rng(3 + nvert)
    b = rng.standard_normal((grid.nelem, 6, grid.Np)) * SCALE6[None, :, None]
    x = lin.create_state()
    lu.solve(x, torch.from_numpy(b).to(lin.device))
    xc = oracle.to_columns(x.cpu().numpy(), grid, nvert)[:, columns]
    bc = oracle.to_columns(b, grid, nvert)[:, columns]
    assert np.array_equal(xc, oracle.band_back(factored, oracle.band_forward(factored, bc, p, q), p, q))
    # against the oracle's own band of the composed law, per state
    wf = oracle.band_lu(want.copy(), p, q)
    ox = oracle.band_back(wf, oracle.band_forward(wf, bc, p, q), p, q)
    for s in range(6):
        rows = np.arange(s, lu.n, 6)
        err = np.abs(xc[rows] - ox[rows]).max() / np.abs(ox[rows]).max()
        assert err <= 1e-11, (s, err)
    lu.close()
    lin.close()
    full.close()


# ---- 7. ARK2GKC step ---------------------------------------------------------------------------

def moist_initial_state(cm, law, grid, full, amp=1e-2):
    aux = full.state_auxiliary.cpu().numpy().copy()
    Q0 = law.init_state_prognostic(grid, aux, 0.0) + amp * perturbation6(law, aux, seed=7)
    return np.ascontiguousarray(Q0), aux


def device_ark(cm, torch, law, grid, Q0, dts, split):
    ode = cm.odesolvers
    full = device_full(cm, law, grid)
    lin = device_linear(cm, law, grid, full.state_auxiliary)
    Q = torch.from_numpy(Q0.copy()).to(full.device)
    solver = ode.ARK2GiraldoKellyConstantinescu(
        full, lin, ode.LinearBackwardEulerSolver(ode.ManyColumnLU(), isadjustable=True), Q,
        dt=dts[0], t0=0.0, split_explicit_implicit=split)
    out = []
    for dt in dts:
        solver.dostep(Q, 1, dt=dt)
        full.synchronize()
        out.append(Q.cpu().numpy().copy())
    solver.close()
    lin.close()
    full.close()
    return out


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("schedule", ["constant", "refactor"])
def test_moist_ark_step_matches_oracle(cm, torch, oracle, split, schedule):
    """cmdg_ark_step on the moist pair against oracle.ark_step with the oracle's full moist law,
    the composed linear law and a six-state oracle column LU, after 1 and 3 steps, from an
    unsaturated moist state away from rest: <= 1e-12 per state of its max-norm.  ``refactor``
    steps dt, dt / 2, dt."""
    law, grid = moist_brick(cm, N=4)
    dt = 1.0
    dts = [dt, dt, dt] if schedule == "constant" else [dt, dt / 2, dt]
    full, _ = aux_of(cm, law, grid)
    Q0, aux0 = moist_initial_state(cm, law, grid, full)
    full.close()
    got = device_ark(cm, torch, law, grid, Q0, dts, split)
    ofull = oracle.OracleDGModel(law, grid, nf_first=0, direction=EVERY, state_auxiliary=aux0.copy())
    olin = ComposedMoistLinear(oracle, cm, law, grid, aux0)
    tableau = cm.odesolvers.ark2gkc_tableau()
    lu = oracle_column_lu6(oracle, olin, grid.topology.stacksize, dts[0] * tableau[1][1][1])
    Q = Q0.copy()
    t = 0.0
    nr = grid.nreal
    for n, step in enumerate(dts):
        oracle.ark_step(ofull, olin, lu, Q, t, step, tableau, split)
        t += step
        if n in (0, 2):
            errs = per_state_errors(got[n][:nr], Q[:nr], STATES6)
            inc = per_state_errors(got[n][:nr] - Q0[:nr], Q[:nr] - Q0[:nr], STATES6)
            print("split=%s %s step %d: state error %s, increment error %s"
                  % (split, schedule, n + 1, ["%.2e" % e for e in errs], ["%.2e" % e for e in inc]))
            observe("moist imex ark state vs oracle (split=%s, %s, %d steps)" % (split, schedule, n + 1),
                    max(errs))
            assert max(errs) <= 1e-12, errs
            assert max(inc) <= 1e-10, inc
    # unsaturated throughout: the moist law's condensate stays zero
    assert np.all(Q[:nr, 5] / Q[:nr, 0] < 5e-3)
    if split and schedule == "refactor":
        again = device_ark(cm, torch, law, grid, Q0, dts, split)
        assert np.array_equal(again[-1][:nr], got[-1][:nr])


# ---- 8. BOMEX ----------------------------------------------------------------------------------

def bomex_brick(cm, N=4, ne=3, nz=16, dx=1600.0):
    """bomex_model(3000) on ne x ne x nz elements (periodic in x and y) of dx x dx x 3000 / nz m:
    a horizontal to vertical node-spacing ratio of dx nz / 3000."""
    M = cm.mesh
    rng = [np.linspace(0.0, dx * ne, ne + 1), np.linspace(0.0, dx * ne, ne + 1), np.linspace(0.0, 3000.0, nz + 1)]
    topl = M.StackedBrickTopology(rng, periodicity=(True, True, False), boundary=((0, 0), (0, 0), (1, 2)))
    grid = M.DiscontinuousSpectralElementGrid(topl, N)
    return cm.moist.bomex_model(3000.0), grid


def run_bomex_imex(cm, torch, law, grid, nsteps):
    dgm = cm.dgmodel
    full = device_full(cm, law, grid)
    lin = device_linear(cm, law, grid, full.state_auxiliary)
    Q = full.init_ode_state(0.0)
    c_h = full.courant(dgm.NONDIFFUSIVE_COURANT, Q, 1.0, 0.0, HORIZONTAL)
    c_v = full.courant(dgm.NONDIFFUSIVE_COURANT, Q, 1.0, 0.0, VERTICAL)
    dt = 0.35 / c_h            # bomex_les.jl: Courant_number 0.35, CFL_direction HorizontalDirection
    Q0 = Q.clone()
    ode = cm.odesolvers
    solver = ode.ARK2GiraldoKellyConstantinescu(full, lin, ode.LinearBackwardEulerSolver(ode.ManyColumnLU()),
                                                Q, dt=dt)
    solver.dostep(Q, nsteps)
    full.synchronize()
    solver.close()
    return full, lin, Q0, Q, dt, 1.0 / c_v


def test_bomex_imex_runs_past_the_vertical_acoustic_limit(cm, torch):
    """All BOMEX sources and surface fluxes, 20 IMEX steps at the horizontal Courant number 0.35:
    finite, and the dt is at least twice the explicit vertical acoustic limit."""
    law, grid = bomex_brick(cm)
    full, lin, Q0, Q, dt, dt_v = run_bomex_imex(cm, torch, law, grid, 20)
    print("BOMEX brick: IMEX dt %.4f s, vertical acoustic limit %.4f s (ratio %.2f)" % (dt, dt_v, dt / dt_v))
    assert dt >= 2 * dt_v
    assert bool(torch.isfinite(Q[:grid.nreal]).all())
    assert not torch.equal(Q, Q0)
    lin.close()
    full.close()


def test_bomex_imex_conserves_mass_and_water(cm, torch):
    """Sources and surface fluxes off (Gravity and default walls only): weightedsum of rho and of
    rho q_tot after 20 IMEX steps within 1e-13 relative of the initial ones."""
    law, grid = bomex_brick(cm)
    law.sources = cm.atmos.SRC_GRAVITY
    law.boundary_conditions = (cm.atmos.BC_ATMOS_DEFAULT, cm.atmos.BC_ATMOS_DEFAULT)
    full, lin, Q0, Q, dt, _ = run_bomex_imex(cm, torch, law, grid, 20)
    R = cm.reductions
    for s in (1, 6):
        a = float(np.sum(R.weightedsum(full, Q0, states=[s])))
        b = float(np.sum(R.weightedsum(full, Q, states=[s])))
        print("state %d: weightedsum %.17e -> %.17e (%.2e)" % (s, a, b, abs(b - a) / abs(a)))
        assert abs(b - a) <= 1e-13 * abs(a), (s, a, b)
    lin.close()
    full.close()


# ---- 9. temporal order -------------------------------------------------------------------------

@pytest.mark.parametrize("split", [False, True])
def test_moist_imex_temporal_order(cm, torch, split):
    """ARK2GKC on a smooth unsaturated moist perturbation: errors at dt, dt/2, dt/4 against dt/16
    over 2 s, dt = 0.2 s (vertical acoustic Courant number near 1); observed orders 1.9 - 2.1."""
    law, grid = moist_brick(cm, N=4)
    full, _ = aux_of(cm, law, grid)
    Q0, _ = moist_initial_state(cm, law, grid, full)
    T, dt0 = 2.0, 0.2
    runs = {}
    for k in (1, 2, 4, 16):
        n = int(round(T * k / dt0))
        runs[k] = device_ark(cm, torch, law, grid, Q0, [dt0 / k] * n, split)[-1]
    dev = full.device
    ref = torch.from_numpy(runs[16]).to(dev)
    err = [full.euclidean_distance(torch.from_numpy(runs[k]).to(dev), ref) for k in (1, 2, 4)]
    orders = [math.log2(err[i] / err[i + 1]) for i in range(2)]
    print("split=%s errors %s observed orders %s" % (split, err, orders))
    assert all(1.9 <= o <= 2.1 for o in orders), orders
    full.close()
