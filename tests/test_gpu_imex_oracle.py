"""The device IMEX path against the oracle: the linear law's tendency (csrc/physics_atmos_linear.h
vs oracle/physics_atmos_linear.c), the column band's assembly, factorisation and solve
(csrc/columnlu.hip vs oracle.probe_band / band_lu / band_forward / band_back) and cmdg_ark_step (csrc/steppers.hip)
vs oracle.ark_step.  Errors are per state (rho, rho u, rho e), each against its own max-norm."""
import ctypes as C

import numpy as np
import pytest

from helpers import observe
from imex_cases import (EVERY, HORIZONTAL, STATE_SCALE, VERTICAL, acoustic_setup, flat_brick,
                        oracle_pair, per_state_errors, per_state_rel, small_sphere, wall_perturbation)

pytestmark = pytest.mark.gpu

VARIANTS = {"plain": {}, "hyper": {"hyper": True}, "smag": {"smag": True}}
CASES = {"sphere": small_sphere, "brick": flat_brick}


def device_full(cm, law, grid, diffusion_direction=None):
    return cm.dgmodel.DGModel(law, grid, direction=EVERY, diffusion_direction=diffusion_direction)


def device_linear(cm, law, grid, full, direction=VERTICAL, nf=0):
    return cm.dgmodel.DGModel(cm.atmos.AtmosAcousticGravityLinearModel(law), grid, direction=direction,
                              numerical_flux_first_order=nf, state_auxiliary=full.state_auxiliary)


@pytest.mark.parametrize("case", ["sphere", "brick"])
@pytest.mark.parametrize("variant", ["plain", "hyper", "smag"])
@pytest.mark.parametrize("N", [4, 5])
def test_linear_tendency_matches_oracle(cm, torch, oracle, case, variant, N):
    """Every accepted configuration of the linear law: Vertical / Every / Horizontal direction,
    Rusanov and central first-order fluxes, the full law plain (NAUX 16), with hyperdiffusion
    (17) or with Smagorinsky (17, its column before the others), on the sphere and on a flat
    brick; a perturbation with normal momentum at the walls (the free-slip reflection), three
    (alpha, beta) pairs.  <= 1e-12 per state."""
    law, grid = CASES[case](cm, N=N, **VARIANTS[variant])
    full = device_full(cm, law, grid)
    aux = full.state_auxiliary.cpu().numpy().copy()
    d = wall_perturbation(law, aux, normal=True) * STATE_SCALE[None, :, None]
    T0 = wall_perturbation(law, aux, normal=True, seed=9) * STATE_SCALE[None, :, None]
    nr = grid.nreal
    dev = full.device
    worst = 0.0
    for direction in (VERTICAL, EVERY, HORIZONTAL):
        for nf in (0, 1):
            lin = device_linear(cm, law, grid, full, direction, nf)
            _, olin = oracle_pair(oracle, law, grid, state_auxiliary=aux, lin_nf=nf,
                                  lin_direction=direction)
            for alpha, beta in ((1.0, 0.0), (1.0, 1.0), (0.5, 2.0)):
                T = torch.from_numpy(T0.copy()).to(dev)
                lin(T, torch.from_numpy(d).to(dev), 0.0, alpha, beta)
                To = T0.copy()
                olin(To, d, 0.0, alpha, beta)
                err = per_state_rel(T.cpu().numpy()[:nr], To[:nr])
                worst = max(worst, err)
                assert err <= 1e-12, (direction, nf, alpha, beta, err)
            lin.close()
    print("%s %s N=%d: worst per-state error %.2e" % (case, variant, N, worst))
    full.close()


def oracle_band_of_columns(oracle, olin, grid, nvert, alpha, columns):
    band, p, q = oracle.probe_band(lambda dQ, Q: olin(dQ, Q, float("nan"), 1.0, 0.0), grid, nvert,
                                   alpha)
    return band[:, :, columns], p, q


def device_bands(lu, columns):
    """(n, P, len(columns)) from export_band's (P, n) per column."""
    return np.stack([lu.export_band(c).T for c in columns], axis=2)


@pytest.mark.parametrize("N", [4, 5])
@pytest.mark.parametrize("nvert", [1, 2, 3, 4, 7])
def test_band_factor_solve_match_oracle(cm, torch, oracle, N, nvert):
    """The assembled band against the oracle's probing of the oracle's linear DG (<= 1e-12 of the
    column's max, the same zero pattern); the factored band against oracle.band_lu applied to
    the device's own assembled band, and the solve against the oracle's substitutions on the
    device's own factors: bit-identical (the same operations in the same order, no contraction
    on either side).  Stacks of 4 and 7 put two and three probed elements of a stack in one
    probing pass; ncol (600 at N = 4, 864 at N = 5) is not a multiple of 64."""
    law, grid = small_sphere(cm, N=N, nvert=nvert)
    full = device_full(cm, law, grid)
    lin = device_linear(cm, law, grid, full)
    aux = full.state_auxiliary.cpu().numpy().copy()
    _, olin = oracle_pair(oracle, law, grid, state_auxiliary=aux)
    alpha = 37.5
    lu = cm.systemsolvers.ColumnLU(lin, alpha)
    assert lu.ncol % 64 != 0
    columns = [0, lu.ncol // 2 + 5, lu.ncol - 1]
    lu.assemble(alpha)
    got = device_bands(lu, columns)
    want, p, q = oracle_band_of_columns(oracle, olin, grid, nvert, alpha, columns)
    assert (lu.p, lu.q) == (p, q)
    for i in range(len(columns)):
        scale = np.abs(want[:, :, i]).max()
        err = np.abs(got[:, :, i] - want[:, :, i]).max() / scale
        assert err <= 1e-12, (columns[i], err)
        assert np.array_equal(got[:, :, i] == 0.0, want[:, :, i] == 0.0)
    lu.update(alpha)
    factored = device_bands(lu, columns)
    ofactored = oracle.band_lu(got.copy(), p, q)
    assert np.array_equal(factored, ofactored)
    rng = np.random.default_rng(3 + nvert)
    b = rng.standard_normal((grid.nelem, 5, grid.Np)) * STATE_SCALE[None, :, None]
    x = lin.create_state()
    lu.solve(x, torch.from_numpy(b).to(lin.device))
    xc = oracle.to_columns(x.cpu().numpy(), grid, nvert)[:, columns]
    bc = oracle.to_columns(b, grid, nvert)[:, columns]
    ox = oracle.band_back(factored, oracle.band_forward(factored, bc, p, q), p, q)
    assert np.array_equal(xc, ox)
    lu.close()
    lin.close()
    full.close()


def ark_case(cm, name):
    if name == "sphere":
        law, grid = small_sphere(cm, N=4, hyper=True)
        return law, grid, 30.0
    law, grid = acoustic_setup(cm, n_horz=3, n_vert=5, N=5)
    return law, grid, 100.0


def device_ark(cm, torch, law, grid, Q0, dts, split):
    """Device ARK2GKC steps of sizes ``dts`` from Q0; the state after every step."""
    ode = cm.odesolvers
    full = device_full(cm, law, grid, diffusion_direction=HORIZONTAL)
    lin = device_linear(cm, law, grid, full)
    Q = torch.from_numpy(Q0.copy()).to(full.device)
    solver = ode.ARK2GiraldoKellyConstantinescu(
        full, lin, ode.LinearBackwardEulerSolver(ode.ManyColumnLU(), isadjustable=True), Q,
        dt=dts[0], t0=0.0, split_explicit_implicit=split)
    out = []
    for dt in dts:
        solver.dostep(Q, 1, dt=dt)
        full.synchronize()
        out.append(Q.cpu().numpy().copy())
    aux = full.state_auxiliary.cpu().numpy().copy()
    solver.close()
    lin.close()
    full.close()
    return out, aux


def initial_state(cm, law, grid, name):
    full = device_full(cm, law, grid)
    aux = full.state_auxiliary.cpu().numpy().copy()
    Q0 = law.init_state_prognostic(grid, aux, 0.0)
    if name == "sphere":          # a state away from rest, momentum normal to the walls included
        Q0 = Q0 + 1e-2 * wall_perturbation(law, aux, normal=True) * STATE_SCALE[None, :, None]
    full.close()
    return np.ascontiguousarray(Q0, dtype=np.float64), aux


@pytest.mark.parametrize("name", ["sphere", "acoustic"])
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("schedule", ["constant", "refactor"])
def test_ark_step_matches_oracle(cm, torch, oracle, name, split, schedule):
    """cmdg_ark_step against oracle.ark_step after 1 and 3 steps: the increment Q_n - Q_0 per
    state <= 1e-10 of its max-norm.  ``refactor`` steps dt, dt / 2, dt: the column matrices are
    reassembled and refactored inside the second and the third step.  The small sphere carries
    hyperdiffusion (N = 4, horizontal diffusion as in the Held-Suarez configuration), the acoustic grid is acousticwave_1d_imex.jl's at 3 x 3 x 6 x 5, N = 5."""
    law, grid, dt = ark_case(cm, name)
    dts = [dt, dt, dt] if schedule == "constant" else [dt, dt / 2, dt]
    Q0, aux0 = initial_state(cm, law, grid, name)
    got, _ = device_ark(cm, torch, law, grid, Q0, dts, split)
    full, lin = oracle_pair(oracle, law, grid, state_auxiliary=aux0.copy(),
                            diffusion_direction=HORIZONTAL)
    tableau = cm.odesolvers.ark2gkc_tableau()
    lu = oracle.OracleColumnLU(lin, grid.topology.stacksize, dts[0] * tableau[1][1][1])
    Q = Q0.copy()
    t = 0.0
    nr = grid.nreal
    for n, step in enumerate(dts):
        oracle.ark_step(full, lin, lu, Q, t, step, tableau, split)
        t += step
        if n in (0, 2):
            inc_dev = got[n][:nr] - Q0[:nr]
            inc_orc = Q[:nr] - Q0[:nr]
            errs = per_state_errors(inc_dev, inc_orc)
            print("%s split=%s %s step %d: increment error per state %s"
                  % (name, split, schedule, n + 1, ["%.2e" % e for e in errs]))
            observe("imex ark increment vs oracle (%s, split=%s, %s, %d steps)"
                    % (name, split, schedule, n + 1), max(errs))
            assert max(errs) <= 1e-10, errs


def test_ark_step_is_deterministic(cm, torch):
    """Two fresh split runs of the two-stream step (the full handle's and the linear handle's
    streams ordered by events) are bit-identical."""
    law, grid, dt = ark_case(cm, "sphere")
    Q0, _ = initial_state(cm, law, grid, "sphere")
    a, _ = device_ark(cm, torch, law, grid, Q0, [dt, dt], True)
    b, _ = device_ark(cm, torch, law, grid, Q0, [dt, dt], True)
    nr = grid.nreal
    assert np.array_equal(a[-1][:nr], b[-1][:nr])


def test_vertically_periodic_stacks_are_refused(cm, torch):
    """A vertically periodic stack couples its top and bottom elements; the band holds only
    neighbouring elements, so the assembly dropped or misattributed that coupling and the solve
    was silently wrong.  The host side and the library (cmdg_columnlu_create itself) refuse it."""
    law, grid = flat_brick(cm, N=4, nvert=3, periodic=True)
    full = device_full(cm, law, grid)
    lin = device_linear(cm, law, grid, full)
    with pytest.raises(cm._lib.CmdgError, match="periodic"):
        cm.systemsolvers.ColumnLU(lin, 10.0)
    h = C.c_void_p()
    lin._torch_ready()
    r = lin.L.cmdg_columnlu_create(lin.handle, 3, 10.0, C.byref(h))
    assert r == -5 and not h.value      # CMDG_ERR_UNSUPPORTED, no handle
    with pytest.raises(cm._lib.CmdgError, match="periodic"):
        cm._lib.check(r, lin.handle)
    lin.close()
    full.close()
