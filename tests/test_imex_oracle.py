"""The oracle's IMEX pieces pinned without a device: AtmosAcousticGravityLinearModel
(oracle/physics_atmos_linear.c) against the central difference of the oracle's full law, the band
LU and substitutions of ManyColumnLU (oracle.band_lu / band_forward / band_back) against
numpy.linalg, the oracle ARK2GiraldoKellyConstantinescu step against the reference's stored
acousticwave_1d_imex.jl result, and the host-side refusal of vertically periodic stacks."""
import math

import numpy as np
import pytest

from imex_cases import (ACOUSTIC_GOLDEN, STATE_SCALE, VERTICAL, acoustic_setup, flat_brick,
                        oracle_pair, per_state_rel, ref_state, small_sphere, wall_perturbation)

CASES = {"sphere": small_sphere, "brick": flat_brick}


def jacobian_errors(O, cm, case, N, normal):
    law, grid = CASES[case](cm, N=N)
    full, lin = oracle_pair(O, law, grid, full_direction=VERTICAL)
    aux = full.state_auxiliary
    Q0 = ref_state(law, aux)
    dl = wall_perturbation(law, aux, normal=normal)
    nr = grid.nreal
    errs = []
    for eps in (1e-2, 1e-3, 1e-4):
        d = dl * (eps * STATE_SCALE)[None, :, None]
        T1, T2, TL = np.zeros_like(Q0), np.zeros_like(Q0), np.zeros_like(Q0)
        full(T1, Q0 + d, 0.0, 1.0, 0.0)
        full(T2, Q0 - d, 0.0, 1.0, 0.0)
        lin(TL, d, 0.0, 1.0, 0.0)
        errs.append(per_state_rel(((T1 - T2) / 2)[:nr], TL[:nr]))
    return errs


@pytest.mark.parametrize("case", ["sphere", "brick"])
@pytest.mark.parametrize("N", [4, 5])
def test_linear_law_is_the_jacobian_tangential(oracle, cm, case, N):
    """Momentum tangential at the walls: the central difference of the full law (VerticalDirection,
    viscosity 0) at the rest state equals the linear law up to O(eps^2) and rounding; per state
    (rho, rho u, rho e) against its own max-norm, the best of three eps is <= 1e-7 (DESIGN: 6e-8)."""
    errs = jacobian_errors(oracle, cm, case, N, normal=False)
    print("%s N=%d tangential: %s" % (case, N, ["%.2e" % e for e in errs]))
    assert min(errs) <= 1e-7


@pytest.mark.parametrize("case", ["sphere", "brick"])
@pytest.mark.parametrize("N", [4, 5])
def test_linear_law_is_the_jacobian_normal(oracle, cm, case, N):
    """Momentum normal to the walls: the free-slip reflection puts a jump 2 (rho u . n) n into the
    Rusanov penalty, weighted by |u . n| in the full law's wavespeed, an O(eps^2) term the central
    difference does not cancel.  It must be the only difference: it scales exactly like eps."""
    errs = jacobian_errors(oracle, cm, case, N, normal=True)
    print("%s N=%d normal: %s" % (case, N, ["%.2e" % e for e in errs]))
    for a, b in zip(errs, errs[1:]):
        assert 9.0 <= a / b <= 11.0, errs
    assert errs[0] > 1e-6          # the reflection is exercised at all


def random_band(rng, n, p, q, ncol):
    """A diagonally dominant band in the device layout (n, p + q + 1, ncol), exact zeros in the
    slots outside the matrix."""
    P = p + q + 1
    band = rng.standard_normal((n, P, ncol))
    band[:, q] = np.abs(band[:, q]) + P + 1.0
    for col in range(n):
        for d in range(P):
            if not 0 <= col + d - q < n:
                band[col, d] = 0.0
    return band


def dense(band, c, p, q):
    n, P, _ = band.shape
    A = np.zeros((n, n))
    for col in range(n):
        for d in range(P):
            row = col + d - q
            if 0 <= row < n:
                A[row, col] = band[col, d, c]
    return A


@pytest.mark.parametrize("nvert", [1, 2, 4])
def test_band_lu_and_substitution_match_numpy(oracle, nvert):
    """N = 4 bandwidths (p = q = 24, n = 25 nvert): L U reproduces the matrix, the two
    substitutions solve it as numpy.linalg.solve does, the slots outside the matrix stay zero."""
    rng = np.random.default_rng(7 + nvert)
    p = q = 5 * 5 - 1
    n, ncol = 25 * nvert, 5
    band = random_band(rng, n, p, q, ncol)
    outside = band == 0.0
    A = [dense(band, c, p, q) for c in range(ncol)]
    lu = oracle.band_lu(band.copy(), p, q)
    assert np.all(lu[outside] == 0.0)
    b = rng.standard_normal((n, ncol))
    x = oracle.band_back(lu, oracle.band_forward(lu, b, p, q), p, q)
    for c in range(ncol):
        D = dense(lu, c, p, q)
        Lm = np.tril(D, -1) + np.eye(n)
        Um = np.triu(D)
        assert np.abs(Lm @ Um - A[c]).max() <= 1e-13 * np.abs(A[c]).max()
        want = np.linalg.solve(A[c], b[:, c])
        assert np.abs(x[:, c] - want).max() <= 1e-13 * np.abs(want).max()


def test_probed_band_is_the_dense_operator(oracle, cm):
    """The probing assembly (stride 3: four elements per stack, so one pass holds two probed
    elements of a stack) equals I - alpha L built one unit vector at a time, with the band's zero
    pattern: no coupling beyond the neighbouring element."""
    law, grid = small_sphere(cm, N=4, nvert=4)
    _, lin = oracle_pair(oracle, law, grid)
    nvert, alpha = 4, 37.5
    band, p, q = oracle.probe_band(lambda dQ, Q: lin(dQ, Q, float("nan"), 1.0, 0.0), grid, nvert,
                                   alpha)
    n = band.shape[0]
    column = 7
    nqh2 = grid.Nq[0] ** 2
    h, ij = divmod(column, nqh2)
    Q = np.zeros((grid.nelem, 5, grid.Np))
    T = np.zeros_like(Q)
    A = np.zeros((n, n))
    rows = [(h * nvert + v, s, ij + nqh2 * k) for v in range(nvert) for k in range(grid.Nq[2])
            for s in range(5)]
    for j, (e, s, node) in enumerate(rows):
        Q[:] = 0.0
        Q[e, s, node] = 1.0
        lin(T, Q, float("nan"), 1.0, 0.0)
        A[:, j] = [Q[e2, s2, n2] + (-alpha) * T[e2, s2, n2] for e2, s2, n2 in rows]
    B = dense(band, column, p, q)
    assert np.array_equal(A, B)


def test_oracle_acousticwave_golden(oracle, cm):
    """acousticwave_1d_imex.jl in Float64 through the oracle alone: N = 5, 10 x 5 elements,
    dt = 100 s, 36 ARK2GKC steps (split_explicit_implicit = false) with LinearBackwardEulerSolver(
    ManyColumnLU()), the order-18 vertical exponential filter after every step; norm(Q) against
    9.5073452847149594e+13 at rtol = sqrt(eps).  As in test_gpu_imex.test_acousticwave_golden the
    tracer's rho chi = 1 stands in as int 1 dV."""
    F, ode = cm.mesh.filters, cm.odesolvers
    law, grid = acoustic_setup(cm)
    full, lin = oracle_pair(oracle, law, grid)
    Q = law.init_state_prognostic(grid, full.state_auxiliary, 0.0)
    Q = np.ascontiguousarray(Q, dtype=np.float64)
    tableau = ode.ark2gkc_tableau()
    dt, nsteps = 100.0, 36
    lu = oracle.OracleColumnLU(lin, grid.topology.stacksize, dt * tableau[1][1][1])
    filt = F.ExponentialFilter(grid, 0, 18)
    target = F.FilterIndices(range(1, 6))
    t = 0.0
    for _ in range(nsteps):
        oracle.ark_step(full, lin, lu, Q, t, dt, tableau, split=False)
        t += dt
        oracle.apply_filter(Q, target, grid, filt, direction=VERTICAL)
    M = grid.vgeo[:grid.nreal, cm.mesh.grids._M, :]
    got = math.sqrt(oracle.weighted_norm2_local(grid, Q) + float(M.sum()))
    rel = abs(got - ACOUSTIC_GOLDEN) / ACOUSTIC_GOLDEN
    print("oracle acoustic wave IMEX: norm(Q) = %.16e, relative error %.3e" % (got, rel))
    assert rel <= math.sqrt(np.finfo(float).eps)


def test_columnlu_refuses_vertically_periodic_stacks(cm):
    """A vertically periodic stack couples its top and bottom elements: the band cannot hold that
    coupling, so the host side refuses the grid before anything is assembled."""
    law, grid = flat_brick(cm, N=4, nvert=3, periodic=True)

    class Stub:                      # only the grid is read before the library is called
        pass
    lin = Stub()
    lin.grid = grid
    with pytest.raises(cm._lib.CmdgError, match="periodic"):
        cm.systemsolvers.ColumnLU(lin, 1.0)
