"""IMEX host pieces (no GPU): the ARK2GiraldoKellyConstantinescu tableau against the reference's
expressions (AdditiveRungeKuttaMethod.jl:839-895) and the LowStorageVariant preconditions
(:157-168); the column solver's bandwidths (columnwise_lu_solver.jl:56-74) and band offsets."""
import math

import numpy as np
import pytest

from cmdg_loader import cm


@pytest.mark.parametrize("paperversion", [False, True])
def test_ark2gkc_tableau_term_by_term(paperversion):
    A_e, A_i, B, C = cm.odesolvers.ark2gkc_tableau(paperversion)
    s2 = math.sqrt(2)
    a32 = (3 + 2 * s2) / 6 if paperversion else 0.5
    want_e = [[0, 0, 0], [2 - s2, 0, 0], [1 - a32, a32, 0]]
    want_i = [[0, 0, 0], [1 - 1 / s2, 1 - 1 / s2, 0], [1 / (2 * s2), 1 / (2 * s2), 1 - 1 / s2]]
    want_b = [1 / (2 * s2), 1 / (2 * s2), 1 - 1 / s2]
    want_c = [0, 2 - s2, 1]
    for i in range(3):
        for j in range(3):
            assert A_e[i][j] == want_e[i][j]
            assert A_i[i][j] == want_i[i][j]
    assert list(B) == want_b and list(C) == want_c
    # LowStorageVariant: B and C shared (one tuple each), the diagonal (0, c, c)
    diag = [A_i[i][i] for i in range(3)]
    assert diag[0] == 0 and diag[1] == diag[2] != 0
    # both tables are consistent: rows sum to C
    for i in range(3):
        assert abs(sum(A_e[i]) - C[i]) < 1e-15 and abs(sum(A_i[i]) - C[i]) < 1e-15
    # second order: b . c = 1/2
    assert abs(sum(b * c for b, c in zip(B, C)) - 0.5) < 1e-15


def test_ark_refuses_a_non_low_storage_diagonal():
    class FakeDG:
        pass
    with pytest.raises(ValueError):
        cm.odesolvers.AdditiveRungeKutta(
            FakeDG(), FakeDG(), cm.odesolvers.LinearBackwardEulerSolver(cm.odesolvers.ManyColumnLU()),
            np.zeros((2, 2)), np.array([[0.25, 0.0], [0.5, 0.25]]), [0.5, 0.5], [0.0, 1.0], None, dt=1.0)
    with pytest.raises(TypeError):
        cm.odesolvers.LinearBackwardEulerSolver(object())


@pytest.mark.parametrize("N", range(1, 8))
def test_bandwidth_formula(N):
    S = cm.systemsolvers
    # lower_bandwidth(N, nstate, eband) = (N + 1) nstate eband - 1; eband = 1 (no gradient flux)
    assert S.lower_bandwidth(N, 5, 1) == (N + 1) * 5 - 1
    assert S.upper_bandwidth(N, 5, 1) == S.lower_bandwidth(N, 5, 1)
    assert S.lower_bandwidth(N, 5, 2) == (N + 1) * 10 - 1


def test_band_offset_is_column_innermost_and_a_bijection():
    S = cm.systemsolvers
    n, p, q, ncol = 30, 9, 9, 7
    P = p + q + 1
    seen = np.zeros(n * P * ncol, dtype=np.int64)
    for col in range(n):
        for d in range(P):
            for c in range(ncol):
                o = S.band_offset(c, col, d, n, p, q, ncol)
                seen[o] += 1
                if c:
                    assert o == S.band_offset(c - 1, col, d, n, p, q, ncol) + 1
    assert np.all(seen == 1)
    assert S.band_bytes(ncol, n, p, q) == seen.size * 8
    # the bench Held-Suarez sphere (estimate quoted in DESIGN.md): 6 x 30 x 30 stacks x 25 columns,
    # n = 5 x 5 x 8 = 200, p = q = 24 -> 10.58 GB
    assert S.band_bytes(6 * 30 * 30 * 25, 200, 24, 24) == 10_584_000_000


def test_isothermal_profile_and_linear_model_refusals():
    A = cm.atmos
    ps = A.PlanetParameters()
    prof = A.IsothermalProfile(ps, 300.0)
    z = np.array([0.0, 5e3, 10e3])
    T, p = prof(z)
    assert np.all(T == 300.0)
    assert p[0] == ps.MSLP
    np.testing.assert_allclose(p, ps.MSLP * np.exp(-ps.grav * z / (ps.R_d * 300.0)), rtol=1e-15)
    no_ref = A.DryAtmosModel(None, orientation=A.ORIENT_SPHERICAL, sources=A.SRC_GRAVITY)
    with pytest.raises(ValueError):
        A.AtmosAcousticGravityLinearModel(no_ref)
    full = A.DryAtmosModel(None, orientation=A.ORIENT_SPHERICAL, ref_state=prof,
                           sources=A.SRC_GRAVITY, boundary_conditions=(1, 1))
    lin = A.AtmosAcousticGravityLinearModel(full)
    assert (lin.ns, lin.naux) == (5, full.naux)
    assert lin.physics_id == 10
    ip, dp = lin.descriptor()
    assert np.array_equal(ip, full.descriptor()[0])
