"""The arithmetic of the AtmosGCMDefault diagnostics on the host (tests/gcm_diagnostics_restatement.py, the
reference's operations in NumPy): the reference's own known answer for VectorGradients / Vorticity
(test/Diagnostics/diagnostic_fields_test.jl:185-249) on its own mesh, the same answer for ``vort2`` from
the restated VorticityModel operator, a rigid rotation that can be checked by hand, and the deviations of
the reference's arithmetic from the solid-body rotation's known answer on the small sphere, which bound
the device test."""
import numpy as np
import pytest

import gcm_diagnostics_cases as GC
import gcm_diagnostics_restatement as R
from cmdg_loader import cm

M = cm.mesh
XMAX = GC.XMAX
TOL = 1e-8          # diagnostic_fields_test.jl:137 (Float64)
fcn_grad = GC.fcn_grad


def reference_field(grid):
    return GC.reference_field(grid), GC.coordinates(grid)


def twelve_errors(grid, vgrad, vort, xyz):
    """err[1:12] of :230-246."""
    nr = grid.nreal
    g = [a[:nr] for a in fcn_grad(*xyz)]
    err = [np.abs(g[m] - vgrad[:, 3 * c + m]).max() for c in range(3) for m in range(3)]
    exact = [g[1] - g[2], g[2] - g[0], g[0] - g[1]]
    return err + [np.abs(vort[:, c] - exact[c]).max() for c in range(3)], exact


@pytest.fixture(scope="module")
def reference_mesh():
    """The mesh of the reference's test: [0, 2500]^3, 13 x 13 x 10 elements, N = (4, 5); every side a
    boundary, so that the restated VorticityModel operator closes the weak form with plus = minus."""
    rng = [np.linspace(0.0, XMAX, 14), np.linspace(0.0, XMAX, 14), np.linspace(0.0, XMAX, 11)]
    topl = M.StackedBrickTopology(rng, boundary=((1, 1), (1, 1), (1, 2)), periodicity=(False,) * 3)
    grid = M.DiscontinuousSpectralElementGrid(topl, (4, 4, 5))
    Q, xyz = reference_field(grid)
    return grid, Q, xyz


def test_reference_known_answer(reference_mesh):
    grid, Q, xyz = reference_mesh
    vgrad = R.vector_gradients(grid, Q)
    errs, _ = twelve_errors(grid, vgrad, R.vorticity(vgrad), xyz)
    print("VectorGradients / Vorticity, max errors:", " ".join("%.2e" % e for e in errs))
    assert len(errs) == 12 and max(errs) < TOL, errs


def test_vort2_known_answer(reference_mesh):
    """The field is continuous across faces: the central face terms cancel in the interior, and on the
    boundary plus = minus closes the integration by parts."""
    grid, Q, xyz = reference_mesh
    vort2 = R.vorticity_model_tendency(grid, R.velocity(Q))
    g = [a[:grid.nreal] for a in fcn_grad(*xyz)]
    exact = [g[1] - g[2], g[2] - g[0], g[0] - g[1]]
    errs = [np.abs(vort2[:, c] - exact[c]).max() for c in range(3)]
    print("vort2, max errors: %.2e %.2e %.2e" % tuple(errs))
    assert max(errs) < TOL, errs


def test_rigid_rotation():
    """u = ω × x, ρ = 1 on a 2 x 2 x 2 brick over [-1, 1]^3 at N = 4: d_m u_c = ε_{c a m} ω_a and Ω = 2 ω.
    The field is linear, so the spectral derivative is exact but for rounding.  A reference-space
    derivative sums Nq rounded products: its error is at most (Nq + 1) eps times sum_r |D[i, r]| max|u|;
    the metric combination (2 / h per direction, two of its three terms zero on a brick) adds two more
    roundings and a vorticity component doubles the bound.  Three times that count, in units of the
    largest product, is the tolerance: about 3e-13 |ω| here, against index or sign errors of order |ω|."""
    om = np.array([0.3, -0.7, 1.1])
    rng = [np.linspace(-1.0, 1.0, 3)] * 3
    topl = M.StackedBrickTopology(rng, boundary=((1, 1), (1, 1), (1, 2)), periodicity=(False,) * 3)
    grid = M.DiscontinuousSpectralElementGrid(topl, 4)
    x = np.stack([grid.vgeo[:, c] for c in (M.grids._x1, M.grids._x2, M.grids._x3)], axis=1)
    Q = np.ones((grid.nelem, 5, grid.Np))
    Q[:, 1:4] = np.cross(om[None, :, None], x, axis=1)
    eps, Nq, h = np.finfo(float).eps, 5, 1.0
    lam = np.abs(np.asarray(grid.D[0])).sum(axis=1).max()
    tol = 3 * (Nq + 3) * eps * lam * (2 / h) * np.abs(Q[:, 1:4]).max()
    want = np.zeros((3, 3))                         # want[c][m] = d_m u_c
    want[0, 1], want[0, 2] = -om[2], om[1]
    want[1, 0], want[1, 2] = om[2], -om[0]
    want[2, 0], want[2, 1] = -om[1], om[0]
    vgrad = R.vector_gradients(grid, Q)
    for c in range(3):
        for m in range(3):
            assert np.abs(vgrad[:, 3 * c + m] - want[c, m]).max() <= tol, (c, m)
    vort = R.vorticity(vgrad)
    vort2 = R.vorticity_model_tendency(grid, R.velocity(Q))
    for c in range(3):
        assert np.abs(vort[:, c] - 2 * om[c]).max() <= 2 * tol
        # (the weak form divides by the mass and sums volume and face terms: the same count again)
        assert np.abs(vort2[:, c] - 2 * om[c]).max() <= 4 * tol
    print("rigid rotation: tolerance %.2e, max vgrad error %.2e, vort %.2e, vort2 %.2e" % (
        tol, max(np.abs(vgrad[:, 3 * c + m] - want[c, m]).max() for c in range(3) for m in range(3)),
        np.abs(vort - 2 * om[None, :, None]).max(), np.abs(vort2 - 2 * om[None, :, None]).max()))


def test_solid_body_rotation_deviations_are_the_recorded_ones():
    """gcm_diagnostics_cases.SOLID_BODY_DEVIATION holds what the reference's arithmetic deviates from the
    known answer on the small Held-Suarez sphere; the device test allows four times each."""
    law, grid, it = GC.sphere()
    Q, aux = GC.solid_body_state(law, grid)
    got = R.collect(law, grid, it, Q, aux)
    want = GC.solid_body_expected(law, it)
    assert list(got) == R.NAMES
    for k, w in want.items():
        dev = float(np.abs(got[k] - w).max())
        print("%-6s deviation %.4e (recorded %.3e), magnitude %.4e" % (k, dev, GC.SOLID_BODY_DEVIATION[k], np.abs(w).max()))
        assert GC.SOLID_BODY_DEVIATION[k] / 1.05 <= dev <= GC.SOLID_BODY_DEVIATION[k], k
