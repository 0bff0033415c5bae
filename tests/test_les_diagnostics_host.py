"""The NumPy restatement of the AtmosLESDefault diagnostics group (les_diagnostics_restatement.py)
against the reference's known answer, test/Diagnostics/sin_test.jl (``u = 5`` and ``cov_w_u = 0.5`` on
every level), and against hand-checkable cases.  The auxiliary state and the gradient flux come from
the CPU oracle's evaluation of the model.  CPU only."""
import numpy as np
import pytest

import les_diagnostics_restatement as R
from cmdg_loader import cm
from helpers import bomex_setup


def _evaluated(oracle, law, grid, Q):
    dg = oracle.OracleDGModel(law, grid)
    T = np.zeros_like(Q)
    dg(T, Q, 0.0, 1.0, 0.0)
    return dg.state_auxiliary, dg.state_gradient_flux


# three elements per direction is the smallest count at which the composite GLL rule integrates
# sin^2 over the 1500 m box (two alias it: cov_w_u is off by 9e-7)
@pytest.mark.parametrize("n", [3, 4])
def test_sine_state_gives_the_reference_known_answer(oracle, n):
    """sin_test.jl:170-190: sum over levels of (u - 5)^2 <= 1e-16, rms(cov_w_u - 0.5) <= 2e-15."""
    law, grid = bomex_setup(nx=n, ny=n, nz=2, N=4, L=1500.0)
    aux0 = law.init_state_auxiliary(grid)
    Q = R.sine_state(law, grid, aux0)
    aux, gf = _evaluated(oracle, law, grid, Q)
    out = R.collect(law, grid, Q, aux, gf)
    du, dc = out["u"] - 5.0, out["cov_w_u"] - 0.5
    print("n = %d: max |u - 5| = %.2e, max |cov_w_u - 0.5| = %.2e" % (n, np.abs(du).max(), np.abs(dc).max()))
    assert (du ** 2).sum() <= 1e-16
    assert np.sqrt((dc ** 2).mean()) <= 2e-15
    # the other means: a sequential sum of m = 25 n^2 nodes is off by at most m eps of its magnitude
    b = 25 * n * n * np.finfo(float).eps
    assert np.abs(out["v"] - 5.0).max() <= b * 5 and np.abs(out["w"] - 10.0).max() <= b * 10
    assert np.abs(out["avg_rho"] - 1.0).max() <= b
    assert list(out)[:5] == ["z", "u", "v", "w", "avg_rho"] and list(out)[-7:-1] == [
        "cld_frac", "cld_top", "cld_base", "cld_cover", "lwp", "iwp"]


def test_level_constant_state_has_no_variance(oracle):
    """The BOMEX initial state depends on z alone: every fluctuation is a rounding error of the level
    mean, at most 2 n eps |x| for a sequential sum of n nodes, so a variance is at most its square."""
    law, grid = bomex_setup(nx=3, ny=3, nz=2, N=4, L=1500.0)
    aux0 = law.init_state_auxiliary(grid)
    Q = law.init_state_prognostic(grid, aux0, 0.0)
    aux, gf = _evaluated(oracle, law, grid, Q)
    out = R.collect(law, grid, Q, aux, gf)
    n = 9 * 25
    b = 2 * n * np.finfo(float).eps
    assert np.abs(out["var_u"]).max() <= (b * 8.75) ** 2
    assert np.abs(out["var_v"]).max() == 0.0 and np.abs(out["var_w"]).max() == 0.0
    assert np.abs(out["tke"]).max() <= (b * 8.75) ** 2
    assert np.abs(out["var_ei"]).max() <= (b * np.abs(out["ei"]).max()) ** 2
    assert np.abs(out["cov_w_u"]).max() == 0.0


def test_onetime_collection_matches_the_horizontal_integral_test():
    """zvals and MH_z on the warped brick of test_horizontal_integral.py: the level's last node and
    the denominators of its level means."""
    import test_horizontal_integral as H

    def warp(a, b, c):
        return (np.sin(2 * np.pi * c) / 16 + a, b + (b - 1 / 2) * np.cos(2 * np.pi * b * c) / 4,
                c + np.sin(2 * np.pi * a) / 20)
    grid = H._warped_brick(warp)
    zvals, MH_z = R.onetime(grid)
    _, K = H._level_means(grid)
    MH = grid.vgeo[:grid.nreal, cm.mesh.grids._MH, :].reshape(-1, H.Nq, H.Nq * H.Nq)
    assert np.array_equal(zvals, K)
    assert np.allclose(MH_z, MH.sum(axis=(0, 2)), rtol=1e-14, atol=0)


def test_cloud_top_and_base_are_nan_without_condensate(oracle):
    MO = cm.moist
    _, grid = bomex_setup(nx=3, ny=3, nz=2, N=4, L=1500.0)
    ps = MO.MoistParameters()
    ref = cm.atmos.DecayingTemperatureProfile(ps, 290.0, 220.0, ps.R_d * 290.0 / ps.grav)
    law = MO.MoistAtmosModel(MO.DensityCurrentSetup(ps), ref, closure=MO.CLOSURE_CONSTANT, coefficient=75.0,
                             param_set=ps)
    aux0 = law.init_state_auxiliary(grid)
    Q = law.init_state_prognostic(grid, aux0, 0.0)
    aux, gf = _evaluated(oracle, law, grid, Q)
    out = R.collect(law, grid, Q, aux, gf)
    assert np.isnan(out["cld_top"]) and np.isnan(out["cld_base"])
    assert out["cld_cover"] == 0.0 and np.all(out["cld_frac"] == 0.0) and out["lwp"] == 0.0 and out["iwp"] == 0.0
