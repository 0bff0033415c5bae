"""The ocean law's column composition (update_auxiliary_state_gradient! of
hydrostatic_boussinesq_model.jl: A.w = -D.div_h u, upward integrals for w and pkin, the reverse
integral of pkin, the surface w through the column) against closed forms, N = 2..5: a third witness
next to the device and its oracle twin, which restate the composition alike.  The velocity is a
product of polynomials the filters leave alone, so w, wz0 and pkin on a stack without wall faces
are known in long double (ocean_orders_cases.analytic_ocean_case).  CPU only."""
import numpy as np
import pytest

from ocean_orders_cases import (ANALYTIC_ORDERS, EPS, PKIN_BOUND, W_ORACLE_BOUND, analytic_errors,
                                analytic_ocean_case, centre_stack, oracle_ocean_model, walled_box)


@pytest.mark.parametrize("box", ["gyre", "windstress"])
@pytest.mark.parametrize("N", ANALYTIC_ORDERS)
def test_oracle_column_composition_equals_closed_forms(cm, oracle, N, box):
    """w and wz0 within 1e-11 of max|w| on the centre stack (the error is the differentiation of
    coordinates of 1e6 m), pkin within 64 eps of max|pkin| (two column kernels on an integrand
    without vertical structure).  Observed maxima: DESIGN.md section 5."""
    law, grid = walled_box(box, N)
    odg = oracle_ocean_model(cm, oracle, law, grid)
    Q, w, wz0, pkin = analytic_ocean_case(law, grid, N)
    stack = centre_stack(grid)
    Q0 = Q.copy()
    odg(np.zeros_like(Q), Q, 0.0, 1.0, 0.0)
    # the filters keep this state: vertical degree N - 2 under the cutoff, no vertical structure in theta
    assert np.abs(Q - Q0).max() < 64 * EPS * np.abs(Q0).max()
    err = analytic_errors(odg.state_auxiliary, stack, w, wz0, pkin)
    print("N = %d %s: oracle against closed forms, w %.1e wz0 %.1e (of max|w|), pkin %.1f eps"
          % (N, box, err["w"], err["wz0"], err.get("pkin", 0.0) / EPS))
    assert np.abs(w[stack]).max() > 1e-5          # a vertical velocity worth the name
    assert err["w"] < W_ORACLE_BOUND and err["wz0"] < W_ORACLE_BOUND, err
    assert law.alpha_T != 0 and err["pkin"] < PKIN_BOUND, err
