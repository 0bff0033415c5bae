"""The oracle's column integrals (integral_oracle.c, what the device must equal bit for bit)
against exact antiderivatives at every order the column kernels are compiled for, N = 1..7: the
integrand is a polynomial of degree N in z times a function of (x, y), so the reference's
quadrature integrates it exactly and a closed form in long double is the expected value.  Uneven
layers, 1 / 2 / 5 elements per stack, stack counts around the 256 // Nq^2 stacks of a device block.
CPU only."""
import numpy as np
import pytest

from cmdg_loader import cm
from ocean_orders_cases import (EPS, INTEGRAL_BOUND, INTEGRAL_NVERT, INTEGRAL_ORDERS, column_grid,
                                integral_errors, integral_stack_counts, one_output_aux,
                                one_output_fields, polynomial_column_case)


@pytest.mark.parametrize("N", INTEGRAL_ORDERS)
def test_oracle_stack_integrals_equal_exact_antiderivatives(oracle, N):
    """Observed on the build host (largest error in eps x max|exact| over nvert and stack count,
    upward / reverse): see DESIGN.md section 5; the bound is 64."""
    src, scale, dst, rsrc, rdst = one_output_fields()
    worst = [0.0, 0.0]
    for nvert in INTEGRAL_NVERT:
        for nstacks in integral_stack_counts(N):
            grid = column_grid(cm, N, nvert, nstacks)
            assert grid.nreal == nstacks * nvert and grid.topology.stacksize == nvert
            f, up, rev = polynomial_column_case(grid, N)
            aux = one_output_aux(grid, f)
            fl = oracle.integral_fields_law(src, scale, dst, rsrc, rdst, 0, aux.shape[1])
            og = oracle.OracleGrid(grid)
            oracle.indefinite_stack_integral(fl, og, None, aux)
            oracle.reverse_indefinite_stack_integral(fl, og, None, aux)
            eu, er = integral_errors(aux, grid.nreal, up, rev)
            worst = [max(worst[0], eu), max(worst[1], er)]
            assert eu * EPS < INTEGRAL_BOUND and er * EPS < INTEGRAL_BOUND, (N, nvert, nstacks, eu, er)
            # the integrand is read, the three spare columns are nobody's
            assert np.array_equal(aux[:, 2], f) and np.isnan(aux[:, 3:]).all()
    print("N = %d: oracle column integrals, worst error %.1f eps (upward) %.1f eps (reverse)"
          % (N, worst[0], worst[1]))


def test_closed_forms_are_consistent():
    """The expected values themselves: upward + reverse = the whole column's integral, the upward
    integral vanishes on the bottom face and the reverse one on the top face."""
    N, nvert = 5, 5
    grid = column_grid(cm, N, nvert, 3)
    f, up, rev = polynomial_column_case(grid, N)
    Nij = grid.Nq[0] * grid.Nq[1]
    up5 = up.reshape(3, nvert, grid.Nq[2], Nij)
    rev5 = rev.reshape(3, nvert, grid.Nq[2], Nij)
    assert not up5[:, 0, 0].any() and not rev5[:, -1, -1].any()
    total = up5[:, -1, -1][:, None, None, :]
    assert np.abs(up5 + rev5 - total).max() < 4 * EPS * np.abs(total).max()
    assert np.abs(f).max() > 0.1
