"""The column kernels of csrc/columns.h (k_stack_integral<NQ, NOUT>, k_reverse_stack_integral<NQ,
NOUT>) at every compiled NQ = 2..8 and NOUT = 1..4: bit for bit against the oracle, and against the
exact antiderivatives of tests/test_integrals_orders_host.py directly, so that a shared error and a
bitwise difference can be told apart from the log.  nvert = 1 (no prefetch), partly filled last
blocks at every SPB = 256 // NQ^2, integration in place, NaN wherever nothing may write.  ``-m gpu``."""
import numpy as np
import pytest

from ocean_orders_cases import (COL_F, EPS, INTEGRAL_BOUND, INTEGRAL_NVERT, INTEGRAL_ORDERS, MANY_NAUX,
                                MANY_NS, column_grid, column_law, integral_errors, integral_stack_counts,
                                many_output_case, one_output_aux, one_output_fields,
                                polynomial_column_case, stacks_per_block, to_gpu)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("nvert", INTEGRAL_NVERT)
@pytest.mark.parametrize("N", INTEGRAL_ORDERS)
def test_stack_integrals_equal_oracle_and_exact_antiderivatives(cm, oracle, torch, N, nvert):
    src, scale, dst, rsrc, rdst = one_output_fields()
    for nstacks in integral_stack_counts(N):
        grid = column_grid(cm, N, nvert, nstacks)
        f, up, rev = polynomial_column_case(grid, N)
        aux0 = one_output_aux(grid, f)
        auxo = aux0.copy()
        fl = oracle.integral_fields_law(src, scale, dst, rsrc, rdst, 0, aux0.shape[1])
        og = oracle.OracleGrid(grid)
        oracle.indefinite_stack_integral(fl, og, None, auxo)
        oracle.reverse_indefinite_stack_integral(fl, og, None, auxo)
        dg = cm.dgmodel.DGModel(column_law(cm), grid)
        aux = to_gpu(torch, aux0)
        dg.indefinite_stack_integral(None, aux, src, dst, scale=scale)
        dg.reverse_indefinite_stack_integral(aux, rsrc, rdst)
        dg.synchronize()
        auxg = aux.cpu().numpy()
        dg.close()
        eu, er = integral_errors(auxg, grid.nreal, up, rev)
        print("N = %d nvert = %d stacks = %d: device against closed forms %.1f eps (upward) %.1f eps "
              "(reverse)" % (N, nvert, nstacks, eu, er))
        bits = np.array_equal(auxg, auxo, equal_nan=True)
        assert eu * EPS < INTEGRAL_BOUND and er * EPS < INTEGRAL_BOUND, (nstacks, eu, er, bits)
        assert bits, (nstacks, np.nanmax(np.abs(auxg - auxo)))       # same order of operations
        assert np.array_equal(auxg[:, COL_F], f) and np.isnan(auxg[:, COL_F + 1:]).all()


@pytest.mark.parametrize("nout", [2, 3, 4, 6])
@pytest.mark.parametrize("N", INTEGRAL_ORDERS)
def test_many_outputs_in_place_equal_oracle(cm, oracle, torch, N, nout):
    """State and auxiliary integrands, scales -2 and 1e-3, output 1 integrated over its own
    integrand's column and output 0 reversed in place (the case the kernels' load / store order is
    written for); 6 outputs = one launch of 4 and one of 2.  Columns nobody names stay NaN."""
    grid = column_grid(cm, N, 2, stacks_per_block(N) + 1)
    Q0, aux0, src, scale, dst, rdst, untouched = many_output_case(grid, nout)
    og = oracle.OracleGrid(grid)
    auxo = aux0.copy()
    fl = oracle.integral_fields_law(src, scale, dst, dst, rdst, MANY_NS, MANY_NAUX)
    oracle.indefinite_stack_integral(fl, og, Q0, auxo)
    oracle.reverse_indefinite_stack_integral(fl, og, Q0, auxo)
    dg = cm.dgmodel.DGModel(column_law(cm), grid)
    aux = to_gpu(torch, aux0)
    dg.indefinite_stack_integral(to_gpu(torch, Q0), aux, src, dst, scale=scale)
    dg.reverse_indefinite_stack_integral(aux, dst, rdst)
    dg.synchronize()
    auxg = aux.cpu().numpy()
    dg.close()
    assert np.isfinite(auxo[:, dst + rdst]).all() and np.abs(auxo[:, dst]).max() > 0
    assert np.array_equal(auxg, auxo, equal_nan=True), np.nanmax(np.abs(auxg - auxo))
    assert np.isnan(auxg[:, untouched]).all()


@pytest.mark.parametrize("N", [2, 5, 6])
def test_ghost_stacks_are_left_alone(cm, oracle, torch, N):
    """Rank 0 of 2: the integrals walk the real stacks; the ghost elements behind them keep their
    NaN in every column."""
    spb = stacks_per_block(N)
    grid = column_grid(cm, N, 2, 2 * (spb + 1), rank=0, size=2)
    assert grid.nelem > grid.nreal and grid.nreal % 2 == 0
    src, scale, dst, rsrc, rdst = one_output_fields()
    f, up, rev = polynomial_column_case(grid, N)
    aux0 = one_output_aux(grid, f)
    aux0[grid.nreal:] = np.nan
    auxo = aux0.copy()
    fl = oracle.integral_fields_law(src, scale, dst, rsrc, rdst, 0, aux0.shape[1])
    og = oracle.OracleGrid(grid)
    oracle.indefinite_stack_integral(fl, og, None, auxo)
    oracle.reverse_indefinite_stack_integral(fl, og, None, auxo)
    dg = cm.dgmodel.DGModel(column_law(cm), grid)
    aux = to_gpu(torch, aux0)
    dg.indefinite_stack_integral(None, aux, src, dst, scale=scale)
    dg.reverse_indefinite_stack_integral(aux, rsrc, rdst)
    dg.synchronize()
    auxg = aux.cpu().numpy()
    dg.close()
    eu, er = integral_errors(auxg, grid.nreal, up, rev)
    assert eu * EPS < INTEGRAL_BOUND and er * EPS < INTEGRAL_BOUND, (eu, er)
    assert np.array_equal(auxg, auxo, equal_nan=True)
    assert np.isnan(auxg[grid.nreal:]).all()


# the recorded composition on the advection-diffusion handle (15 auxiliary columns: coordinates, velocity,
# diffusion tensor): a scaled gradient-flux column copied into the column that is integrand and result
# of output 0, a state integrand, an auxiliary integrand (the velocity), a scale of 1e-3; output 1
# reversed in place; the surface value of output 0 through the column into a column of its own
CHAIN_COPY = (0, 6, -1.5)
CHAIN_SRC = [(0, 6), (1, 0), (0, 3), (1, 0)]
CHAIN_SCALE = [1.0, -2.0, 0.5, 1e-3]
CHAIN_DST = [6, 7, 8, 9]
CHAIN_SURF = (6, 10)


@pytest.mark.parametrize("nout", [1, 2, 3, 4])
@pytest.mark.parametrize("N", INTEGRAL_ORDERS)
def test_column_chain_equals_the_sequence_and_the_oracle(cm, oracle, torch, monkeypatch, N, nout):
    """k_column_chain<NQ, NOUT> at every compiled NQ and NOUT (the ocean laws record NOUT = 2 at
    NQ = 3..6 only): one evaluation with CMDG_FUSED_COLUMNS = 2 against 0, tendency and auxiliary
    state bit for bit, and the auxiliary state bit for bit against the composition spelled out with
    the oracle's integrals from the device's own gradient flux."""
    nvert = 5
    grid = column_grid(cm, N, nvert, stacks_per_block(N) + 1)
    law = column_law(cm)
    src, scale, dst = CHAIN_SRC[:nout], CHAIN_SCALE[:nout], CHAIN_DST[:nout]
    rev = [dst[1]] if nout > 1 else []
    aux0 = law.init_state_auxiliary(grid)
    Q0 = np.random.default_rng(N).standard_normal((grid.nelem, 1, grid.Np))
    res = []
    for fused in ("0", "2"):
        monkeypatch.setenv("CMDG_FUSED_COLUMNS", fused)
        dg = cm.dgmodel.DGModel(law, grid, state_auxiliary=aux0.copy())
        dg.set_rhs_hooks(gradflux_to_aux=[CHAIN_COPY], integral=dict(src=src, scale=scale, dst=dst),
                         reverse_integral=dict(rsrc=rev, rdst=rev) if rev else None,
                         surface_to_column=[CHAIN_SURF])
        T = to_gpu(torch, np.zeros_like(Q0))
        dg(T, to_gpu(torch, Q0), 0.0, 1.0, 0.0)
        dg.synchronize()
        res.append((T.cpu().numpy(), dg.state_auxiliary.cpu().numpy(), dg.state_gradient_flux.cpu().numpy()))
        dg.set_rhs_hooks()
        dg.close()
    (T0, A0, G0), (T2, A2, G2) = res
    assert np.isfinite(T0).all() and np.isfinite(A0).all()
    assert np.array_equal(G0, G2) and np.array_equal(A0, A2) and np.array_equal(T0, T2)
    # the composition on the host
    A = aux0.copy()
    A[:, CHAIN_COPY[1]] = CHAIN_COPY[2] * G0[:, CHAIN_COPY[0]]
    og = oracle.OracleGrid(grid)
    fl = oracle.integral_fields_law(src, scale, dst, dst, dst, 1, A.shape[1])
    oracle.indefinite_stack_integral(fl, og, Q0, A)
    if rev:
        rl = oracle.integral_fields_law([(0, rev[0])], [1.0], rev, rev, rev, 1, A.shape[1])
        oracle.reverse_indefinite_stack_integral(rl, og, Q0, A)
    Nij = grid.Nq[0] * grid.Nq[1]
    A5 = A.reshape(grid.nelem // nvert, nvert, A.shape[1], grid.Nq[2], Nij)
    A5[:, :, CHAIN_SURF[1]] = A5[:, -1, CHAIN_SURF[0], -1, :][:, None, None, :]
    assert np.abs(A[:, dst]).max() > 0 and not np.array_equal(A[:, CHAIN_SURF[1]], aux0[:, CHAIN_SURF[1]])
    assert np.array_equal(A2, A), np.abs(A2 - A).max()
