"""HydrostaticBoussinesq and ShallowWater at the compiled orders other than 4 (N = 2, 3, 5; every
test of test_gpu_ocean.py and test_gpu_split_explicit.py runs at N = 4): tendency and hooks, wall
boundary conditions under LSRK54, Courant numbers, the fused column operators (k_column_chain<NQ, 2>,
k_flow_deviation<NQ> at NQ = 3, 4, 6), the split-explicit exchange and steps, one partition, and
the column composition against closed forms at N = 2..5.  The bodies are those of the N = 4 tests
(ocean_orders_cases.py).  ``-m gpu``."""
import numpy as np
import pytest

from helpers import rel_linf, split_explicit_setup
from ocean_orders_cases import (ANALYTIC_ORDERS, EPS, PKIN_BOUND, TOL, W_ORACLE_BOUND, analytic_errors,
                                analytic_ocean_case, centre_stack, check_exchange_functions,
                                check_fused_columns_equal_sequence, check_ocean_courant,
                                check_ocean_multirank_matches_single_rank, check_ocean_tendency_and_aux,
                                check_split_explicit_steps, close_ocean_model, oracle_ocean_model, to_gpu,
                                walled_box)

pytestmark = pytest.mark.gpu
ORDERS = (2, 3, 5)


@pytest.mark.parametrize("variant", ["spindown", "advection_rotating"])
@pytest.mark.parametrize("N", ORDERS)
def test_ocean_tendency_and_aux_match_oracle_at_order(cm, oracle, torch, N, variant):
    check_ocean_tendency_and_aux(cm, oracle, torch, variant, N=N, alpha_beta=((1.0, 1.0), (0.5, 2.0)))


@pytest.mark.parametrize("box", ["gyre", "windstress"])
@pytest.mark.parametrize("N", ORDERS)
def test_walled_boxes_match_oracle_at_order(cm, oracle, torch, N, box):
    """No-slip walls and floor, free-slip floor, kinematic stress and temperature flux at the
    surface: one evaluation and two LSRK54 steps with the law's hooks."""
    law, grid = walled_box(box, N)
    odg = oracle_ocean_model(cm, oracle, law, grid)
    dg = cm.dgmodel.DGModel(law, grid)
    keep = cm.ocean.install_hydrostatic_boussinesq_hooks(dg)
    Q0 = law.init_state_prognostic(grid, odg.state_auxiliary, 0.0)
    rng = np.random.default_rng(2)
    Q0[:, 0:2] = 0.05 * rng.standard_normal(Q0[:, 0:2].shape)
    Q0[:, 2] = 0.1 * rng.standard_normal(Q0[:, 2].shape)
    To = np.zeros_like(Q0)
    odg(To, Q0.copy(), 0.0, 1.0, 0.0)
    Tg = to_gpu(torch, np.zeros_like(Q0))
    dg(Tg, to_gpu(torch, Q0), 0.0, 1.0, 0.0)
    Tn = Tg.cpu().numpy()
    for s in range(4):
        assert rel_linf(Tn[:, s], To[:, s]) < TOL, s
    dt = 60.0
    Qo, dQo = Q0.copy(), np.zeros_like(Q0)
    for i in range(2):
        oracle.lsrk54_step(odg, Qo, dQo, i * dt, dt)
    Q = to_gpu(torch, Q0)
    dQ = torch.zeros_like(Q)
    dg.lsrk_run(Q, dQ, 0.0, dt, 2, oracle.RKA, oracle.RKB, oracle.RKC)
    dg.synchronize()
    Qn = Q.cpu().numpy()
    assert np.isfinite(Qo).all()
    for s in range(4):
        assert rel_linf(Qn[:, s], Qo[:, s]) < TOL, s
    close_ocean_model(dg, keep)


@pytest.mark.parametrize("N", ORDERS)
def test_ocean_courant_numbers_match_oracle_at_order(cm, oracle, torch, N):
    check_ocean_courant(cm, oracle, torch, *walled_box("gyre", N))


@pytest.mark.parametrize("N", ORDERS)
def test_fused_column_operators_equal_the_recorded_sequence_at_order(cm, torch, monkeypatch, N):
    check_fused_columns_equal_sequence(
        cm, torch, monkeypatch,
        [lambda: walled_box("gyre", N), lambda: split_explicit_setup(True, Nx=3, Ny=2, Nz=3, N=N)[:2]])


@pytest.mark.parametrize("N", ORDERS)
def test_exchange_functions_match_oracle_at_order(cm, oracle, torch, N):
    check_exchange_functions(cm, oracle, torch, N=N)


@pytest.mark.parametrize("N", ORDERS)
def test_split_explicit_steps_match_oracle_at_order(cm, oracle, torch, N):
    check_split_explicit_steps(cm, oracle, torch, True, 300.0, N=N)


@pytest.mark.parametrize("N", ORDERS)
def test_two_node_extrusion_is_refused_at_other_orders(cm, torch, N):
    """The barotropic model on a two-node extrusion is compiled next to N = 4 only."""
    law2, g2 = split_explicit_setup(True, Nx=3, Ny=2, Nz=3, N=N, N_extrusion=1)[2:]
    with pytest.raises(cm._lib.CmdgError) as err:
        cm.dgmodel.DGModel(law2, g2, numerical_flux_first_order=cm.balancelaws.CentralNumericalFluxFirstOrder)
    assert "mixed polynomial orders compiled in: (4, 1)" in str(err.value), str(err.value)


def test_ocean_local_multirank_matches_single_rank_at_order_3(cm, torch):
    """The hooks on ghost stacks need nghost % nvertelem == 0: halos of Np = 64 elements."""
    grids = check_ocean_multirank_matches_single_rank(cm, torch, N=3)
    assert all(g.nelem > g.nreal and (g.nelem - g.nreal) % 3 == 0 for g in grids)


@pytest.mark.parametrize("box", ["gyre", "windstress"])
@pytest.mark.parametrize("N", ANALYTIC_ORDERS)
def test_column_composition_equals_closed_forms(cm, oracle, torch, N, box):
    """The inputs of tests/test_ocean_orders_host.py: w, wz0 and pkin of the centre stack at 1e-12
    of the oracle and within the host test's bounds of the closed forms."""
    law, grid = walled_box(box, N)
    odg = oracle_ocean_model(cm, oracle, law, grid)
    Q, w, wz0, pkin = analytic_ocean_case(law, grid, N)
    stack = centre_stack(grid)
    odg(np.zeros_like(Q), Q.copy(), 0.0, 1.0, 0.0)
    dg = cm.dgmodel.DGModel(law, grid)
    keep = cm.ocean.install_hydrostatic_boussinesq_hooks(dg)
    dg(to_gpu(torch, np.zeros_like(Q)), to_gpu(torch, Q), 0.0, 1.0, 0.0)
    dg.synchronize()
    auxg = dg.state_auxiliary.cpu().numpy()
    close_ocean_model(dg, keep)
    err = analytic_errors(auxg, stack, w, wz0, pkin)
    print("N = %d %s: device against closed forms, w %.1e wz0 %.1e (of max|w|), pkin %.1f eps"
          % (N, box, err["w"], err["wz0"], err["pkin"] / EPS))
    for c, name in ((1, "w"), (2, "pkin"), (3, "wz0")):
        sc = np.abs(odg.state_auxiliary[stack, c]).max()
        assert np.abs(auxg[stack, c] - odg.state_auxiliary[stack, c]).max() / sc < TOL, name
    assert err["w"] < W_ORACLE_BOUND and err["wz0"] < W_ORACLE_BOUND, err
    assert err["pkin"] < PKIN_BOUND, err
