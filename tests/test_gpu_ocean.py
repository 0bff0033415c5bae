"""Hydrostatic Boussinesq ocean model on the GPU: right-hand side with the law's
update_auxiliary_state! / update_auxiliary_state_gradient! hooks (filters, column integrals)
against the oracle, multi-rank against single-rank, and the reference's regression
(test_3D_spindown.jl + StateCheck refvals) run end to end on the device.  ``-m gpu``."""
import numpy as np
import pytest

from helpers import (ocean_gyre_setup, ocean_spindown_setup, ocean_windstress_setup, rel_linf,
                     split_explicit_setup)
from ocean_orders_cases import (check_fused_columns_equal_sequence, check_ocean_courant,
                                check_ocean_multirank_matches_single_rank, check_ocean_tendency_and_aux)
from test_ocean_oracle import GOLD, GYRE, WIND, check_against_refvals, check_gyre_refvals

pytestmark = pytest.mark.gpu
TOL = 1e-12


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "no HIP device: the product path has no CPU fallback"
    return t


def _gpu(torch, a):
    x = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return x


@pytest.mark.parametrize("variant", ["spindown", "advection_rotating"])
def test_ocean_tendency_and_aux_match_oracle(cm, oracle, torch, variant):
    check_ocean_tendency_and_aux(cm, oracle, torch, variant)


def test_ocean_local_multirank_matches_single_rank(cm, torch):
    check_ocean_multirank_matches_single_rank(cm, torch)


def test_spindown_reference_regression_on_the_gpu(cm, torch):
    """test_3D_spindown.jl end to end: 720 LSRK144 steps, error against the analytic solution
    and the StateCheck table."""
    O = cm.ocean
    law, grid = ocean_spindown_setup()
    dg = cm.dgmodel.DGModel(law, grid)
    keep = O.install_hydrostatic_boussinesq_hooks(dg)
    Q = dg.init_ode_state(0.0)
    solver = cm.odesolvers.LSRK144NiegemannDiehlBusch(dg, Q, dt=120.0)
    solver.dostep(Q, nsteps=720)
    dg.synchronize()
    Qe = dg.init_ode_state(86400.0)
    err = dg.euclidean_distance(Q, Qe) / dg.norm(Qe)
    assert err < 0.005
    assert abs(err - GOLD["error_printed_by_reference"]) < 1e-10
    check_against_refvals(Q.cpu().numpy(), dg.state_auxiliary.cpu().numpy(), rtol=5e-12)
    dg.set_rhs_hooks()
    for f in keep:
        f.close()
    dg.close()


def test_ocean_gyre_short_reference_regression_on_the_gpu(cm, oracle, torch):
    """test_ocean_gyre_short.jl end to end on the device + tendency parity with the oracle for
    the wind-stress / temperature-flux / no-slip boundary conditions."""
    O, F = cm.ocean, cm.mesh.filters
    law, grid = ocean_gyre_setup()
    dg = cm.dgmodel.DGModel(law, grid)
    keep = O.install_hydrostatic_boussinesq_hooks(dg)
    odg = oracle.OracleDGModel(law, grid)
    oracle.hydrostatic_boussinesq_hooks(odg, F.CutoffFilter(grid, 3), F.ExponentialFilter(grid, 1, 8))
    Q0 = law.init_state_prognostic(grid, odg.state_auxiliary, 0.0)
    rng = np.random.default_rng(2)
    Q0[:, 0:2] = 0.05 * rng.standard_normal(Q0[:, 0:2].shape)
    Q0[:, 2] = 0.1 * rng.standard_normal(Q0[:, 2].shape)
    To = np.zeros_like(Q0)
    odg(To, Q0.copy(), 0.0, 1.0, 0.0)
    Tg = _gpu(torch, np.zeros_like(Q0))
    dg(Tg, _gpu(torch, Q0), 0.0, 1.0, 0.0)
    Tn = Tg.cpu().numpy()
    for s in range(4):
        assert rel_linf(Tn[:, s], To[:, s]) < TOL, s
    Q = dg.init_ode_state(0.0)
    solver = cm.odesolvers.LSRK144NiegemannDiehlBusch(dg, Q, dt=120.0)
    solver.dostep(Q, nsteps=30)
    dg.synchronize()
    assert check_gyre_refvals(Q.cpu().numpy(), dg.state_auxiliary.cpu().numpy()) == 32
    dg.set_rhs_hooks()
    for f in keep:
        f.close()
    dg.close()


def test_windstress_short_reference_regression_on_the_gpu(cm, torch):
    O = cm.ocean
    law, grid = ocean_windstress_setup()
    dg = cm.dgmodel.DGModel(law, grid)
    keep = O.install_hydrostatic_boussinesq_hooks(dg)
    Q = dg.init_ode_state(0.0)
    solver = cm.odesolvers.LSRK144NiegemannDiehlBusch(dg, Q, dt=180.0)
    solver.dostep(Q, nsteps=20)
    dg.synchronize()
    table = [r for r in WIND["explicit_cpu"] if r[1] != "θ"]
    assert check_gyre_refvals(Q.cpu().numpy(), dg.state_auxiliary.cpu().numpy(), table=table, rtol=2e-11) == 28
    dg.set_rhs_hooks()
    for f in keep:
        f.close()
    dg.close()


def test_ocean_courant_numbers_and_dt_match_oracle(cm, oracle, torch):
    """src/Ocean/HydrostaticBoussinesq/Courant.jl: the four local Courant numbers in the
    directions calculate_dt uses them, and the resulting time step."""
    check_ocean_courant(cm, oracle, torch, *ocean_gyre_setup())


def test_ocean_gyre_long_reference_regression_on_the_gpu(cm, torch):
    """test_ocean_gyre_long.jl: 20^3 elements, 4e6 x 4e6 x 1000 m, one simulated day of explicit
    LSRK144 steps with dt = calculate_dt(Courant number 0.4) adjusted to divide the day (620
    steps of 139.35 s), against the `long` StateCheck rows."""
    O = cm.ocean
    law, grid = ocean_gyre_setup(Nx=20, Ny=20, Nz=20, L=4e6)
    dg = cm.dgmodel.DGModel(law, grid)
    keep = O.install_hydrostatic_boussinesq_hooks(dg)
    Q = dg.init_ode_state(0.0)
    dt = law.calculate_dt(lambda k, d: dg.courant(k, Q, 1.0, 0.0, d), 0.4)
    nsteps = int(np.ceil(86400.0 / dt))            # solver_configs.jl:247-249
    assert nsteps == 620
    dt = 86400.0 / nsteps
    solver = cm.odesolvers.LSRK144NiegemannDiehlBusch(dg, Q, dt=dt)
    solver.dostep(Q, nsteps=nsteps)
    dg.synchronize()
    n = check_gyre_refvals(Q.cpu().numpy(), dg.state_auxiliary.cpu().numpy(), rtol=1e-10,
                           table=GYRE["long"])
    assert n == 32
    dg.set_rhs_hooks()
    for f in keep:
        f.close()
    dg.close()


def test_fused_column_operators_equal_the_recorded_sequence(cm, torch, monkeypatch):
    """The column operators of the recorded update_auxiliary_state_gradient! composition run as
    one launch (columns.h k_column_chain: copy + upward integrals + reverse integral + surface
    value) and the flow deviation as one (k_flow_deviation); CMDG_FUSED_COLUMNS=0 issues them one
    by one.  Same arithmetic in the same order: state and every auxiliary column bit for bit,
    for the uncoupled gyre and for the coupled box with its flow deviation."""
    check_fused_columns_equal_sequence(
        cm, torch, monkeypatch,
        [ocean_gyre_setup, lambda: split_explicit_setup(True, Nx=4, Ny=3, Nz=3)[:2]])
