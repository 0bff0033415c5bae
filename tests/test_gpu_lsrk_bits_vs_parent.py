"""What ``cmdg_lsrk_run`` leaves in the caller's arrays keeps the bits recorded before the
instruction diet of the fused tendency + LSRK update (uniform quotients of the parameter block moved
to the host, see AtmosParams / test_atmos_params_host_constants.py): Q, dQ and the two refreshed
auxiliary columns (moisture.theta_v, air_T) after 3 LSRK54 steps, ``array_equal`` against the
fixtures under tests/golden/lsrk_bits_*.npz, with the gradient-argument hand-off on and off.

Cases (the smallest at which each code path exists):
  hs_2x2x2  Held-Suarez, 6x2x2x2 stacked cubed sphere (48 elements, N = 4, dt = 0.15, the
            benchmark's law and the perturbation of bench.parity_check): cube-edge neighbours, both
            boundary levels, no interior level;
  hs_2x2x3  the same with 3 levels (72 elements): one interior level;
  rb_2x2x2  dry rising bubble, 2x2x2 brick, dt = 0.01: SmagorinskyLilly (USE_GF = true, no
            hand-off), so a second instantiation reads the changed parameter block.
The fixtures come from scripts/make_golden_lsrk_bits.py (tests/golden/README_lsrk_bits.txt says on
which commit); on that commit the two hand-off settings gave the same bits, so one array set per
case serves both.
"""
import argparse
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 20250117  # bench.parity_check
NSTEPS = 3
CASES = ("hs_2x2x2", "hs_2x2x3", "rb_2x2x2")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def fixture_path(case):
    return os.path.join(GOLDEN, "lsrk_bits_%s.npz" % case)


def _setup(cm, case):
    """(law, grid, (direction, diffusion_direction), dt, perturb)"""
    if case.startswith("hs_"):
        import bench
        nvert = int(case[-1])
        args = argparse.Namespace(nhorz=None, nvert=8, scaling="weak", connectivity="full")
        law, grid, direction, dt, _ = bench.build_workload(cm, "heldsuarez", 0, 1, 4, args,
                                                           nhorz=2, nvert=nvert)
        assert grid.nreal == grid.nelem == 6 * 2 * 2 * nvert and dt == 0.15
        return law, grid, direction, dt, True
    from helpers import rising_bubble_setup
    law, grid = rising_bubble_setup(nx=2, ny=2, nz=2)
    return law, grid, (0, 0), 0.01, False


def run_case(cm, torch, case, handoff):
    """3 LSRK54 steps through cmdg_lsrk_run on a fresh handle: float64 Q, dQ and the two refreshed
    auxiliary columns as the call leaves them, and whether the run took the hand-off."""
    law, grid, direction, dt, perturb = _setup(cm, case)
    dg = cm.dgmodel.DGModel(law, grid, direction=direction[0], diffusion_direction=direction[1],
                            device="cuda:0")
    dg.set_option(cm._lib.OPT_GRADARG_HANDOFF, handoff)
    if perturb:
        Q0 = law.init_state_prognostic(grid, dg.state_auxiliary.cpu().numpy(), 0.0)
        rng = np.random.default_rng(SEED)
        Q0[:, 1:4] += 0.5 * rng.standard_normal(Q0[:, 1:4].shape)
        Q0[:, 4] *= 1 + 1e-3 * rng.standard_normal(Q0[:, 4].shape)
        Q = torch.from_numpy(Q0).to("cuda:0")
    else:
        Q = dg.init_ode_state(0.0)
    solver = cm.odesolvers.LSRK54CarpenterKennedy(dg, Q, dt=dt)
    solver.dostep(Q, nsteps=NSTEPS)
    dg.synchronize()
    out = {"Q": Q.cpu().numpy().astype(np.float64),
           "dQ": solver.dQ.cpu().numpy().astype(np.float64),
           "aux_refreshed": dg.state_auxiliary[:, -2:].cpu().numpy().astype(np.float64)}
    used = dg.query("GRADARG_HANDOFF")
    dg.close()
    assert all(np.isfinite(v).all() for v in out.values())
    return out, used


@pytest.fixture(scope="module")
def golden():
    return {case: dict(np.load(fixture_path(case))) for case in CASES}


@pytest.mark.parametrize("handoff", [1, 0])
@pytest.mark.parametrize("case", CASES)
def test_bits_of_the_recorded_run(cm, torch, golden, case, handoff):
    got, used = run_case(cm, torch, case, handoff)
    assert used == (1 if handoff and case.startswith("hs_") else 0)
    want = golden[case]
    for name in ("Q", "dQ", "aux_refreshed"):
        assert got[name].shape == want[name].shape, name
        # array_equal on the values and on the bit patterns (the sign of a zero counts)
        assert np.array_equal(got[name], want[name]), name
        assert np.array_equal(got[name].view(np.int64), want[name].view(np.int64)), name
