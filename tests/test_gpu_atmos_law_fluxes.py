"""The dry law's own Roe / HLLC / LMARS fluxes on the device, on moving states with walls
(``-m gpu``): ``DryAtmos<true,true,false,false,true>`` (orientation + hydrostatic reference
state) and ``DryAtmos<false,false,false,false,true>`` (plain) against the CPU oracle at operator
level.  The oracle's pointwise fluxes are pinned to an independent restatement of the reference
in tests/test_atmos_law_fluxes_host.py.

States come from tests/atmos_nf_cases.py: noise around the reference state (or the vortex's far
field) at Mach scale 1, so that every face node sees a jump; on 27 to 162 elements all four HLLC
branches, both LMARS directions and all four Roe sign patterns occur, wall nodes see supersonic
normal flow through the free-slip ghost state, and on the shell the normals are not axis-aligned.
``p_ref`` and ``Phi`` carry per-node noise too, so that the two sides of a face differ in them
(on a smooth reference state they never do, and reading the wrong side would go unnoticed).
Each test asserts that census on the host (with the restatement's branch output) before anything
is launched.

One evaluation with ``alpha, beta = 0.5, 2.0`` on a random old tendency is held to 1e-12 per
state column (the suite's ``TOL``); two fused LSRK54 steps from a mild state (the Mach-1 noise
does not survive two steps in the oracle itself) to 1e-11 (``TOL_ATMOS``)."""
import numpy as np
import pytest

import atmos_nf_cases as Cs
from helpers import observe, rel_linf
from test_gpu_orders_partitioned import ALPHA, BETA, TOL, TOL_ATMOS, _Case, _gpu

pytestmark = pytest.mark.gpu
T_RHS = 0.2
FLUXES = {"Roe": 2, "HLLC": 3, "LMARS": 4}
_SHARED = {}


def shared(key, make):
    """The host-side part of a case (law, grid, auxiliary state, state, old tendency, census),
    computed once and left unchanged."""
    if key not in _SHARED:
        _SHARED[key] = make()
    return _SHARED[key]


def host_case(oracle, kind, subtract, level):
    def make():
        if kind == "vortex":
            law, grid = Cs.vortex_setup(**level)
        else:
            law, grid = Cs.walled_setup(kind, subtract, **level)
        aux = oracle.OracleDGModel(law, grid, nf_first=1, direction=0).state_auxiliary
        if kind != "vortex":
            Cs.roughen(law, grid, aux)
        Q0 = law.init_state_prognostic(grid, aux, 0.0)
        T0 = np.random.default_rng(3).standard_normal(Q0.shape)
        return law, grid, aux, Q0, T0, Cs.census(law, grid, Q0, aux)
    return shared((kind, subtract, tuple(sorted(level.items()))), make)


def check_rhs(cm, oracle, torch, kind, subtract, name):
    law, grid, aux, Q0, T0, census = host_case(oracle, kind, subtract, Cs.HARD)
    Cs.assert_hard_census(census, walls=kind != "vortex")
    nf, nr = FLUXES[name], grid.nreal
    odg = oracle.OracleDGModel(law, grid, nf_first=nf, direction=0, state_auxiliary=aux.copy())
    To = T0.copy()
    odg(To, Q0.copy(), T_RHS, ALPHA, BETA)
    assert np.isfinite(To[:nr]).all()
    dg = cm.dgmodel.DGModel(law, grid, numerical_flux_first_order=nf, direction=0,
                            state_auxiliary=aux.copy())
    Q, T = _gpu(torch, Q0), _gpu(torch, T0)
    dg(T, Q, T_RHS, ALPHA, BETA)
    dg.synchronize()
    Tn = T.cpu().numpy()
    dg.close()
    assert np.isfinite(Tn[:nr]).all()
    tag = "atmos law fluxes %s %s subtract_off=%s: rhs" % (kind, name, subtract)
    for s in range(5):
        assert observe(tag, rel_linf(Tn[:nr, s], To[:nr, s])) < TOL, s


@pytest.mark.parametrize("name", list(FLUXES))
@pytest.mark.parametrize("subtract", [False, True])
def test_walled_box(cm, oracle, torch, subtract, name):
    """27 elements, flat orientation, walls at the bottom and the top; with ``subtract_off`` the
    ``m.subtract`` lines of all three fluxes run on operands that do not cancel."""
    check_rhs(cm, oracle, torch, "LES", subtract, name)


@pytest.mark.parametrize("name", list(FLUXES))
def test_cubed_sphere_shell(cm, oracle, torch, name):
    """162 elements: normals that are not axis-aligned, orientation flips between panels, walls at
    both radii."""
    check_rhs(cm, oracle, torch, "GCM", True, name)


@pytest.mark.parametrize("name", list(FLUXES))
def test_plain_variant(cm, oracle, torch, name):
    """The variant without orientation and reference state, which the isentropic vortex (subsonic)
    never takes through HLLC's outer branches or Roe's supersonic sign patterns."""
    check_rhs(cm, oracle, torch, "vortex", False, name)


@pytest.mark.parametrize("name", ["HLLC", "LMARS"])
def test_walled_box_on_a_partition(cm, oracle, torch, name):
    """The box on two ranks of one process, ``subtract_off``: across the cut the plus side's state
    comes out of a receive buffer (ghost elements of Q are NaN) and its ``Phi`` and ``p_ref`` out of
    the rank's ghost elements of the auxiliary state; compared with the oracle on the whole grid
    through ``topology.globalelems``.  12 and 15 real elements, both interior lists empty."""
    case = _Case(cm, oracle, torch, "atmos law fluxes LES " + name,
                 lambda r, s: Cs.walled_setup("LES", True, rank=r, size=s, rough_init=True, **Cs.HARD), 2,
                 lists=[(0, 12), (0, 15)], epb=1, gradflux=False, model_kw=dict(direction=0),
                 t_rhs=T_RHS, flux=FLUXES[name])
    Cs.assert_hard_census(Cs.census(case.law, case.grid, case.Q0, case.odg.state_auxiliary))
    case.check_group_rhs()


@pytest.mark.parametrize("name", list(FLUXES))
@pytest.mark.parametrize("kind", ["LES", "GCM"])
def test_fused_lsrk_update(cm, oracle, torch, kind, name):
    """Two LSRK54 steps of ``lsrk_run`` at Courant number 0.1 from the mild state (``a = 0.01``,
    Mach scale 0.05), ``subtract_off``, against ``oracle.lsrk54_step``."""
    law, grid, aux, Q0, _, _ = host_case(oracle, kind, True, Cs.MILD)
    nf, nr, nsteps = FLUXES[name], grid.nreal, 2
    odg = oracle.OracleDGModel(law, grid, nf_first=nf, direction=0, state_auxiliary=aux.copy())
    dt = oracle.calculate_dt(odg, Q0.copy(), 0.1)
    Qo, dQo = Q0.copy(), np.zeros_like(Q0)
    for i in range(nsteps):
        oracle.lsrk54_step(odg, Qo, dQo, i * dt, dt)
    assert np.isfinite(Qo[:nr]).all()
    assert rel_linf(Qo[:nr, 1:4], Q0[:nr, 1:4]) > 1e-3            # the steps moved the state
    dg = cm.dgmodel.DGModel(law, grid, numerical_flux_first_order=nf, direction=0,
                            state_auxiliary=aux.copy())
    Q = _gpu(torch, Q0)
    dQ = torch.zeros_like(Q)
    dg.lsrk_run(Q, dQ, 0.0, dt, nsteps, oracle.RKA, oracle.RKB, oracle.RKC)
    dg.synchronize()
    Qn = Q.cpu().numpy()
    dg.close()
    assert np.isfinite(Qn[:nr]).all()
    tag = "atmos law fluxes %s %s: %d steps" % (kind, name, nsteps)
    for s in range(5):
        assert observe(tag, rel_linf(Qn[:nr, s], Qo[:nr, s])) < TOL_ATMOS, s
