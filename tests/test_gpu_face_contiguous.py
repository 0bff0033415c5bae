"""Face-contiguous ("ring") intermediates of a hand-off run and the lift weight of the face digest.

Inside ``cmdg_lsrk_run`` every evaluation that reads the gradient-argument records hands its
Laplacians from ``k_divgrad`` to ``k_gradlap`` as 32-byte records in the ring order (``ring_slot``,
cmdg_common.h), gathers their plus side through ``facePr`` and writes the caller's
``Qhypervisc_div`` only in the run's last evaluation; the run's first evaluation and every other
call take the ordinary kernels.  Same expressions on the same operands, so ``CMDG_OPT_GRADARG_HANDOFF`` on and off must
leave the same bits in everything a caller can see: Q, dQ, every auxiliary column, the caller's
``Qhypervisc_div`` and ``cmdg_export_hypervisc_grad``.  Equality is on ``tobytes()`` (signed zeros
and NaN payloads count).  ``faceW = vMI * sM`` is read by the gradient, Laplacian and
gradient-of-Laplacian passes of every law: one evaluation of three other laws against the oracle.

Shapes, each the smallest that can still go wrong: the 6x2x2x2 stacked cubed sphere (every element
lies on a cube edge: every face-to-face orientation and flip), a 3x3x2 brick with lateral walls
(plus side = minus side on lateral faces) and the same brick periodic (the neighbours of an element
across opposite faces are neighbours of each other)."""
import numpy as np
import pytest

from helpers import (bomex_setup, held_suarez_setup, pseudo1d_setup, rel_linf, rising_bubble_setup,
                     variable_degree_setup)

pytestmark = pytest.mark.gpu
TOL = 1e-12
ONE_STAGE = ([0.0], [1.0], [0.0])   # forward Euler as a 2N tableau: one evaluation per step


def _lsrk54(cm, dg, Q):
    s = cm.odesolvers.LSRK54CarpenterKennedy(dg, Q)
    return s.RKA, s.RKB, s.RKC


def _gpu(torch, a):
    x = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return x


def _perturbed(law, grid, aux, seed=20250117):
    Q0 = law.init_state_prognostic(grid, aux, 0.0)
    rng = np.random.default_rng(seed)
    Q0[:, 1:4] += 0.5 * rng.standard_normal(Q0[:, 1:4].shape)
    Q0[:, 4] *= 1 + 1e-3 * rng.standard_normal(Q0[:, 4].shape)
    return Q0


def _sphere(N):
    law, grid, d, dd = held_suarez_setup(n_horz=2, n_vert=2, N=N)
    assert grid.nreal == 48 and grid.nelem == 48
    return law, grid, d, dd


def _brick(cm, periodic):
    """The hyperdiffusive dry law (DryBiharmonic, horizontal) on 3 x 3 x 2 elements."""
    A, M = cm.atmos, cm.mesh
    ps = A.PlanetParameters()
    rng = [np.linspace(0.0, 1500.0, 4), np.linspace(0.0, 1500.0, 4), np.linspace(0.0, 1000.0, 3)]
    topl = M.StackedBrickTopology(rng, periodicity=(periodic, periodic, False),
                                  boundary=((0, 0), (0, 0), (1, 2)) if periodic else ((1, 1), (1, 1), (1, 2)))
    grid = M.DiscontinuousSpectralElementGrid(topl, 4)
    law = A.DryAtmosModel(A.RisingBubbleSetup(ps, xc=750.0, zc=300.0, rc=300.0), orientation=A.ORIENT_FLAT,
                          ref_state=A.DryAdiabaticProfile(ps, 300.0, 0.0), viscosity=0.0,
                          hyperdiffusion_timescale=3600.0, sources=A.SRC_GRAVITY,
                          boundary_conditions=(A.BC_ATMOS_DEFAULT, A.BC_ATMOS_DEFAULT), param_set=ps)
    assert grid.nreal == 18
    return law, grid, 0, 1


def _run(cm, torch, setup, option, nsteps, dt, tableau=None):
    """A fresh handle, the perturbed state, one ``cmdg_lsrk_run``: the bytes of everything a caller
    can see, and what the query key says."""
    law, grid, d, dd = setup
    dg = cm.dgmodel.DGModel(law, grid, direction=d, diffusion_direction=dd, device="cuda:0")
    dg.set_option(cm._lib.OPT_GRADARG_HANDOFF, option)
    Q = _gpu(torch, _perturbed(law, grid, dg.state_auxiliary.cpu().numpy()))
    dQ = torch.zeros_like(Q)
    rka, rkb, rkc = tableau or _lsrk54(cm, dg, Q)
    dg.lsrk_run(Q, dQ, 0.0, dt, nsteps, rka, rkb, rkc)
    dg.synchronize()
    assert bool(torch.isfinite(Q).all())
    aux = dg.state_auxiliary.cpu().numpy()
    out = {"Q": Q.cpu().numpy().tobytes(), "dQ": dQ.cpu().numpy().tobytes(),
           "Qhypervisc_div": dg.Qhypervisc_div.cpu().numpy().tobytes(),
           "Qhypervisc_grad": dg.Qhypervisc_grad.cpu().numpy().tobytes()}
    for c in range(aux.shape[1]):
        out["aux column %d" % c] = np.ascontiguousarray(aux[:, c]).tobytes()
    used = dg.query("GRADARG_HANDOFF")
    dg.close()
    return out, used


def _on_equals_off(cm, torch, setup, nsteps, dt, tableau=None, used=1):
    on, used_on = _run(cm, torch, setup, 1, nsteps, dt, tableau)
    off, used_off = _run(cm, torch, setup, 0, nsteps, dt, tableau)
    assert used_on == used and used_off == 0
    assert on.keys() == off.keys()
    for name in on:
        assert on[name] == off[name], name
    # (the hyperdiffusion arrays are live: a comparison of zeros would prove nothing)
    if setup[0].nhyper > 0:
        assert any(on["Qhypervisc_div"]) and any(on["Qhypervisc_grad"])


@pytest.fixture(scope="module")
def hs48():
    return _sphere(4)


@pytest.mark.parametrize("nsteps", [1, 2, 3])
def test_sphere_on_equals_off(cm, torch, hs48, nsteps):
    """LSRK54 on the 48-element sphere, N = 4: 1 step (the ordinary first evaluation, four ring
    evaluations), 2 and 3 steps (ring evaluations across step boundaries)."""
    _on_equals_off(cm, torch, hs48, nsteps, 2.0)


@pytest.mark.parametrize("N", [2, 3])
def test_sphere_other_orders(cm, torch, N):
    _on_equals_off(cm, torch, _sphere(N), 2, 2.0)


def test_mixed_order_handle_keeps_the_ordinary_kernels(cm, torch):
    """(N_h, N_v) = (4, 2) is compiled for advection-diffusion alone, a law without hyperdiffusion:
    the handle is not hand-off eligible, the query says so either way, and the option changes nothing."""
    law, grid, dt = variable_degree_setup(level=1, orders=(4, 2))
    out = []
    for option in (1, 0):
        dg = cm.dgmodel.DGModel(law, grid)
        dg.set_option(cm._lib.OPT_GRADARG_HANDOFF, option)
        Q = dg.init_ode_state(0.0)
        dQ = torch.zeros_like(Q)
        dg.lsrk_run(Q, dQ, 0.0, dt, 2, *_lsrk54(cm, dg, Q))
        dg.synchronize()
        assert dg.query("GRADARG_HANDOFF") == 0
        out.append((Q.cpu().numpy().tobytes(), dQ.cpu().numpy().tobytes()))
        dg.close()
    assert out[0] == out[1]


@pytest.mark.parametrize("periodic", [False, True], ids=["walls", "periodic"])
def test_brick_on_equals_off(cm, torch, periodic):
    _on_equals_off(cm, torch, _brick(cm, periodic), 2, 0.05)


@pytest.mark.parametrize("nsteps,used", [(1, 0), (2, 1), (3, 1)])
def test_one_stage_tableau(cm, torch, hs48, nsteps, used):
    """The planner's edge cases.  One step of a one-stage tableau is a run of one evaluation: nothing
    to hand on, the query says 0.  Two steps are a run of exactly two evaluations -- the ordinary
    one, then a ring evaluation that is also the run's last and must write the caller's
    Qhypervisc_div; three have a ring evaluation in the middle that does not."""
    _on_equals_off(cm, torch, hs48, nsteps, 0.5, ONE_STAGE, used=used)


def test_two_evaluations_of_lsrk_coefficients(cm, torch, hs48):
    """A two-stage 2N tableau, one step: exactly two evaluations with the fused update ending in Q."""
    _on_equals_off(cm, torch, hs48, 1, 1.0, ([0.0, -0.5], [0.5, 1.0], [0.0, 0.5]))


def test_rhs_after_a_ring_run_matches_oracle(cm, torch, oracle, hs48):
    """Nothing ordinary may read a ring-ordered buffer: after a hand-off run, one ``cmdg_rhs`` on
    the same handle against the oracle, with the hyperdiffusion arrays it leaves."""
    law, grid, d, dd = hs48
    odg = oracle.OracleDGModel(law, grid, nf_first=0, direction=d, diffusion_direction=dd)
    dg = cm.dgmodel.DGModel(law, grid, direction=d, diffusion_direction=dd, device="cuda:0")
    Q = _gpu(torch, _perturbed(law, grid, odg.state_auxiliary))
    dQ = torch.zeros_like(Q)
    dg.lsrk_run(Q, dQ, 0.0, 2.0, 1, *_lsrk54(cm, dg, Q))
    dg.synchronize()
    assert dg.query("GRADARG_HANDOFF") == 1
    Tg = dg.create_state()
    torch.cuda.synchronize()
    dg(Tg, Q, 2.0, 1.0, 0.0)
    dg.synchronize()
    Qh = Q.cpu().numpy()
    To = np.zeros_like(Qh)
    odg(To, Qh.copy(), 2.0, 1.0, 0.0)
    Tn = Tg.cpu().numpy()
    for s in range(law.ns):
        assert rel_linf(Tn[:, s], To[:, s]) < TOL, s
    for name, a, b in (("hvdiv", dg.Qhypervisc_div, odg.Qhypervisc_div),
                       ("hvgrad", dg.Qhypervisc_grad, odg.Qhypervisc_grad)):
        a = a.cpu().numpy()
        for s in range(b.shape[1]):
            if np.abs(b[:, s]).max() > 0:
                assert rel_linf(a[:, s], b[:, s]) < TOL, (name, s)
    dg.close()


def _one_evaluation(cm, torch, oracle, law, grid, Q0, nstate):
    odg = oracle.OracleDGModel(law, grid)
    dg = cm.dgmodel.DGModel(law, grid)
    if Q0 is None:
        Q0 = law.init_state_prognostic(grid, odg.state_auxiliary, 0.0)
    To = np.zeros_like(Q0)
    odg(To, Q0.copy(), 0.2, 1.0, 0.0)
    Tg = _gpu(torch, np.zeros_like(Q0))
    dg(Tg, _gpu(torch, Q0), 0.2, 1.0, 0.0)
    Tn = Tg.cpu().numpy()
    for s in range(nstate):
        assert rel_linf(Tn[:, s], To[:, s]) < TOL, s
    if law.ngradflux > 0:
        gfg = dg.state_gradient_flux.cpu().numpy()
        for s in range(law.ngradflux):
            sc = max(np.abs(odg.state_gradient_flux[:, s]).max(), 1e-300)
            assert np.abs(gfg[:, s] - odg.state_gradient_flux[:, s]).max() / sc < TOL, s
    dg.close()


def test_lift_weight_advection_diffusion(cm, torch, oracle):
    law, grid, _ = pseudo1d_setup(Ne=3, N=4)
    aux = oracle.OracleDGModel(law, grid).state_auxiliary
    Q0 = law.init_state_prognostic(grid, aux, 0.0)
    Q0 = Q0 + 1e-3 * np.random.default_rng(4).standard_normal(Q0.shape)
    _one_evaluation(cm, torch, oracle, law, grid, Q0, 1)


def test_lift_weight_smagorinsky_bubble(cm, torch, oracle):
    law, grid = rising_bubble_setup(nx=2, ny=2, nz=2)
    aux = oracle.OracleDGModel(law, grid).state_auxiliary
    Q0 = law.init_state_prognostic(grid, aux, 0.0)
    rng = np.random.default_rng(3)
    Q0[:, 1:4] += Q0[:, 0:1] * 3.0 * rng.standard_normal(Q0[:, 1:4].shape)
    _one_evaluation(cm, torch, oracle, law, grid, Q0, 5)


def test_lift_weight_bomex_order_six(cm, torch, oracle):
    law, grid = bomex_setup(nx=2, ny=2, nz=4, N=6)
    law.maxiter, law.tolerance = 40, 1e-11          # converged saturation adjustment
    aux = oracle.OracleDGModel(law, grid).state_auxiliary
    Q0 = law.init_state_prognostic(grid, aux, 0.0)
    rng = np.random.default_rng(6)
    Q0[:, 1:4] += Q0[:, 0:1] * 0.5 * rng.standard_normal(Q0[:, 1:4].shape)
    Q0[:, 5] *= 1 + 0.05 * rng.random(Q0[:, 5].shape)
    _one_evaluation(cm, torch, oracle, law, grid, Q0, 6)
