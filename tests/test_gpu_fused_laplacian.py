"""CMDG_OPT_FUSED_LAPLACIAN: a hand-off evaluation forms gradients and Laplacians in one launch.

Inside ``cmdg_lsrk_run`` every evaluation that reads the gradient-argument records launches
``k_lapfused`` in place of ``k_gradients<GARG_IN>`` + ``k_divgrad<RING>`` where the handle is
eligible (horizontal diffusion, every lateral face interior, a unique opposite face node): the
element forms the neighbour's gradient at the shared face nodes itself, from the neighbour's
records and create-time tables, and grad G never goes to memory.  Same expressions on the same
operands in the same order, so the option on and off must leave the same bits in everything a
caller can see: Q, dQ, every auxiliary column, the caller's ``Qhypervisc_div`` and
``cmdg_export_hypervisc_grad``.  Equality is on ``tobytes()``.  ``cmdg_query(FUSED_LAPLACIAN)``
counts the fused evaluations of the last run: all but the first on an eligible handle, else 0.

Shapes, each the smallest that can still go wrong: the 6x2x2x2 sphere (every element on a cube
edge, three panels at every corner, every face orientation and flip), the 6x3x3x2 sphere
(panel-interior elements, second-ring nodes reached across a panel edge), the periodic 3x3x2 brick
(the neighbours across opposite faces are neighbours of each other); the brick with lateral walls
and the sphere with diffusion in every direction keep the two kernels."""
import numpy as np
import pytest

from helpers import held_suarez_setup

pytestmark = pytest.mark.gpu
ONE_STAGE = ([0.0], [1.0], [0.0])   # forward Euler as a 2N tableau: one evaluation per step
NSTEPS = 3


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


def _sphere(n_horz, N, nelem):
    law, grid, d, dd = held_suarez_setup(n_horz=n_horz, n_vert=2, N=N)
    assert grid.nreal == nelem and grid.nelem == nelem
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


def _run(cm, torch, setup, option, dt, tableau):
    """A fresh handle, the perturbed state, one ``cmdg_lsrk_run`` of NSTEPS steps: the bytes of
    everything a caller can see, and what the two query keys say."""
    law, grid, d, dd = setup
    dg = cm.dgmodel.DGModel(law, grid, direction=d, diffusion_direction=dd, device="cuda:0")
    dg.set_option(cm._lib.OPT_FUSED_LAPLACIAN, option)
    Q = _gpu(torch, _perturbed(law, grid, dg.state_auxiliary.cpu().numpy()))
    dQ = torch.zeros_like(Q)
    rka, rkb, rkc = tableau or _lsrk54(cm, dg, Q)
    dg.lsrk_run(Q, dQ, 0.0, dt, NSTEPS, rka, rkb, rkc)
    dg.synchronize()
    assert bool(torch.isfinite(Q).all())
    aux = dg.state_auxiliary.cpu().numpy()
    out = {"Q": Q.cpu().numpy().tobytes(), "dQ": dQ.cpu().numpy().tobytes(),
           "Qhypervisc_div": dg.Qhypervisc_div.cpu().numpy().tobytes(),
           "Qhypervisc_grad": dg.Qhypervisc_grad.cpu().numpy().tobytes()}
    for c in range(aux.shape[1]):
        out["aux column %d" % c] = np.ascontiguousarray(aux[:, c]).tobytes()
    counts = (dg.query("GRADARG_HANDOFF"), dg.query("FUSED_LAPLACIAN"))
    dg.close()
    return out, counts


def _on_equals_off(cm, torch, setup, dt, fused):
    """LSRK54 (5 evaluations per step) and the one-stage tableau, NSTEPS steps each.  fused: is the
    handle eligible -- then every evaluation of a run but its first is fused."""
    for tableau, nstages in ((None, 5), (ONE_STAGE, 1)):
        on, (handoff_on, fused_on) = _run(cm, torch, setup, 1, dt, tableau)
        off, (handoff_off, fused_off) = _run(cm, torch, setup, 0, dt, tableau)
        assert handoff_on == 1 and handoff_off == 1
        assert fused_on == (nstages * NSTEPS - 1 if fused else 0), (nstages, fused_on)
        assert fused_off == 0
        assert on.keys() == off.keys()
        for name in on:
            assert on[name] == off[name], (nstages, name)
        # (the hyperdiffusion arrays are live: a comparison of zeros would prove nothing)
        assert any(on["Qhypervisc_div"]) and any(on["Qhypervisc_grad"])


def test_sphere_48_is_fused(cm, torch):
    _on_equals_off(cm, torch, _sphere(2, 4, 48), 2.0, fused=True)


def test_sphere_108_is_fused(cm, torch):
    _on_equals_off(cm, torch, _sphere(3, 4, 108), 2.0, fused=True)


def test_periodic_brick_is_fused(cm, torch):
    _on_equals_off(cm, torch, _brick(cm, True), 0.05, fused=True)


def test_brick_with_lateral_walls_keeps_two_kernels(cm, torch):
    _on_equals_off(cm, torch, _brick(cm, False), 0.05, fused=False)


def test_every_direction_diffusion_keeps_two_kernels(cm, torch):
    """(The biharmonic coefficient is scaled for the horizontal spacing, ~2 000 km; across 4 km
    vertical spacings its stable step is ~(4 / 2000)^4 of the horizontal one: hence the tiny dt.)"""
    law, grid, d, dd = _sphere(2, 4, 48)
    _on_equals_off(cm, torch, (law, grid, d, 0), 1e-8, fused=False)   # 0: EveryDirection


@pytest.mark.parametrize("N", [2, 3])
def test_sphere_other_orders_are_fused(cm, torch, N):
    """k_lapfused is instantiated wherever the hand-off is: N = 2 .. 4."""
    _on_equals_off(cm, torch, _sphere(2, N, 48), 2.0, fused=True)
