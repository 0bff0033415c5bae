"""The fused Laplacian pass (``k_lapfused``) with the in-face line of the neighbour taken from the
sibling face lanes through LDS, on the shapes the exchange can get wrong.

A face lane of ``k_lapfused`` gathers only the neighbour's line of records normal to the shared
face; the line inside the face is the records the other lanes of the same face and level hold,
which they hand each other through an exchange array indexed [face][level][index along the
neighbour's face].  A slot written under the wrong level or the wrong index changes bits, because
the seeded perturbation differs from node to node.  As in ``test_gpu_fused_laplacian.py`` the
option on and off must leave the same bytes in everything a caller can see, and
``cmdg_query(FUSED_LAPLACIAN)`` counts the fused evaluations.

Shapes: the 6x2x2x3 sphere (72 elements: three levels of elements, the middle one without a
vertical boundary) at N = 2, 3 and 4, whose instantiations have exchange arrays of their own
sizes; the periodic 3x3x3 brick at N = 4; and the sphere at N = 4 with a one-stage tableau and two
steps, which is exactly one fused launch: a difference there points at the launch itself and not
at five stages of feedback."""
import numpy as np
import pytest

from helpers import held_suarez_setup

pytestmark = pytest.mark.gpu
ONE_STAGE = ([0.0], [1.0], [0.0])   # forward Euler as a 2N tableau: one evaluation per step


def _gpu(torch, a):
    x = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return x


def _perturbed(law, grid, aux, seed=20250612):
    Q0 = law.init_state_prognostic(grid, aux, 0.0)
    rng = np.random.default_rng(seed)
    Q0[:, 1:4] += 0.5 * rng.standard_normal(Q0[:, 1:4].shape)
    Q0[:, 4] *= 1 + 1e-3 * rng.standard_normal(Q0[:, 4].shape)
    return Q0


def _sphere(N):
    law, grid, d, dd = held_suarez_setup(n_horz=2, n_vert=3, N=N)
    assert grid.nreal == 72 and grid.nelem == 72
    return law, grid, d, dd


def _brick(cm):
    """The hyperdiffusive dry law (DryBiharmonic, horizontal) on the periodic 3 x 3 x 3 brick."""
    A, M = cm.atmos, cm.mesh
    ps = A.PlanetParameters()
    rng = [np.linspace(0.0, 1500.0, 4), np.linspace(0.0, 1500.0, 4), np.linspace(0.0, 1500.0, 4)]
    topl = M.StackedBrickTopology(rng, periodicity=(True, True, False), boundary=((0, 0), (0, 0), (1, 2)))
    grid = M.DiscontinuousSpectralElementGrid(topl, 4)
    law = A.DryAtmosModel(A.RisingBubbleSetup(ps, xc=750.0, zc=300.0, rc=300.0), orientation=A.ORIENT_FLAT,
                          ref_state=A.DryAdiabaticProfile(ps, 300.0, 0.0), viscosity=0.0,
                          hyperdiffusion_timescale=3600.0, sources=A.SRC_GRAVITY,
                          boundary_conditions=(A.BC_ATMOS_DEFAULT, A.BC_ATMOS_DEFAULT), param_set=ps)
    assert grid.nreal == 27
    return law, grid, 0, 1


def _run(cm, torch, setup, option, dt, tableau, nsteps):
    """A fresh handle, the perturbed state, one ``cmdg_lsrk_run``: the bytes of everything a caller
    can see, and what the two query keys say."""
    law, grid, d, dd = setup
    dg = cm.dgmodel.DGModel(law, grid, direction=d, diffusion_direction=dd, device="cuda:0")
    dg.set_option(cm._lib.OPT_FUSED_LAPLACIAN, option)
    Q = _gpu(torch, _perturbed(law, grid, dg.state_auxiliary.cpu().numpy()))
    dQ = torch.zeros_like(Q)
    if tableau is None:
        s = cm.odesolvers.LSRK54CarpenterKennedy(dg, Q)
        tableau = (s.RKA, s.RKB, s.RKC)
    dg.lsrk_run(Q, dQ, 0.0, dt, nsteps, *tableau)
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


def _on_equals_off(cm, torch, setup, dt, tableau, nstages, nsteps):
    on, (handoff_on, fused_on) = _run(cm, torch, setup, 1, dt, tableau, nsteps)
    off, (handoff_off, fused_off) = _run(cm, torch, setup, 0, dt, tableau, nsteps)
    assert handoff_on == 1 and handoff_off == 1
    assert fused_on == nstages * nsteps - 1, fused_on   # every evaluation of the run but its first
    assert fused_off == 0
    assert on.keys() == off.keys()
    for name in on:
        assert on[name] == off[name], name
    # (the hyperdiffusion arrays are live: a comparison of zeros would prove nothing)
    assert any(on["Qhypervisc_div"]) and any(on["Qhypervisc_grad"])


@pytest.mark.parametrize("N", [2, 3, 4])
def test_sphere_72_three_levels(cm, torch, N):
    _on_equals_off(cm, torch, _sphere(N), 2.0, None, 5, 2)


def test_periodic_brick_27_three_levels(cm, torch):
    _on_equals_off(cm, torch, _brick(cm), 0.05, None, 5, 2)


def test_sphere_72_one_fused_launch(cm, torch):
    """One-stage tableau, two steps: the first evaluation keeps the two kernels, the second is the
    one fused launch, and Qhypervisc_div and the exported gradient are what it left."""
    _on_equals_off(cm, torch, _sphere(4), 2.0, ONE_STAGE, 1, 2)
