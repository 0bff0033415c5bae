"""The nodal auxiliary refresh of the gradient-argument hand-off (CMDG_OPT_GRADARG_HANDOFF) rides
only in the last hand-off update of a ``cmdg_lsrk_run``: the dry atmosphere's refreshed columns
(moisture.theta_v, air_T) are read by no pass, and between two stages of such a run nothing else can
see them, so every other hand-off update would write values the next one overwrites unread.  What a
caller sees when the call returns -- Q, dQ, every auxiliary column -- must keep the bits of the
ordinary kernels, ``cmdg_query(CMDG_Q_GRADARG_REFRESHES)`` must say how many updates carried the
refresh, and a run that did not take the hand-off must refresh as before.

Shapes: the 6x2x2x2 stacked cubed sphere (48 elements, N = 4) of test_gpu_gradarg_handoff.py, the
smallest with interior faces on every side and both boundary faces; the perturbed state used there.
Comparisons are on the bit patterns.
"""
import argparse

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 20250117  # bench.parity_check


def _workload(cm, nhorz, nvert, rank=0, size=1):
    import bench
    args = argparse.Namespace(nhorz=None, nvert=8, scaling="weak", connectivity="full")
    law, grid, direction, dt, _ = bench.build_workload(cm, "heldsuarez", rank, size, 4, args,
                                                       nhorz=nhorz, nvert=nvert)
    return law, grid, direction, dt


def _perturbed(law, grid, aux, seed=SEED):
    """The perturbed initial state of bench.parity_check."""
    Q0 = law.init_state_prognostic(grid, aux, 0.0)
    rng = np.random.default_rng(seed)
    Q0[:, 1:4] += 0.5 * rng.standard_normal(Q0[:, 1:4].shape)
    Q0[:, 4] *= 1 + 1e-3 * rng.standard_normal(Q0[:, 4].shape)
    return Q0


@pytest.fixture(scope="module")
def hs48(cm):
    law, grid, direction, dt = _workload(cm, 2, 2)
    assert grid.nreal == 48 and grid.nelem == 48
    return law, grid, direction, dt


def _model(cm, hs, option):
    law, grid, direction, _ = hs
    dg = cm.dgmodel.DGModel(law, grid, direction=direction[0], diffusion_direction=direction[1],
                            device="cuda:0")
    dg.set_option(cm._lib.OPT_GRADARG_HANDOFF, option)
    return dg


def _bits(t):
    import torch
    return t.detach().clone().view(torch.int64)


def _snapshot(dg, solver, Q):
    dg.synchronize()
    return _bits(Q), _bits(solver.dQ), _bits(dg.state_auxiliary)


def _assert_same(torch, on, off):
    for name, a, b in zip(("Q", "dQ", "aux"), on, off):
        assert torch.equal(a, b), name
    # every auxiliary column, theta_v and air_T (the last two) among them, one by one for the message
    for c in range(on[2].shape[1]):
        assert torch.equal(on[2][:, c], off[2][:, c]), "aux column %d" % c


def _lsrk54(cm):
    return cm.odesolvers.LSRK54CarpenterKennedy


def _lsrk144(cm):
    return cm.odesolvers.LSRK144NiegemannDiehlBusch


def _euler(cm):
    """Forward Euler as a one-stage 2N tableau."""
    def make(dg, Q, dt=0.0, t0=0.0):
        return cm.odesolvers.LowStorageRungeKutta2N(dg, (0.0,), (1.0,), (0.0,), Q, dt=dt, t0=t0)
    return make


def _run(cm, torch, hs, option, nsteps, make_solver, prepare=None, dt=None):
    """A fresh handle, the perturbed state, one ``lsrk_run`` of ``nsteps``: the (Q, dQ, aux) bits,
    the auxiliary state before the run and what the two query keys say."""
    dg = _model(cm, hs, option)
    if prepare:
        prepare(dg)
    aux0 = _bits(dg.state_auxiliary)
    Q0 = _perturbed(hs[0], hs[1], dg.state_auxiliary.cpu().numpy())
    Q = torch.from_numpy(Q0).to("cuda:0")
    solver = make_solver(dg, Q, dt=hs[3] if dt is None else dt)
    solver.dostep(Q, nsteps=nsteps)
    snap = _snapshot(dg, solver, Q)
    used, refreshes = dg.query("GRADARG_HANDOFF"), dg.query("GRADARG_REFRESHES")
    dg.close()
    assert torch.isfinite(snap[0].view(torch.float64)).all()
    return snap, aux0, used, refreshes


@pytest.mark.parametrize("scheme,nsteps", [("lsrk54", 1), ("lsrk54", 2), ("lsrk54", 3), ("lsrk144", 1)])
def test_on_equals_off_bit_for_bit_one_refresh(cm, torch, hs48, scheme, nsteps):
    """LSRK54: 5 K - 1 hand-off updates in K steps, LSRK144: 13 (an even stage count, so the work
    states alternate the other way round); one of them refreshes."""
    make = _lsrk54(cm) if scheme == "lsrk54" else _lsrk144(cm)
    on, _, used_on, refreshes_on = _run(cm, torch, hs48, 1, nsteps, make)
    off, _, used_off, refreshes_off = _run(cm, torch, hs48, 0, nsteps, make)
    assert (used_on, refreshes_on) == (1, 1)
    assert (used_off, refreshes_off) == (0, 0)
    _assert_same(torch, on, off)


def test_one_stage_tableau(cm, torch, hs48):
    """Forward Euler, two steps: the only hand-off update is that of the first step, and a
    one-stage tableau refreshes in every update."""
    dt = 0.1 * hs48[3]
    on, _, used_on, refreshes_on = _run(cm, torch, hs48, 1, 2, _euler(cm), dt=dt)
    off, _, used_off, refreshes_off = _run(cm, torch, hs48, 0, 2, _euler(cm), dt=dt)
    assert (used_on, refreshes_on) == (1, 1)
    assert (used_off, refreshes_off) == (0, 0)
    _assert_same(torch, on, off)


def _refreshed(torch, snap, aux0):
    """theta_v and air_T are no longer what the handle was created with."""
    return all(not torch.equal(snap[2][:, c], aux0[:, c]) for c in (-2, -1))


def test_fallback_step_filter_refreshes_as_before(cm, torch, hs48):
    keep = []

    def with_filter(dg):
        F = cm.mesh.filters
        keep.append(F.make_device_filter(dg, F.ExponentialFilter(hs48[1], 0, 20),
                                         F.AtmosFilterPerturbations(hs48[0])))
        dg.set_filters(step_filter=keep[-1])
    on, aux0, used_on, refreshes_on = _run(cm, torch, hs48, 1, 2, _lsrk54(cm), prepare=with_filter)
    off, _, used_off, refreshes_off = _run(cm, torch, hs48, 0, 2, _lsrk54(cm), prepare=with_filter)
    assert (used_on, refreshes_on) == (0, 0) and (used_off, refreshes_off) == (0, 0)
    _assert_same(torch, on, off)
    assert _refreshed(torch, on, aux0)


def test_fallback_handle_with_ghosts_refreshes_as_before(cm, torch):
    """Rank 0 of a two-rank sphere whose only neighbour is the process itself (as in
    test_gpu_halo.py)."""
    hs = _workload(cm, 2, 2, rank=0, size=2)
    grid = hs[1]
    nn = len(grid.nabrtorank)
    assert nn >= 1 and grid.nelem > grid.nreal
    grid.nabrtorank = [0] * nn

    def connect(dg):
        dg.comm_init_rccl(cm.dgmodel.rccl_unique_id(), 0, 1)
    on, aux0, used_on, refreshes_on = _run(cm, torch, hs, 1, 1, _lsrk54(cm), prepare=connect)
    off, _, used_off, refreshes_off = _run(cm, torch, hs, 0, 1, _lsrk54(cm), prepare=connect)
    assert (used_on, refreshes_on) == (0, 0) and (used_off, refreshes_off) == (0, 0)
    nr = grid.nreal
    _assert_same(torch, [x[:nr] for x in on], [x[:nr] for x in off])
    assert _refreshed(torch, [x[:nr] for x in on], aux0[:nr])


def test_fallback_law_with_gradient_flux_refreshes_as_before(cm, torch):
    """The dry rising bubble (SmagorinskyLilly: USE_GF = true) on a 2x2x2 brick."""
    from helpers import rising_bubble_setup
    setup = rising_bubble_setup(nx=2, ny=2, nz=2)
    law, grid = setup[0], setup[1]
    out = []
    for option in (1, 0):
        dg = cm.dgmodel.DGModel(law, grid, direction=0, device="cuda:0")
        dg.set_option(cm._lib.OPT_GRADARG_HANDOFF, option)
        aux0 = _bits(dg.state_auxiliary)
        Q = dg.init_ode_state(0.0)
        solver = cm.odesolvers.LSRK54CarpenterKennedy(dg, Q, dt=0.01)
        solver.dostep(Q, nsteps=1)
        out.append(_snapshot(dg, solver, Q))
        assert dg.query("GRADARG_HANDOFF") == 0 and dg.query("GRADARG_REFRESHES") == 0
        dg.close()
    _assert_same(torch, out[0], out[1])
    assert _refreshed(torch, out[0], aux0)


def _aux_of_last_input(cm, torch, hs, Q_start, t0, nsteps):
    """theta_v and air_T as ``update_auxiliary_state!`` leaves them for the state that enters the
    last evaluation of an ``nsteps`` LSRK54 run from ``Q_start``: the ordinary kernels
    (hand-off off) take nsteps - 1 steps and the first four stages of one more, then one plain
    evaluation of that state refreshes the auxiliary state."""
    dg = _model(cm, hs, 0)
    Q = Q_start.clone()
    solver = _lsrk54(cm)(dg, Q, dt=hs[3], t0=t0)
    if nsteps > 1:
        solver.dostep(Q, nsteps=nsteps - 1)
    # (a 2N stage uses the coefficients up to its own alone, and dQ enters a step scaled by RKA[0] = 0)
    dg.lsrk_run(Q, solver.dQ, solver.t, hs[3], 1, solver.RKA[:4], solver.RKB[:4], solver.RKC[:4])
    dg.synchronize()
    T = dg.create_state()
    torch.cuda.synchronize()
    dg(T, Q, solver.t + solver.RKC[4] * hs[3], 1.0, 0.0)
    dg.synchronize()
    want = _bits(dg.state_auxiliary)[:, -2:].clone()
    dg.close()
    return want


def test_nothing_trusted_across_calls(cm, torch, hs48):
    """A run, a plain evaluation of another state, a second run: bit for bit what the ordinary
    kernels leave, and after each run theta_v / air_T belong to the input of its last evaluation."""
    law, grid, _, dt = hs48

    def sequence(option):
        dg = _model(cm, hs48, option)
        aux0 = dg.state_auxiliary.cpu().numpy()
        Q = torch.from_numpy(_perturbed(law, grid, aux0)).to("cuda:0")
        other = torch.from_numpy(_perturbed(law, grid, aux0, seed=SEED + 1)).to("cuda:0")
        solver = _lsrk54(cm)(dg, Q, dt=dt)
        T = dg.create_state()
        torch.cuda.synchronize()
        starts = [(Q.clone(), solver.t)]
        solver.dostep(Q, nsteps=1)
        first = _snapshot(dg, solver, Q)
        counts = [(dg.query("GRADARG_HANDOFF"), dg.query("GRADARG_REFRESHES"))]
        dg(T, other, solver.t, 1.0, 0.0)
        mid = _snapshot(dg, solver, Q) + (_bits(T),)
        starts.append((Q.clone(), solver.t))
        solver.dostep(Q, nsteps=2)
        second = _snapshot(dg, solver, Q)
        counts.append((dg.query("GRADARG_HANDOFF"), dg.query("GRADARG_REFRESHES")))
        dg.close()
        return first, mid, second, counts, starts
    on, off = sequence(1), sequence(0)
    assert on[3] == [(1, 1), (1, 1)] and off[3] == [(0, 0), (0, 0)]
    for a, b in zip(on[:3], off[:3]):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    for snap, (Q_start, t0), nsteps in zip((on[0], on[2]), on[4], (1, 2)):
        want = _aux_of_last_input(cm, torch, hs48, Q_start, t0, nsteps)
        assert torch.equal(snap[2][:, -2:], want)
    # the evaluation in between refreshed for the state it was given, not for the run's
    assert not torch.equal(on[1][2][:, -2:], on[0][2][:, -2:])
