"""CMDG_OPT_GRADARG_HANDOFF: inside ``cmdg_lsrk_run`` the fused update of a stage forms the next
stage's gradient arguments and does the nodal auxiliary refresh for the updated state; the next
gradient pass reads those records.  Same expressions on the same operands, so everything a caller
can see -- Q, dQ, every auxiliary column -- must end a run with the bits the ordinary kernels
leave, and the path must only be taken where it is safe: single-rank Held-Suarez-type handles
without filters, and never across calls.

Shapes: the 6x2x2x2 stacked cubed sphere (48 elements, N = 4) is the smallest with cube corners,
a vertical interior face, top and bottom boundaries and lateral neighbours of rotated orientation.
Comparisons are on the bit patterns (NaN-safe and stricter than ``torch.equal`` on signed zeros).
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


def _same(a, b):
    import torch
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _snapshot(dg, solver, Q):
    dg.synchronize()
    return _bits(Q), _bits(solver.dQ), _bits(dg.state_auxiliary)


def _run(cm, torch, hs, option, nsteps, prepare=None):
    """A fresh handle, the perturbed state, one ``lsrk_run`` of ``nsteps``: (Q, dQ, aux) bits and
    what the query key says."""
    dg = _model(cm, hs, option)
    if prepare:
        prepare(dg)
    Q0 = _perturbed(hs[0], hs[1], dg.state_auxiliary.cpu().numpy())
    Q = torch.from_numpy(Q0).to("cuda:0")
    solver = cm.odesolvers.LSRK54CarpenterKennedy(dg, Q, dt=hs[3])
    solver.dostep(Q, nsteps=nsteps)
    snap = _snapshot(dg, solver, Q)
    used = dg.query("GRADARG_HANDOFF")
    dg.close()
    return snap, used


@pytest.mark.parametrize("nsteps", [1, 3])
def test_on_equals_off_bit_for_bit(cm, torch, hs48, nsteps):
    """nsteps = 1: bootstrap evaluation, four hand-offs, final plain update; 3: hand-offs across
    step boundaries too."""
    on, used_on = _run(cm, torch, hs48, 1, nsteps)
    off, used_off = _run(cm, torch, hs48, 0, nsteps)
    assert used_on == 1 and used_off == 0
    assert torch.isfinite(on[0].view(torch.float64)).all()
    for name, a, b in zip(("Q", "dQ", "aux"), on, off):
        assert torch.equal(a, b), name
    # every auxiliary column, the refreshed ones among them (one by one, for the message)
    for c in range(on[2].shape[1]):
        assert torch.equal(on[2][:, c], off[2][:, c]), "aux column %d" % c


def test_no_trust_across_calls(cm, torch, hs48):
    """The records a run leaves behind are never read by the next call: the caller may have
    changed Q in between."""
    law, grid, _, dt = hs48
    dg = _model(cm, hs48, 1)
    aux0 = dg.state_auxiliary.cpu().numpy()
    Q = torch.from_numpy(_perturbed(law, grid, aux0)).to("cuda:0")
    second = _perturbed(law, grid, aux0, seed=SEED + 1)
    solver = cm.odesolvers.LSRK54CarpenterKennedy(dg, Q, dt=dt)
    solver.dostep(Q, nsteps=1)
    dg.synchronize()
    Q.copy_(torch.from_numpy(second))
    torch.cuda.synchronize()
    solver.dostep(Q, nsteps=1)
    got = _snapshot(dg, solver, Q)
    assert dg.query("GRADARG_HANDOFF") == 1
    dg.close()
    fresh = _model(cm, hs48, 1)
    Qf = torch.from_numpy(second).to("cuda:0")
    sf = cm.odesolvers.LSRK54CarpenterKennedy(fresh, Qf, dt=dt, t0=dt)
    sf.dostep(Qf, nsteps=1)
    want = _snapshot(fresh, sf, Qf)
    fresh.close()
    assert torch.equal(got[0], want[0]), "Q"
    assert torch.equal(got[2], want[2]), "aux"


def test_evaluation_between_two_runs(cm, torch, hs48):
    """dg(T, Q, ...) between two runs takes the ordinary kernels and disturbs nothing."""
    def sequence(option):
        law, grid, _, dt = hs48
        dg = _model(cm, hs48, option)
        Q = torch.from_numpy(_perturbed(law, grid, dg.state_auxiliary.cpu().numpy())).to("cuda:0")
        solver = cm.odesolvers.LSRK54CarpenterKennedy(dg, Q, dt=dt)
        T = dg.create_state()
        torch.cuda.synchronize()
        solver.dostep(Q, nsteps=1)
        dg.synchronize()
        dg(T, Q, solver.t, 1.0, 0.0)
        mid = _snapshot(dg, solver, Q) + (_bits(T),)
        solver.dostep(Q, nsteps=1)
        end = _snapshot(dg, solver, Q)
        used = dg.query("GRADARG_HANDOFF")
        dg.close()
        return mid + end, used
    on, used_on = sequence(1)
    off, used_off = sequence(0)
    assert used_on == 1 and used_off == 0
    assert _same(on, off)


def test_fallback_step_filter(cm, torch, hs48):
    """A step filter (bench.py --filter) rewrites Q between steps: the handle keeps the ordinary path."""
    keep = []

    def with_filter(dg):
        F = cm.mesh.filters
        keep.append(F.make_device_filter(dg, F.ExponentialFilter(hs48[1], 0, 20),
                                         F.AtmosFilterPerturbations(hs48[0])))
        dg.set_filters(step_filter=keep[-1])
    on, used_on = _run(cm, torch, hs48, 1, 2, prepare=with_filter)
    off, used_off = _run(cm, torch, hs48, 0, 2, prepare=with_filter)
    assert used_on == 0 and used_off == 0
    assert _same(on, off)


def test_fallback_handle_with_ghosts(cm, torch):
    """Rank 0 of a two-rank sphere whose only neighbour is the process itself (as in
    test_gpu_halo.py): a handle with ghost elements keeps the ordinary path."""
    hs = _workload(cm, 2, 2, rank=0, size=2)
    grid = hs[1]
    nn = len(grid.nabrtorank)
    send = np.asarray(grid.nabrtovmapsend).reshape(nn, 2)
    recv = np.asarray(grid.nabrtovmaprecv).reshape(nn, 2)
    assert nn >= 1 and grid.nelem > grid.nreal
    assert ((send[:, 1] - send[:, 0]) == (recv[:, 1] - recv[:, 0])).all()
    grid.nabrtorank = [0] * nn

    def connect(dg):
        dg.comm_init_rccl(cm.dgmodel.rccl_unique_id(), 0, 1)
    on, used_on = _run(cm, torch, hs, 1, 1, prepare=connect)
    off, used_off = _run(cm, torch, hs, 0, 1, prepare=connect)
    assert used_on == 0 and used_off == 0
    nr = grid.nreal
    assert all(torch.equal(a[:nr], b[:nr]) for a, b in zip(on, off))


def test_fallback_law_with_gradient_flux(cm, torch):
    """The dry rising bubble (SmagorinskyLilly: USE_GF = true) on a 2x2x2 brick."""
    from helpers import rising_bubble_setup
    setup = rising_bubble_setup(nx=2, ny=2, nz=2)
    law, grid = setup[0], setup[1]
    out = []
    for option in (1, 0):
        dg = cm.dgmodel.DGModel(law, grid, direction=0, device="cuda:0")
        dg.set_option(cm._lib.OPT_GRADARG_HANDOFF, option)
        Q = dg.init_ode_state(0.0)
        solver = cm.odesolvers.LSRK54CarpenterKennedy(dg, Q, dt=0.01)
        solver.dostep(Q, nsteps=1)
        out.append(_snapshot(dg, solver, Q))
        assert dg.query("GRADARG_HANDOFF") == 0
        dg.close()
    assert _same(out[0], out[1])


def test_against_the_oracle(cm, torch, oracle):
    """Two steps on the 6x3x3x2 sphere of bench.parity_check with the hand-off on, against
    O.lsrk54_step at the project's tolerance for it."""
    O = oracle
    law, grid, direction, dt = hs = _workload(cm, 3, 2)
    dg = _model(cm, hs, 1)
    odg = O.OracleDGModel(law, grid, nf_first=0, direction=direction[0],
                          diffusion_direction=direction[1])
    Q0 = _perturbed(law, grid, odg.state_auxiliary)
    Q = torch.from_numpy(Q0.copy()).to("cuda:0")
    solver = cm.odesolvers.LSRK54CarpenterKennedy(dg, Q, dt=dt)
    solver.dostep(Q, nsteps=2)
    dg.synchronize()
    assert dg.query("GRADARG_HANDOFF") == 1
    Qo, dQo = Q0.copy(), np.zeros_like(Q0)
    for s in range(2):
        O.lsrk54_step(odg, Qo, dQo, s * dt, dt)
    Qg = Q.cpu().numpy()
    nr = grid.nreal
    err = [float(np.abs(Qg[:nr, s] - Qo[:nr, s]).max() / np.abs(Qo[:nr, s]).max()) for s in range(law.ns)]
    print("state rel Linf per state after 2 steps:", err)
    dg.close()
    assert max(err) < 1e-12, err
