"""Split-explicit barotropic / baroclinic ocean stepper on the GPU (BASELINE config 5):
the exchange functions and whole slow steps against the oracle, and the reference's five
regression runs (test/Ocean/SplitExplicit/test_spindown_long.jl + StateCheck tables) end to end
on the device through ``cmdg_split_explicit_step``.  ``-m gpu``."""
import numpy as np
import pytest

from helpers import (check_split_explicit_table, rel_linf, split_explicit_fields,
                     split_explicit_schedule, split_explicit_setup)
from ocean_orders_cases import (check_exchange_functions, check_split_explicit_steps,
                                close_split_explicit_pair, scaled_linf, split_explicit_device_pair,
                                split_explicit_oracle_pair)
from test_split_explicit_oracle import GOLD, relaxed

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


def _device_pair(cm, torch, law3, g3, law2, g2):
    return split_explicit_device_pair(cm, law3, g3, law2, g2)


def _oracle_pair(cm, oracle, law3, g3, law2, g2):
    return split_explicit_oracle_pair(cm, oracle, law3, g3, law2, g2)


_close = close_split_explicit_pair
_scaled = scaled_linf


def test_exchange_functions_match_oracle(cm, oracle, torch):
    check_exchange_functions(cm, oracle, torch)


@pytest.mark.parametrize("coupled,dt_slow", [(True, 1800.0), (True, 300.0), (False, 300.0)])
def test_split_explicit_steps_match_oracle(cm, oracle, torch, coupled, dt_slow):
    check_split_explicit_steps(cm, oracle, torch, coupled, dt_slow)


@pytest.mark.parametrize("name,coupled,dt_slow", [
    ("uncoupled", False, 300.0), ("coupled", True, 300.0), ("thirty_minutes", True, 1800.0),
    ("sixty_minutes", True, 3600.0), ("ninety_minutes", True, 5400.0)])
def test_device_split_explicit_reproduces_reference_tables(cm, oracle, torch, name, coupled,
                                                           dt_slow):
    """test_spindown_long.jl: one simulated day, all five configurations, checked against the
    reference's StateCheck rows and the analytic-solution bound of run_split_explicit."""
    law3, g3, law2, g2 = split_explicit_setup(coupled)
    dg3, dg2, keep = _device_pair(cm, torch, law3, g3, law2, g2)
    Q3g, Q2g = dg3.init_ode_state(0.0), dg2.init_ode_state(0.0)
    dt, nsteps = split_explicit_schedule(dt_slow)
    se = cm.ocean.SplitExplicitSolver(dg3, dg2, Q3g, Q2g, dt, 300.0)
    se.dostep(Q3g, Q2g, nsteps)
    Q3, Q2 = Q3g.cpu().numpy(), Q2g.cpu().numpy()
    A3, A2 = dg3.state_auxiliary.cpu().numpy(), dg2.state_auxiliary.cpu().numpy()
    fields = split_explicit_fields(Q3, A3, Q2, A2, g2)
    check_split_explicit_table(GOLD[name], relaxed(GOLD["parr"]), fields, slack=3.0)
    for law, g, Q, A in ((law3, g3, Q3, A3), (law2, g2, Q2, A2)):
        Qe = law.init_state_prognostic(g, A, 86400.0)
        err = np.sqrt(oracle.weighted_norm2_local(g, Q, Qe) / oracle.weighted_norm2_local(g, Qe))
        assert err < 0.005
    _close(dg3, dg2, keep)


@pytest.mark.parametrize("N_extrusion", [None, 1])
def test_shallow_water_alone_reproduces_reference_table(cm, oracle, torch, N_extrusion):
    """test/Ocean/ShallowWater/test_2D_spindown.jl on the device (five- and two-node extrusion)."""
    from test_shallow_water_oracle import GOLD as G2, plane_fields, shallow_spindown_setup
    law, grid, dt, nsteps = shallow_spindown_setup(N_extrusion)
    dg = cm.dgmodel.DGModel(law, grid,
                            numerical_flux_first_order=cm.balancelaws.CentralNumericalFluxFirstOrder)
    Q = dg.init_ode_state(0.0)
    solver = cm.odesolvers.LSRK54CarpenterKennedy(dg, Q, dt=dt)
    solver.dostep(Q, nsteps=nsteps)
    dg.synchronize()
    Qn = Q.cpu().numpy()
    check_split_explicit_table(G2["explicit"], G2["parr"], plane_fields(Qn, grid), slack=2.0)
    Qe = law.init_state_prognostic(grid, dg.state_auxiliary.cpu().numpy(), 86400.0)
    err = np.sqrt(oracle.weighted_norm2_local(grid, Qn, Qe) / oracle.weighted_norm2_local(grid, Qe))
    assert err < 0.005
    dg.close()


@pytest.mark.parametrize("priority", [0, 1])
@pytest.mark.parametrize("size", [2, 3])
def test_partitioned_split_explicit_matches_single_rank(cm, torch, size, priority, monkeypatch):
    """The coupled stepper on a column partition (per-rank slow / fast pairs connected through
    the local transport, driven by cmdg_group_split_explicit_step) against the one-rank run:
    the flow deviation of ghost stacks is integrated from the received face pencils, so the
    result does not depend on the partition -- nor on the halo streams' priority (round 3's
    failure with CMDG_HALO_PRIORITY=1 was a fill of the lazily allocated LSRK work states that
    was not ordered before the first stage; test_priority_halo_streams_first_use_in_a_process)."""
    monkeypatch.setenv("CMDG_HALO_PRIORITY", str(priority))
    _partitioned_pair_against_single_rank(cm, torch, size)


def _partitioned_pair_against_single_rank(cm, torch, size, N_extrusion=None, before_launch=None):
    """Two coupled slow steps of the one-rank pair and of the ``size``-rank pairs from the same
    perturbed state, compared element by element (u, eta, u_d of the 3-D model; eta, U of the
    barotropic one).  ``before_launch(rank, slow, fast)`` sees every per-rank pair once it is
    connected and before anything runs (test_gpu_orders_partitioned.py)."""
    O = cm.ocean
    central = cm.balancelaws.CentralNumericalFluxFirstOrder
    law3, g3, law2, g2 = split_explicit_setup(True, Nx=4, Ny=3, Nz=3, N_extrusion=N_extrusion)
    dg3 = cm.dgmodel.DGModel(law3, g3)
    keep1 = O.install_hydrostatic_boussinesq_hooks(dg3)
    dg2 = cm.dgmodel.DGModel(law2, g2, numerical_flux_first_order=central)
    rng = np.random.default_rng(11)
    Q3h = law3.init_state_prognostic(g3, dg3.state_auxiliary.cpu().numpy(), 600.0)
    Q3h[:, 0:2] += 0.02 * rng.standard_normal(Q3h[:, 0:2].shape)
    Q2h = law2.init_state_prognostic(g2, dg2.state_auxiliary.cpu().numpy(), 600.0)
    by3 = {int(g): Q3h[i] for i, g in enumerate(g3.topology.globalelems[:g3.nreal])}
    by2 = {int(g): Q2h[i] for i, g in enumerate(g2.topology.globalelems[:g2.nreal])}
    Q3, Q2 = _gpu(torch, Q3h), _gpu(torch, Q2h)
    se1 = O.SplitExplicitSolver(dg3, dg2, Q3, Q2, 1800.0, 300.0)
    se1.dostep(Q3, Q2, 2)
    ref3 = {int(g): Q3[i].cpu().numpy() for i, g in enumerate(g3.topology.globalelems[:g3.nreal])}
    ref2 = {int(g): Q2[i].cpu().numpy() for i, g in enumerate(g2.topology.globalelems[:g2.nreal])}
    refud = {int(g): dg3.state_auxiliary[i, 4:6].cpu().numpy()
             for i, g in enumerate(g3.topology.globalelems[:g3.nreal])}
    slows, fasts, Q3s, Q2s, grids, keeps = [], [], [], [], [], []
    for r in range(size):
        l3, gr3, l2, gr2 = split_explicit_setup(True, Nx=4, Ny=3, Nz=3, N_extrusion=N_extrusion,
                                                rank=r, size=size)
        assert gr2.nreal * 3 == gr3.nreal and (gr3.nelem - gr3.nreal) == 3 * (gr2.nelem - gr2.nreal)
        d3 = cm.dgmodel.DGModel(l3, gr3)
        keeps.append(O.install_hydrostatic_boussinesq_hooks(d3))
        d2 = cm.dgmodel.DGModel(l2, gr2, numerical_flux_first_order=central)
        q3 = np.full((gr3.nelem, 4, gr3.Np), np.nan)
        for i, g in enumerate(gr3.topology.globalelems[:gr3.nreal]):
            q3[i] = by3[int(g)]
        q2 = np.full((gr2.nelem, 3, gr2.Np), np.nan)
        for i, g in enumerate(gr2.topology.globalelems[:gr2.nreal]):
            q2[i] = by2[int(g)]
        slows.append(d3)
        fasts.append(d2)
        grids.append((gr3, gr2))
        Q3s.append(_gpu(torch, q3))
        Q2s.append(_gpu(torch, q2))
    cm.dgmodel.connect_local(slows)
    cm.dgmodel.connect_local(fasts)
    if before_launch is not None:
        for r in range(size):
            before_launch(r, slows[r], fasts[r])
    solvers = [O.SplitExplicitSolver(d3, d2, q3, q2, 1800.0, 300.0)
               for d3, d2, q3, q2 in zip(slows, fasts, Q3s, Q2s)]
    torch.cuda.synchronize()
    O.SplitExplicitSolver.group_dostep(solvers, Q3s, Q2s, 2)
    for (gr3, gr2), d3, q3, q2 in zip(grids, slows, Q3s, Q2s):
        q3n, q2n, aud = q3.cpu().numpy(), q2.cpu().numpy(), d3.state_auxiliary[:, 4:6].cpu().numpy()
        for i, g in enumerate(gr3.topology.globalelems[:gr3.nreal]):
            for s in (0, 2):
                sc = max(np.abs(ref3[int(g)][s]).max(), 1e-3)
                assert np.abs(q3n[i, s] - ref3[int(g)][s]).max() / sc < 1e-11, (s, i)
            assert np.abs(aud[i] - refud[int(g)]).max() < 1e-11
        for i, g in enumerate(gr2.topology.globalelems[:gr2.nreal]):
            for s in (0, 1):
                sc = max(np.abs(ref2[int(g)][s]).max(), 1e-3)
                assert np.abs(q2n[i, s] - ref2[int(g)][s]).max() / sc < 1e-11, (s, i)
    for d3, k in zip(slows + [dg3], keeps + [keep1]):
        d3.set_rhs_hooks()
        for f in k:
            f.close()
        d3.close()
    for d2 in fasts + [dg2]:
        d2.close()


def test_group_step_failure_names_the_pair(cm, torch):
    """A fast handle of the wrong grid as pair 1 (the one-rank barotropic operator next to a rank-1
    slow model): the coupling check of pair 1 fails before anything is launched, and every handle
    of the call -- the wrapper reads slows[0] -- carries the reason and the pair that failed."""
    O = cm.ocean
    central = cm.balancelaws.CentralNumericalFluxFirstOrder
    law2, g2 = split_explicit_setup(True, Nx=4, Ny=3, Nz=3)[2:]
    dg2 = cm.dgmodel.DGModel(law2, g2, numerical_flux_first_order=central)
    slows, fasts, keeps = [], [], []
    for r in range(2):
        l3, gr3, l2, gr2 = split_explicit_setup(True, Nx=4, Ny=3, Nz=3, rank=r, size=2)
        slows.append(cm.dgmodel.DGModel(l3, gr3))
        keeps.append(O.install_hydrostatic_boussinesq_hooks(slows[-1]))
        fasts.append(cm.dgmodel.DGModel(l2, gr2, numerical_flux_first_order=central))
    cm.dgmodel.connect_local(slows)
    cm.dgmodel.connect_local(fasts)
    pair_fast = [fasts[0], dg2]
    Q3s = [d.create_state() for d in slows]
    Q2s = [d.create_state() for d in pair_fast]
    solvers = [O.SplitExplicitSolver(d3, d2, q3, q2, 1800.0, 300.0)
               for d3, d2, q3, q2 in zip(slows, pair_fast, Q3s, Q2s)]
    with pytest.raises(cm._lib.CmdgError) as err:
        O.SplitExplicitSolver.group_dostep(solvers, Q3s, Q2s, 1)
    msg = str(err.value)
    assert "one element per stack" in msg and "pair 1" in msg, msg
    for d3, k in zip(slows, keeps):
        d3.set_rhs_hooks()
        for f in k:
            f.close()
        d3.close()
    for d2 in fasts + [dg2]:
        d2.close()


def test_priority_halo_streams_first_use_in_a_process():
    """Round 3's ordering failure showed only on the FIRST partitioned step of a process (later
    handles found the freed work states' pages still holding valid numbers): a fresh process with
    high-priority halo streams, three handle generations, each equal to the one-rank run."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, CMDG_HALO_PRIORITY="1")
    env.pop("CMDG_DBG_WORK_MEMSET", None)
    r = subprocess.run([sys.executable, os.path.join(root, "scripts", "probe", "priority_order_diag.py")],
                       capture_output=True, text=True, timeout=600, env=env, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("trial") and "worst" in l]
    assert len(lines) == 3 and all(l.endswith("OK") for l in lines), r.stdout[-2000:]


def test_rotating_box_split_explicit_meets_the_reference_bound(cm, oracle, torch):
    """test/Ocean/SplitExplicit/test_coriolis.jl: the rotating box (f = f_o in both models),
    coupled, 15 simulated days of 300 s steps; the reference's criterion is the distance to the
    analytic inertia-gravity solution, < 0.005 for the 3-D and the 2-D state
    (split_explicit.jl:100-106)."""
    O = cm.ocean
    law3, g3, law2, g2 = split_explicit_setup(True, rotating=True, N_extrusion=1)
    dg3 = cm.dgmodel.DGModel(law3, g3)
    keep = O.install_hydrostatic_boussinesq_hooks(dg3)
    dg2 = cm.dgmodel.DGModel(law2, g2,
                             numerical_flux_first_order=cm.balancelaws.CentralNumericalFluxFirstOrder)
    Q3g, Q2g = dg3.init_ode_state(0.0), dg2.init_ode_state(0.0)
    se = O.SplitExplicitSolver(dg3, dg2, Q3g, Q2g, 300.0, 300.0)
    se.dostep(Q3g, Q2g, 15 * 288)
    for law, g, Q, dg in ((law3, g3, Q3g, dg3), (law2, g2, Q2g, dg2)):
        Qn = Q.cpu().numpy()
        Qe = law.init_state_prognostic(g, dg.state_auxiliary.cpu().numpy(), 15 * 86400.0)
        err = np.sqrt(oracle.weighted_norm2_local(g, Qn, Qe) / oracle.weighted_norm2_local(g, Qe))
        assert err < 0.005, err
    assert np.abs(Q3g.cpu().numpy()[:, 1]).max() > 1e-3       # the Coriolis force built up v
    dg3.set_rhs_hooks()
    for f in keep:
        f.close()
    dg3.close()
    dg2.close()


def test_rotating_split_explicit_steps_match_oracle(cm, oracle, torch):
    law3, g3, law2, g2 = split_explicit_setup(True, Nx=3, Ny=2, Nz=3, rotating=True)
    o3, o2 = _oracle_pair(cm, oracle, law3, g3, law2, g2)
    dg3, dg2, keep = _device_pair(cm, torch, law3, g3, law2, g2)
    Q3 = law3.init_state_prognostic(g3, o3.state_auxiliary, 0.0)
    Q2 = law2.init_state_prognostic(g2, o2.state_auxiliary, 0.0)
    Q3g, Q2g = _gpu(torch, Q3), _gpu(torch, Q2)
    se_o = oracle.SplitExplicitOracle(o3, o2, Q3, Q2, 1800.0, 300.0)
    se = cm.ocean.SplitExplicitSolver(dg3, dg2, Q3g, Q2g, 1800.0, 300.0)
    t = 0.0
    for _ in range(3):
        se_o.dostep(Q3, Q2, t)
        t += 1800.0
    se.dostep(Q3g, Q2g, 3)
    Qn3, Qn2 = Q3g.cpu().numpy(), Q2g.cpu().numpy()
    for s in (0, 1, 2):
        assert _scaled(Qn3[:, s], Q3[:, s]) < TOL, s
    for s in (0, 1, 2):
        assert _scaled(Qn2[:, s], Q2[:, s]) < TOL, s
    _close(dg3, dg2, keep)


def test_full_size_ocean_box_properties(cm, torch):
    """BASELINE configs[4] at the size ``bench.py --workload ocean-split-explicit`` runs
    (48 x 48 x 16 elements, 36 864 three-dimensional elements, 2 304 columns), where the oracle is
    too slow: (1) determinism -- two runs of two slow steps from the same state are bit identical
    (every accumulation has a fixed order, the two streams are ordered by events); (2) the
    barotropic continuity equation conserves the volume: the integral of eta over the periodic
    box stays at its initial value to rounding; (3) everything stays finite."""
    import bench
    law3, g3, law2, g2, dt_slow, dt_fast = bench.ocean_setup(cm, 48, 16)
    assert g3.nreal == 36864 and g2.nreal == 2304
    runs = []
    for _ in range(2):
        dg3, dg2, keep = _device_pair(cm, torch, law3, g3, law2, g2)
        Q3, Q2 = dg3.init_ode_state(0.0), dg2.init_ode_state(0.0)
        M2 = dg2._vgeo[:g2.nreal, 9, :]
        eta0 = (M2 * Q2[:g2.nreal, 0, :]).sum().item()
        scale = (M2 * Q2[:g2.nreal, 0, :].abs()).sum().item()
        se = cm.ocean.SplitExplicitSolver(dg3, dg2, Q3, Q2, dt_slow, dt_fast)
        se.dostep(Q3, Q2, 2)
        eta1 = (M2 * Q2[:g2.nreal, 0, :]).sum().item()
        assert abs(eta1 - eta0) < 1e-11 * scale, (eta0, eta1, scale)
        assert torch.isfinite(Q3[:g3.nreal]).all() and torch.isfinite(Q2[:g2.nreal]).all()
        assert (Q2[:g2.nreal, 0, :] != dg2.init_ode_state(0.0)[:g2.nreal, 0, :]).any()
        runs.append((Q3[:g3.nreal].clone(), Q2[:g2.nreal].clone()))
        _close(dg3, dg2, keep)
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_split_explicit_through_rccl_equals_device_copies(cm, torch):
    """The partitioned split-explicit step as ``bench.py --workload ocean-split-explicit --gpus N``
    runs it -- one (slow, fast) pair per process, each model with its own RCCL communicator --
    rehearsed on one GPU: rank 0 of a 2-rank box with itself as every neighbour.  The ghost data
    is then the rank's own, so the numbers mean nothing physically, but every exchange of both
    models (Q and the gradient flux of the 3-D model with its hooks on the ghost stacks, Q and the
    gradient flux of the barotropic model, direct and pipelined) goes through ncclSend / ncclRecv
    groups, and must give what the same exchanges give through device copies, bit for bit."""
    import bench
    out = []
    for transport in ("rccl", "local"):
        law3, g3, law2, g2, dt_slow, dt_fast = bench.ocean_setup(cm, 4, 3, rank=0, size=2,
                                                                  connectivity="face")
        for g in (g3, g2):
            nn = len(g.nabrtorank)
            send = np.asarray(g.nabrtovmapsend).reshape(nn, 2)
            recv = np.asarray(g.nabrtovmaprecv).reshape(nn, 2)
            assert nn >= 1 and all(send[n][1] - send[n][0] == recv[n][1] - recv[n][0] for n in range(nn))
            g.nabrtorank = [0] * nn
        dg3, dg2, keep = _device_pair(cm, torch, law3, g3, law2, g2)
        if transport == "rccl":
            for d in (dg3, dg2):
                d.comm_init_rccl(cm.dgmodel.rccl_unique_id(), 0, 1)
        else:
            cm.dgmodel.connect_local([dg3])
            cm.dgmodel.connect_local([dg2])
        Q3, Q2 = dg3.init_ode_state(0.0), dg2.init_ode_state(0.0)
        se = cm.ocean.SplitExplicitSolver(dg3, dg2, Q3, Q2, dt_slow, dt_fast)
        if transport == "rccl":
            se.dostep(Q3, Q2, 2)
        else:
            cm.ocean.SplitExplicitSolver.group_dostep([se], [Q3], [Q2], 2)
        assert dg2.query("DIRECT_SEND") == 1 and dg2.query("HALO_PIPELINE") == 1
        assert dg3.query("DIRECT_SEND") == 1 and dg3.query("DIRECT_RECV") == 0      # hooks: unpacked
        out.append((Q3[:g3.nreal].clone(), Q2[:g2.nreal].clone()))
        assert torch.isfinite(out[-1][0]).all() and torch.isfinite(out[-1][1]).all()
        _close(dg3, dg2, keep)
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])

