"""Device reductions of state arrays (cmdg_reduce, reductions.py): MPIStateArrays.jl:583-807 --
weightedsum in double-double, dot, p-norms with and without dims = (1, 3), euclidean_distance,
sum / maximum / minimum, all-reduced across ranks -- and the conservation callback built on them
(Callbacks.jl:415-440)."""
import ctypes as C
import math

import numpy as np
import pytest

from helpers import held_suarez_setup, pseudo1d_setup

pytestmark = pytest.mark.gpu
VM = 9


def _gpu(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _M(grid):
    return grid.vgeo[: grid.nreal, VM, :]


# ---- exact references ------------------------------------------------------------------------
def _split(a):
    c = 134217729.0 * a                  # Veltkamp: 2^27 + 1
    hi = c - (c - a)
    return hi, a - hi


def _two_prod(a, b):
    """Dekker: p + e == a * b exactly (numpy has no fma)"""
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return p, e


def _exact_wsum(M, A):
    """the correctly rounded sum of M .* A over every entry, A (nreal, ns, Np)"""
    p, e = _two_prod(np.broadcast_to(M[:, None, :], A.shape), A)
    return math.fsum(np.concatenate([p.reshape(-1), e.reshape(-1)]))


def _ulps(x, ref):
    return abs(x - ref) / math.ulp(ref)


def _cancelling_state(grid, ns, seed):
    """per state: sum of M .* A is about 1e-11 of sum |M .* A| (condition number ~1e11: far
    beyond double, well inside double-double's ~1e-32)"""
    rng = np.random.default_rng(seed)
    nr, M = grid.nreal, _M(grid)
    Q = np.zeros((grid.nelem, ns, grid.Np))
    A = rng.standard_normal((nr, ns, grid.Np)) * 10.0 ** rng.integers(-3, 4, (nr, ns, grid.Np))
    j = np.unravel_index(np.argmax(M), M.shape)
    for s in range(ns):
        for _ in range(3):              # each pass removes what is left, down to rounding
            S = _exact_wsum(M, A[:, s:s + 1])
            A[j[0], s, j[1]] -= S / M[j]
        # then put back a remainder of 1e-11 of the magnitude, on a node of its own
        A[0, s, 0] += (-1) ** s * 1e-11 * np.abs(M[:, None, :] * A[:, s:s + 1]).sum() / M[0, 0]
    Q[:nr] = A
    return Q


@pytest.fixture(scope="module")
def sphere(cm, torch):
    law, grid, d, dd = held_suarez_setup(n_horz=3, n_vert=2)
    dg = cm.dgmodel.DGModel(law, grid, direction=d, diffusion_direction=dd)
    yield law, grid, dg
    dg.close()


@pytest.fixture(scope="module")
def cancel(sphere, torch):
    law, grid, dg = sphere
    Q = _cancelling_state(grid, 5, 1)
    return Q, _gpu(torch, Q)


# ---- 1. weightedsum is exact -----------------------------------------------------------------
def test_weightedsum_is_exact_on_cancelling_data(cm, sphere, cancel):
    R = cm.reductions
    law, grid, dg = sphere
    Q, Qd = cancel
    nr, M = grid.nreal, _M(grid)
    A = Q[:nr]
    for states in (None, [2], [1, 3, 5], [5, 4]):
        cols = [s - 1 for s in states] if states else list(range(5))
        exact = _exact_wsum(M, A[:, cols])
        terms = (M[:, None, :] * A[:, cols]).reshape(-1)
        assert 1e10 <= np.abs(terms).sum() / abs(exact) <= 1e13   # the data cancels
        dev = R.weightedsum(dg, Qd, states)
        assert _ulps(dev, exact) <= 1.0, (states, dev, exact)
        assert _ulps(float(np.sum(terms)), exact) >= 1000          # plain double sums are far off
    # the top-level export is the same function
    assert cm.weightedsum(dg, Qd, [2]) == R.weightedsum(dg, Qd, [2])
    for s in range(1, 6):
        exact = _exact_wsum(M, A[:, s - 1:s])
        assert _ulps(R.weightedsum(dg, Qd, [s]), exact) <= 1.0


# ---- 2. the reference's reduction cases (test/Arrays/reductions.jl:14-55) ----------------------
def test_reference_reduction_cases(cm, sphere, torch):
    R = cm.reductions
    law, grid, dg = sphere
    nr, Np, ns = grid.nreal, grid.Np, 5
    # A = reshape(1:prod(localsize), localsize) in the (Np, nstate, nelem) memory image
    A = np.arange(1, Np * ns * nr + 1, dtype=np.float64).reshape(nr, ns, Np)
    B = np.arange(Np * ns * nr, 0, -1, dtype=np.float64).reshape(nr, ns, Np)
    pad = lambda X: np.concatenate([X, np.zeros((grid.nelem - nr, ns, Np))]) if grid.nelem > nr else X
    QA, QB = _gpu(torch, pad(A)), _gpu(torch, pad(B))
    fs = lambda x: math.fsum(np.asarray(x, dtype=np.float64).reshape(-1))
    assert R.norm(dg, QA, 1, False) == fs(np.abs(A))
    assert R.norm(dg, QA, 2, False) == math.sqrt(fs(A * A))         # integers: A^2 exact
    assert R.norm(dg, QA, math.inf, False) == np.abs(A).max()
    per = lambda f: np.array([f(A[:, s]) for s in range(ns)])
    assert np.array_equal(R.norm(dg, QA, 2, False, dims=(1, 3)), per(lambda X: math.sqrt(fs(X * X))))
    assert np.array_equal(R.norm(dg, QA, 1, False, dims=(1, 3)), per(lambda X: fs(np.abs(X))))
    assert np.array_equal(R.norm(dg, QA, math.inf, False, dims=(1, 3)), per(lambda X: np.abs(X).max()))
    assert R.dot(dg, QA, QB, False) == fs(A * B)                    # products < 2^53: exact
    # euclidean_distance is weighted (the weights of the grid exist)
    M = _M(grid)[:, None, :]
    ref = np.sqrt(np.sum(M.astype(np.longdouble) * (A - B).astype(np.longdouble) ** 2))
    assert _ulps(R.euclidean_distance(dg, QA, QB), float(ref)) <= 2
    # C = fill(rank + 1): sum / maximum / minimum, with and without dims
    Cn = np.full((nr, ns, Np), 1.0)
    Cn[:, 2] = 3.0
    Cn[0, 4, 7] = -2.5
    QC = _gpu(torch, pad(Cn))
    assert R.mapreduce(dg, "sum", QC) == fs(Cn)
    assert np.array_equal(R.mapreduce(dg, "sum", QC, dims=(1, 3)), [fs(Cn[:, s]) for s in range(ns)])
    assert R.mapreduce(dg, "max", QC) == 3.0 and R.mapreduce(dg, "min", QC) == -2.5
    assert list(R.mapreduce(dg, "max", QC, dims=(1, 3))) == [1.0, 1.0, 3.0, 1.0, 1.0]
    assert list(R.mapreduce(dg, "min", QC, dims=(1, 3))) == [1.0, 1.0, 3.0, 1.0, -2.5]
    with pytest.raises(ValueError):
        R.norm(dg, QA, 2, dims=(1, 2))


# ---- 3. weighted norms and dot -----------------------------------------------------------------
@pytest.mark.parametrize("p", [1.0, 2.0, 3.5])
def test_weighted_norm_and_dot(cm, sphere, torch, p):
    R = cm.reductions
    law, grid, dg = sphere
    rng = np.random.default_rng(int(p * 10))
    Q = rng.standard_normal((grid.nelem, 5, grid.Np)) * 3.0
    P = rng.standard_normal((grid.nelem, 5, grid.Np))
    Qd, Pd = _gpu(torch, Q), _gpu(torch, P)
    nr = grid.nreal
    M = _M(grid)[:, None, :].astype(np.longdouble)
    A, B = Q[:nr].astype(np.longdouble), P[:nr].astype(np.longdouble)
    # the sum to a few ulp, then the finishing power in double, as the reference applies it
    # (r .^ (1 // p) with 1 / p rounded to double: for p = 3.5 that alone moves the result by
    # ln(r) * ulp(1 / p), several ulp)
    fin = lambda x: x if p == 1.0 else math.sqrt(x) if p == 2.0 else x ** (1.0 / p)
    ref = fin(float(np.sum(M * np.abs(A) ** p)))
    assert _ulps(R.norm(dg, Qd, p), ref) <= 4
    refs = [fin(float(np.sum(M[:, 0] * np.abs(A[:, s]) ** p))) for s in range(5)]
    per = R.norm(dg, Qd, p, dims=(1, 3))
    assert all(_ulps(x, r) <= 4 for x, r in zip(per, refs)), (per, refs)
    refd = float(np.sum(M * A * B))
    assert abs(R.dot(dg, Qd, Pd) - refd) <= 4 * math.ulp(refd) + 1e-18 * float(np.sum(np.abs(M * A * B)))
    assert R.norm(dg, Qd, math.inf, True) == R.norm(dg, Qd, math.inf, False) == np.abs(Q[:nr]).max()


# ---- 4. ghosts and NaN -------------------------------------------------------------------------
def test_ghosts_are_never_read_and_nan_propagates(cm, torch):
    R = cm.reductions
    law, grid, d, dd = held_suarez_setup(n_horz=3, n_vert=2, rank=0, size=2)
    assert grid.nelem > grid.nreal
    dg = cm.dgmodel.DGModel(law, grid, direction=d, diffusion_direction=dd)
    nr = grid.nreal
    Q = np.random.default_rng(9).standard_normal((grid.nelem, 5, grid.Np)) + 0.5
    Q[nr:] = 0.0
    G = Q.copy()
    G[nr:] = np.nan
    Qd, Gd = _gpu(torch, Q), _gpu(torch, G)
    calls = [lambda X: R.weightedsum(dg, X), lambda X: R.norm(dg, X, 2), lambda X: R.norm(dg, X, 3.5),
             lambda X: R.norm(dg, X, math.inf), lambda X: R.mapreduce(dg, "sum", X),
             lambda X: R.mapreduce(dg, "max", X), lambda X: R.mapreduce(dg, "min", X),
             lambda X: R.dot(dg, X, X), lambda X: R.euclidean_distance(dg, X, 2 * X),
             lambda X: R.mapreduce(dg, "max", X, dims=(1, 3)), lambda X: R.norm(dg, X, 1, dims=(1, 3))]
    for f in calls:
        a, b = np.asarray(f(Qd)), np.asarray(f(Gd))
        assert np.isfinite(b).all() and np.array_equal(a, b)
    G[nr // 2, 3, 17] = np.nan
    Gd = _gpu(torch, G)
    for f in calls[:9]:
        assert math.isnan(f(Gd))
    for f in calls[9:]:
        v = f(Gd)
        assert math.isnan(v[3]) and np.isfinite(np.delete(v, 3)).all()
    dg.close()


# ---- 5. partition invariance -------------------------------------------------------------------
def _ops(R):
    one = [("weightedsum", lambda d, A, B: R.weightedsum(d, A), lambda g, A, B: R.group_weightedsum(g, A)),
           ("weightedsum[2,4]", lambda d, A, B: R.weightedsum(d, A, [2, 4]),
            lambda g, A, B: R.group_weightedsum(g, A, [2, 4])),
           ("dot", lambda d, A, B: R.dot(d, A, B), lambda g, A, B: R.group_dot(g, A, B)),
           ("dot unweighted", lambda d, A, B: R.dot(d, A, B, False), lambda g, A, B: R.group_dot(g, A, B, False)),
           ("distance", lambda d, A, B: R.euclidean_distance(d, A, B),
            lambda g, A, B: R.group_euclidean_distance(g, A, B))]
    for p in (1, 2, 3.5, math.inf):
        for w in (True, False):
            for dims in (None, (1, 3)):
                one.append(("norm %s %s %s" % (p, w, dims),
                            lambda d, A, B, p=p, w=w, dims=dims: R.norm(d, A, p, w, dims),
                            lambda g, A, B, p=p, w=w, dims=dims: R.group_norm(g, A, p, w, dims)))
    for op in ("sum", "max", "min"):
        for dims in (None, (1, 3)):
            one.append(("%s %s" % (op, dims), lambda d, A, B, op=op, dims=dims: R.mapreduce(d, op, A, dims),
                        lambda g, A, B, op=op, dims=dims: R.group_mapreduce(g, op, A, dims)))
    return one


@pytest.mark.parametrize("size", [2, 3])
def test_group_reduce_equals_single_handle_bit_for_bit(cm, sphere, cancel, torch, size):
    R = cm.reductions
    law, grid, dg = sphere
    Q, Qd = cancel
    P = np.random.default_rng(12).standard_normal(Q.shape)
    Pd = _gpu(torch, P)
    gl = grid.topology.globalelems[: grid.nreal]
    byQ = {int(g): Q[i] for i, g in enumerate(gl)}
    byP = {int(g): P[i] for i, g in enumerate(gl)}
    dgs, Qs, Ps = [], [], []
    for r in range(size):
        lr, gr, d, dd = held_suarez_setup(n_horz=3, n_vert=2, rank=r, size=size)
        dgs.append(cm.dgmodel.DGModel(lr, gr, direction=d, diffusion_direction=dd))
        q = np.full((gr.nelem, 5, gr.Np), np.nan)           # ghosts NaN: never read
        p = np.full((gr.nelem, 5, gr.Np), np.nan)
        for i, g in enumerate(gr.topology.globalelems[: gr.nreal]):
            q[i], p[i] = byQ[int(g)], byP[int(g)]
        Qs.append(_gpu(torch, q))
        Ps.append(_gpu(torch, p))
    cm.dgmodel.connect_local(dgs)
    for name, single, group in _ops(R):
        a, b = np.asarray(single(dg, Qd, Pd)), np.asarray(group(dgs, Qs, Ps))
        assert np.isfinite(a).all(), name
        assert np.array_equal(a, b), (name, a, b)
    # a rank of a connected group is refused by cmdg_reduce, with the entry to use instead
    with pytest.raises(cm._lib.CmdgError, match="cmdg_group_reduce"):
        R.weightedsum(dgs[0], Qs[0])
    for d in dgs:
        d.close()


# ---- 6. the RCCL path --------------------------------------------------------------------------
def test_rccl_reduce_equals_local_bit_for_bit(cm, sphere, cancel, torch):
    R = cm.reductions
    law, grid, dg = sphere
    Q, Qd = cancel
    Pd = _gpu(torch, np.random.default_rng(13).standard_normal(Q.shape))
    lr, gr, d, dd = held_suarez_setup(n_horz=3, n_vert=2)
    dgr = cm.dgmodel.DGModel(lr, gr, direction=d, diffusion_direction=dd)
    dgr.comm_init_rccl(cm.dgmodel.rccl_unique_id(), 0, 1)
    for name, single, _ in _ops(R):
        a, b = np.asarray(single(dg, Qd, Pd)), np.asarray(single(dgr, Qd, Pd))
        assert np.array_equal(a, b), (name, a, b)
    # cmdg_reduce_local + cmdg_reduce_combine is what cmdg_reduce does on one rank
    desc, keep = R.make_desc(cm._lib.RED_WEIGHTEDSUM, 5)
    parts = R.reduce_local(dgr, desc, Qd)
    assert parts.shape == (1, 2) and parts[0, 1] != 0.0       # the low part carries information
    assert R.combine(desc, parts[None])[0] == R.weightedsum(dgr, Qd)
    dgr.close()


def test_device_entries_refuse_bad_arguments(cm, sphere, cancel):
    R, L = cm.reductions, cm._lib
    law, grid, dg = sphere
    Q, Qd = cancel
    for p in (0.0, -2.0, float("nan")):
        with pytest.raises(L.CmdgError, match="p > 0"):
            R.norm(dg, Qd, p)
    with pytest.raises(L.CmdgError, match="out of range"):
        R.weightedsum(dg, Qd, [6])
    for op in (L.RED_DOT, L.RED_DISTANCE):
        desc, keep = R.make_desc(op, 5)
        out = (C.c_double * 1)()
        assert dg.L.cmdg_reduce(dg.handle, C.byref(desc), Qd.data_ptr(), None, out) == -1
        assert b"need B" in dg.L.cmdg_last_error(dg.handle)


# ---- 7. determinism and ordering ---------------------------------------------------------------
def test_repeated_calls_are_bitwise_identical(cm, sphere, cancel):
    R = cm.reductions
    law, grid, dg = sphere
    Q, Qd = cancel
    for f in (lambda: R.weightedsum(dg, Qd), lambda: R.norm(dg, Qd, 3.5, dims=(1, 3)),
              lambda: R.mapreduce(dg, "max", Qd, dims=(1, 3))):
        first = np.asarray(f())
        for _ in range(9):
            assert np.array_equal(np.asarray(f()), first)


def test_weightedsum_waits_for_an_async_run(cm, torch):
    R, O = cm.reductions, cm.odesolvers
    law, grid, d, dd = held_suarez_setup(n_horz=3, n_vert=2)
    dg = cm.dgmodel.DGModel(law, grid, direction=d, diffusion_direction=dd)
    dg.set_option(cm._lib.OPT_ASYNC_RUN, 1)
    Q = dg.init_ode_state(0.0)
    rng = np.random.default_rng(4)
    Q[:, 1:4] += 2.0 * Q[:, 0:1] * _gpu(torch, rng.standard_normal((grid.nelem, 3, grid.Np)))
    before = R.weightedsum(dg, Q, [2])
    s = O.LSRK54CarpenterKennedy(dg, Q, dt=0.2)
    dg.lsrk_run(Q, s.dQ, 0.0, 0.2, 20, s.RKA, s.RKB, s.RKC)
    right_after = R.weightedsum(dg, Q, [2])              # issued while the run may still be queued
    dg.synchronize()
    assert right_after == R.weightedsum(dg, Q, [2])
    assert right_after != before                          # the run changed the momentum
    dg.set_option(cm._lib.OPT_ASYNC_RUN, 0)
    dg.close()


# ---- 8. conservation through the device sum ----------------------------------------------------
@pytest.fixture(scope="module")
def box(cm, torch):
    law, grid, _ = pseudo1d_setup(Ne=3)
    dg = cm.dgmodel.DGModel(law, grid)
    yield law, grid, dg
    dg.close()


@pytest.mark.parametrize("target", [(1,), None])
def test_tmar_filter_keeps_the_weightedsum(cm, box, torch, target):
    """filter.jl:382-392: TMAR leaves the weighted sum within 10 eps."""
    F, R = cm.mesh.filters, cm.reductions
    law, grid, dg = box
    x = grid.vgeo[:, 12, :]
    Q = _gpu(torch, (np.abs(x) - 0.1)[:, None, :])
    before = R.weightedsum(dg, Q)
    assert R.mapreduce(dg, "min", Q) < 0
    F.apply(Q, target, dg, F.TMARFilter())
    assert R.mapreduce(dg, "min", Q) >= 0
    assert math.isclose(R.weightedsum(dg, Q), before, rel_tol=10 * np.finfo(float).eps)


def test_mass_preserving_versus_regular_filter(cm, sphere, torch):
    """filter.jl:478-501: per state, the mass-preserving cutoff filter keeps weightedsum (≈) and
    the regular one does not."""
    F, R = cm.mesh.filters, cm.reductions
    law, grid, dg = sphere
    Q0 = np.random.default_rng(2).standard_normal((grid.nelem, 5, grid.Np)) + 3.0
    for cls, conserved in (("MassPreservingCutoffFilter", True), ("CutoffFilter", False)):
        Q = _gpu(torch, Q0)
        before = [R.weightedsum(dg, Q, [s]) for s in (1, 2, 3)]
        F.apply(Q, range(1, 4), dg, getattr(F, cls)(grid, 2))
        after = [R.weightedsum(dg, Q, [s]) for s in (1, 2, 3)]
        for b, a in zip(before, after):
            assert math.isclose(a, b, rel_tol=math.sqrt(np.finfo(float).eps)) == conserved


def test_cons_callback_in_solve(cm, torch):
    R, O = cm.reductions, cm.odesolvers
    law, grid, d, dd = held_suarez_setup(n_horz=3, n_vert=2)
    dg = cm.dgmodel.DGModel(law, grid, direction=d, diffusion_direction=dd)
    Q = dg.init_ode_state(0.0)
    rng = np.random.default_rng(4)
    Q[:, 1:4] += 2.0 * Q[:, 0:1] * _gpu(torch, rng.standard_normal((grid.nelem, 3, grid.Np)))
    Q0 = Q.clone()
    cb = cm.ConsCallback(dg, "ρ", 1e-10)
    calls = []
    t = O.solve(Q, O.LSRK54CarpenterKennedy(dg, Q, dt=0.2), numberofsteps=4,
                callbacks=[(1, cb), (2, lambda solver, Q, t: calls.append(t))])
    assert t == pytest.approx(0.8)
    assert cb.delta is not None and abs(cb.delta) <= 1e-10
    print("Held-Suarez, 4 LSRK54 steps: |δρ| = %.3e" % abs(cb.delta))
    assert calls == [pytest.approx(0.4), pytest.approx(0.8)]
    # without callbacks the same steps give the same state
    Q2 = Q0.clone()
    O.solve(Q2, O.LSRK54CarpenterKennedy(dg, Q2, dt=0.2), numberofsteps=4)
    assert torch.equal(Q, Q2)
    # a state perturbed between steps is caught at threshold 0
    Q3 = Q0.clone()
    nr = grid.nreal

    def perturb(solver, Q, t):
        Q[:nr, 0] *= 1.0 + 1e-9
    strict = R.ConsCallback(dg, "ρ", 0.0)
    with pytest.raises(R.ConservationError, match="δρ"):
        O.solve(Q3, O.LSRK54CarpenterKennedy(dg, Q3, dt=0.2), numberofsteps=4,
                callbacks=[(1, perturb), (1, strict)])
    with pytest.raises(ValueError):
        R.ConsCallback(dg, "q_tot", 1e-10)
    dg.close()
