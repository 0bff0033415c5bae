"""cmdg_reduce_combine (include/cmdg.h) on hand-made partials: the host half of every all-reduced
reduction (MPIStateArrays.jl:583-807).  It needs no GPU."""
import math

import numpy as np
import pytest


def _R(cm):
    return cm.reductions, cm._lib


def _dd(rng, scale):
    """a normalized double-double pair (hi, lo) with |lo| <= ulp(hi) / 2"""
    hi = rng.standard_normal() * scale
    lo = rng.uniform(-0.5, 0.5) * math.ulp(hi)
    s = hi + lo
    return s, (hi - s) + lo


def test_rank_order_combine_is_the_correctly_rounded_exact_sum(cm):
    R, L = _R(cm)
    rng = np.random.default_rng(7)
    d, _ = R.make_desc(L.RED_WEIGHTEDSUM, 5)
    for nranks in (1, 2, 3, 7, 64):
        for trial in range(40):
            # magnitudes spread over many binades and signs mixed, with cancellation
            P = np.array([[_dd(rng, 10.0 ** rng.integers(-20, 20))] for _ in range(nranks)])
            if trial % 2:
                P[-1, 0, 0] = -P[:-1, 0, 0].sum()        # the sum of the hi parts nearly cancels
            exact = math.fsum(P.reshape(-1))
            assert R.combine(d, P)[0] == exact, (nranks, trial)


def test_combine_of_extreme_cancellation_and_one_rank_per_state(cm):
    R, L = _R(cm)
    # 1e16 + 1 - 1e16 across ranks: plain double addition in rank order gives 0
    P = np.array([[[1e16, 1.0]], [[-1e16, 0.0]]])
    d, _ = R.make_desc(L.RED_SUM, 1)
    assert R.combine(d, P)[0] == 1.0
    # per state: nout = 3 partials per rank, each combined on its own
    rng = np.random.default_rng(3)
    P = np.array([[_dd(rng, 1e3) for _ in range(3)] for _ in range(4)])
    d, _ = R.make_desc(L.RED_SUM, 3, per_state=True)
    out = R.combine(d, P)
    assert out.shape == (3,)
    for o in range(3):
        assert out[o] == math.fsum(P[:, o, :].reshape(-1))
    # a subset of 2 states per state
    d, _ = R.make_desc(L.RED_WEIGHTEDSUM, 5, states=[1, 4], per_state=True)
    assert R.combine(d, P[:, :2]).shape == (2,)


def test_round_half_even_across_partials(cm):
    R, L = _R(cm)
    d, _ = R.make_desc(L.RED_SUM, 1)
    half = math.ulp(1.0) / 2
    # 1 + ulp/2 is a tie (rounds to 1); a tiny positive partial beyond it rounds up
    assert R.combine(d, np.array([[[1.0, half]], [[0.0, 0.0]]]))[0] == 1.0
    assert R.combine(d, np.array([[[1.0, half]], [[1e-300, 0.0]]]))[0] == 1.0 + 2 * half
    assert R.combine(d, np.array([[[1.0, half]], [[-1e-300, 0.0]]]))[0] == 1.0


@pytest.mark.parametrize("p", [1.0, 2.0, 3.5, 0.5])
def test_p_finishing(cm, p):
    R, L = _R(cm)
    P = np.array([[[2.0, 0.0]], [[7.25, 0.0]], [[1e-3, 0.0]]])
    s = math.fsum(P.reshape(-1))
    d, _ = R.make_desc(L.RED_NORM, 4, p=p)
    want = s if p == 1.0 else math.sqrt(s) if p == 2.0 else s ** (1.0 / p)
    assert R.combine(d, P)[0] == want
    d, _ = R.make_desc(L.RED_DISTANCE, 4)
    assert R.combine(d, P)[0] == math.sqrt(s)
    d, _ = R.make_desc(L.RED_DOT, 4)                      # dot: no power
    assert R.combine(d, P)[0] == s


def test_max_min_and_nan_propagation(cm):
    R, L = _R(cm)
    P = np.array([[[3.0, 0.0], [-1.0, 0.0]], [[5.0, 0.0], [-7.0, 0.0]], [[4.0, 0.0], [2.0, 0.0]]])
    dmax, _ = R.make_desc(L.RED_MAX, 2, per_state=True)
    dmin, _ = R.make_desc(L.RED_MIN, 2, per_state=True)
    dinf, _ = R.make_desc(L.RED_NORM, 2, p=math.inf, per_state=True)
    assert list(R.combine(dmax, P)) == [5.0, 2.0]
    assert list(R.combine(dmin, P)) == [3.0, -7.0]
    assert list(R.combine(dinf, P)) == [5.0, 2.0]          # partials are already |A| maxima
    for where in (0, 1, 2):                                 # NaN on the first, middle or last rank
        Q = P.copy()
        Q[where, 0, 0] = np.nan
        for d in (dmax, dmin, dinf):
            out = R.combine(d, Q)
            assert math.isnan(out[0]) and not math.isnan(out[1])
    dsum, _ = R.make_desc(L.RED_SUM, 2, per_state=True)
    Q = P.copy()
    Q[1, 1, 1] = np.nan
    out = R.combine(dsum, Q)
    assert not math.isnan(out[0]) and math.isnan(out[1])


def test_combine_refuses_bad_arguments(cm):
    R, L = _R(cm)
    P = np.zeros((1, 1, 2))
    for p in (0.0, -1.0, float("nan")):
        d, _ = R.make_desc(L.RED_NORM, 3, p=p)
        with pytest.raises(L.CmdgError, match="p > 0"):
            R.combine(d, P)
    d, _ = R.make_desc(L.RED_WEIGHTEDSUM, 3, states=[0, 3])
    with pytest.raises(L.CmdgError, match="out of range"):
        R.combine(d, P)
    d, _ = R.make_desc(L.RED_WEIGHTEDSUM, 3, states=[-1])
    with pytest.raises(L.CmdgError, match="out of range"):
        R.combine(d, P)
    d, _ = R.make_desc(99, 3)
    with pytest.raises(L.CmdgError, match="unknown op"):
        R.combine(d, P)
    d, _ = R.make_desc(L.RED_SUM, 0)
    with pytest.raises(L.CmdgError, match="nstate"):
        R.combine(d, P)
    lib = L.lib()
    d, _ = R.make_desc(L.RED_SUM, 1)
    import ctypes as C
    out = (C.c_double * 1)()
    assert lib.cmdg_reduce_combine(C.byref(d), P.ctypes.data, 0, out) == -1
    assert lib.cmdg_reduce_combine(None, P.ctypes.data, 1, out) == -1
    assert lib.cmdg_reduce_combine(C.byref(d), None, 1, out) == -1


def test_device_entries_refuse_without_a_handle(cm):
    """The three device entries check their handle before anything else (no GPU is touched)."""
    import ctypes as C
    R, L = _R(cm)
    lib = L.lib()
    d, _ = R.make_desc(L.RED_SUM, 1)
    out = (C.c_double * 2)()
    assert lib.cmdg_reduce(None, C.byref(d), None, None, out) == -1
    assert lib.cmdg_reduce_local(None, C.byref(d), None, None, out) == -1
    assert lib.cmdg_group_reduce(None, 1, C.byref(d), None, None, out) == -1
