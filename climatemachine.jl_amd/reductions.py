"""Reductions of state arrays, all-reduced across ranks, on the device.

Reference: ``src/Arrays/MPIStateArrays.jl``: ``weightedsum(Q, states)`` ``:655-674`` (double-double
accumulation), ``dot(Q1, Q2, weighted)`` ``:608-626``, ``norm(Q, p, weighted; dims)`` ``:583-604``
(implementations ``:676-768``), ``euclidean_distance`` ``:628-644`` and ``sum`` / ``maximum`` /
``minimum`` through ``mapreduce`` ``:775-807``; ``ConsCallback`` ``src/Driver/Callbacks/
Callbacks.jl:415-440``.

Each function takes the ``DGModel`` whose grid the array lives on (its ``vgeo`` supplies the
weights M) and calls ``cmdg_reduce``: the kernels of ``csrc/reductions.hip`` reduce this rank's
real elements in double-double, and a handle with an RCCL communicator all-gathers the partials
and combines them in rank order, so every rank returns the same bits.  Handles connected with
``dgmodel.connect_local`` (one process plays every rank) use the ``group_*`` forms.  ``dims=(1, 3)``
gives one value per state, as a numpy array.  State indices are 1-based, as in ``FilterIndices``.
"""
import ctypes as C

import numpy as np

from . import _lib

__all__ = ["weightedsum", "norm", "dot", "euclidean_distance", "mapreduce", "group_weightedsum",
           "group_norm", "group_dot", "group_euclidean_distance", "group_mapreduce", "make_desc",
           "reduce_local", "combine", "ConsCallback", "ConservationError"]

_MAPREDUCE = {"sum": _lib.RED_SUM, "max": _lib.RED_MAX, "min": _lib.RED_MIN}


def _per_state(dims):
    if dims is None or dims == slice(None):
        return False
    if tuple(dims) == (1, 3):
        return True
    raise ValueError("dims: None (one value) or (1, 3) (one value per state), not %r" % (dims,))


def make_desc(op, nstate, states=None, p=2.0, weighted=True, per_state=False):
    """``cmdg_reduce_desc`` for ``op`` (``_lib.RED_*``) over ``nstate`` columns; ``states`` are
    0-based here.  Returns ``(desc, keepalive)``."""
    d = _lib.CmdgReduceDesc()
    d.op, d.p, d.weighted = int(op), float(p), int(bool(weighted))
    d.per_state, d.nstate = int(bool(per_state)), int(nstate)
    keep = None
    if states is not None:
        keep = (C.c_int32 * len(states))(*[int(s) for s in states])
        d.states, d.nstates = C.cast(keep, C.c_void_p), len(states)
    return d, keep


def _nout(d):
    return (d.nstates if d.states else d.nstate) if d.per_state else 1


def _one(out, d):
    v = np.array(out[:], dtype=np.float64)
    return v if d.per_state else float(v[0])


def _run(dg, d, A, B):
    out = (C.c_double * _nout(d))()
    dg._torch_ready()
    _lib.check(dg.L.cmdg_reduce(dg.handle, C.byref(d), A.data_ptr(),
                                B.data_ptr() if B is not None else None, out), dg.handle)
    return _one(out, d)


def _run_group(dgs, d, As, Bs):
    L = _lib.lib()
    n = len(dgs)
    out = (C.c_double * _nout(d))()
    for g in dgs:
        g._torch_ready()
    handles = (C.c_void_p * n)(*[g.handle for g in dgs])
    pa = (C.c_void_p * n)(*[a.data_ptr() for a in As])
    pb = (C.c_void_p * n)(*[b.data_ptr() for b in Bs]) if Bs is not None else None
    _lib.check(L.cmdg_group_reduce(handles, n, C.byref(d), pa, pb, out), dgs[0].handle)
    return _one(out, d)


def _states0(states):
    if states is None:
        return None
    states = [int(s) for s in states]
    if any(s < 1 for s in states):
        raise ValueError("weightedsum: states are 1-based")
    return [s - 1 for s in states]


# ---- one handle (a single rank, or one rank of an RCCL communicator) ---------------------------
def weightedsum(dg, Q, states=None):
    """``weightedsum(Q, states)``: sum of M .* Q[:, states, :] over the real elements, accumulated
    in double-double and rounded once."""
    d, keep = make_desc(_lib.RED_WEIGHTEDSUM, Q.shape[1], _states0(states))
    return _run(dg, d, Q, None)


def norm(dg, Q, p=2, weighted=True, dims=None):
    """``norm(Q, p, weighted; dims)``: p = 1, 2, any finite p > 0 or ``math.inf`` (the weights are
    ignored for p = inf, MPIStateArrays.jl:589)."""
    d, keep = make_desc(_lib.RED_NORM, Q.shape[1], None, p, weighted, _per_state(dims))
    return _run(dg, d, Q, None)


def dot(dg, A, B, weighted=True):
    """``dot(Q1, Q2, weighted)``."""
    d, keep = make_desc(_lib.RED_DOT, A.shape[1], None, 2.0, weighted)
    return _run(dg, d, A, B)


def euclidean_distance(dg, A, B):
    """``euclidean_distance(A, B)``: sqrt(sum of M .* (A - B).^2)."""
    d, keep = make_desc(_lib.RED_DISTANCE, A.shape[1])
    return _run(dg, d, A, B)


def mapreduce(dg, op, Q, dims=None):
    """``sum(Q)`` / ``maximum(Q)`` / ``minimum(Q)`` (op ``"sum"``, ``"max"``, ``"min"``), with
    ``dims=(1, 3)`` one value per state."""
    d, keep = make_desc(_MAPREDUCE[op], Q.shape[1], None, 2.0, False, _per_state(dims))
    return _run(dg, d, Q, None)


# ---- handles connected with dgmodel.connect_local (rank r = dgs[r]) ----------------------------
def group_weightedsum(dgs, Qs, states=None):
    d, keep = make_desc(_lib.RED_WEIGHTEDSUM, Qs[0].shape[1], _states0(states))
    return _run_group(dgs, d, Qs, None)


def group_norm(dgs, Qs, p=2, weighted=True, dims=None):
    d, keep = make_desc(_lib.RED_NORM, Qs[0].shape[1], None, p, weighted, _per_state(dims))
    return _run_group(dgs, d, Qs, None)


def group_dot(dgs, As, Bs, weighted=True):
    d, keep = make_desc(_lib.RED_DOT, As[0].shape[1], None, 2.0, weighted)
    return _run_group(dgs, d, As, Bs)


def group_euclidean_distance(dgs, As, Bs):
    d, keep = make_desc(_lib.RED_DISTANCE, As[0].shape[1])
    return _run_group(dgs, d, As, Bs)


def group_mapreduce(dgs, op, Qs, dims=None):
    d, keep = make_desc(_MAPREDUCE[op], Qs[0].shape[1], None, 2.0, False, _per_state(dims))
    return _run_group(dgs, d, Qs, None)


# ---- the two halves of an all-reduce the caller does itself -----------------------------------
def reduce_local(dg, d, A, B=None):
    """``cmdg_reduce_local``: this rank's unrounded partials, an ``(nout, 2)`` array of (hi, lo)."""
    out = (C.c_double * (2 * _nout(d)))()
    dg._torch_ready()
    _lib.check(dg.L.cmdg_reduce_local(dg.handle, C.byref(d), A.data_ptr(),
                                      B.data_ptr() if B is not None else None, out), dg.handle)
    return np.array(out[:], dtype=np.float64).reshape(-1, 2)


def combine(d, partials):
    """``cmdg_reduce_combine`` (host only): ``partials`` of shape ``(nranks, nout, 2)`` in rank
    order -> ``nout`` finished values."""
    L = _lib.lib()
    P = np.ascontiguousarray(partials, dtype=np.float64)
    nranks = P.shape[0] if P.ndim == 3 else 1
    out = (C.c_double * _nout(d))()
    st = L.cmdg_reduce_combine(C.byref(d), P.ctypes.data, nranks, out)
    if st != 0:
        raise _lib.CmdgError("libcmdg: %s (%d): %s" % (
            L.cmdg_status_string(st).decode(), st, L.cmdg_last_error(None).decode()))
    return np.array(out[:], dtype=np.float64)


# ---- the conservation check (Callbacks.jl:415-440) ---------------------------------------------
class ConservationError(RuntimeError):
    pass


class ConsCallback:
    """``ConsCallback(bl, varname, error_threshold, show)``: ``init`` records Σvar₀ =
    ``weightedsum(Q, idx)``; every call computes δ = (Σvar - Σvar₀) / Σvar₀, keeps it in
    ``self.delta`` and raises ``ConservationError`` when |δ| > ``error_threshold``.  The variable
    is found by name among the law's ``state_names()``.  Use with
    ``odesolvers.solve(..., callbacks=[(every_n_steps, ConsCallback(...))])``."""

    def __init__(self, dg, varname, error_threshold, show=False):
        names = list(dg.balance_law.state_names())
        if varname not in names:
            raise ValueError("ConsCallback: %r is not a prognostic variable of the law (%s)"
                             % (varname, ", ".join(names)))
        self.dg, self.varname = dg, varname
        self.error_threshold, self.show = float(error_threshold), bool(show)
        self.states = [names.index(varname) + 1]
        self.sum0 = None
        self.delta = None

    def init(self, solver, Q, t):
        self.sum0 = weightedsum(self.dg, Q, self.states)

    def __call__(self, solver, Q, t):
        s = weightedsum(self.dg, Q, self.states)
        self.delta = (s - self.sum0) / self.sum0
        if abs(self.delta) > self.error_threshold:
            raise ConservationError("abs(δ%s) > %s" % (self.varname, self.error_threshold))
        if self.show:
            print("Conservation\n    simtime = %8.2f\n    abs(δ%s) = %.5e"
                  % (t, self.varname, abs(self.delta)))
        return None

