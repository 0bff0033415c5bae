"""Direct stiffness summation: host-side mirror of ``ClimateMachine.Mesh.DSS``.

Reference: ``src/Numerics/Mesh/DSS.jl`` -- ``dss!`` :21-76, ``dss3d_CPU!`` :128-165,
``dss_vertex!`` :190-214, ``dss_edge!`` :244-278, ``dss_face!`` :296-316.

``dss!`` makes a DG field single-valued at the nodes that elements share: after a ghost exchange
every copy of a shared vertex, edge node or face node holds the sum over the copies (divide by
``dss`` of ones, or of the mass matrix, for an average).  The tables come from the topology
(``vtconn, vtconnoff, edgconn, edgconnoff, fcconn``, built at first access) and from the grid
(``vertmap, edgemap, facemap``); the summation is device work (``cmdg_dss_*`` of include/cmdg.h,
csrc/dss.hip) and equals the reference's host loops bit for bit.

Supported is what the reference supports: a 3-D stacked topology built with
``connectivity = "full"`` and at least three points in the vertical.  Everything else -- a 2-D
grid, ``connectivity = "face"``, an unstacked ``BrickTopology``, a vertical order below 2 (a
``DGFVModel`` grid among them), orders without an interior face node -- has ``nothing`` for a table
or a map in the reference and is refused here with ``ValueError`` before the library is called.

Tensors are in the reference's layout, ``Q (nelem, nstate, Np)`` (numpy shapes are the reversed
Julia shapes), float64, with the ghost elements in place.
"""
import ctypes as C

import numpy as np

__all__ = ["DSS", "dss", "dss_apply", "group_dss", "CmdgDssDesc"]


class CmdgDssDesc(C.Structure):
    """``cmdg_dss_desc`` of include/cmdg.h."""
    _fields_ = [
        ("Nq", C.c_int32 * 3), ("nelem", C.c_int64), ("nreal", C.c_int64),
        ("nvt", C.c_int64), ("vtconn", C.c_void_p), ("vtconnoff", C.c_void_p),
        ("nedg", C.c_int64), ("edgconn", C.c_void_p), ("edgconnoff", C.c_void_p),
        ("nfc", C.c_int64), ("fcconn", C.c_void_p),
        ("vertmap", C.c_void_p), ("edgemap", C.c_void_p), ("Nemax", C.c_int64),
        ("facemap", C.c_void_p), ("Nfmax", C.c_int64),
    ]


def check_supported(grid):
    """Raise ``ValueError`` where the reference has ``nothing`` for a DSS table or map."""
    t = grid.topology
    if grid.dim != 3:
        raise ValueError("dss: the reference sums 3-D grids only, this grid is %d-D" % grid.dim)
    if not getattr(t, "isstacked", False):
        raise ValueError("dss: needs a stacked topology (StackedBrickTopology, StackedCubedSphereTopology); "
                         "an unstacked one has no DSS tables in the reference")
    if t.elemtovert is None:
        raise ValueError('dss: the topology was built with connectivity = "face"; the DSS tables need '
                         'connectivity = "full"')
    if grid.N[2] < 2:
        raise ValueError("dss: vertical polynomial order %d; the reference has vertex, edge and face maps "
                         "from order 2 on (a DGFVModel grid has none)" % grid.N[2])
    if grid.vertmap is None or grid.edgemap is None or grid.facemap is None:
        raise ValueError("dss: polynomial orders %s have no interior face node; the reference has no face map "
                         "for them" % (tuple(grid.N),))
    if any(x is None for x in (t.vtconn, t.vtconnoff, t.edgconn, t.edgconnoff, t.fcconn)):
        raise ValueError("dss: the topology has no DSS tables")


class DSS:
    """``DSS(grid)``: the descriptor of ``grid``'s DSS tables and the ``cmdg_dss`` object made from
    it, created on a torch device at first use and freed by :meth:`close`."""

    def __init__(self, grid):
        check_supported(grid)
        t = grid.topology
        self.Nq = tuple(int(q) for q in grid.Nq)
        self.Np = int(grid.Np)
        self.nelem, self.nreal = int(t.nelem), int(t.nreal)
        i64 = lambda a: np.ascontiguousarray(a, dtype=np.int64)
        self.vtconn, self.vtconnoff = i64(t.vtconn), i64(t.vtconnoff)
        self.edgconn, self.edgconnoff = i64(t.edgconn), i64(t.edgconnoff)
        self.fcconn = i64(t.fcconn)                       # (5, nfc): Julia (nfc, 5)
        self.vertmap, self.edgemap, self.facemap = i64(grid.vertmap), i64(grid.edgemap), i64(grid.facemap)
        self._dev = {}

    def descriptor(self):
        """``cmdg_dss_desc`` over this object's host arrays (which must outlive the call)."""
        d = CmdgDssDesc()
        for i in range(3):
            d.Nq[i] = self.Nq[i]
        d.nelem, d.nreal = self.nelem, self.nreal
        d.nvt, d.vtconn, d.vtconnoff = len(self.vtconnoff) - 1, self.vtconn.ctypes.data, self.vtconnoff.ctypes.data
        d.nedg, d.edgconn, d.edgconnoff = (len(self.edgconnoff) - 1, self.edgconn.ctypes.data,
                                           self.edgconnoff.ctypes.data)
        d.nfc, d.fcconn = self.fcconn.shape[1], self.fcconn.ctypes.data
        d.vertmap = self.vertmap.ctypes.data
        d.edgemap, d.Nemax = self.edgemap.ctypes.data, self.edgemap.shape[2]
        d.facemap, d.Nfmax = self.facemap.ctypes.data, self.facemap.shape[2]
        return d

    def device_object(self, device):
        """The ``cmdg_dss`` object on torch device ``device`` (created at first use)."""
        import torch
        from .. import _lib
        device = torch.device(device)
        key = (device.type, torch.cuda.current_device() if device.index is None else device.index)
        if key not in self._dev:
            d = self.descriptor()
            h = C.c_void_p()
            with torch.cuda.device(key[1]):
                _lib.check(_lib.lib().cmdg_dss_create(None, C.byref(d), C.byref(h)))
            self._dev[key] = h
        return self._dev[key]

    def info(self, device):
        """``(groups, members, most members of one group, nodes touched)`` of the flattened tables."""
        from .. import _lib
        out = (C.c_int64 * 4)()
        _lib.check(_lib.lib().cmdg_dss_info(self.device_object(device), C.cast(out, C.c_void_p)))
        return tuple(out)

    def close(self):
        dev, self._dev = getattr(self, "_dev", {}), {}
        if dev:
            from .. import _lib
            for h in dev.values():
                _lib.lib().cmdg_dss_destroy(None, h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _of(grid_or_dss):
    """The :class:`DSS` of a grid (made once and kept on the grid) or the object itself."""
    if isinstance(grid_or_dss, DSS):
        return grid_or_dss
    obj = getattr(grid_or_dss, "_dss_object", None)
    if obj is None:
        obj = DSS(grid_or_dss)
        grid_or_dss._dss_object = obj
    return obj


def _check(Q, obj):
    import torch
    from .. import _lib
    if Q.dtype != torch.float64 or not Q.is_contiguous() or not Q.is_cuda:
        raise _lib.CmdgError("Q must be a contiguous float64 device tensor")
    if Q.dim() != 3 or Q.shape[0] != obj.nelem or Q.shape[2] != obj.Np:
        raise _lib.CmdgError("Q has shape %s: not a state of this grid, (%d, nstate, %d)"
                             % (tuple(Q.shape), obj.nelem, obj.Np))


def dss_apply(Q, grid_or_dss, dg=None):
    """The summation alone, in place (``dss3d_CPU!``): the ghost elements of ``Q`` must hold their
    owners' values.  With ``dg`` the kernel is enqueued on that model's compute stream, behind what
    is queued there, and the call returns without waiting (follow with ``dg.synchronize()``), as a
    device filter's ``apply`` does; without, it runs on the library's default stream, for any
    polynomial orders, and the call returns when it is done."""
    import torch
    from .. import _lib
    obj = _of(grid_or_dss)
    _check(Q, obj)
    it = obj.device_object(Q.device)
    h = dg.handle if dg is not None else None
    torch.cuda.current_stream(Q.device).synchronize()
    with torch.cuda.device(Q.device):
        _lib.check(_lib.lib().cmdg_dss_apply(h, it, Q.data_ptr(), Q.shape[1]), h)


def dss(Q, dg):
    """``dss!(Q, grid)`` for a state-like tensor of ``dg``: ghost exchange, then the summation;
    returns when ``Q`` is complete.  The :class:`DSS` object is kept on ``dg.grid``."""
    import torch
    from .. import _lib
    obj = _of(dg.grid)
    _check(Q, obj)
    it = obj.device_object(Q.device)
    torch.cuda.current_stream(Q.device).synchronize()
    with torch.cuda.device(Q.device):
        _lib.check(_lib.lib().cmdg_dss(dg.handle, it, Q.data_ptr(), Q.shape[1]), dg.handle)


def group_dss(dgs, Qs):
    """``dss!`` on every rank of one process (models connected with ``dgmodel.connect_local``):
    exchange on all, sum on all, wait for all (``cmdg_group_dss``)."""
    import torch
    from .. import _lib
    if len(dgs) != len(Qs) or not dgs:
        raise _lib.CmdgError("as many arrays as models, at least one")
    objs = [_of(d.grid) for d in dgs]
    for Q, obj in zip(Qs, objs):
        _check(Q, obj)
        if Q.shape[1] != Qs[0].shape[1]:
            raise _lib.CmdgError("the arrays differ in their number of states")
    n = len(dgs)
    its = (C.c_void_p * n)(*[obj.device_object(Q.device).value for obj, Q in zip(objs, Qs)])
    hs = (C.c_void_p * n)(*[d.handle for d in dgs])
    qs = (C.c_void_p * n)(*[Q.data_ptr() for Q in Qs])
    torch.cuda.current_stream(Qs[0].device).synchronize()
    with torch.cuda.device(Qs[0].device):
        _lib.check(_lib.lib().cmdg_group_dss(hs, n, its, qs, Qs[0].shape[1]), dgs[0].handle)
