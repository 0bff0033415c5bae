"""Interpolation of DG states onto box and latitude-longitude grids: host-side mirror of
``ClimateMachine.Mesh.Interpolation``.

Reference: ``src/Numerics/Mesh/Interpolation.jl`` -- ``InterpolationBrick`` :132-376,
``InterpolationCubedSphere`` :700-1044, ``invert_trilear_mapping_hex!`` :1068-1251,
``interpolate_local!`` :397-570 / :1265-1317, ``project_cubed_sphere!`` :1332-1414,
``dimensions`` :572-587 / :1416-1439, ``accumulate_interpolated_data!`` :1453-1561.

The two constructors are one-time host work (numpy, vectorised over the output points; no
GPU needed).  They produce, per rank, the element offsets ``offset`` (0-based prefix sums,
``nreal + 1`` entries), the reference coordinates ``xi1, xi2, xi3`` of every local point and
its 1-based int32 index triple ``i1, i2, i3`` into the output grid -- ``(x1, x2, x3)`` for the
brick, ``(long, lat, rad)`` for the sphere.  The barycentric weights, the coincidence flags and
the scaling the reference keeps per point (``flg``, ``fac``) are the device library's business
(``cmdg_interp_*`` of include/cmdg.h, csrc/interpolation.hip).

:func:`interpolate_local`, :func:`project_cubed_sphere` and
:func:`accumulate_interpolated_data` work on torch device tensors in the reference's layouts
(numpy shapes are the reversed Julia shapes): ``Q (nelem, nstate, Np)``, ``v (nstate, Npl)``,
``fiv (nstate, n3, n2, n1)``.  Gathering the per-rank ``v`` across processes is left to the
caller; several ranks of one process are scattered into one ``fiv`` in one call.
"""
import ctypes as C
import math
from collections import OrderedDict

import numpy as np

from .topologies import equiangular_cubed_sphere_unwarp

__all__ = [
    "InterpolationBrick", "InterpolationCubedSphere",
    "invert_trilinear_mapping_hex", "trilinear_map", "sind", "cosd",
    "interpolate_local", "project_cubed_sphere", "accumulate_interpolated_data", "dimensions",
    "CmdgInterpDesc",
]

_EPS = float(np.finfo(np.float64).eps)


def sind(x):
    """``sind``: exact at multiples of 90 degrees, as Julia's (argument reduced in degrees)."""
    x = np.remainder(np.asarray(x, dtype=np.float64) + 180.0, 360.0) - 180.0   # [-180, 180)
    x = np.where(x > 90.0, 180.0 - x, np.where(x < -90.0, -180.0 - x, x))
    return np.sin(np.deg2rad(x))


def cosd(x):
    """``cosd(x) = sind(90 - |x|)`` on the reduced argument."""
    x = np.remainder(np.asarray(x, dtype=np.float64) + 180.0, 360.0) - 180.0
    return sind(90.0 - np.abs(x))


def trilinear_map(xi, X):
    """``x(xi)`` of the trilinear map of eight corners: ``xi (n, 3)``, ``X (n, 8, 3)`` with corner
    ``v`` at ``xi_d = +1`` where bit ``d`` of ``v`` is set.  Reference: Interpolation.jl:1105-1158
    (same association of the sums)."""
    p = 1 + xi
    m = 1 - xi
    m1, m2, m3 = m[:, 0, None], m[:, 1, None], m[:, 2, None]
    p1, p2, p3 = p[:, 0, None], p[:, 1, None], p[:, 2, None]
    return (m1 * (m2 * (m3 * X[:, 0] + p3 * X[:, 4]) + p2 * (m3 * X[:, 2] + p3 * X[:, 6]))
            + p1 * (m2 * (m3 * X[:, 1] + p3 * X[:, 5]) + p2 * (m3 * X[:, 3] + p3 * X[:, 7]))) / 8.0


def _ijac_times(xi, X, d):
    """``J(xi)^-1 d`` by cofactors.  Reference: Interpolation.jl:1160-1251."""
    p = 1 + xi
    m = 1 - xi
    m1, m2, m3 = m[:, 0, None], m[:, 1, None], m[:, 2, None]
    p1, p2, p3 = p[:, 0, None], p[:, 1, None], p[:, 2, None]
    # columns of the Jacobian, each (n, 3): d x / d xi_1, d xi_2, d xi_3
    c1 = (m2 * (m3 * (X[:, 1] - X[:, 0]) + p3 * (X[:, 5] - X[:, 4]))
          + p2 * (m3 * (X[:, 3] - X[:, 2]) + p3 * (X[:, 7] - X[:, 6]))) / 8.0
    c2 = (m1 * (m3 * (X[:, 2] - X[:, 0]) + p3 * (X[:, 6] - X[:, 4]))
          + p1 * (m3 * (X[:, 3] - X[:, 1]) + p3 * (X[:, 7] - X[:, 5]))) / 8.0
    c3 = (m1 * (m2 * (X[:, 4] - X[:, 0]) + p2 * (X[:, 6] - X[:, 2]))
          + p1 * (m2 * (X[:, 5] - X[:, 1]) + p2 * (X[:, 7] - X[:, 3]))) / 8.0
    J11, J21, J31 = c1[:, 0], c1[:, 1], c1[:, 2]
    J12, J22, J32 = c2[:, 0], c2[:, 1], c2[:, 2]
    J13, J23, J33 = c3[:, 0], c3[:, 1], c3[:, 2]
    C11 = J22 * J33 - J23 * J32
    C12 = -J21 * J33 + J23 * J31
    C13 = J21 * J32 - J22 * J31
    C21 = -J12 * J33 + J13 * J32
    C22 = J11 * J33 - J13 * J31
    C23 = -J11 * J32 + J12 * J31
    C31 = J12 * J23 - J13 * J22
    C32 = -J11 * J23 + J13 * J21
    C33 = J11 * J22 - J12 * J21
    det = J11 * C11 + J12 * C12 + J13 * C13
    return np.stack([(C11 * d[:, 0] + C21 * d[:, 1] + C31 * d[:, 2]) / det,
                     (C12 * d[:, 0] + C22 * d[:, 1] + C32 * d[:, 2]) / det,
                     (C13 * d[:, 0] + C23 * d[:, 1] + C33 * d[:, 2]) / det], axis=1)


def invert_trilinear_mapping_hex(X, x, tol, max_it=10):
    """Newton inverse of the trilinear map, vectorised over points: ``X (n, 8, 3)`` corners,
    ``x (n, 3)`` targets; returns ``xi (n, 3)`` clamped to ``[-1, 1]``.  Every point iterates
    until its own residual is within ``tol``, as the reference's scalar loop does.
    Reference: ``invert_trilear_mapping_hex!``, Interpolation.jl:1068-1103."""
    n = x.shape[0]
    xi = np.zeros((n, 3))
    d = trilinear_map(xi, X) - x
    act = np.flatnonzero(np.sqrt((d * d).sum(axis=1)) > tol)
    ctr = 0
    while act.size:
        Xa, xa = X[act], x[act]
        xa_i = xi[act] - _ijac_times(xi[act], Xa, d[act])
        xi[act] = xa_i
        da = trilinear_map(xa_i, Xa) - xa
        d[act] = da
        err = np.sqrt((da * da).sum(axis=1))
        ctr += 1
        if ctr > max_it and (err > tol).any():
            raise RuntimeError(
                "invert_trilinear_mapping_hex: Newton-Raphson not converging to desired tolerance "
                "after max_it = %d iterations; err = %g; toler = %g" % (max_it, err.max(), tol))
        act = act[err > tol]
    return np.clip(xi, -1.0, 1.0)


def _group_by_element(el, nreal):
    """Stable grouping of points (given in the reference's visiting order) by local element:
    returns the permutation and the 0-based prefix sums ``offset (nreal + 1)``."""
    order = np.argsort(el, kind="stable")
    offset = np.zeros(nreal + 1, dtype=np.int64)
    np.cumsum(np.bincount(el, minlength=nreal), out=offset[1:])
    return order, offset


class _Interpolation:
    """What both kinds share: the point tables and the lazily created device object."""
    is_sphere = False

    def _finish(self, grid, offset, xi, triples, dims):
        self.Nq = tuple(int(q) for q in grid.Nq)
        self.m_xi = [np.ascontiguousarray(x, dtype=np.float64) for x in grid.xi]
        self.Nel = int(grid.nreal)
        self.offset = np.ascontiguousarray(offset, dtype=np.int64)
        self.Npl = int(self.offset[-1])
        self.xi1, self.xi2, self.xi3 = (np.ascontiguousarray(x, dtype=np.float64) for x in xi)
        self.i1, self.i2, self.i3 = (np.ascontiguousarray(i, dtype=np.int32) for i in triples)
        self.dims = tuple(int(n) for n in dims)
        self.Np = int(np.prod(self.dims))
        self._dev = {}

    # -- device side -----------------------------------------------------------------
    def descriptor(self):
        """``cmdg_interp_desc`` over this object's host arrays (which must outlive the call)."""
        d = CmdgInterpDesc()
        for i in range(3):
            d.Nq[i] = self.Nq[i]
            d.xi_nodes[i] = self.m_xi[i].ctypes.data
        d.nelem, d.npoints = self.Nel, self.Npl
        d.offset = self.offset.ctypes.data
        d.xi1, d.xi2, d.xi3 = self.xi1.ctypes.data, self.xi2.ctypes.data, self.xi3.ctypes.data
        d.i1, d.i2, d.i3 = self.i1.ctypes.data, self.i2.ctypes.data, self.i3.ctypes.data
        d.n1, d.n2, d.n3 = self.dims
        if self.is_sphere:
            self._lat = np.ascontiguousarray(self.lat_grd, dtype=np.float64)
            self._long = np.ascontiguousarray(self.long_grd, dtype=np.float64)
            d.lat_grd, d.long_grd = self._lat.ctypes.data, self._long.ctypes.data
        return d

    def device_object(self, device):
        """The ``cmdg_interp`` of this object on torch device ``device`` (created at first use)."""
        import torch
        from .. import _lib
        device = torch.device(device)
        key = (device.type, torch.cuda.current_device() if device.index is None else device.index)
        if key not in self._dev:
            L = _lib.lib()
            d = self.descriptor()
            h = C.c_void_p()
            with torch.cuda.device(key[1]):
                _lib.check(L.cmdg_interp_create(None, C.byref(d), C.byref(h)))
            self._dev[key] = h
        return self._dev[key]

    def close(self):
        dev, self._dev = getattr(self, "_dev", {}), {}
        if dev:
            from .. import _lib
            for h in dev.values():
                _lib.lib().cmdg_interp_destroy(None, h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class InterpolationBrick(_Interpolation):
    """``InterpolationBrick(grid, xbnd, x1g, x2g, x3g)``: the output points are the tensor grid
    ``x1g x x2g x x3g`` (ascending).  An element takes the index range its corner extrema reach
    (tolerance ``4 eps``); a point on a shared element boundary goes to the first local element
    that reaches it (the reference's ``marker``), and ``xi = 2 (x - xmin) / (xmax - xmin) - 1``.
    Within an element the points run with ``i1`` fastest.  Reference: Interpolation.jl:132-376."""

    def __init__(self, grid, xbnd, x1g, x2g, x3g):
        toler = 4 * _EPS
        self.xbnd = np.asarray(xbnd, dtype=np.float64)
        xg = [np.ascontiguousarray(x, dtype=np.float64) for x in (x1g, x2g, x3g)]
        for x in xg:
            assert x.ndim == 1 and (np.diff(x) > 0).all(), "output grid axes must be ascending"
        self.x1g, self.x2g, self.x3g = xg
        n = [len(x) for x in xg]
        nreal = grid.nreal
        ec = np.asarray(grid.topology.elemtocoord, dtype=np.float64)[:nreal]     # (nreal, 8, 3)
        lo, hi = ec.min(axis=1), ec.max(axis=1)
        st = np.zeros((nreal, 3), dtype=np.int64)
        en = np.zeros((nreal, 3), dtype=np.int64)
        some = np.ones(nreal, dtype=bool)
        for d in range(3):
            s = np.searchsorted(xg[d], lo[:, d] - toler, side="left")    # findfirst(xg >= lo - toler)
            ok = s < n[d]
            ok &= xg[d][np.minimum(s, n[d] - 1)] <= hi[:, d] + toler
            st[:, d] = s
            en[:, d] = np.searchsorted(xg[d], hi[:, d] + toler, side="right") - 1   # findlast(<=)
            some &= ok & (en[:, d] >= s)
        # marker: the first element (lowest local number) that reaches a point owns it
        owner = np.full((n[2], n[1], n[0]), -1, dtype=np.int64)
        for el in np.flatnonzero(some)[::-1]:
            owner[st[el, 2]:en[el, 2] + 1, st[el, 1]:en[el, 1] + 1, st[el, 0]:en[el, 0] + 1] = el
        owner = owner.reshape(-1)
        lin = np.flatnonzero(owner >= 0)                  # visiting order: i1 fastest, then i2, i3
        order, offset = _group_by_element(owner[lin], nreal)
        lin = lin[order]
        el = owner[lin]
        i = [lin % n[0], (lin // n[0]) % n[1], lin // (n[0] * n[1])]
        xi = [2 * (xg[d][i[d]] - lo[el, d]) / (hi[el, d] - lo[el, d]) - 1 for d in range(3)]
        self._finish(grid, offset, xi, [k + 1 for k in i], n)


class InterpolationCubedSphere(_Interpolation):
    """``InterpolationCubedSphere(grid, vert_range, nhor, lat_grd, long_grd, rad_grd;
    nr_toler)``: latitudes and longitudes in degrees.  Every ``(rad, lat, long)`` point is
    converted to Cartesian coordinates, unwarped onto the cubed shell
    (``topologies.equiangular_cubed_sphere_unwarp``), located by the closed
    formulas for face, horizontal cell and level, mapped to this rank's local element (through
    the partitioner's ``origsendorder``) and its trilinear element map is inverted by Newton
    iteration to ``nr_toler`` (default ``10 eps vert_range[0]``).  Index triples are
    ``(long, lat, rad)``.  Reference: Interpolation.jl:700-1044."""
    is_sphere = True

    def __init__(self, grid, vert_range, nhor, lat_grd, long_grd, rad_grd, nr_toler=None):
        topl = grid.topology
        vr = np.asarray(vert_range, dtype=np.float64)
        toler1 = _EPS * vr[0] * 2.0
        toler2 = _EPS * 4.0
        if nr_toler is None:
            nr_toler = _EPS * vr[0] * 10.0
        self.nr_toler = float(nr_toler)
        self.lat_grd = np.ascontiguousarray(lat_grd, dtype=np.float64)
        self.long_grd = np.ascontiguousarray(long_grd, dtype=np.float64)
        self.rad_grd = np.ascontiguousarray(rad_grd, dtype=np.float64)
        n_lat, n_long, n_rad = len(self.lat_grd), len(self.long_grd), len(self.rad_grd)
        self.n_lat, self.n_long, self.n_rad = n_lat, n_long, n_rad
        nhor = int(nhor)
        nvert = len(vr) - 1
        nreal = grid.nreal
        nblck = nhor * nhor * nvert
        dh = 2.0 / nhor
        # global element number -> local element (glob_ord = origsendorder, :742-749)
        glob_ord = np.asarray(topl.origsendorder, dtype=np.int64)
        glob = ((glob_ord[:, None] - 1) * nvert + np.arange(1, nvert + 1)[None, :]).reshape(-1)
        glob_to_loc = np.full(6 * nblck + 1, -1, dtype=np.int64)
        glob_to_loc[glob[:nreal]] = np.arange(nreal)
        # vertical level of every radius (:762-781)
        rad = self.rad_grd
        l_nrm = np.searchsorted(vr, rad, side="right").astype(np.int64)
        low, high = rad <= vr[0], rad >= vr[-1]
        if (vr[0] - rad[low] >= toler1).any():
            raise ValueError("fatal error, rad lower than inner radius")
        if (rad[high] - vr[-1] >= toler1).any():
            raise ValueError("fatal error, rad greater than outer radius")
        l_nrm[low], l_nrm[high] = 1, nvert
        # Cartesian coordinates, visiting order rad (slowest), lat, long (fastest)
        cl, sl = cosd(self.lat_grd), sind(self.lat_grd)
        x1 = ((rad[:, None] * cl[None, :])[:, :, None] * cosd(self.long_grd)[None, None, :]).reshape(-1)
        x2 = ((rad[:, None] * cl[None, :])[:, :, None] * sind(self.long_grd)[None, None, :]).reshape(-1)
        x3 = np.broadcast_to((rad[:, None] * sl[None, :])[:, :, None], (n_rad, n_lat, n_long)).reshape(-1)
        radp = np.repeat(rad, n_lat * n_long)
        lvl = np.repeat(l_nrm, n_lat * n_long)
        uw = np.stack(equiangular_cubed_sphere_unwarp(x1, x2, x3), axis=1)
        u = uw / radp[:, None]

        def cell(a):                 # min(div(a + 1, dh) + 1, nhor) with Julia's float div
            a = a + 1
            return np.minimum(np.round((a - np.fmod(a, dh)) / dh).astype(np.int64) + 1, nhor)

        l1, l2, l3 = cell(u[:, 0]), cell(u[:, 1]), cell(u[:, 2])
        faces = [np.abs(u[:, 0] + 1) < toler2, np.abs(u[:, 1] + 1) < toler2,
                 np.abs(u[:, 0] - 1) < toler2, np.abs(u[:, 2] - 1) < toler2,
                 np.abs(u[:, 1] - 1) < toler2, np.abs(u[:, 2] + 1) < toler2]
        horz = [(nhor - l2) + (l3 - 1) * nhor, (l1 - 1) + (l3 - 1) * nhor,
                (l2 - 1) + (l3 - 1) * nhor, (l1 - 1) + (l2 - 1) * nhor,
                (l1 - 1) + (nhor - l3) * nhor, (l1 - 1) + (nhor - l2) * nhor]
        el_glob = np.full(len(u), -1, dtype=np.int64)
        todo = np.ones(len(u), dtype=bool)
        for f in range(6):                               # the reference's if / elseif order
            m = todo & faces[f]
            el_glob[m] = lvl[m] + horz[f][m] * nvert + nblck * f
            todo &= ~m
        if todo.any():
            raise ValueError("error: unwrapped grid does not lie on any of the 6 faces")
        loc = glob_to_loc[el_glob]
        lin = np.flatnonzero(loc >= 0)
        order, offset = _group_by_element(loc[lin], nreal)
        lin = lin[order]
        el = loc[lin]
        ec = np.asarray(topl.elemtocoord, dtype=np.float64)
        xi = np.empty((len(lin), 3))
        for s in range(0, len(lin), 1 << 18):            # bounded temporaries
            sl_ = slice(s, s + (1 << 18))
            xi[sl_] = invert_trilinear_mapping_hex(ec[el[sl_]], uw[lin[sl_]], self.nr_toler)
        k = lin % n_long
        j = (lin // n_long) % n_lat
        i = lin // (n_long * n_lat)
        self.x_unwarped = uw[lin]                        # (Npl, 3): what the Newton inverse targets
        self.element = el
        self._finish(grid, offset, [xi[:, 0], xi[:, 1], xi[:, 2]], [k + 1, j + 1, i + 1],
                     (n_long, n_lat, n_rad))
        self.longi, self.lati, self.radi = self.i1, self.i2, self.i3


def dimensions(intrp):
    """``dimensions(interpol)``: name -> (axis values, attributes), Interpolation.jl:572-587
    and :1416-1439."""
    if intrp.is_sphere:
        return OrderedDict([
            ("long", (intrp.long_grd, OrderedDict([("units", "degrees_east"),
                                                   ("long_name", "longitude")]))),
            ("lat", (intrp.lat_grd, OrderedDict([("units", "degrees_north"),
                                                 ("long_name", "latitude")]))),
            ("level", (intrp.rad_grd, OrderedDict([("units", "m"), ("long_name", "level")]))),
        ])
    return OrderedDict([("x", (intrp.x1g, OrderedDict())), ("y", (intrp.x2g, OrderedDict())),
                        ("z", (intrp.x3g, OrderedDict()))])


# ---- device side ------------------------------------------------------------------------
class CmdgInterpDesc(C.Structure):
    """``cmdg_interp_desc`` of include/cmdg.h."""
    _fields_ = [
        ("Nq", C.c_int32 * 3), ("nelem", C.c_int64), ("npoints", C.c_int64),
        ("xi_nodes", C.c_void_p * 3), ("offset", C.c_void_p),
        ("xi1", C.c_void_p), ("xi2", C.c_void_p), ("xi3", C.c_void_p),
        ("i1", C.c_void_p), ("i2", C.c_void_p), ("i3", C.c_void_p),
        ("n1", C.c_int64), ("n2", C.c_int64), ("n3", C.c_int64),
        ("lat_grd", C.c_void_p), ("long_grd", C.c_void_p),
    ]


def _check_tensor(name, t, shape):
    import torch
    from .. import _lib
    if t.dtype != torch.float64 or not t.is_contiguous() or not t.is_cuda:
        raise _lib.CmdgError("%s must be a contiguous float64 device tensor" % name)
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise _lib.CmdgError("%s has shape %s, expected %s" % (name, tuple(t.shape), tuple(shape)))


def interpolate_local(intrp, Q, v, dg=None):
    """``interpolate_local!(intrp, Q.data, v)``: ``v[s, p]`` = the tensor-product Lagrange
    interpolant of state ``s`` of the point's element at its ``xi``.  With ``dg`` the kernel is
    ordered on that model's compute stream after any deferred run of it; without, it runs on the
    library's default stream, for any polynomial orders.  Returns when ``v`` is complete, as the
    reference does."""
    import torch
    from .. import _lib
    nstate = Q.shape[1]
    _check_tensor("Q", Q, None)
    _check_tensor("v", v, (nstate, intrp.Npl))
    if Q.shape[2] != int(np.prod(intrp.Nq)) or Q.shape[0] < intrp.Nel:
        raise _lib.CmdgError("Q has shape %s: not a state of this interpolation's grid" % (tuple(Q.shape),))
    it = intrp.device_object(Q.device)
    h = dg.handle if dg is not None else None
    torch.cuda.current_stream(Q.device).synchronize()
    with torch.cuda.device(Q.device):
        _lib.check(_lib.lib().cmdg_interp_apply(h, it, Q.data_ptr(), nstate, Q.shape[0],
                                                v.data_ptr()), h)
    if dg is not None:
        dg.synchronize()


def project_cubed_sphere(intrp, v, uvwi, dg=None):
    """``project_cubed_sphere!(intrp, v, uvwi)``: the three 1-based columns ``uvwi`` of ``v``
    hold Cartesian components and are replaced by the components along the unit vectors in
    longitudinal, latitudinal and radial direction at each point."""
    import torch
    from .. import _lib
    _check_tensor("v", v, (v.shape[0], intrp.Npl))
    if len(uvwi) != 3:
        raise _lib.CmdgError("length(uvwi) is not 3")
    it = intrp.device_object(v.device)
    cols = (C.c_int32 * 3)(*[int(c) for c in uvwi])
    h = dg.handle if dg is not None else None
    torch.cuda.current_stream(v.device).synchronize()
    with torch.cuda.device(v.device):
        _lib.check(_lib.lib().cmdg_interp_project(h, it, v.data_ptr(), v.shape[0], cols), h)
    if dg is not None:
        dg.synchronize()


def accumulate_interpolated_data(intrps, ivs, fiv, dg=None):
    """``accumulate_interpolated_data!(intrp, iv, fiv)`` for the ranks of one process:
    ``fiv[s, i3, i2, i1] = iv[s, p]`` through every rank's index triples.  ``intrps`` / ``ivs``
    are one object and tensor or equally long lists of them (rank by rank)."""
    import torch
    from .. import _lib
    if isinstance(intrps, _Interpolation):
        intrps, ivs = [intrps], [ivs]
    if len(intrps) != len(ivs) or not intrps:
        raise _lib.CmdgError("as many interpolated arrays as interpolation objects, at least one")
    nstate = fiv.shape[0]
    _check_tensor("fiv", fiv, (nstate,) + tuple(intrps[0].dims[::-1]))
    for intrp, iv in zip(intrps, ivs):
        _check_tensor("iv", iv, (nstate, intrp.Npl))
    n = len(intrps)
    its = (C.c_void_p * n)(*[intrp.device_object(fiv.device).value for intrp in intrps])
    vs = (C.c_void_p * n)(*[iv.data_ptr() for iv in ivs])
    h = dg.handle if dg is not None else None
    torch.cuda.current_stream(fiv.device).synchronize()
    with torch.cuda.device(fiv.device):
        _lib.check(_lib.lib().cmdg_interp_scatter(h, its, n, vs, nstate, fiv.data_ptr()), h)
    if dg is not None:
        dg.synchronize()
