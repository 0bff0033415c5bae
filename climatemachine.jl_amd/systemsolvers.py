"""Host side of the system solvers.  ``ManyColumnLU``
(src/Numerics/SystemSolvers/columnwise_lu_solver.jl): the
banded column matrices of ``I - alpha L`` for a vertical-direction DG model, factored and solved
on the device (csrc/columnlu.hip, ``cmdg_columnlu_*`` in include/cmdg.h).
``GeneralizedMinimalResidual`` (generalized_minimal_residual_solver.jl): restarted GMRES on
``I - alpha L`` for a linear model of any direction on any grid, single rank (csrc/gmres.hip,
``cmdg_gmres_*``).

Band layout on the device: ``band[(col * P + d) * ncol + c]``, ``P = p + q + 1``,
``d = row - col + q``, ``c`` the column (horizontal node ``i + Nq j`` of stack ``h`` is column
``h Nq^2 + i + Nq j``); the reference's ``A[i, j, d + 1, col + 1, h + 1]``."""
import ctypes as C
import math
import warnings

import numpy as np

from . import _lib

__all__ = ["ManyColumnLU", "ColumnLU", "lower_bandwidth", "upper_bandwidth", "band_offset",
           "band_bytes", "GeneralizedMinimalResidual", "GmresSolver", "GmresInfo"]


def lower_bandwidth(N, nstate, eband):
    """``lower_bandwidth(N, nstate, eband) = (N + 1) nstate eband - 1`` (columnwise_lu_solver.jl:69)."""
    return (N + 1) * nstate * eband - 1


upper_bandwidth = lower_bandwidth


def band_offset(column, row, diag, n, p, q, ncol):
    """Offset (in doubles) of band entry ``diag`` (``d = matrix row - matrix column + q``) of
    matrix column ``row`` of column ``column`` in the device band."""
    assert 0 <= column < ncol and 0 <= row < n and 0 <= diag <= p + q
    return (row * (p + q + 1) + diag) * ncol + column


def band_bytes(ncol, n, p, q):
    """Bytes of the device band: ``ncol n (p + q + 1) 8``."""
    return ncol * n * (p + q + 1) * 8


class ManyColumnLU:
    """``ManyColumnLU()``: one banded LU per column of the vertical operator."""


class ColumnLU:
    """``prefactorize(EulerOperator(linear_dg, -alpha), ManyColumnLU(), Q, nothing, NaN)``:
    assembles and factors ``I - alpha L`` for every column of ``linear_dg`` (a
    ``VerticalDirection`` ``DGModel`` on a stacked grid)."""

    def __init__(self, linear_dg, alpha):
        g = linear_dg.grid
        if not (g.topology.isstacked and g.topology.stacksize):
            raise _lib.CmdgError("ManyColumnLU needs a stacked grid")
        self.dg = linear_dg
        self.nvert = int(g.topology.stacksize)
        _check_stack_order(g, self.nvert)
        _check_stack_ends(g, self.nvert)
        h = C.c_void_p()
        linear_dg._torch_ready()
        _lib.check(linear_dg.L.cmdg_columnlu_create(linear_dg.handle, self.nvert, float(alpha),
                                                    C.byref(h)), linear_dg.handle)
        self.handle = h
        info = (C.c_int64 * 8)()
        _lib.check(linear_dg.L.cmdg_columnlu_info(h, C.cast(info, C.c_void_p)), linear_dg.handle)
        self.n, self.p, self.q, self.ncol, self.band_bytes = [int(v) for v in info[:5]]

    @property
    def alpha(self):
        a = C.c_double()
        _lib.check(self.dg.L.cmdg_columnlu_alpha(self.handle, C.cast(C.byref(a), C.c_void_p)))
        return a.value

    def update(self, alpha):
        """``update_backward_Euler_solver!``: reassemble and refactor for ``alpha``."""
        _lib.check(self.dg.L.cmdg_columnlu_update(self.handle, float(alpha)), self.dg.handle)

    def assemble(self, alpha):
        """``I - alpha L`` into the band, unfactored (for ``export_band``)."""
        _lib.check(self.dg.L.cmdg_columnlu_assemble(self.handle, float(alpha)), self.dg.handle)

    def solve(self, Q, Qrhs):
        """``linearsolve!``: ``Q = (I - alpha L)^-1 Qrhs`` on the real elements."""
        self.dg._torch_ready()
        _lib.check(self.dg.L.cmdg_columnlu_solve(self.handle, Q.data_ptr(), Qrhs.data_ptr()),
                   self.dg.handle)

    def export_band(self, column):
        """The band of one column in the reference's layout, ``(p + q + 1, n)`` (``A[d, col]``)."""
        P = self.p + self.q + 1
        out = np.empty(self.n * P)
        _lib.check(self.dg.L.cmdg_columnlu_export_band(self.handle, int(column), out.ctypes.data),
                   self.dg.handle)
        return out.reshape(self.n, P).T.copy()

    def close(self):
        if getattr(self, "handle", None):
            self.dg.L.cmdg_columnlu_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GeneralizedMinimalResidual:
    """``GeneralizedMinimalResidual(Q; M, rtol, atol)``: the restart length and the tolerances of
    the restarted GMRES of Saad and Schultz.  ``Q`` only shapes the solver's arrays (here: ignored,
    the device solver takes the shape of its linear model).  The reference's default
    ``M = min(20, eltype(Q))`` cannot be evaluated; 20 is what it means."""

    def __init__(self, Q=None, M=20, rtol=math.sqrt(2.0 ** -52), atol=2.0 ** -52):
        M, rtol, atol = int(M), float(rtol), float(atol)
        if not 1 <= M <= _lib.GMRES_MAX_M:
            raise ValueError("GeneralizedMinimalResidual: M must be 1 to %d, not %d" % (_lib.GMRES_MAX_M, M))
        if not rtol >= 0 or not atol >= 0:
            raise ValueError("GeneralizedMinimalResidual: rtol and atol must be >= 0 (rtol = %r, "
                             "atol = %r)" % (rtol, atol))
        self.M, self.rtol, self.atol = M, rtol, atol


class GmresInfo:
    """What one solve did: ``iterations``, ``converged``, ``residual_norm``, ``threshold``."""

    def __init__(self, c):
        self.iterations, self.converged = int(c.iterations), bool(c.converged)
        self.residual_norm, self.threshold = float(c.residual_norm), float(c.threshold)

    def __eq__(self, other):
        return (self.iterations, self.converged, self.residual_norm, self.threshold) == (
            other.iterations, other.converged, other.residual_norm, other.threshold)

    def __repr__(self):
        return "GmresInfo(iterations=%d, converged=%s, residual_norm=%r, threshold=%r)" % (
            self.iterations, self.converged, self.residual_norm, self.threshold)


class GmresSolver:
    """``setup_backward_Euler_solver(LinearBackwardEulerSolver(gmres), Q, alpha, linear_dg)``: the
    device solver of ``(I - alpha L) Q = Qrhs`` for ``linear_dg``, a ``DGModel`` of any direction on
    a stacked or unstacked grid (one rank)."""

    def __init__(self, linear_dg, alpha, gmres):
        self.dg, self.gmres = linear_dg, gmres
        self._warned = False
        h = C.c_void_p()
        linear_dg._torch_ready()
        _lib.check(linear_dg.L.cmdg_gmres_create(linear_dg.handle, gmres.M, gmres.rtol, gmres.atol,
                                                 C.byref(h)), linear_dg.handle)
        self.handle = h
        self.update(alpha)

    def update(self, alpha):
        """``update_backward_Euler_solver!``: nothing to factor, the new alpha is recorded."""
        self.alpha = float(alpha)
        _lib.check(self.dg.L.cmdg_gmres_prepare(self.handle, self.alpha), self.dg.handle)

    def _note(self, infos):
        for i in infos:
            if not i.converged and not self._warned:
                self._warned = True
                warnings.warn("Solver did not attain convergence after %d iterations" % i.iterations,
                              RuntimeWarning, stacklevel=3)
        return infos

    def solve(self, Q, Qrhs, t=0.0, max_iters=None, alpha=None):
        """``linearsolve!``: ``Q`` holds the initial guess and receives the solution; ``max_iters``
        defaults to ``length(Q)``.  Returns a ``GmresInfo``; an unconverged solve warns once."""
        self.dg._torch_ready()
        info = _lib.CmdgGmresInfo()
        _lib.check(self.dg.L.cmdg_gmres_solve(
            self.handle, self.alpha if alpha is None else float(alpha), Q.data_ptr(), Qrhs.data_ptr(),
            float(t), -1 if max_iters is None else int(max_iters), C.byref(info)), self.dg.handle)
        return self._note([GmresInfo(info)])[0]

    def step_info(self):
        """The solves of the last step that drove this solver, in order."""
        n = C.c_int32()
        _lib.check(self.dg.L.cmdg_gmres_step_info(self.handle, 0, None, C.cast(C.byref(n), C.c_void_p)))
        out = (_lib.CmdgGmresInfo * max(n.value, 1))()
        _lib.check(self.dg.L.cmdg_gmres_step_info(self.handle, n.value, C.cast(out, C.c_void_p),
                                                  C.cast(C.byref(n), C.c_void_p)))
        return self._note([GmresInfo(out[i]) for i in range(n.value)])

    def fits(self, M, free_bytes):
        """The size check of ``cmdg_gmres_create`` against ``free_bytes``: the bytes of the Krylov
        basis, or ``CmdgError`` naming them when they do not fit."""
        b = C.c_int64()
        _lib.check(self.dg.L.cmdg_gmres_fits(self.dg.handle, int(M), int(free_bytes),
                                             C.cast(C.byref(b), C.c_void_p)), self.dg.handle)
        return b.value

    def close(self):
        if getattr(self, "handle", None):
            self.dg.L.cmdg_gmres_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _check_stack_order(grid, nvert):
    """The solver's columns assume the reference's element order: stack after stack, bottom to
    top (e = v + nvert h, radius increasing with v)."""
    from .mesh import grids as G
    nr = grid.nreal
    if nr % nvert:
        raise _lib.CmdgError("ManyColumnLU: the real elements are not whole stacks")
    x = np.stack([grid.vgeo[:nr, c, 0] for c in (G._x1, G._x2, G._x3)])
    r = np.sqrt((x * x).sum(axis=0)).reshape(-1, nvert)
    z = grid.vgeo[:nr, G._x3, 0].reshape(-1, nvert)
    ok = np.all(np.diff(r, axis=1) > 0) or np.all(np.diff(z, axis=1) > 0)
    if not ok:
        raise _lib.CmdgError("ManyColumnLU: the real elements are not ordered bottom to top "
                             "within each stack")


def _check_stack_ends(grid, nvert):
    """Every stack ends in boundary faces, bottom and top.  A vertically periodic stack couples its
    top and bottom elements; the band holds only neighbouring elements, so that coupling would be
    dropped and the solve silently wrong (the library refuses it as well)."""
    etb = np.asarray(grid.elemtobndy)[:grid.nreal].reshape(-1, nvert, 6)
    if np.any(etb[:, 0, 4] == 0) or np.any(etb[:, -1, 5] == 0):
        raise _lib.CmdgError("ManyColumnLU: vertically periodic stacks are not supported (a stack's "
                             "bottom or top element has no boundary face; the band cannot hold "
                             "the coupling of its top and bottom elements)")
