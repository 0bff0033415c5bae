"""The ``AtmosLESDefault`` diagnostics group of the reference (``src/Diagnostics/
atmos_les_default.jl``; ``atmos_common.jl``, ``thermo.jl``, ``helpers.jl``): density-weighted
horizontal means, variances and vertical eddy fluxes on every level of a stacked grid, plus the cloud
statistics of the moist law, formed on the device (``csrc/diagnostics.hip``; the nodal
thermodynamics is the law's ``les_diagnostics``).

    diag = AtmosLESDefault(dg)
    diag.init()
    prof = diag.collect(Q, t)          # OrderedDict: "z", "u", ..., "cov_w_ei", [..., "cld_frac", ..., "iwp"]

Levels: ``L = Nqk * nvertelem``, level ``evk = Nqk * ev + k`` (0-based).  Every sum is accumulated in
double-double from the rounded terms the reference writes and combined in a fixed order, so a
collection returns the same bits every time.  Out of scope: NetCDF output (``AtmosLESDefaultCallback``
keeps the series and writes an ``.npz``), the other diagnostics groups, and ``qr``, ``qs``, ``rwp``,
``swp`` (no precipitation model).
"""
import ctypes as C
from collections import OrderedDict

import numpy as np
import torch

from . import _lib

__all__ = ["AtmosLESDefault", "AtmosLESDefaultCallback", "group_collect", "group_init", "SIMPLE_NAMES", "HO_NAMES",
           "SIMPLE_NAMES_MOIST", "HO_NAMES_MOIST", "NODAL_NAMES", "NODAL_NAMES_MOIST", "CLOUD_NAMES"]

# vars_atmos_les_default_simple / _ho (atmos_les_default.jl:96-127, 296-330), prefix-filtered
SIMPLE_NAMES = ["u", "v", "w", "avg_rho", "rho", "temp", "pres", "thd", "et", "ei", "ht", "hi", "w_ht_sgs"]
SIMPLE_NAMES_MOIST = ["qt", "ql", "qi", "qv", "thv", "thl", "w_qt_sgs"]
HO_NAMES = ["var_u", "var_v", "var_w", "w3", "tke", "var_ei", "cov_w_u", "cov_w_v", "cov_w_rho", "cov_w_thd",
            "cov_w_ei"]
HO_NAMES_MOIST = ["var_qt", "var_thl", "cov_w_qt", "cov_w_ql", "cov_w_qi", "cov_w_qv", "cov_w_thv", "cov_w_thl",
                  "cov_qt_thl", "cov_qt_ei"]
CLOUD_NAMES = ["cld_frac", "cld_top", "cld_base", "cld_cover", "lwp", "iwp"]
# columns of the nodal array D (vars_thermo, thermo.jl:6-28, and the two sub-grid terms)
NODAL_NAMES = ["temp", "pres", "θ_dry", "e_int", "h_tot", "h_int", "d_h_tot_3"]
NODAL_NAMES_MOIST = ["q_liq", "q_ice", "q_vap", "θ_vir", "θ_liq_ice", "has_condensate", "d_q_tot_3"]


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class AtmosLESDefault:
    """``setup_atmos_default_diagnostics(::AtmosLESConfigType, ...)`` for one ``DGModel`` (or one rank
    of a ``connect_local`` group, through ``group_init`` / ``group_collect``)."""

    def __init__(self, dg):
        g = dg.grid
        self.dg, self.L_ = dg, dg.L
        # (the library refuses, with the reason: a law without the diagnostics, a grid that is not
        # stacked, a vertical order of 0)
        self.nvertelem = int(getattr(g.topology, "stacksize", 0) or 0)
        sizes = (C.c_int32 * 4)()
        _lib.check(dg.L.cmdg_les_query(dg.handle, self.nvertelem, C.cast(sizes, C.c_void_p)), dg.handle)
        self.ndiag, self.nsimple, self.nho, self.nlevels = (int(v) for v in sizes)
        self.moist = self.nsimple > len(SIMPLE_NAMES)
        self.simple_names = SIMPLE_NAMES + (SIMPLE_NAMES_MOIST if self.moist else [])
        self.ho_names = HO_NAMES + (HO_NAMES_MOIST if self.moist else [])
        self.nodal_names = NODAL_NAMES + (NODAL_NAMES_MOIST if self.moist else [])
        self.omega = np.ascontiguousarray(g.omega[-1], dtype=np.float64)
        self.zvals = self.MH_z = None
        self._scratch = None
        self.raw = None

    # -- helpers ------------------------------------------------------------------------------
    def _check_Q(self, Q):
        law, g = self.dg.balance_law, self.dg.grid
        if tuple(Q.shape) != (g.nelem, law.ns, g.Np):
            raise ValueError("AtmosLESDefault: Q has shape %s, the model's state is %s"
                             % (tuple(Q.shape), (g.nelem, law.ns, g.Np)))

    def _evaluate(self, Q, t):
        if self._scratch is None:
            self._scratch = self.dg.create_state()
        self.dg(self._scratch, Q, t)

    def _buffers(self):
        L = self.nlevels
        return dict(simple_sums=np.zeros((L, self.nsimple)), simple_avgs=np.zeros((L, self.nsimple)),
                    ho_sums=np.zeros((L, self.nho)), ho_avgs=np.zeros((L, self.nho)),
                    cloud_levels=np.zeros((L, 6)), cloud_scalars=np.zeros(8))

    @staticmethod
    def _result(buf):
        r = _lib.CmdgLesResult()
        for k, a in buf.items():
            setattr(r, k, a.ctypes.data)
        return r

    def _profiles(self, buf):
        """The reference's ``varvals`` (:823-863) from the arrays of one collection."""
        self.raw = buf
        out = OrderedDict(z=self.zvals.copy())
        for i, n in enumerate(self.simple_names):
            out[n] = buf["simple_avgs"][:, i].copy()
        for i, n in enumerate(self.ho_names):
            out[n] = buf["ho_avgs"][:, i].copy()
        if self.moist:
            cl, cs = buf["cloud_levels"], buf["cloud_scalars"]
            out["cld_frac"] = cl[:, 0] / cl[:, 1]
            out["cld_top"], out["cld_base"], out["cld_cover"] = float(cs[0]), float(cs[1]), float(cs[2])
            out["lwp"], out["iwp"] = float(cs[3]), float(cs[4])
        return out

    # -- the group's three functions -------------------------------------------------------------
    def init(self):
        """``atmos_collect_onetime``: ``zvals`` and ``MH_z`` (kept on the object and on the device)."""
        z, m = np.zeros(self.nlevels), np.zeros(self.nlevels)
        self.dg._torch_ready()
        _lib.check(self.L_.cmdg_les_init(self.dg.handle, self.nvertelem, _ptr(self.omega), _ptr(z), _ptr(m)),
                   self.dg.handle)
        self.zvals, self.MH_z = z, m
        return self

    def nodal(self, Q, t=0.0):
        """The nodal array ``D``, ``(nelem, ndiag, Np)``, from ``(Q, aux, gradient flux)`` as the last
        evaluation left them; columns ``nodal_names``."""
        self._check_Q(Q)
        g = self.dg.grid
        D = torch.zeros((g.nelem, self.ndiag, g.Np), dtype=torch.float64, device=self.dg.device)
        self.dg._torch_ready()
        _lib.check(self.L_.cmdg_les_nodal(self.dg.handle, Q.data_ptr(), float(t), D.data_ptr()), self.dg.handle)
        return D

    def collect(self, Q, t=0.0, evaluate=True):
        """``atmos_les_default_collect``: an ordered dict ``name -> (L,)`` array, ``z`` first, scalars
        for the cloud statistics.  ``evaluate``: first evaluate the model at ``(Q, t)`` into a scratch
        tendency so that ``aux.moisture`` and the gradient flux belong to ``Q``; ``False`` reads what
        the last evaluation left, as the reference does.  The raw sums stay in ``self.raw``."""
        self._check_Q(Q)
        if self.zvals is None:
            raise ValueError("AtmosLESDefault.collect: init() has not run")
        if evaluate:
            self._evaluate(Q, t)
        buf = self._buffers()
        res = self._result(buf)
        self.dg._torch_ready()
        _lib.check(self.L_.cmdg_les_collect(self.dg.handle, Q.data_ptr(), float(t), C.byref(res)), self.dg.handle)
        return self._profiles(buf)


def _handles(diags):
    return (C.c_void_p * len(diags))(*[d.dg.handle for d in diags])


def group_init(diags):
    """``init`` for the ranks of a ``dgmodel.connect_local`` group (``diags[r]`` on rank ``r``)."""
    d0 = diags[0]
    z, m = np.zeros(d0.nlevels), np.zeros(d0.nlevels)
    for d in diags:
        d.dg._torch_ready()
    _lib.check(d0.L_.cmdg_group_les_init(C.cast(_handles(diags), C.c_void_p), len(diags), d0.nvertelem,
                                         _ptr(d0.omega), _ptr(z), _ptr(m)), d0.dg.handle)
    for d in diags:
        d.zvals, d.MH_z = z.copy(), m.copy()


def group_collect(dgs, Qs, t=0.0, evaluate=True, diags=None):
    """One collection over the local ranks ``dgs`` (``Qs[r]`` on rank ``r``): the partial sums of the
    ranks are combined in rank order.  ``diags``: the ranks' ``AtmosLESDefault`` objects of an earlier
    call (returned as the second value), so that the one-time collection is not repeated."""
    from . import dgmodel
    if diags is None:
        diags = [AtmosLESDefault(dg) for dg in dgs]
        group_init(diags)
    for d, Q in zip(diags, Qs):
        d._check_Q(Q)
    if evaluate:
        scr = []
        for d in diags:
            if d._scratch is None:
                d._scratch = d.dg.create_state()
            scr.append(d._scratch)
        dgmodel.group_rhs(dgs, scr, Qs, t)
    d0 = diags[0]
    buf = d0._buffers()
    res = d0._result(buf)
    for d in diags:
        d.dg._torch_ready()
    qs = (C.c_void_p * len(Qs))(*[Q.data_ptr() for Q in Qs])
    _lib.check(d0.L_.cmdg_group_les_collect(C.cast(_handles(diags), C.c_void_p), len(diags),
                                            C.cast(qs, C.c_void_p), float(t), C.byref(res)), d0.dg.handle)
    return d0._profiles(buf), diags


class AtmosLESDefaultCallback:
    """The group as a callback of ``odesolvers.solve(..., callbacks=[(every_n_steps, cb)])``: every call
    collects at ``(Q, t)`` (after an evaluation there), appends ``(t, profiles)`` to ``self.records`` and
    hands it to ``sink(t, profiles)`` if one is given.  ``save(path)`` writes the series as an ``.npz``:
    ``time (nt,)``, ``z (L,)`` and one ``(nt, L)`` or ``(nt,)`` array per variable."""

    def __init__(self, dg, sink=None):
        self.diag = AtmosLESDefault(dg)
        self.sink = sink
        self.records = []

    def init(self, solver, Q, t):
        self.diag.init()

    def __call__(self, solver, Q, t):
        prof = self.diag.collect(Q, t, evaluate=True)
        self.records.append((float(t), prof))
        if self.sink is not None:
            self.sink(float(t), prof)
        return None

    def series(self):
        out = OrderedDict(time=np.array([t for t, _ in self.records]))
        if self.records:
            out["z"] = self.records[0][1]["z"]
            for name in self.records[0][1]:
                if name != "z":
                    out[name] = np.array([p[name] for _, p in self.records])
        return out

    def save(self, path):
        np.savez(path, **self.series())
        return path
