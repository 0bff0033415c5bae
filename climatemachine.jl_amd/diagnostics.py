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

The ``AtmosGCMDefault`` group (``src/Diagnostics/atmos_gcm_default.jl``, ``diagnostic_fields.jl``,
``vorticity_balancelaw.jl``) is the second half of this module: ``VectorGradients``, ``Vorticity``,
``VorticityModel``, ``AtmosGCMDefault`` and ``AtmosGCMDefaultCallback``.

    diag = AtmosGCMDefault(dg, interpol).init()
    out = diag.collect(Q, t)           # OrderedDict: "long", "lat", "level", "u", ..., "vort", "vort2"
"""
import ctypes as C
from collections import OrderedDict

import numpy as np
import torch

from . import _lib
from .balancelaws import VorticityModel

__all__ = ["AtmosLESDefault", "AtmosLESDefaultCallback", "group_collect", "group_init", "SIMPLE_NAMES", "HO_NAMES",
           "SIMPLE_NAMES_MOIST", "HO_NAMES_MOIST", "NODAL_NAMES", "NODAL_NAMES_MOIST", "CLOUD_NAMES",
           "VectorGradients", "Vorticity", "VorticityModel", "AtmosGCMDefault", "AtmosGCMDefaultCallback",
           "group_collect_gcm", "group_init_gcm", "gcm_nodal", "GCM_NAMES", "GCM_NODAL_NAMES", "VGRAD_NAMES"]

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


def _refuse_tracers(who, dg):
    # the reference's default groups have no tracer variables; the device columns are laid out for
    # the tracer-free state
    if getattr(dg.balance_law, "ntracers", 0):
        raise ValueError("%s: a model with tracers is not served (the diagnostics are compiled for the "
                         "tracer-free dry law)" % who)


class AtmosLESDefault:
    """``setup_atmos_default_diagnostics(::AtmosLESConfigType, ...)`` for one ``DGModel`` (or one rank
    of a ``connect_local`` group, through ``group_init`` / ``group_collect``)."""

    def __init__(self, dg):
        g = dg.grid
        _refuse_tracers("AtmosLESDefault", dg)
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


# ---- AtmosGCMDefault (src/Diagnostics/atmos_gcm_default.jl, diagnostic_fields.jl) ------------------
# vars_atmos_gcm_default_simple_3d of a dry model (:96-115), in the reference's order
GCM_NAMES = ["u", "v", "w", "rho", "temp", "pres", "thd", "et", "ei", "ht", "hi", "vort", "vort2"]
# columns of the packed nodal array G of the group's nodal pass (csrc/kernels.h k_gcm_nodal)
GCM_NODAL_NAMES = ["ρ", "ρu", "ρv", "ρw", "ρe", "temp", "pres", "θ_dry", "e_int", "h_tot", "h_int", "Ω₁", "Ω₂", "Ω₃"]
VGRAD_NAMES = ["∂₁u₁", "∂₂u₁", "∂₃u₁", "∂₁u₂", "∂₂u₂", "∂₃u₂", "∂₁u₃", "∂₂u₃", "∂₃u₃"]
GCM_REQUIRES_SPHERE = "Diagnostics (AtmosGCMDefault): currently requires `InterpolationCubedSphere`!"


def _check_state(who, dg, Q):
    law, g = dg.balance_law, dg.grid
    if tuple(Q.shape) != (g.nelem, law.ns, g.Np):
        raise ValueError("%s: Q has shape %s, the model's state is %s" % (who, tuple(Q.shape), (g.nelem, law.ns, g.Np)))


class VectorGradients:
    """``VectorGradients(dg, Q)`` (diagnostic_fields.jl:75-127): the gradient of ``u = ρu / ρ`` on
    the real elements, ``data (nelem_real, 9, Np)`` on the device with the nine named views
    (``∂₁u₁, ∂₂u₁, ∂₃u₁, ∂₁u₂, ...``; ``self["∂₂u₃"]`` or ``self.views``)."""

    def __init__(self, dg, Q):
        _check_state("VectorGradients", dg, Q)
        g = dg.grid
        self.data = torch.zeros((g.nreal, 9, g.Np), dtype=torch.float64, device=dg.device)
        dg._torch_ready()
        _lib.check(dg.L.cmdg_vector_gradients(dg.handle, Q.data_ptr(), self.data.data_ptr()), dg.handle)
        self.views = OrderedDict((n, self.data[:, i, :]) for i, n in enumerate(VGRAD_NAMES))

    def __getitem__(self, name):
        return self.views[name]


class Vorticity:
    """``Vorticity(dg, vgrad)`` (diagnostic_fields.jl:356-396): ``data (nelem_real, 3, Np)`` and the
    views ``Ω₁, Ω₂, Ω₃``."""

    def __init__(self, dg, vgrad):
        g = dg.grid
        if tuple(vgrad.data.shape) != (g.nreal, 9, g.Np):
            raise ValueError("Vorticity: vgrad has shape %s, expected %s" % (tuple(vgrad.data.shape), (g.nreal, 9, g.Np)))
        self.data = torch.zeros((g.nreal, 3, g.Np), dtype=torch.float64, device=dg.device)
        dg._torch_ready()
        _lib.check(dg.L.cmdg_vorticity(dg.handle, vgrad.data.data_ptr(), self.data.data_ptr()), dg.handle)
        self.Ω1, self.Ω2, self.Ω3 = (self.data[:, i, :] for i in range(3))
        self.views = OrderedDict([("Ω₁", self.Ω1), ("Ω₂", self.Ω2), ("Ω₃", self.Ω3)])

    def __getitem__(self, name):
        return self.views[name]


def gcm_nodal(dg, Q, t=0.0, G=None, u=None):
    """The nodal pass of the GCM group on any grid (``cmdg_gcm_nodal``): fills and returns ``G (nelem,
    14, Np)`` (columns ``GCM_NODAL_NAMES``) and ``u (nelem, 3, Np)``; real elements are written."""
    _check_state("gcm_nodal", dg, Q)
    g = dg.grid
    if G is None:
        G = torch.zeros((g.nelem, len(GCM_NODAL_NAMES), g.Np), dtype=torch.float64, device=dg.device)
    if u is None:
        u = torch.zeros((g.nelem, 3, g.Np), dtype=torch.float64, device=dg.device)
    dg._torch_ready()
    _lib.check(dg.L.cmdg_gcm_nodal(dg.handle, Q.data_ptr(), float(t), G.data_ptr(), u.data_ptr()), dg.handle)
    return G, u


class AtmosGCMDefault:
    """``setup_atmos_default_diagnostics(::AtmosGCMConfigType, ...)`` for one ``DGModel`` and one
    ``InterpolationCubedSphere`` of its grid (or one rank of a ``connect_local`` group, through
    ``group_collect_gcm``).

        diag = AtmosGCMDefault(dg, interpol).init()
        out = diag.collect(Q, t)     # OrderedDict: "long", "lat", "level", "u", ..., "vort", "vort2"

    A collection is the nodal pass (one launch: the packed array ``G`` and the velocity), one
    evaluation of the ``VorticityModel`` handle, two interpolations (``G`` and ``Ω_bl``), the
    finishing kernel and one copy of the finished ``(13, nlevel, nlat, nlong)`` grid to the host."""

    def __init__(self, dg, interpol):
        from .mesh.interpolation import InterpolationCubedSphere
        if not isinstance(interpol, InterpolationCubedSphere):
            raise ValueError(GCM_REQUIRES_SPHERE)
        _refuse_tracers("AtmosGCMDefault", dg)
        if interpol.Nel != dg.grid.nreal or tuple(interpol.Nq) != tuple(int(q) for q in dg.grid.Nq):
            raise ValueError("AtmosGCMDefault: the interpolation was built for another grid")
        self.dg, self.interpol, self.L_ = dg, interpol, dg.L
        self.vdg = self.vstate = self.vdQ = self.dims = None
        self.G = self.vG = self.vB = self.fiv = None

    def init(self):
        """``atmos_gcm_default_init``: the ``VorticityModel`` handle on the same grid (central
        fluxes), its zero state and its tendency, and ``dimensions(interpol)`` with ``level``
        reduced by the planet radius (:263-267)."""
        from .balancelaws import CentralNumericalFluxFirstOrder
        from .dgmodel import DGModel
        from .mesh.interpolation import dimensions
        dg, it, g = self.dg, self.interpol, self.dg.grid
        self.vdg = DGModel(VorticityModel(), g, numerical_flux_first_order=CentralNumericalFluxFirstOrder,
                           device=dg.device)
        self.vstate = self.vdg.init_ode_state(0.0)
        self.vdQ = self.vdg.create_state()
        dims = dimensions(it)
        radius = float(dg.balance_law.ps.planet_radius)
        dims["level"] = (dims["level"][0] - radius, dims["level"][1])
        self.dims = dims
        z = dict(dtype=torch.float64, device=dg.device)
        self.G = torch.zeros((g.nelem, len(GCM_NODAL_NAMES), g.Np), **z)
        self.vG = torch.zeros((len(GCM_NODAL_NAMES), it.Npl), **z)
        self.vB = torch.zeros((3, it.Npl), **z)
        self.fiv = torch.zeros((len(GCM_NAMES),) + tuple(it.dims[::-1]), **z)
        self._host = torch.empty(self.fiv.shape, dtype=torch.float64, pin_memory=True)   # staging of the copy-out
        return self

    def close(self):
        if self.vdg is not None:
            self.vdg.close()
            self.vdg = None

    # -- the steps of a collection ------------------------------------------------------------------
    def nodal(self, Q, t=0.0):
        """The nodal pass: ``G (nelem, 14, Np)`` (columns ``GCM_NODAL_NAMES``) and ``u`` in the
        auxiliary array of the ``VorticityModel`` handle; both are returned."""
        if self.vdg is None:
            raise ValueError("AtmosGCMDefault.collect: init() has not run")
        return gcm_nodal(self.dg, Q, t, self.G, self.vdg.state_auxiliary)

    def _interpolate(self):
        """``interpolate_local!`` of ``G`` and of ``Ω_bl`` on the vorticity handle's stream."""
        it, L, h = self.interpol.device_object(self.dg.device), self.L_, self.vdg.handle
        g = self.dg.grid
        _lib.check(L.cmdg_interp_apply(h, it, self.G.data_ptr(), self.G.shape[1], g.nelem, self.vG.data_ptr()), h)
        _lib.check(L.cmdg_interp_apply(h, it, self.vdQ.data_ptr(), 3, g.nelem, self.vB.data_ptr()), h)

    def _result(self, copy=True):
        """The one copy-out: the finished grid into the pinned staging buffer (the handle has been
        synchronised).  ``copy=False`` hands out views of that buffer."""
        out = OrderedDict()
        for k in ("long", "lat", "level"):
            out[k] = np.array(self.dims[k][0], dtype=np.float64)
        self._host.copy_(self.fiv, non_blocking=True)
        torch.cuda.current_stream(self.dg.device).synchronize()
        host = self._host.numpy()
        for i, n in enumerate(GCM_NAMES):
            out[n] = host[i].copy() if copy else host[i]
        return out

    def collect(self, Q, t=0.0, copy=True):
        """``atmos_gcm_default_collect`` at ``(Q, t)``: an ordered dict with the axes ``long``,
        ``lat``, ``level`` and the 13 variables ``GCM_NAMES`` as ``(nlevel, nlat, nlong)`` arrays.
        ``copy=False``: the arrays are views of this object's pinned staging buffer, which the next
        collection overwrites (a grid of 1 x 1 degree x 31 levels is 210 MB: the private copies cost
        more than the collection)."""
        self.nodal(Q, t)
        self.vdg(self.vdQ, self.vstate, 0.0)
        self._interpolate()
        h = self.vdg.handle
        its = (C.c_void_p * 1)(self.interpol.device_object(self.dg.device).value)
        vG, vB = (C.c_void_p * 1)(self.vG.data_ptr()), (C.c_void_p * 1)(self.vB.data_ptr())
        _lib.check(self.L_.cmdg_interp_gcm_finish(h, its, 1, vG, vB, self.fiv.data_ptr()), h)
        self.vdg.synchronize()
        return self._result(copy)


def group_init_gcm(diags):
    """``init`` for the ranks of a ``connect_local`` group; the ranks' ``VorticityModel`` handles are
    connected in the same way, so that their exterior faces read exchanged ghosts."""
    from . import dgmodel
    for d in diags:
        d.init()
    if len(diags) > 1:
        dgmodel.connect_local([d.vdg for d in diags])


def group_collect_gcm(dgs, Qs, interpols, t=0.0, diags=None, copy=True):
    """One collection over the local ranks ``dgs`` (``Qs[r]``, ``interpols[r]`` on rank ``r``).  ``u`` is
    exchanged once before it enters the ghost auxiliary columns of the ``VorticityModel`` handles (the
    reference reads ``Q``'s exchanged ghosts, :341-346), and the ranks' finished points are scattered
    into one grid.  Returns the variables and the ranks' ``AtmosGCMDefault`` objects (hand them back
    as ``diags`` so that the one-time set-up is not repeated)."""
    from . import dgmodel
    if diags is None:
        diags = [AtmosGCMDefault(dg, it) for dg, it in zip(dgs, interpols)]
        group_init_gcm(diags)
    vdgs = [d.vdg for d in diags]
    for d, Q in zip(diags, Qs):
        d.nodal(Q, t)
    if len(diags) > 1:
        dgmodel.group_halo(vdgs, [v.state_auxiliary for v in vdgs])
        dgmodel.group_rhs(vdgs, [d.vdQ for d in diags], [d.vstate for d in diags], 0.0)
    else:
        vdgs[0](diags[0].vdQ, diags[0].vstate, 0.0)
    d0 = diags[0]
    for d in diags:
        d._interpolate()
        d.vdg.synchronize()
    n = len(diags)
    its = (C.c_void_p * n)(*[d.interpol.device_object(d0.dg.device).value for d in diags])
    vG = (C.c_void_p * n)(*[d.vG.data_ptr() for d in diags])
    vB = (C.c_void_p * n)(*[d.vB.data_ptr() for d in diags])
    h = d0.vdg.handle
    _lib.check(d0.L_.cmdg_interp_gcm_finish(h, its, n, vG, vB, d0.fiv.data_ptr()), h)
    d0.vdg.synchronize()
    return d0._result(copy), diags


class AtmosGCMDefaultCallback:
    """The group as a callback of ``odesolvers.solve(..., callbacks=[(every_n_steps, cb)])``: every call
    collects at ``(Q, t)``, appends ``(t, variables)`` to ``self.records`` and hands it to
    ``sink(t, variables)`` if one is given.  ``save(path)`` writes the series as an ``.npz``: ``time
    (nt,)``, the axes ``long``, ``lat``, ``level`` and one ``(nt, nlevel, nlat, nlong)`` array per
    variable."""
    AXES = ("long", "lat", "level")

    def __init__(self, dg, interpol, sink=None):
        self.diag = AtmosGCMDefault(dg, interpol)
        self.sink = sink
        self.records = []

    def init(self, solver, Q, t):
        self.diag.init()

    def __call__(self, solver, Q, t):
        out = self.diag.collect(Q, t)
        self.records.append((float(t), out))
        if self.sink is not None:
            self.sink(float(t), out)
        return None

    def series(self):
        out = OrderedDict(time=np.array([t for t, _ in self.records]))
        if self.records:
            first = self.records[0][1]
            for name in first:
                out[name] = first[name] if name in self.AXES else np.array([p[name] for _, p in self.records])
        return out

    def save(self, path):
        np.savez(path, **self.series())
        return path
