"""NumPy restatement of the reference's ``AtmosLESDefault`` diagnostics group
(``src/Diagnostics/atmos_les_default.jl``, ``atmos_common.jl``, ``thermo.jl``, ``helpers.jl``): the two
traversals of ``atmos_les_default_collect`` in the reference's loop order (``@traverse_dg_grid``: eh, ev,
k, j, i) with plain double sums.  The terms of a node are formed for all nodes at once (each is the
same chain of rounded operations the reference writes) and then accumulated per level in visit
order (``np.cumsum`` adds sequentially).  Thermodynamics.jl is not in the reference tree: the nodal
quantities restate its published formulas from the equilibrium state in ``aux.moisture``, as the
device law does.

Arrays are ``(nelem, nvar, Np)``; only the ``grid.nreal`` real elements are visited.
"""
from collections import OrderedDict

import numpy as np

from cmdg_loader import cm

G = cm.mesh.grids

SIMPLE = ["u", "v", "w", "avg_rho", "rho", "temp", "pres", "thd", "et", "ei", "ht", "hi", "w_ht_sgs"]
SIMPLE_MOIST = ["qt", "ql", "qi", "qv", "thv", "thl", "w_qt_sgs"]
HO = ["var_u", "var_v", "var_w", "w3", "tke", "var_ei", "cov_w_u", "cov_w_v", "cov_w_rho", "cov_w_thd", "cov_w_ei"]
HO_MOIST = ["var_qt", "var_thl", "cov_w_qt", "cov_w_ql", "cov_w_qi", "cov_w_qv", "cov_w_thv", "cov_w_thl",
            "cov_qt_thl", "cov_qt_ei"]
NODAL = ["temp", "pres", "θ_dry", "e_int", "h_tot", "h_int", "d_h_tot_3"]
NODAL_MOIST = ["q_liq", "q_ice", "q_vap", "θ_vir", "θ_liq_ice", "has_condensate", "d_q_tot_3"]


def is_moist(law):
    return law.physics_id == cm.balancelaws.PHYSICS_MOIST_ATMOS


def _nu3(law, Q, aux, gf):
    """The vertical entry of the closure's diagonal viscosity (``turbulence_tensors``,
    TurbulenceClosures.jl:372-408 constant viscosity, :476-497 SmagorinskyLilly)."""
    ps = law.ps
    rho = Q[:, 0]
    if is_moist(law):
        closure, coeff, kinematic, delta = law.closure, law.coefficient, law.kinematic, aux[:, law.off_turb]
    else:
        closure = 1 if law.C_smag is not None else 0
        coeff = law.C_smag if closure else law.viscosity
        kinematic, delta = not law.dynamic_viscosity, aux[:, law.off_turb] if closure else None
    if closure == 0:
        return coeff + 0.0 * rho if kinematic else coeff / rho
    if closure != 1:
        raise NotImplementedError("restatement: constant viscosity and SmagorinskyLilly only")
    S = gf[:, 3:9]
    N2 = gf[:, 9]
    norm2 = (S[:, 0] * S[:, 0] + 2 * (S[:, 1] * S[:, 1]) + 2 * (S[:, 2] * S[:, 2]) + S[:, 3] * S[:, 3]
             + 2 * (S[:, 4] * S[:, 4]) + S[:, 5] * S[:, 5])
    normS = np.sqrt(2 * norm2)
    eps = np.spacing(np.abs(normS))
    Ri = N2 / (normS * normS + eps)
    c = np.clip(1.0 - Ri * ps.inv_Pr_turb, 0.0, 1.0)
    fb2 = np.sqrt(c)
    cd = coeff * delta
    nu0 = normS * (cd * cd) + 1e-5
    k = [aux[:, law.off_phi + 1 + d] / ps.grav for d in range(3)]
    dk = nu0 * k[0] + nu0 * k[1] + nu0 * k[2]
    nv = k[2] * dk
    nh = nu0 - nv
    return nh + nv * fb2


def nodal(law, Q, aux, gf):
    """``compute_thermo!`` (thermo.jl:33-68) and the two sub-grid terms of
    ``atmos_les_default_simple_sums!`` (:168-170, 218-219): ``(nelem, 7 | 14, Np)``."""
    ps = law.ps
    moist = is_moist(law)
    rho = Q[:, 0]
    rhoinv = 1 / rho
    e_tot = Q[:, 4] / rho
    rhoe_kin = rhoinv * (Q[:, 1] * Q[:, 1] + Q[:, 2] * Q[:, 2] + Q[:, 3] * Q[:, 3]) / 2
    has_phi = moist or law.orientation != cm.atmos.ORIENT_NONE
    rhoe_pot = rho * (aux[:, law.off_phi] if has_phi else -0.0)
    e_int = rhoinv * (Q[:, 4] - rhoe_kin - rhoe_pot)
    if moist:
        T, ql, qi = aux[:, law.off_moist], aux[:, law.off_moist + 2], aux[:, law.off_moist + 3]
        qt = Q[:, 5] / rho
        eps = ps.R_v / ps.R_d
        R_m = ps.R_d * (1 + (eps - 1) * qt - eps * (ql + qi))
        cp_m = ps.cp_d + (ps.cp_v - ps.cp_d) * qt + (ps.cp_l - ps.cp_v) * ql + (ps.cp_i - ps.cp_v) * qi
        kappa = R_m / cp_m
    else:
        T = ps.T_0 + e_int / ps.cv_d
        R_m, kappa = ps.R_d, ps.R_d / ps.cp_d
    p = R_m * rho * T
    thd = T / (p / ps.MSLP) ** kappa
    RT = R_m * T
    Dt = _nu3(law, Q, aux, gf) * ps.inv_Pr_turb
    cols = [T, p, thd, e_int, e_tot + RT, e_int + RT, (-Dt) * gf[:, 2]]
    if moist:
        ngt = 10 if law.closure == 2 else 7
        cols += [ql, qi, np.maximum(qt - ql - qi, 0.0), R_m / ps.R_d * thd,
                 thd * (1 - (ps.LH_v0 * ql + ps.LH_s0 * qi) / (cp_m * T)),
                 (ql + qi > 0).astype(np.float64), (-Dt) * gf[:, 3 + ngt + 2]]
    return np.stack(cols, axis=1)


def _shape(grid):
    Nq, Nqk = grid.N[0] + 1, grid.N[-1] + 1
    nvert = int(grid.topology.stacksize)
    return Nq, Nqk, nvert, grid.nreal // nvert


def _level_sums(grid, T):
    """``sums[evk][v] += T[ijk, v, e]`` in the order of ``@traverse_dg_grid`` (helpers.jl:6-28)."""
    Nq, Nqk, nvert, nhorz = _shape(grid)
    nv = T.shape[1]
    X = T[:grid.nreal].reshape(nhorz, nvert, nv, Nqk, Nq * Nq)
    out = np.zeros((Nqk * nvert, nv))
    for ev in range(nvert):
        for k in range(Nqk):
            for v in range(nv):
                out[Nqk * ev + k, v] = np.cumsum(X[:, ev, v, k, :].ravel())[-1]
    return out


def level_index(grid):
    """``evk`` of every node, ``(nreal, Np)``."""
    Nq, Nqk, nvert, nhorz = _shape(grid)
    ev = np.arange(grid.nreal) % nvert
    k = np.arange(grid.Np) // (Nq * Nq)
    return Nqk * ev[:, None] + k[None, :]


def onetime(grid):
    """``atmos_collect_onetime`` (atmos_common.jl:12-38): ``zvals`` (the last node visited on the
    level) and ``MH_z`` of this rank."""
    Nq, Nqk, nvert, nhorz = _shape(grid)
    x3 = grid.vgeo[:grid.nreal, G._x3].reshape(nhorz, nvert, Nqk, Nq * Nq)
    zvals = x3[-1, :, :, -1].reshape(-1).copy()
    MH_z = _level_sums(grid, grid.vgeo[:, G._MH][:, None, :])[:, 0]
    return zvals, MH_z


def simple_terms(law, grid, Q, D):
    """The terms of ``atmos_les_default_simple_sums!`` (:145-222) and, for the moist law, the two
    water-path terms (:666-667), left to right."""
    MH, rho = grid.vgeo[:, G._MH], Q[:, 0]
    t = [MH * Q[:, 1], MH * Q[:, 2], MH * Q[:, 3], MH * rho, MH * rho * rho, MH * D[:, 0] * rho,
         MH * D[:, 1] * rho, MH * D[:, 2] * rho, MH * Q[:, 4], MH * D[:, 3] * rho, MH * D[:, 4] * rho,
         MH * D[:, 5] * rho, MH * D[:, 6] * rho]
    if is_moist(law):
        t += [MH * Q[:, 5], MH * D[:, 7] * rho, MH * D[:, 8] * rho, MH * D[:, 9] * rho, MH * D[:, 10] * rho,
              MH * D[:, 11] * rho, MH * D[:, 13] * rho, MH * D[:, 7] * rho * rho, MH * D[:, 8] * rho * rho]
    return np.stack(t, axis=1)


def finish_simple(sums, MH_z, nsimple):
    """:687-773: ``avg = S / MH_z``, then every variable but ``avg_rho`` (and both water-path sums) is
    divided by ``avg_rho``."""
    avg = sums / MH_z[:, None]
    ar = avg[:, 3].copy()
    for v in range(avg.shape[1]):
        if v != 3:
            avg[:, v] = avg[:, v] / ar
    return avg


def ho_terms(law, grid, Q, D, avgs):
    """The terms of ``atmos_les_default_ho_sums!`` (:350-446) about the finished simple averages
    ``avgs`` ``(L, nsimple)`` of the node's level."""
    MH, rho = grid.vgeo[:, G._MH], Q[:, 0]
    ha = avgs[level_index(grid)]                       # (nreal, Np, nsimple)
    pad = np.zeros((Q.shape[0] - grid.nreal,) + ha.shape[1:])
    ha = np.concatenate([ha, pad], axis=0)
    up = Q[:, 1] / rho - ha[..., 0]
    vp = Q[:, 2] / rho - ha[..., 1]
    wp = Q[:, 3] / rho - ha[..., 2]
    eip = D[:, 3] - ha[..., 9]
    thdp = D[:, 2] - ha[..., 7]
    a, b, c = MH * (up * up) * rho, MH * (vp * vp) * rho, MH * (wp * wp) * rho
    t = [a, b, c, MH * (wp * wp * wp) * rho, 0.5 * (a + b + c), MH * (eip * eip) * rho, MH * wp * up * rho,
         MH * wp * vp * rho, MH * wp * (rho - ha[..., 3]) * rho, MH * wp * thdp * rho, MH * wp * eip * rho]
    if is_moist(law):
        qtp = Q[:, 5] / rho - ha[..., 13]
        qlp, qip, qvp = D[:, 7] - ha[..., 14], D[:, 8] - ha[..., 15], D[:, 9] - ha[..., 16]
        thvp, thlp = D[:, 10] - ha[..., 17], D[:, 11] - ha[..., 18]
        t += [MH * (qtp * qtp) * rho, MH * (thlp * thlp) * rho, MH * wp * qtp * rho, MH * wp * qlp * rho,
              MH * wp * qip * rho, MH * wp * qvp * rho, MH * wp * thvp * rho, MH * wp * thlp * rho,
              MH * qtp * thlp * rho, MH * qtp * eip * rho]
    return np.stack(t, axis=1)


def finish_ho(sums, MH_z, avg_rho):
    """:815-846."""
    return sums / MH_z[:, None] / avg_rho[:, None]


def water_path(levels, grid):
    """``sum(ρq_z .* Mvert)`` with ``Mvert = ω_k JcV[1, k, ev, eh = 1]`` (:781-790), added in order."""
    Nq, Nqk, nvert, nhorz = _shape(grid)
    JcV = grid.vgeo[:grid.nreal, G._JcV].reshape(nhorz, nvert, Nqk, Nq * Nq)
    Mvert = (np.asarray(grid.omega[-1])[None, :] * JcV[0, :, :, 0]).reshape(-1)
    s = 0.0
    for x in levels * Mvert:
        s += x
    return float(s)


def collect(law, grid, Q, aux, gf, D=None):
    """``atmos_les_default_collect`` (:567-871) on one rank: an ordered dict of the reference's
    ``varvals`` plus ``z``; the raw arrays under ``"_raw"``."""
    moist = is_moist(law)
    Nq, Nqk, nvert, nhorz = _shape(grid)
    D = nodal(law, Q, aux, gf) if D is None else D
    zvals, MH_z = onetime(grid)
    names = SIMPLE + (SIMPLE_MOIST if moist else [])
    ho_names = HO + (HO_MOIST if moist else [])
    ssum = _level_sums(grid, simple_terms(law, grid, Q, D))
    savg = finish_simple(ssum, MH_z, len(names))
    hsum = _level_sums(grid, ho_terms(law, grid, Q, D, savg[:, :len(names)]))
    havg = finish_ho(hsum, MH_z, savg[:, 3])
    out = OrderedDict(z=zvals)
    for i, n in enumerate(names):
        out[n] = savg[:, i]
    for i, n in enumerate(ho_names):
        out[n] = havg[:, i]
    raw = dict(simple_sums=ssum[:, :len(names)], simple_avgs=savg[:, :len(names)], ho_sums=hsum, ho_avgs=havg,
               MH_z=MH_z, D=D)
    if moist:
        hc = D[:grid.nreal, 12].reshape(nhorz, nvert, Nqk, Nq * Nq)
        count = hc.sum(axis=(0, 3)).reshape(-1)                 # (integers: exact)
        ncol = float(nhorz * Nq * Nq)
        out["cld_frac"] = count / ncol
        with_c = zvals[count > 0]
        out["cld_top"] = float(with_c.max()) if with_c.size else float("nan")
        out["cld_base"] = float(with_c.min()) if with_c.size else float("nan")
        out["cld_cover"] = float((hc.sum(axis=(1, 2)) > 0).sum()) / ncol
        out["lwp"] = water_path(savg[:, len(names)], grid)
        out["iwp"] = water_path(savg[:, len(names) + 1], grid)
        raw.update(count=count, ncol=ncol, liq_z=savg[:, len(names)], ice_z=savg[:, len(names) + 1])
    out["_raw"] = raw
    return out


def sine_state(law, grid, aux):
    """The state of test/Diagnostics/sin_test.jl: rho = 1, u = v = 5 + 2 sin(2 pi (x + y) / 1500),
    w = 10 + 0.5 sin(...), on the law's own initial specific internal energy and total water."""
    Q0 = law.init_state_prognostic(grid, aux, 0.0)
    rho0 = Q0[:, 0]
    e_spec = (Q0[:, 4] - (Q0[:, 1] ** 2 + Q0[:, 2] ** 2 + Q0[:, 3] ** 2) / (2 * rho0)) / rho0   # e_int + Phi
    x, y = aux[:, 0], aux[:, 1]
    s = np.sin(2 * np.pi * (x + y) / 1500.0)
    u, w = 5 + 2 * s, 10 + 0.5 * s
    Q = np.zeros_like(Q0)
    Q[:, 0] = 1.0
    Q[:, 1], Q[:, 2], Q[:, 3] = u, u, w
    Q[:, 4] = e_spec + (u * u + u * u + w * w) / 2
    if Q.shape[1] > 5:
        Q[:, 5] = Q0[:, 5] / rho0
    return Q


def cloudy_state(law, grid, aux, zmax=3000.0):
    """A BOMEX-profile state with a cloud inside the box and horizontal structure: total water raised
    by 30 % between 700 m and 1300 m over two thirds of the box in x (saturated with a wide margin
    there) and lowered by 10 % elsewhere (unsaturated), a smooth perturbation of the three velocities,
    and of the total water inside the cloud."""
    Q = law.init_state_prognostic(grid, aux, 0.0)
    x, y, z = aux[:, 0], aux[:, 1], aux[:, 2]
    Lx = float(grid.vgeo[:, G._x1].max())
    sx, cy = np.sin(2 * np.pi * x / Lx), np.cos(2 * np.pi * y / Lx)
    rho = Q[:, 0]
    Q[:, 1] += rho * 1.0 * sx * cy
    Q[:, 2] += rho * 0.5 * np.cos(2 * np.pi * x / Lx)
    Q[:, 3] += rho * 0.3 * np.sin(2 * np.pi * (x + y) / Lx) * np.sin(np.pi * z / zmax)
    if Q.shape[1] > 5:
        cloud = (z >= 700.0) & (z <= 1300.0) & (x < 2 * Lx / 3)
        Q[:, 5] *= np.where(cloud, 1.3 * (1 + 0.005 * sx * cy), 0.9)
    return Q
