"""The dry AtmosModel's own numerical fluxes, restated pointwise in NumPy (test infrastructure).

Written from the reference, ``src/Atmos/Model/AtmosModel.jl``: ``RoeNumericalFlux`` :1003-1130,
``HLLCNumericalFlux`` :1154-1276, ``LMARSNumericalFlux`` :1515-1604, with the first-order fluxes of
``tendencies_mass.jl:5-7``, ``tendencies_momentum.jl:13-29`` and ``tendencies_energy.jl:7-21`` and the
closed forms of a dry ``PhaseDry`` state (Thermodynamics.jl): ``e_int = e_tot - |u|^2 / 2 - Phi``,
``T = T_0 + e_int / cv_d``, ``p = rho R_d T``, ``c = sqrt(cp_d / cv_d R_d T)``, ``h_tot = e_tot +
R_d T``.  It shares no text with the device functor or with the oracle's C, and it works on arrays
of face-node pairs in whatever floating-point type it is asked for (``np.float64`` or
``np.longdouble``), so that the longdouble run gives the double one its own rounding envelope.

Prognostic state ``rho, rho u (3), rho e``; the auxiliary columns it reads are ``Phi`` at
``off_phi`` (with an orientation) and the reference pressure at ``off_ref + 1`` (with a reference
state and ``subtract_off``).
"""
import numpy as np

ROE, HLLC, LMARS = 2, 3, 4


class Switches:
    """What the law is configured with: the constants of the parameter set (taken as the doubles
    they are) and the three switches of the model."""

    def __init__(self, ps, orientation, ref_state, subtract_off, off_phi=3, off_ref=None):
        self.R_d, self.cp_d, self.cv_d, self.T_0 = (float(ps.R_d), float(ps.cp_d), float(ps.cv_d),
                                                    float(ps.T_0))
        self.orientation, self.ref_state = bool(orientation), bool(ref_state)
        self.subtract_off = bool(subtract_off) and self.ref_state
        self.off_phi = off_phi
        self.off_ref = (off_phi + (4 if self.orientation else 0)) if off_ref is None else off_ref

    @classmethod
    def of(cls, law):
        return cls(law.ps, law.orientation != 0, law.ref_state is not None, law.subtract_off,
                   law.off_phi, law.off_ref)


class _Side:
    """One side of the face: primitive and thermodynamic fields of ``(Q, aux)``."""

    def __init__(self, sw, n, Q, aux, ft):
        c = lambda v: ft(v)
        self.rho = Q[:, 0]
        self.rhou = Q[:, 1:4]
        self.rhoe = Q[:, 4]
        self.u = self.rhou / self.rho[:, None]
        self.un = (self.u * n).sum(axis=1)
        self.e = self.rhoe / self.rho
        self.Phi = aux[:, sw.off_phi] if sw.orientation else np.zeros_like(self.rho)
        e_int = self.e - (self.u * self.u).sum(axis=1) / 2 - self.Phi
        self.T = c(sw.T_0) + e_int / c(sw.cv_d)
        self.p = self.rho * c(sw.R_d) * self.T
        self.c = np.sqrt(c(sw.cp_d) / c(sw.cv_d) * c(sw.R_d) * self.T)
        self.h = self.e + c(sw.R_d) * self.T
        self.p_ref = aux[:, sw.off_ref + 1] if sw.subtract_off else np.zeros_like(self.rho)
        # flux_first_order' * n: mass, momentum (Advect + PressureGradient), energy (Advect + Pressure)
        self.Fn = np.empty_like(Q)
        self.Fn[:, 0] = self.rho * self.un
        self.Fn[:, 1:4] = self.rhou * self.un[:, None] + (self.p - self.p_ref)[:, None] * n
        self.Fn[:, 4] = self.un * self.rhoe + self.un * self.p


def physical_normal_flux(sw, n, Q, aux, dtype=np.float64):
    """``flux_first_order!(...)' * n`` of one state."""
    ft = np.dtype(dtype).type
    n, Q, aux = (np.asarray(a, dtype=dtype) for a in (n, Q, aux))
    return _Side(sw, n, Q, aux, ft).Fn


def _roe_average(rm, rp, vm, vp):
    sm, sp = np.sqrt(rm), np.sqrt(rp)
    if vm.ndim == 2:
        sm, sp = sm[:, None], sp[:, None]
    return (sm * vm + sp * vp) / (sm + sp)


def numerical_flux(nf, sw, n, QM, auxM, QP, auxP, dtype=np.float64):
    """``numerical_flux_first_order!`` for ``nf`` in (ROE, HLLC, LMARS) at ``k`` face-node pairs:
    ``n (k, 3)``, ``QM, QP (k, 5)``, ``auxM, auxP (k, naux)``.  Returns ``(fluxn (k, 5), info)``;
    ``info`` says which way every sample went:

    * ``hllc``: 0 for ``0 <= S-``, 1 for ``S- < 0 <= S0``, 2 for ``S0 < 0 <= S+``, 3 otherwise;
    * ``lmars_up``: ``u_half > 0``;
    * ``roe_signs``: ``(k, 3)`` signs of ``u~n - c~``, ``u~n``, ``u~n + c~``;
    * ``tie``: the distance of ``S-``, ``S0``, ``S+`` and ``u_half`` from zero, the smallest of
      the four, over the larger sound speed of the pair (all three fluxes are evaluated for it);
    * ``un_over_c``: ``|u- . n| / c-``."""
    ft = np.dtype(dtype).type
    n, QM, auxM, QP, auxP = (np.asarray(a, dtype=dtype) for a in (n, QM, auxM, QP, auxP))
    M, P = _Side(sw, n, QM, auxM, ft), _Side(sw, n, QP, auxP, ft)
    info = {}

    # ---- Roe: central flux minus half the upwinded jump in characteristic variables
    rho_t = np.sqrt(M.rho * P.rho)
    u_t = _roe_average(M.rho, P.rho, M.u, P.u)
    h_t = _roe_average(M.rho, P.rho, M.h, P.h)
    c_t = np.sqrt(_roe_average(M.rho, P.rho, M.c ** 2, P.c ** 2))
    utn = (u_t * n).sum(axis=1)
    info["roe_signs"] = np.stack([np.sign(utn - c_t), np.sign(utn), np.sign(utn + c_t)],
                                 axis=1).astype(int)
    # ---- HLLC wave speeds
    Sm = np.minimum(M.un - M.c, P.un - P.c)
    Sp = np.maximum(M.un + M.c, P.un + P.c)
    S0 = ((P.p - M.p + M.rho * M.un * (Sm - M.un) - P.rho * P.un * (Sp - P.un))
          / (M.rho * (Sm - M.un) - P.rho * (Sp - P.un)))
    branch = np.where(0 <= Sm, 0, np.where(0 <= S0, 1, np.where(0 <= Sp, 2, 3)))
    info["hllc"] = branch
    # ---- LMARS interface velocity and pressure (beta = 1); p is the perturbation pressure when
    # the reference state is subtracted, and the sound speed is the minus side's
    pm, pp = M.p - M.p_ref, P.p - P.p_ref
    u_half = (P.un + M.un) / 2 - 1 / (M.rho + P.rho) / M.c * (pp - pm)
    p_half = (pp + pm) / 2 - ((M.rho + P.rho) * M.c) / 4 * (P.un - M.un)
    up = u_half > 0
    info["lmars_up"] = up
    cmax = np.maximum(M.c, P.c)
    info["tie"] = np.minimum(np.minimum(np.abs(Sm), np.abs(S0)),
                             np.minimum(np.abs(Sp), np.abs(u_half))) / cmax
    info["un_over_c"] = np.abs(M.un) / M.c

    if nf == ROE:
        drho, dp, du = P.rho - M.rho, P.p - M.p, P.u - M.u
        dun = (du * n).sum(axis=1)
        w1 = np.abs(utn - c_t) * (dp - rho_t * c_t * dun) / (2 * c_t ** 2)
        w2 = np.abs(utn + c_t) * (dp + rho_t * c_t * dun) / (2 * c_t ** 2)
        w3 = np.abs(utn) * (drho - dp / c_t ** 2)
        w4 = np.abs(utn) * rho_t
        F = (M.Fn + P.Fn) / 2
        F[:, 0] -= (w1 + w2 + w3) / 2
        F[:, 1:4] -= (w1[:, None] * (u_t - c_t[:, None] * n) + w2[:, None] * (u_t + c_t[:, None] * n)
                      + w3[:, None] * u_t + w4[:, None] * (du - dun[:, None] * n)) / 2
        # Phi is the minus side's (gravitational_potential(balance_law, state_auxiliary-))
        F[:, 4] -= (w1 * (h_t - c_t * utn) + w2 * (h_t + c_t * utn)
                    + w3 * ((u_t * u_t).sum(axis=1) / 2 + M.Phi - ft(sw.T_0) * ft(sw.cv_d))
                    + w4 * ((u_t * du).sum(axis=1) - utn * dun)) / 2
        return F, info

    if nf == HLLC:
        p0 = (P.p + M.p + M.rho * (Sm - M.un) * (S0 - M.un) + P.rho * (Sp - P.un) * (S0 - P.un)) / 2
        pD = np.zeros_like(QM)
        pD[:, 1:4] = (p0 - (M.p_ref + P.p_ref) / 2)[:, None] * n
        pD[:, 4] = p0 * S0
        col = lambda v: v[:, None]
        with np.errstate(divide="ignore", invalid="ignore"):
            star_m = (col(S0) * (col(Sm) * QM - M.Fn) + col(Sm) * pD) / col(Sm - S0)
            star_p = (col(S0) * (col(Sp) * QP - P.Fn) + col(Sp) * pD) / col(Sp - S0)
        b = col(branch)
        F = np.where(b == 0, M.Fn, np.where(b == 1, star_m, np.where(b == 2, star_p, P.Fn)))
        return F, info

    if nf == LMARS:
        F = np.empty_like(QM)
        F[:, 0] = np.where(up, M.rho, P.rho) * u_half
        F[:, 1:4] = np.where(up[:, None], M.rhou, P.rhou) * u_half[:, None] + p_half[:, None] * n
        F[:, 4] = np.where(up, M.rho * M.h, P.rho * P.h) * u_half
        return F, info

    raise ValueError("nf = %r: ROE, HLLC or LMARS" % (nf,))
