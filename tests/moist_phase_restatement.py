"""The equilibrium moist thermodynamics of the LES law (csrc/physics_moist.h, oracle/physics_moist.c),
stated a third time: from the physics, in mpmath at 40 digits, with no device or oracle code.  It takes
the constants of ``MoistParameters`` and none of its methods.

What is written differently from the two twins, on purpose:
  * the internal energy is a sum over the four species (dry air, vapour, liquid, ice), each with its
    own heat capacity and its own reference energy, not ``cv_m (T - T_0) + ...``;
  * ``R_m`` and ``cp_m`` are mass-weighted sums over the species, not the ``q_tot, q_liq, q_ice`` forms;
  * the saturation vapour pressure is the closed form DESIGN.md states (``LH_0`` and ``dcp`` weighted
    by the liquid fraction), and ``p_vs_clausius_clapeyron`` integrates the Clausius-Clapeyron
    relation numerically with the same weights: the two must agree, which settles ``pow`` / ``exp``
    forms without anybody's program text;
  * the equilibrium temperature is the root of ``e_int(T, partition(T)) = e_int`` by bisection on
    [150, 400] K: no derivative, so no ``dlam`` term to get wrong.

``newton_float64`` is a plain double copy of the Newton recurrence the law runs.  It is used only to
prove that the inputs of tests/golden/moist_phase_cases.npz converge: it is not a reference.

mpmath is needed by everything but ``constants``, ``newton_float64`` and ``load_cases``.
"""
import math
import os

import numpy as np

try:
    import mpmath as mp
except ImportError:          # the GPU tests read the fixture only
    mp = None

DIGITS = 40
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "moist_phase_cases.npz")
NAMES = ("R_d", "cp_d", "cv_d", "T_0", "MSLP", "R_v", "cp_v", "cp_l", "cp_i", "LH_v0", "LH_s0",
         "T_triple", "T_freeze", "T_icenuc", "p_triple", "T_min")
GROUPS = ("ice", "mixed", "warm", "near T_freeze", "near T_icenuc", "barely saturated", "unsaturated",
          "clamped start")
INPUTS = ("rho", "q_tot", "e_int")
OUTPUTS = ("T", "q_liq", "q_ice", "theta_v", "q_vap", "R_m", "cp_m", "pres", "theta_dry", "theta_vir",
           "theta_liq_ice", "h_int")
T_LO, T_HI = 150, 400


def constants(ps):
    """The doubles the law hands to the device, by name."""
    k = {n: float(getattr(ps, n)) for n in NAMES if n != "p_triple"}
    k["p_triple"] = float(ps.press_triple)
    return k


def load_cases():
    with np.load(FIXTURE) as f:
        return {n: f[n] for n in f.files}


# ---- 40 digits --------------------------------------------------------------------------------------
def exact(k):
    """The same constants as mpf (a double converts exactly)."""
    return {n: mp.mpf(v) for n, v in k.items()}


def liquid_fraction(c, T):
    if T >= c["T_freeze"]:
        return mp.mpf(1)
    if T <= c["T_icenuc"]:
        return mp.mpf(0)
    return (T - c["T_icenuc"]) / (c["T_freeze"] - c["T_icenuc"])


def _latent(c, T):
    """``LH_0`` and ``dcp = cp_v - cp_condensate`` of the phase mixture at ``T``."""
    lam = liquid_fraction(c, T)
    LH_0 = lam * c["LH_v0"] + (1 - lam) * c["LH_s0"]
    dcp = lam * (c["cp_v"] - c["cp_l"]) + (1 - lam) * (c["cp_v"] - c["cp_i"])
    return LH_0, dcp


def p_vs(c, T):
    """Saturation vapour pressure, closed form: Clausius-Clapeyron with constant heat capacities,
    integrated from the triple point."""
    LH_0, dcp = _latent(c, T)
    return (c["p_triple"] * (T / c["T_triple"]) ** (dcp / c["R_v"])
            * mp.exp((LH_0 - dcp * c["T_0"]) / c["R_v"] * (1 / c["T_triple"] - 1 / T)))


def p_vs_clausius_clapeyron(c, T):
    """d ln p / dT = L(T') / (R_v T'^2) with L(T') = LH_0 + dcp (T' - T_0), by quadrature from the
    triple point; the weights are those of ``liquid_fraction(T)``, held over the path."""
    LH_0, dcp = _latent(c, T)
    integral = mp.quad(lambda x: (LH_0 + dcp * (x - c["T_0"])) / (c["R_v"] * x * x), [c["T_triple"], T])
    return c["p_triple"] * mp.exp(integral)


def q_vs(c, T, rho):
    return p_vs(c, T) / (rho * c["R_v"] * T)


def partition(c, T, rho, q_tot):
    """Equilibrium condensate: what exceeds saturation, split by the liquid fraction."""
    q_c = max(q_tot - q_vs(c, T, rho), mp.mpf(0))
    lam = liquid_fraction(c, T)
    return lam * q_c, (1 - lam) * q_c


def e_int_species(c, T, q_tot, q_liq, q_ice):
    """Specific internal energy, species by species, about ``T_0``: vapour carries ``e_int_v0 =
    LH_v0 - R_v T_0``, ice ``-e_int_i0 = -(LH_s0 - LH_v0)``."""
    dT = T - c["T_0"]
    q_vap = q_tot - q_liq - q_ice
    cv_v = c["cp_v"] - c["R_v"]
    e_int_v0 = c["LH_v0"] - c["R_v"] * c["T_0"]
    e_int_i0 = c["LH_s0"] - c["LH_v0"]
    return ((1 - q_tot) * c["cv_d"] * dT + q_vap * (cv_v * dT + e_int_v0) + q_liq * c["cp_l"] * dT
            + q_ice * (c["cp_i"] * dT - e_int_i0))


def e_int_equil(c, T, rho, q_tot):
    q_liq, q_ice = partition(c, T, rho, q_tot)
    return e_int_species(c, T, q_tot, q_liq, q_ice)


def root_T(c, e_int, rho, q_tot):
    """``T*`` with ``e_int_equil(T*) = e_int``: bisection on [150, 400] K down to 1e-36 K."""
    lo, hi = mp.mpf(T_LO), mp.mpf(T_HI)
    assert e_int_equil(c, lo, rho, q_tot) < e_int < e_int_equil(c, hi, rho, q_tot)
    while hi - lo > mp.mpf(10) ** -36:
        mid = (lo + hi) / 2
        if e_int_equil(c, mid, rho, q_tot) < e_int:
            lo = mid
        else:
            hi = mid
    return (lo + hi) / 2


def T_all_vapour(c, e_int, q_tot):
    """The temperature of ``e_int`` with no condensate (the unsaturated closed form)."""
    cv_v = c["cp_v"] - c["R_v"]
    e_int_v0 = c["LH_v0"] - c["R_v"] * c["T_0"]
    return c["T_0"] + (e_int - q_tot * e_int_v0) / ((1 - q_tot) * c["cv_d"] + q_tot * cv_v)


def derived(c, T, rho, q_tot, e_int):
    """Every stored output from its definition, at the equilibrium temperature ``T``."""
    q_liq, q_ice = partition(c, T, rho, q_tot)
    q_vap = q_tot - q_liq - q_ice
    R_m = (1 - q_tot) * c["R_d"] + q_vap * c["R_v"]
    cp_m = (1 - q_tot) * c["cp_d"] + q_vap * c["cp_v"] + q_liq * c["cp_l"] + q_ice * c["cp_i"]
    pres = rho * R_m * T
    theta_dry = T / (pres / c["MSLP"]) ** (R_m / cp_m)
    theta_vir = R_m / c["R_d"] * theta_dry
    theta_liq_ice = theta_dry * (1 - (c["LH_v0"] * q_liq + c["LH_s0"] * q_ice) / (cp_m * T))
    return dict(T=T, q_liq=q_liq, q_ice=q_ice, theta_v=theta_vir, q_vap=q_vap, R_m=R_m, cp_m=cp_m, pres=pres,
                theta_dry=theta_dry, theta_vir=theta_vir, theta_liq_ice=theta_liq_ice, h_int=e_int + R_m * T)


def answers(k, rho, q_tot, e_int):
    """The outputs of one case (three doubles in), rounded to double."""
    with mp.workdps(DIGITS):
        c = exact(k)
        rho, q_tot, e_int = mp.mpf(float(rho)), mp.mpf(float(q_tot)), mp.mpf(float(e_int))
        out = derived(c, root_T(c, e_int, rho, q_tot), rho, q_tot, e_int)
        return {n: float(out[n]) for n in OUTPUTS}


# ---- the Newton recurrence in double ------------------------------------------------------------------
def newton_float64(k, e_int, rho, q_tot, maxiter=40, tol=1e-11):
    """The law's saturation adjustment in plain Python floats.  Returns ``(T, steps, stopped)``:
    ``steps`` Newton steps were taken (0 for an unsaturated state), ``stopped`` says whether the last
    one was shorter than ``tol`` (always true for an unsaturated state)."""
    cv_v = k["cp_v"] - k["R_v"]
    e_v0 = k["LH_v0"] - k["R_v"] * k["T_0"]
    e_i0 = k["LH_s0"] - k["LH_v0"]

    def lam_of(T):
        if T > k["T_freeze"]:
            return 1.0
        if T > k["T_icenuc"]:
            return (T - k["T_icenuc"]) / (k["T_freeze"] - k["T_icenuc"])
        return 0.0

    def cv_m(ql, qi):
        return k["cv_d"] + (cv_v - k["cv_d"]) * q_tot + (k["cp_l"] - cv_v) * ql + (k["cp_i"] - cv_v) * qi

    def qvs_of(T):
        lam = lam_of(T)
        LH_0 = lam * k["LH_v0"] + (1 - lam) * k["LH_s0"]
        dcp = lam * (k["cp_v"] - k["cp_l"]) + (1 - lam) * (k["cp_v"] - k["cp_i"])
        pvs = (k["p_triple"] * math.pow(T / k["T_triple"], dcp / k["R_v"])
               * math.exp((LH_0 - dcp * k["T_0"]) / k["R_v"] * (1 / k["T_triple"] - 1 / T)))
        return pvs / (rho * k["R_v"] * T)

    T = k["T_0"] + (e_int - q_tot * e_v0) / cv_m(0.0, 0.0)
    if T < k["T_min"]:
        T = k["T_min"]
    if q_tot <= qvs_of(T) and T > k["T_min"]:
        return T, 0, True
    for it in range(maxiter):
        lam, qvs = lam_of(T), qvs_of(T)
        qc = max(q_tot - qvs, 0.0)
        ql, qi = lam * qc, (1 - lam) * qc
        f = cv_m(ql, qi) * (T - k["T_0"]) + (q_tot - ql) * e_v0 - qi * (e_v0 + e_i0) - e_int
        L = lam * k["LH_v0"] + (1 - lam) * k["LH_s0"]
        dlam = 1 / (k["T_freeze"] - k["T_icenuc"]) if k["T_icenuc"] < T < k["T_freeze"] else 0.0
        dqvs = qvs * L / (k["R_v"] * T * T)
        dcvm = cv_v - lam * k["cp_l"] - (1 - lam) * k["cp_i"]
        fp = cv_m(ql, qi) + (e_v0 + (1 - lam) * e_i0 + (T - k["T_0"]) * dcvm) * dqvs + (ql + qi) * e_i0 * dlam
        dT = f / fp
        T -= dT
        if abs(dT) < tol:
            return T, it + 1, True
    return T, maxiter, False
