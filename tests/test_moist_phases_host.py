"""The saturation adjustment of the moist law in the ice, mixed and warm regimes against a 40-digit
statement of the physics (tests/moist_phase_restatement.py, tests/golden/moist_phase_cases.npz, written
by scripts/make_golden_moist_phases.py).  CPU only: the fixture is what it claims to be, its inputs lie
where the law's Newton recurrence converges, and the oracle (oracle/physics_moist.c) is held to it at
the bounds the device is held to in tests/test_gpu_moist_phases.py:

    |T - T_ref| <= 1e-11 K (the stopping tolerance),  |q_liq - ref|, |q_ice - ref| <= 1e-12 q_tot,
    theta_v to 1e-12 relative, no condensate at all in unsaturated air.
"""
import ctypes as C

import numpy as np
import pytest

import moist_phase_restatement as R
from helpers import cm, moist_converged_law, observe, rising_bubble_setup, tile_moist_phase_cases

COUNTS = {"ice": 96, "mixed": 128, "warm": 96, "near T_freeze": 48, "near T_icenuc": 48,
          "barely saturated": 32, "unsaturated": 64, "clamped start": 16}


@pytest.fixture(scope="module")
def cases():
    return R.load_cases()


@pytest.fixture(scope="module")
def k():
    return R.constants(cm.moist.MoistParameters())


def _group(cases, name):
    return cases["group"] == R.GROUPS.index(name)


def test_fixture_holds_the_cases_it_names(cases, k):
    """Counts, the input box (rho in [0.3, 1.3], q_tot <= 0.04), and that every group sits in the
    regime it is named after."""
    n = len(cases["group"])
    assert n == sum(COUNTS.values()) and set(cases) == {"group"} | set(R.INPUTS) | set(R.OUTPUTS)
    for name, count in COUNTS.items():
        assert int(_group(cases, name).sum()) == count, name
    assert cases["rho"].min() >= 0.3 and cases["rho"].max() <= 1.3
    assert 0 < cases["q_tot"].min() and cases["q_tot"].max() <= 0.04
    T, ql, qi = cases["T"], cases["q_liq"], cases["q_ice"]
    Tf, Ti = k["T_freeze"], k["T_icenuc"]
    g = _group(cases, "ice")
    assert (T[g] >= 200).all() and (T[g] <= 232.9).all() and (ql[g] == 0).all() and (qi[g] > 0).all()
    g = _group(cases, "mixed")
    assert (T[g] >= 233.1).all() and (T[g] <= 273.1).all() and (ql[g] > 0).all() and (qi[g] > 0).all()
    g = _group(cases, "warm")
    assert (T[g] >= 273.2).all() and (T[g] <= 305).all() and (ql[g] > 0).all() and (qi[g] == 0).all()
    for name, edge in (("near T_freeze", Tf), ("near T_icenuc", Ti)):
        g = _group(cases, name)
        assert (np.abs(T[g] - edge) <= 1e-3).all() and ((ql + qi)[g] > 0).all()
        assert (T[g] < edge).sum() >= 12 and (T[g] > edge).sum() >= 12, name       # both sides of the kink
    g = _group(cases, "barely saturated")
    rel = (ql + qi)[g] / cases["q_vap"][g]
    assert (rel >= 0.99e-9).all() and (rel <= 1.01e-6).all()
    assert (T[g] < Ti).any() and ((T[g] > Ti) & (T[g] < Tf)).any() and (T[g] > Tf).any()
    g = _group(cases, "unsaturated")
    assert (ql[g] == 0).all() and (qi[g] == 0).all() and (cases["q_vap"][g] == cases["q_tot"][g]).all()
    assert (T[g] < Ti).any() and (T[g] > Tf).any()
    g = _group(cases, "clamped start")
    cv_v, e_v0 = k["cp_v"] - k["R_v"], k["LH_v0"] - k["R_v"] * k["T_0"]
    T1 = k["T_0"] + (cases["e_int"][g] - cases["q_tot"][g] * e_v0) / (
        k["cv_d"] + (cv_v - k["cv_d"]) * cases["q_tot"][g])
    assert (T1 < k["T_min"] - 1).all() and (T[g] >= 200).all() and (qi[g] > 0.01).all()


def test_fixture_is_fresh(cases, k):
    """Every tenth case recomputed at 40 digits gives the stored doubles, bit for bit."""
    pytest.importorskip("mpmath")
    for i in range(0, len(cases["group"]), 10):
        out = R.answers(k, *(cases[n][i] for n in R.INPUTS))
        for name in R.OUTPUTS:
            assert out[name] == cases[name][i], (i, name, out[name], cases[name][i])


def test_clausius_clapeyron_gives_the_closed_form(k):
    """p_triple exp(int_{T_triple}^{T} (LH_0 + dcp (T' - T_0)) / (R_v T'^2) dT') by quadrature, with the
    weights of the liquid fraction at T, equals the closed form to 1e-30 relative: in the pure phases
    this is the physics, and it settles the exponent of the power and the sign inside the
    exponential.  The species-sum energy closes the pure-phase latent heats the same way: the energy
    of vapour less that of the condensate at T is L(T) - R_v T."""
    mp = pytest.importorskip("mpmath")
    with mp.workdps(R.DIGITS):
        c = R.exact(k)
        temps = [200, 215.5, 232.9, 233, 233.1, 240, 253.075, 266, 273.1, 273.15, 273.16, 273.2, 290, 305]
        worst = mp.mpf(0)
        for T in temps:
            T = mp.mpf(T)
            a, b = R.p_vs(c, T), R.p_vs_clausius_clapeyron(c, T)
            worst = max(worst, abs(a - b) / b)
        assert worst <= mp.mpf(10) ** -30, worst
        assert abs(R.p_vs(c, c["T_triple"]) - c["p_triple"]) <= mp.mpf(10) ** -35 * c["p_triple"]
        # well-known values: 611.657 Pa at the triple point, about 3.5 kPa at 300 K over liquid and
        # about 1.3e1 Pa at 233 K over ice (Murphy & Koop 2005 give 12.8 Pa)
        assert 3400 < R.p_vs(c, mp.mpf(300)) < 3700 and 11 < R.p_vs(c, mp.mpf(233)) < 14
        for T, q in ((mp.mpf(290), "l"), (mp.mpf(220), "i")):
            one, zero = mp.mpf(1), mp.mpf(0)
            e_vap = R.e_int_species(c, T, one, zero, zero)
            e_con = R.e_int_species(c, T, one, one if q == "l" else zero, one if q == "i" else zero)
            LH_0, dcp = R._latent(c, T)
            assert abs((e_vap - e_con) - (LH_0 + dcp * (T - c["T_0"]) - c["R_v"] * T)) <= mp.mpf(10) ** -30


def test_newton_in_double_converges_on_every_case(cases, k):
    """The reference box: with maxiter 40 and tolerance 1e-11 the recurrence stops by itself in fewer
    than 40 steps on every case of the fixture, within 1e-11 K of the 40-digit root.  No case is
    excluded."""
    worst, most = 0.0, 0
    for i in range(len(cases["group"])):
        T, steps, stopped = R.newton_float64(k, *(float(cases[n][i]) for n in ("e_int", "rho", "q_tot")))
        assert stopped and steps < 40, (i, R.GROUPS[cases["group"][i]], steps)
        assert (steps == 0) == (cases["group"][i] == R.GROUPS.index("unsaturated")), i
        err = abs(T - cases["T"][i])
        assert err <= 1e-11, (i, R.GROUPS[cases["group"][i]], err)
        worst, most = max(worst, err), max(most, steps)
    print("float64 Newton: worst |T - root| = %.2e K, most steps %d" % (worst, most))


def test_oracle_adjustment_matches_the_fixture(oracle, cases, k):
    """``orc_moist_saturation_adjustment`` on every case, and theta_v from the oracle's nodal refresh of
    the cases tiled over the smallest bubble grid, at the device's bounds."""
    law = moist_converged_law()
    ph = oracle.OraclePhysics(law)
    L = oracle.lib()
    ql, qi, eb = C.c_double(), C.c_double(), C.c_double()
    dT, dql, dqi = 0.0, 0.0, 0.0
    unsat = _group(cases, "unsaturated")
    for i in range(len(cases["group"])):
        rho, qt, e = (float(cases[n][i]) for n in R.INPUTS)
        T = L.orc_moist_saturation_adjustment(ph.c, e, rho, qt, C.byref(ql), C.byref(qi), C.byref(eb))
        dT = max(dT, abs(T - cases["T"][i]))
        dql = max(dql, abs(ql.value - cases["q_liq"][i]) / qt)
        dqi = max(dqi, abs(qi.value - cases["q_ice"][i]) / qt)
        if unsat[i]:
            assert ql.value == 0 and qi.value == 0, i
    print("oracle: |dT| %.2e K, |dq_liq| / q_tot %.2e, |dq_ice| / q_tot %.2e" % (dT, dql, dqi))
    assert observe("moist phases oracle |T - T_ref| (K)", dT) <= 1e-11
    assert observe("moist phases oracle |q_liq - ref| / q_tot", dql) <= 1e-12
    assert observe("moist phases oracle |q_ice - ref| / q_tot", dqi) <= 1e-12
    _, grid = rising_bubble_setup(nx=2, ny=2, nz=2, N=4)
    odg = oracle.OracleDGModel(law, grid)
    Q, idx = tile_moist_phase_cases(grid, odg.state_auxiliary, cases)
    odg.update_auxiliary_state(Q, 0.0, "real")
    aux = odg.state_auxiliary
    dth = np.abs(aux[:, 16] / cases["theta_v"][idx] - 1).max()
    print("oracle on the grid: theta_v rel. %.2e, |dT| %.2e K" % (dth, np.abs(aux[:, 15] - cases["T"][idx]).max()))
    assert observe("moist phases oracle theta_v rel.", dth) <= 1e-12
    assert np.abs(aux[:, 15] - cases["T"][idx]).max() <= 1e-11
    assert np.abs((aux[:, 17] - cases["q_liq"][idx]) / cases["q_tot"][idx]).max() <= 1e-12
    assert np.abs((aux[:, 18] - cases["q_ice"][idx]) / cases["q_tot"][idx]).max() <= 1e-12
