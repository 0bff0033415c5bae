"""MRI-GARK tableaus (odesolvers.MRIGARK_TABLEAUS) and their orders, on the host: the reference's
consistency checks of every table, exact rational conversion, and the two-rate problem of
ode_tests_convergence.jl:614-770 (Sandu 2019, problem 8.2) stepped by the NumPy restatement of
both dostep!s (tests/mrigark_restatement.py)."""
import math
from fractions import Fraction

import numpy as np
import pytest

from cmdg_loader import cm
from mrigark_restatement import explicit_step, implicit_step

ode = cm.odesolvers
EPS = 2.0 ** -52
EXPLICIT = (("MRIGARKERK33aSandu", 3), ("MRIGARKERK45aSandu", 4))
IMPLICIT = (("MRIGARKESDIRK24LSA", 2), ("MRIGARKESDIRK23LSA", 2), ("MRIGARKIRK21aSandu", 2),
            ("MRIGARKESDIRK34aSandu", 3), ("MRIGARKESDIRK46aSandu", 4))
FAST = {"LSRK54": None, "LSRK144": ode.LSRK144_COEFFICIENTS}


def lsrk54_tableau():
    f = lambda n, d: float(Fraction(n, d))
    RKA = (0.0, f(-567301805773, 1357537059087), f(-2404267990393, 2016746695238),
           f(-3550918686646, 2091501179385), f(-1275806237668, 842570457699))
    RKB = (f(1432997174477, 9575080441755), f(5161836677717, 13612068292357),
           f(1720146321549, 2090206949498), f(3134564353537, 4481467310338),
           f(2277821191437, 14882151754819))
    RKC = (0.0, f(1432997174477, 9575080441755), f(2526269341429, 6820363962896),
           f(2006345519317, 3224310063776), f(2802321613138, 2924317926251))
    return RKA, RKB, RKC


FAST["LSRK54"] = lsrk54_tableau()


def test_every_scheme_is_listed():
    assert set(ode.MRIGARK_TABLEAUS) == {n for n, _ in EXPLICIT + IMPLICIT}


@pytest.mark.parametrize("name", [n for n, _ in EXPLICIT])
def test_explicit_tables(name):
    """Δc = rowsum(Γ_0) (exact), Γ_k ./ Δc and γ̂_k / Δc[end] rounded once from the exact
    rationals; Σ Δc = 1; the scaled Γ_0 rows sum to 1."""
    Gs, ghs = ode.MRIGARK_TABLEAUS[name][1]()
    G, gh, dc = ode.mrigark_explicit_coefficients(Gs, ghs)
    dcx = [sum(r, Fraction(0)) for r in Gs[0]]
    assert sum(dcx) == 1
    assert list(dc) == [float(x) for x in dcx]
    for k, Gk in enumerate(Gs):
        for i, row in enumerate(Gk):
            for j, x in enumerate(row):
                assert G[k][i][j] == float(Fraction(x) / dcx[i])
            assert all(G[k][i][j] == 0 for j in range(i + 1, len(row)))      # lower triangular
        assert list(gh[k]) == [float(Fraction(x) / dcx[-1]) for x in ghs[k]]
    for i in range(len(dc)):
        assert abs(sum(Fraction(x) for x in Gs[0][i]) / dcx[i] - 1) == 0


def test_erk33a_delta_parameter():
    a = ode.MRIGARK_TABLEAUS["MRIGARKERK33aSandu"][1]()
    b = ode.MRIGARK_TABLEAUS["MRIGARKERK33aSandu"][1](delta=Fraction(-1, 2))
    assert a == b
    G0 = a[0][0]
    assert G0[1] == [Fraction(-4, 12), Fraction(8, 12), 0]        # (-6δ - 7)/12, (6δ + 11)/12
    assert a[0][1][2][2] == Fraction(-1, 2)


@pytest.mark.parametrize("name", [n for n, _ in IMPLICIT])
def test_implicit_tables(name):
    """The decoupled structure: (2 nstages, nstages + 1) tables, even rows summing to 0 (2 eps),
    the odd rows' sums Δc adding up to 1, one implicit diagonal value (one alpha per step)."""
    Gs, ghs = ode.MRIGARK_TABLEAUS[name][1]()
    G, gh, dc = ode.mrigark_implicit_coefficients(Gs, ghs)
    ns = len(dc)
    assert G.shape[1:] == (2 * ns, ns + 1)
    assert abs(sum(dc) - 1) <= 4 * EPS
    diag = {G[0][2 * s + 1][s + 1] for s in range(ns)}
    assert len(diag) == 1 and diag.pop() > 0
    for k, Gk in enumerate(Gs):
        for i, row in enumerate(Gk):
            for j, x in enumerate(row):
                want = float(x) if isinstance(x, Fraction) else x
                assert G[k][i][j] == want
    if isinstance(Gs[0][0][0], Fraction):
        assert list(dc) == [float(sum(r, Fraction(0))) for r in Gs[0][0::2]]


def test_esdirk24lsa_reference_checks():
    """A ≈ [0; accumulate(Γ0)[2:2:end]], Δc ≈ rowsum(Γ0), the L-stability bound on γ and the
    stage-time order c3 in (2γ, 1) refused otherwise."""
    A, dc, G = ode.esdirk24lsa_base()
    acc = np.cumsum(np.asarray(G), axis=0)
    assert np.allclose(np.vstack([np.zeros((1, 4)), acc[1::2]]), A, rtol=0, atol=1e-15)
    assert np.allclose([sum(r) for r in G], dc, rtol=0, atol=1e-15)
    b = np.asarray(A[-1])
    assert abs(b.sum() - 1) <= 4 * EPS
    assert abs(2 * (np.asarray(A).T @ b).sum() - 1) <= 8 * EPS
    with pytest.raises(ValueError, match="gamma"):
        ode.esdirk24lsa_base(gamma=0.18)
    with pytest.raises(ValueError, match="gamma"):
        ode.esdirk24lsa_base(gamma=0.5)
    with pytest.raises(ValueError, match="c3"):
        ode.esdirk24lsa_base(gamma=0.3, c3=0.55)
    G2 = ode.MRIGARK_TABLEAUS["MRIGARKESDIRK24LSA"][1](gamma=0.25)[0][0]
    assert G2[1][1] == 0.25


def test_esdirk_lambda_cubic():
    lam = ode._esdirk_lambda()
    assert abs(-1 + 9 * lam - 18 * lam ** 2 + 6 * lam ** 3) <= 2 * EPS
    G = ode.MRIGARK_TABLEAUS["MRIGARKESDIRK34aSandu"][1]()[0][0]
    assert G[1][1] == lam and G[3][2] == lam and G[5][3] == lam


def test_implicit_table_checks_refuse():
    with pytest.raises(ValueError, match="sum to 0"):
        ode.mrigark_implicit_coefficients(([[Fraction(1), 0], [Fraction(1, 2), Fraction(1, 2)]],),
                                          ([0, 0],))


# -- the two-rate problem (ode_tests_convergence.jl:614-770) --------------------------------------
OMEGA, LF, LS, XI, AL = 20.0, -10.0, -1.0, 0.1, 1.0
ETA_FS = ((1 - XI) / AL) * (LF - LS)
ETA_SF = -XI * AL * (LF - LS)
OM = ((LF, ETA_FS), (ETA_SF, LS))


def _g(Q, t):
    yf, ys = Q[0], Q[1]
    return (-3 + yf * yf - math.cos(OMEGA * t)) / (2 * yf), (-2 + ys * ys - math.cos(t)) / (2 * ys)


def rhs_fast_inc(dQ, Q, t):
    gf, gs = _g(Q, t)
    dQ[0] += OM[0][0] * gf + OM[0][1] * gs - OMEGA * math.sin(OMEGA * t) / (2 * Q[0])


def rhs_slow(R, Q, t):
    gf, gs = _g(Q, t)
    R[0] = 0.0
    R[1] = OM[1][0] * gf + OM[1][1] * gs - math.sin(t) / (2 * Q[1])


def be_solve(Q, Qhat, alpha, t):
    """ODETestConvNonLinBE: Q = Qhat + alpha rhs_slow(Q, t) in closed form."""
    Q[0] = yf = Qhat[0]
    gf = (-3 + yf * yf - math.cos(OMEGA * t)) / (2 * yf)
    a = 2 - alpha * OM[1][1]
    b = -2 * (Qhat[1] + alpha * OM[1][0] * gf)
    c = alpha * (OM[1][1] * (2 + math.cos(t)) + math.sin(t))
    Q[1] = (-b + math.sqrt(b * b - 4 * a * c)) / (2 * a)


def exact(t):
    return np.array([math.sqrt(3 + math.cos(OMEGA * t)), math.sqrt(2 + math.cos(t))])


def run_two_rate(name, fast, slow_dt, finaltime=1.0):
    kind, make = ode.MRIGARK_TABLEAUS[name]
    Gs, ghs = make()
    coeff = ode.mrigark_explicit_coefficients if kind == "explicit" else ode.mrigark_implicit_coefficients
    G, _, dc = coeff(Gs, ghs)
    G = G.tolist()
    dc = dc.tolist()
    Q = exact(0.0)
    dQ = np.zeros(2)
    Rs = [np.zeros(2) for _ in dc]
    Qhat = np.zeros(2)
    fast_dt = slow_dt / OMEGA
    t = 0.0
    while t < finaltime:                      # solve!(Q, solver; timeend) with adjustfinalstep
        dt = min(slow_dt, finaltime - t)
        if kind == "explicit":
            explicit_step(Q, t, dt, G, dc, rhs_slow, rhs_fast_inc, dQ, FAST[fast], fast_dt, Rs)
        else:
            implicit_step(Q, t, dt, G, dc, rhs_slow, be_solve, rhs_fast_inc, dQ, FAST[fast], fast_dt,
                          Rs, Qhat)
        t = finaltime if t + slow_dt > finaltime else t + slow_dt
    return float(np.linalg.norm(Q - exact(finaltime)))


@pytest.mark.parametrize("fast", ["LSRK54", "LSRK144"])
@pytest.mark.parametrize("name,order", EXPLICIT + IMPLICIT)
def test_two_rate_convergence(name, order, fast):
    """Slow dt 2^-7, 2^-8, 2^-9, fast dt = slow dt / ω, final time 1: the last observed rate is
    within 0.3 of the scheme's order."""
    err = [run_two_rate(name, fast, 2.0 ** -k) for k in (7, 8, 9)]
    rate = [math.log2(err[i] / err[i + 1]) for i in range(2)]
    print("%s / %s: errors %s rates %s" % (name, fast, err, rate))
    assert abs(rate[-1] - order) <= 0.3, (err, rate)
