"""The oracle's Roe / HLLC / LMARS fluxes of the dry atmosphere law, pointwise, on moving states
(CPU only): against the independent NumPy restatement (tests/atmos_nf_restatement.py, written
from the reference's source) in extended precision, and against properties that need no
restatement.  The device is compared with this oracle in tests/test_gpu_atmos_law_fluxes.py.

Sample: ``K`` random admissible pairs, ``rho`` and ``T`` within 10 % of (1 kg/m^3, 280 K),
``u = c(T) N(0, I)`` (Mach scale 1), ``Phi`` in [0, 5e5] and ``p_ref`` within 10 % of ``p`` drawn
independently on the two sides, unit normals uniform on the sphere; auxiliary columns the fluxes
have no business reading are NaN.  Before anything is compared the census of the sample is
asserted: every HLLC branch, both LMARS directions and all four Roe sign patterns are populated
and no sample sits at a tie.

Bounds.  ``FACTOR`` is the issue's: the oracle may differ from the longdouble restatement by 8
times the double restatement's own rounding envelope.  ``PROP`` bounds the exact identities in
units of eps times the largest entry of the flux column: each flux is some 40 operations on
terms no larger than a few times that entry, and the HLLC star state divides by ``S- - S0`` or
``S+ - S0``, at least one sound speed, where the numerator carries ``|S|`` up to ``|u.n| + c``
(five sound speeds in this sample): 40 x 5, rounded up to 256."""
import numpy as np
import pytest

import atmos_nf_restatement as R
from atmos_nf_cases import ROE_PATTERNS, conserved, soundspeed
from cmdg_loader import cm
from helpers import observe

A = cm.atmos
EPS = np.finfo(float).eps
K = 4000
FACTOR = 8
PROP = 256 * EPS
FLUXES = {"Roe": R.ROE, "HLLC": R.HLLC, "LMARS": R.LMARS}
CONFIGS = [(False, False), (True, False), (True, True)]     # (orientation + reference state, subtract_off)
IDS = ["plain", "oriented", "oriented-subtract"]


def make_law(oriented, subtract):
    ps = A.PlanetParameters()
    if not oriented:
        return A.DryAtmosModel(None, orientation=A.ORIENT_NONE, ref_state=None, param_set=ps)
    return A.DryAtmosModel(None, orientation=A.ORIENT_FLAT,
                           ref_state=A.DecayingTemperatureProfile(ps, 290.0, 220.0, 8e3),
                           subtract_off=subtract, sources=A.SRC_GRAVITY,
                           boundary_conditions=(A.BC_ATMOS_DEFAULT, A.BC_ATMOS_DEFAULT), param_set=ps)


def unit_normals(rng, k):
    n = rng.standard_normal((k, 3))
    return n / np.sqrt((n * n).sum(axis=1))[:, None]


def make_aux(law, Phi, p_ref, rho_ref):
    aux = np.full((len(Phi), law.naux), np.nan)
    if law.orientation != A.ORIENT_NONE:
        aux[:, law.off_phi] = Phi
    if law.ref_state is not None:
        aux[:, law.off_ref] = rho_ref
        aux[:, law.off_ref + 1] = p_ref
    return aux


def side(law, rng, k, mach=1.0, Phi=None, rel_ref=None):
    """One side of ``k`` pairs: primitives, state and auxiliary state."""
    ps = law.ps
    rho = 1.0 * (1 + 0.1 * rng.uniform(-1, 1, k))
    T = 280.0 * (1 + 0.1 * rng.uniform(-1, 1, k))
    u = mach * soundspeed(ps, T)[:, None] * rng.standard_normal((k, 3))
    draw_phi, draw_ref = rng.uniform(0.0, 5e5, k), 1 + 0.1 * rng.uniform(-1, 1, k)
    Phi = draw_phi if Phi is None else Phi
    if law.orientation == A.ORIENT_NONE:
        Phi = np.zeros(k)
    rel_ref = draw_ref if rel_ref is None else rel_ref
    aux = make_aux(law, Phi, rel_ref * (rho * ps.R_d * T), rho * rel_ref)
    return dict(rho=rho, T=T, u=u, Phi=Phi, Q=conserved(ps, rho, T, u, Phi), aux=aux)


def rebuild(law, s, **changed):
    """``s`` with some primitives replaced; the auxiliary state is kept."""
    d = dict(s, **changed)
    d["Q"] = conserved(law.ps, d["rho"], d["T"], d["u"], d["Phi"])
    return d


class Sample:
    def __init__(self, oriented, subtract):
        self.law = make_law(oriented, subtract)
        self.sw = R.Switches.of(self.law)
        rng = np.random.default_rng(20 + 2 * oriented + subtract)
        self.n = unit_normals(rng, K)
        self.M, self.P = side(self.law, rng, K), side(self.law, rng, K)
        self.args = (self.n, self.M["Q"], self.M["aux"], self.P["Q"], self.P["aux"])
        self.f64 = {nf: R.numerical_flux(nf, self.sw, *self.args) for nf in FLUXES.values()}
        self.fld = {nf: R.numerical_flux(nf, self.sw, *self.args, dtype=np.longdouble)
                    for nf in FLUXES.values()}


_SAMPLES = {}


def sample(oriented, subtract):
    key = (oriented, subtract)
    if key not in _SAMPLES:
        _SAMPLES[key] = Sample(*key)
    return _SAMPLES[key]


def colmax(F):
    """Scale of every state column; the three momentum columns share one."""
    m = np.abs(np.asarray(F, dtype=np.float64)).max(axis=0)
    m[1:4] = m[1:4].max()
    return m


def assert_close(tag, got, want, bound=PROP):
    rel = (np.abs(got - want).max(axis=0) / colmax(want)).max()
    assert observe("atmos law fluxes host: %s, eps" % tag, rel / EPS) * EPS <= bound, tag


def star(law, nf, n, M, P):
    return oracle_mod().atmos_nf_pointwise(law, nf, n, M["Q"], M["aux"], P["Q"], P["aux"])


def oracle_mod():
    from oracle import oracle as O
    O.build()
    return O


@pytest.mark.parametrize("oriented,subtract", CONFIGS, ids=IDS)
def test_census_of_the_sample(oriented, subtract):
    """Every branch the three fluxes have is in the sample, in double and in longdouble alike."""
    s = sample(oriented, subtract)
    info = s.f64[R.HLLC][1]
    hllc = np.bincount(info["hllc"], minlength=4) / K
    assert hllc.min() >= 0.02, hllc
    up = info["lmars_up"].mean()
    assert 0.25 <= up <= 0.75, up
    for p in ROE_PATTERNS:
        assert (info["roe_signs"] == np.array(p)).all(axis=1).any(), p
    assert info["tie"].min() >= 1e-6, info["tie"].min()
    ld = s.fld[R.HLLC][1]
    for key in ("hllc", "lmars_up", "roe_signs"):
        assert np.array_equal(info[key], ld[key]), key


@pytest.mark.parametrize("name", list(FLUXES))
@pytest.mark.parametrize("oriented,subtract", CONFIGS, ids=IDS)
def test_oracle_against_the_longdouble_restatement(oracle, oriented, subtract, name):
    """Per state column: ``d64`` is the largest difference between the restatement in double and
    in longdouble over the sample, the reference's own rounding envelope; the oracle, a second
    code that orders the same operations differently, stays within ``FACTOR`` of it (or of one
    eps of the column, whichever is larger)."""
    s, nf = sample(oriented, subtract), FLUXES[name]
    got = oracle.atmos_nf_pointwise(s.law, nf, *s.args)
    assert np.isfinite(got).all()
    f64, fld = s.f64[nf][0], s.fld[nf][0]
    for col in range(5):
        d64 = float(np.abs(f64[:, col] - fld[:, col]).max())
        err = float(np.abs(got[:, col] - fld[:, col]).max())
        env = max(d64, EPS * float(np.abs(fld[:, col]).max()))
        ratio = observe("atmos law fluxes host: %s %s oracle / envelope" %
                        (name, IDS[CONFIGS.index((oriented, subtract))]), err / env)
        assert ratio <= FACTOR, (col, err, d64)


@pytest.mark.parametrize("name", list(FLUXES))
@pytest.mark.parametrize("oriented,subtract", CONFIGS, ids=IDS)
def test_consistency(oracle, oriented, subtract, name):
    """``F*(q, q, n) = F(q) . n``."""
    s = sample(oriented, subtract)
    got = star(s.law, FLUXES[name], s.n, s.M, s.M)
    assert_close("consistency " + name, got, R.physical_normal_flux(s.sw, s.n, s.M["Q"], s.M["aux"]))


@pytest.mark.parametrize("name", ["Roe", "HLLC"])
@pytest.mark.parametrize("oriented,subtract", CONFIGS, ids=IDS)
def test_conservation_with_equal_auxiliary_state(oracle, oriented, subtract, name):
    """``F*(q-, q+, n) = -F*(q+, q-, -n)`` for Roe and HLLC when both sides carry the same
    auxiliary state.  LMARS is deliberately not here: the reference divides the pressure jump by
    ``c-`` and multiplies the velocity jump by ``c-``, the minus side's sound speed alone
    (AtmosModel.jl:1567-1568), so swapping the sides changes the flux, and the oracle follows it."""
    s = sample(oriented, subtract)
    P = dict(rebuild(s.law, s.P, Phi=s.M["Phi"]), aux=s.M["aux"])
    fwd = star(s.law, FLUXES[name], s.n, s.M, P)
    bwd = star(s.law, FLUXES[name], -s.n, P, s.M)
    assert_close("conservation " + name, fwd, -bwd)


def test_lmars_is_not_conservative_by_construction(oracle):
    """The statement above, checked: with ``c-`` replaced by ``c+`` through swapping the sides
    the LMARS flux moves by far more than rounding."""
    s = sample(False, False)
    fwd = star(s.law, R.LMARS, s.n, s.M, s.P)
    bwd = star(s.law, R.LMARS, -s.n, s.P, s.M)
    assert (np.abs(fwd + bwd).max(axis=0) / colmax(fwd)).max() > 1e-6


def _contact(s, rng, mach_n):
    """Pairs with equal ``p`` and equal ``u . n = mach_n c-`` (sign included), different ``rho``
    and different tangential velocity, the auxiliary state of the minus side on both."""
    law, n, M = s.law, s.n, s.M
    rhoP = M["rho"] * (1 + 0.1 * rng.uniform(-1, 1, K))
    TP = M["T"] * M["rho"] / rhoP                                    # p = rho R_d T
    un = mach_n * soundspeed(law.ps, M["T"])

    def with_un(u):
        return u - ((u * n).sum(axis=1) - un)[:, None] * n

    uM = with_un(M["u"])
    uP = with_un(0.3 * soundspeed(law.ps, TP)[:, None] * rng.standard_normal((K, 3)))
    Mc = rebuild(law, M, u=uM)
    Pc = dict(rebuild(law, M, rho=rhoP, T=TP, u=uP), aux=M["aux"])
    return Mc, Pc, un


@pytest.mark.parametrize("name", ["HLLC", "LMARS"])
@pytest.mark.parametrize("oriented,subtract", CONFIGS, ids=IDS)
def test_isolated_contact_gives_the_upwind_flux(oracle, oriented, subtract, name):
    """Equal ``p`` and equal ``u . n``, different ``rho`` and tangential ``u``: HLLC resolves the
    contact exactly (``S0 = u . n``, ``p0 = p``) and LMARS reduces to ``u_half = u . n``,
    ``p_half = p``; both return the physical flux of the upwind side."""
    s = sample(oriented, subtract)
    rng = np.random.default_rng(5)
    mach_n = rng.uniform(0.05, 0.8, K) * np.where(rng.random(K) < 0.5, -1.0, 1.0)
    Mc, Pc, un = _contact(s, rng, mach_n)
    got = star(s.law, FLUXES[name], s.n, Mc, Pc)
    FM = R.physical_normal_flux(s.sw, s.n, Mc["Q"], Mc["aux"])
    FP = R.physical_normal_flux(s.sw, s.n, Pc["Q"], Pc["aux"])
    assert (un > 0).any() and (un < 0).any()
    assert_close("isolated contact " + name, got, np.where((un > 0)[:, None], FM, FP))


@pytest.mark.parametrize("oriented,subtract", CONFIGS, ids=IDS)
def test_hllc_supersonic_pairs_take_one_side(oracle, oriented, subtract):
    """``S- >= 0`` returns ``F(q-) . n``, ``S+ < 0`` returns ``F(q+) . n``."""
    s = sample(oriented, subtract)
    law, n = s.law, s.n
    for sign, pick in ((1.0, "M"), (-1.0, "P")):
        def fast(d):
            un = sign * 1.5 * soundspeed(law.ps, d["T"])
            return rebuild(law, d, u=d["u"] - ((d["u"] * n).sum(axis=1) - un)[:, None] * n)
        M, P = fast(s.M), fast(s.P)
        info = R.numerical_flux(R.HLLC, s.sw, n, M["Q"], M["aux"], P["Q"], P["aux"])[1]
        assert (info["hllc"] == (0 if sign > 0 else 3)).all()
        want = R.physical_normal_flux(s.sw, n, *((M["Q"], M["aux"]) if pick == "M" else (P["Q"], P["aux"])))
        assert_close("HLLC supersonic " + pick, star(law, R.HLLC, n, M, P), want)


@pytest.mark.parametrize("name", list(FLUXES))
@pytest.mark.parametrize("oriented,subtract", CONFIGS, ids=IDS)
def test_rotation(oracle, oriented, subtract, name):
    """Rotating ``u-``, ``u+`` and ``n`` by an orthogonal matrix rotates the momentum flux and
    leaves the mass and the energy flux alone."""
    s = sample(oriented, subtract)
    Rm = np.linalg.qr(np.random.default_rng(11).standard_normal((3, 3)))[0]
    assert abs(Rm[0, 1]) > 1e-3 and abs(Rm[1, 2]) > 1e-3          # no axis is kept
    rot = lambda v: v @ Rm.T
    M2, P2 = rebuild(s.law, s.M, u=rot(s.M["u"])), rebuild(s.law, s.P, u=rot(s.P["u"]))
    n2 = rot(s.n)
    i1 = s.f64[FLUXES[name]][1]
    i2 = R.numerical_flux(FLUXES[name], s.sw, n2, M2["Q"], M2["aux"], P2["Q"], P2["aux"])[1]
    assert np.array_equal(i1["hllc"], i2["hllc"]) and np.array_equal(i1["lmars_up"], i2["lmars_up"])
    F1 = star(s.law, FLUXES[name], s.n, s.M, s.P)
    F2 = star(s.law, FLUXES[name], n2, M2, P2)
    want = F1.copy()
    want[:, 1:4] = rot(F1[:, 1:4])
    assert_close("rotation " + name, F2, want)


@pytest.mark.parametrize("name", list(FLUXES))
def test_subtract_off_moves_the_momentum_flux_by_the_reference_pressure(oracle, name):
    """With the same reference pressure on both sides (so that ``u . n``, ``u_half`` and the branch
    do not move) ``subtract_off`` changes the HLLC and the LMARS momentum flux by ``-p_ref n`` and
    nothing else.  For Roe the two sides may differ: the dissipation does not depend on
    ``subtract_off``, the central part moves by ``-(p_ref- + p_ref+) / 2 n``."""
    on, off = sample(True, True), make_law(True, False)
    o = on.law.off_ref + 1
    M, P = on.M, on.P
    if name != "Roe":
        P = dict(P, aux=P["aux"].copy())
        P["aux"][:, o] = M["aux"][:, o]
    F_on = star(on.law, FLUXES[name], on.n, M, P)
    F_off = star(off, FLUXES[name], on.n, M, P)
    want = F_off.copy()
    want[:, 1:4] -= ((M["aux"][:, o] + P["aux"][:, o]) / 2)[:, None] * on.n
    assert_close("subtract_off " + name, F_on, want)
    assert (np.abs(F_on - F_off).max(axis=0)[1:4] > 1e3).all()       # p_ref is some 8e4 Pa
