"""The NumPy restatement of the ESDGModel (tests/esdg_restatement.py) against the reference's own
properties, with the reference's tolerances (test/Numerics/ESDGMethods/DryAtmos/run_tests.jl): the
yardstick the device kernels are held to in tests/test_gpu_esdg.py.  No GPU."""
import numpy as np
import pytest

from cmdg_loader import cm
import esdg_restatement as R
from esdg_cases import approx, case_a

E = cm.esdg
EPS = np.finfo(np.float64).eps


def _law(dtype=np.float64):
    ps = cm.atmos.PlanetParameters()
    return R.Law(ps.cp_d, ps.cv_d, ps.Omega, (), dtype)


def _random_states(rng, n):
    """``[1, 2, 2, 2, 1] .* rand(5) + [3, -1, -1, -1, 100]`` (:218-219), n of them."""
    return [np.array(sc) * rng.random(n) + off for sc, off in zip((1, 2, 2, 2, 1), (3, -1, -1, -1, 100))]


def test_entropy_variable_round_trip():
    """:216-231, for the restatement and for the package's host transforms."""
    rng = np.random.default_rng(7)
    q = _random_states(rng, 64)
    L = _law()
    back, _ = L.entropy_variables_to_state(L.state_to_entropy_variables(q))
    for s in range(5):
        assert approx(q[s], back[s]).all()
    Q = np.stack(q)[None]                                   # (1, 5, n)
    back, _ = E.entropy_variables_to_state(E.state_to_entropy_variables(Q))
    assert approx(Q, back).all()
    assert np.array_equal(E.state_to_entropy_variables(Q)[0], np.stack(L.state_to_entropy_variables(q)))
    assert np.array_equal(E.state_to_entropy(Q)[0], L.state_to_entropy(q))


def test_tadmor_shuffle():
    """:233-286: H_12 beta_1 - H_21 beta_2 = psi_1 - psi_2 with psi = rho u, rtol = sqrt(eps)."""
    rng = np.random.default_rng(8)
    L = _law()
    q1, q2 = _random_states(rng, 64), _random_states(rng, 64)
    b1, b2 = L.state_to_entropy_variables(q1), L.state_to_entropy_variables(q2)
    H12, H21 = L.flux_ec(q1, q2), L.flux_ec(q2, q1)
    for d in range(3):
        lhs = sum(H12[d][s] * b1[s] for s in range(5)) - sum(H21[d][s] * b2[s] for s in range(5))
        assert approx(lhs, q1[1 + d] - q2[1 + d]).all()


@pytest.mark.parametrize("kind", [R.EC, R.CENTRAL, R.KG])
def test_consistency(kind):
    """F(q, q) = f(q) for the three volume fluxes."""
    rng = np.random.default_rng(9)
    L = _law()
    q = _random_states(rng, 64)
    H, F = L.volume_flux(kind, q, q), L.flux_first_order(q)
    for d in range(3):
        for s in range(5):
            assert approx(H[d][s], F[d][s], atol=10 * EPS, rtol=np.sqrt(EPS)).all()


def test_logave():
    """Against (a - b) / (log a - log b) in longdouble for ratios 1 + 1e-12 .. 1e3, and a == b."""
    ld = np.longdouble
    ratios = np.concatenate([1 + np.logspace(-12, 0, 49), np.logspace(0.5, 3, 11)])
    for b in (0.37, 1.0, 42.0):
        a = ratios * b
        al, bl = a.astype(ld), ld(b)
        # log a - log b = log1p((a - b) / b): the difference of two logarithms itself loses
        # eps_longdouble / |log zeta|, 1e-7 at zeta = 1 + 1e-12, and would be no yardstick there
        exact = (al - bl) / np.log1p((al - bl) / bl)
        got = R.logave(a, np.full_like(a, b))
        # the series branch is exact to u^5 / 11 < eps^5; the log branch loses eps / |log zeta| near one
        # through zeta - 1 alone, which 2 f = 2 (zeta - 1) / (zeta + 1) shares: 8 eps covers both
        assert np.max(np.abs(got.astype(ld) - exact) / exact) <= 8 * EPS
        # both orders of the arguments agree
        assert np.max(np.abs(R.logave(np.full_like(a, b), a) - got) / got) <= 8 * EPS
        assert R.logave(np.array([b]), np.array([b]))[0] == b
    one = np.array([1.0])
    assert R.logave(one, one * (1 + 1e-9))[0] == pytest.approx(1 + 0.5e-9, rel=4 * EPS)


@pytest.fixture(scope="module")
def operators():
    """Grid A at N = 4 with the three models of check_operators (:82-197), evaluated once."""
    law, grid, aux, _ = case_a(4)
    Q = law.init_state_prognostic(grid, aux)
    out = {}
    for name, vf, sf in (("volume", R.EC, R.NONE), ("surface", R.NONE, R.EC), ("full", R.EC, R.EC)):
        op = R.ESDGRestatement(law, grid, vf, sf, state_auxiliary=aux)
        T = np.zeros_like(Q)
        op(T, Q, 0.0)
        out[name] = T
    op = R.ESDGRestatement(law, grid, state_auxiliary=aux)
    return grid, Q, op.entropy_variables(Q), out


def check_operator_identities(grid, Q, beta, T):
    """The three identities of check_operators (:107-207); shared with the device test."""
    K = grid.nreal
    Mw = grid.vgeo[:K, 9, :]
    nfp = grid.Nfp[0]
    s = grid.sgeo[:K, :, :nfp, :]
    idM = grid.vmapM[:K, :, :nfp] - 1
    e, n = idM // grid.Np, idM % grid.Np
    psi = [Q[e, 1 + d, n] for d in range(3)]
    surface = np.sum(s[..., 3] * (s[..., 0] * psi[0] + s[..., 1] * psi[1] + s[..., 2] * psi[2]), axis=(1, 2))
    volume = np.sum(beta[:K, :5, :] * Mw[:, None, :] * T["volume"][:K], axis=(1, 2))
    assert approx(surface, volume, atol=10 * EPS, rtol=np.sqrt(EPS)).all()
    surface_integral = np.sum(beta[:K, :5, :] * Mw[:, None, :] * T["surface"][:K])
    assert approx(np.sum(volume), -surface_integral)
    integral = np.sum(beta[:K, :5, :] * Mw[:, None, :] * T["full"][:K])
    assert abs(integral) <= np.sqrt(np.spacing(abs(np.sum(volume))))
    return np.sum(volume), surface_integral, integral


def test_check_operators(operators):
    grid, Q, beta, T = operators
    print("volume %.16e surface %.16e full %.3e" % check_operator_identities(grid, Q, beta, T))


def test_longdouble_runs():
    """The restatement is dtype-generic: one evaluation in longdouble agrees with float64 to 1e-12."""
    law, grid, aux, _ = case_a(3, Ne=(3, 3, 3))
    Q = law.init_state_prognostic(grid, aux)
    T = np.zeros_like(Q)
    R.ESDGRestatement(law, grid, R.KG, R.MATRIX, state_auxiliary=aux,
                      matrix=dict(Mcut=0.1, low_mach=True, kinetic_energy_preserving=True))(T, Q)
    ld = np.longdouble
    Tl = np.zeros(Q.shape, dtype=ld)
    R.ESDGRestatement(law, grid, R.KG, R.MATRIX, state_auxiliary=aux, dtype=ld,
                      matrix=dict(Mcut=0.1, low_mach=True, kinetic_energy_preserving=True))(Tl, Q.astype(ld))
    assert Tl.dtype == ld
    assert np.max(np.abs(T - Tl)) / np.max(np.abs(Tl)) <= 1e-12
