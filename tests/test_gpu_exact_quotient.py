"""The shared-reciprocal quotient of csrc/exact_quotient.h on the device (``-m gpu``), bit for bit.

1. ``quot(a, pair(b))`` against ``a / b``, both evaluated by one kernel (``cmdg_probe_quot``): the
   operand classes of tests/test_exact_quotient_host.py -- the dry law's uniform divisors, random
   normal pairs, divisors with all-ones and near-power-of-two significands, numerators within an ulp
   of exact multiples -- and every pairing of +-0, +-inf, NaN and ordinary values.  NaN equals NaN;
   everything else is compared as int64.
2. The dry law's pointwise functions (flux_first_order, wavespeed, source, gradient_argument of the
   Held-Suarez instantiation) through ``cmdg_probe_dry_atmos_pointwise``: one thread per point on
   the device against the same text on the host, where ``quot`` is the division.  Points: nodes of
   the 72-element sphere with the seeded perturbation, a third of them with ``rho u`` set to +0, -0
   or a mix of both.  The latitude's sine and cosine are inputs (libm differs between the two sides).
   Everything is compared as int64 except the energy source of the Held-Suarez forcing, whose
   ``pow`` and ``log`` come from two different math libraries: it is held to the bound worked out at
   ``SE_BOUND``.  What reaches the energy source from a quotient (T, sigma) reaches the fluxes and
   the momentum source too, which are compared exactly.
3. Two LSRK54 steps of ``cmdg_lsrk_run`` on the 6x2x2x3 sphere at N = 4 (72 elements) and on the
   hyperdiffusive 3x3x3 brick of test_gpu_lapfused_lines.py: the sha256 of ``tobytes()`` of Q, dQ,
   the hyperdiffusion arrays and every auxiliary column against tests/golden/exact_quotient_bits.json,
   recorded by scripts/make_golden_exact_quotient.py with the library of the commit before the
   quotient helper (tests/golden/README_exact_quotient.txt).
"""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import test_gpu_lapfused_lines as L

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "exact_quotient_bits.json")
# name -> (setup, dt); two steps of the five-stage scheme each
CASES = {"sphere_6x2x2x3_N4": (lambda cm: L._sphere(4), 2.0),
         "brick_3x3x3_hyper": (lambda cm: L._brick(cm), 0.05)}
NSTEPS = 2


def digests(cm, torch, case):
    """sha256 of everything a caller can see after the run, by array name."""
    setup, dt = CASES[case]
    out, counts = L._run(cm, torch, setup(cm), 1, dt, None, NSTEPS)
    assert counts[0] == 1  # (the hand-off update is the kernel in question)
    return {k: hashlib.sha256(v).hexdigest() for k, v in out.items()}


# ---- operands ------------------------------------------------------------------------------

def _from_fields(sign, expo, mant):
    u = (sign.astype(np.uint64) << np.uint64(63)) | ((expo + 1023).astype(np.uint64) << np.uint64(52)) | mant
    return u.view(np.float64)


def _random_normal(rng, n, lim):
    return _from_fields(rng.integers(0, 2, n), rng.integers(-lim, lim + 1, n),
                        rng.integers(0, 1 << 52, n, dtype=np.uint64))


def _hard_divisors():
    ones = (1 << 52) - 1
    out = []
    for e in range(-3, 4):
        for k in range(8):
            for m in (ones - k, k, ones >> k, (ones << (4 * k)) & ones):
                out.append(_from_fields(np.array([0]), np.array([e]), np.array([m], dtype=np.uint64))[0])
    return np.array(out)


def operands(uniform):
    """(a, b): float64 arrays of equal length, a few hundred thousand pairs."""
    rng = np.random.default_rng(20250117)
    A, B = [], []
    for b in uniform:
        A.append(_random_normal(rng, 5000, 200)), B.append(np.full(5000, b))
    A.append(_random_normal(rng, 200000, 300)), B.append(_random_normal(rng, 200000, 300))
    hard = _hard_divisors()
    A.append(_random_normal(rng, 200 * hard.size, 100)), B.append(np.repeat(hard, 200))
    A.append(np.tile(hard, hard.size)), B.append(np.repeat(hard, hard.size))
    b = np.concatenate([_random_normal(rng, 20000, 50), rng.choice(hard, 20000)])
    k = np.concatenate([rng.integers(1, 4097, 30000).astype(np.float64), _random_normal(rng, 10000, 30)])
    a = k * b
    for step in (0, 1, -1):
        A.append((a.view(np.int64) + step).view(np.float64)), B.append(b)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -3.0, 9.81, 1e5, 7.0e-3, -2.5e7])
    A.append(np.tile(special, special.size)), B.append(np.repeat(special, special.size))
    return np.concatenate(A), np.concatenate(B)


def _same_bits(x, y):
    return (x.view(np.int64) == y.view(np.int64)) | (np.isnan(x) & np.isnan(y))


def _uniform_divisors(law):
    _, dp = law.descriptor()
    return [float(dp[6]), float(dp[4]), float(dp[8]), float(dp[1])]  # grav, cv_d, MSLP, tau


def test_device_quot_has_the_bits_of_the_division(cm, torch):
    law = L._sphere(4)[0]
    a, b = operands(_uniform_divisors(law) + [3600.0, 86400.0, 0.3])
    ta, tb = L._gpu(torch, a), L._gpu(torch, b)
    q, d = torch.empty_like(ta), torch.empty_like(ta)
    lib = cm._lib.lib()
    assert lib.cmdg_probe_quot(ta.data_ptr(), tb.data_ptr(), q.data_ptr(), d.data_ptr(), a.size) == 0
    q, d = q.cpu().numpy(), d.cpu().numpy()
    with np.errstate(all="ignore"):
        host = a / b
    # the device's own division is IEEE: the host's bits (NaN payloads aside)
    ok_div = _same_bits(d, host)
    ok = _same_bits(q, d)
    print("quot vs /: %d pairs, %d differ; device / vs host /: %d differ" % (a.size, (~ok).sum(), (~ok_div).sum()))
    assert ok_div.all(), (a[~ok_div][:5], b[~ok_div][:5])
    assert ok.all(), [(x.hex(), y.hex()) for x, y in zip(a[~ok][:5], b[~ok][:5])]


# ---- pointwise law functions ---------------------------------------------------------------

def _pointwise(cm, law, where, arrays, n, xp_ptr):
    ip, dp = law.descriptor()
    ipa = (C.c_int32 * 16)(*[int(v) for v in ip])
    dpv = np.concatenate([np.asarray(dp, dtype=np.float64), np.zeros(64)])[:64]
    dpa = (C.c_double * 64)(*[float(v) for v in dpv])
    lib = cm._lib.lib()
    rc = lib.cmdg_probe_dry_atmos_pointwise(C.cast(ipa, C.c_void_p), C.cast(dpa, C.c_void_p), where,
                                            *[xp_ptr(x) for x in arrays], n)
    assert rc == 0, rc
    return dpv


def test_pointwise_law_functions_device_equals_host(cm, torch):
    law, grid, d, dd = L._sphere(4)
    dg = cm.dgmodel.DGModel(law, grid, direction=d, diffusion_direction=dd, device="cuda:0")
    aux_all = dg.state_auxiliary.cpu().numpy()
    dg.close()
    Q_all = L._perturbed(law, grid, aux_all)
    assert aux_all.shape[1:] == (17, 125) and Q_all.shape[1:] == (5, 125)
    # (element, column, node) -> one row per node
    Q_all, aux_all = (x.transpose(0, 2, 1).reshape(-1, x.shape[1]) for x in (Q_all, aux_all))
    sel = np.arange(0, Q_all.shape[0], 7)      # 1286 nodes of all three levels
    Q, aux = np.ascontiguousarray(Q_all[sel]), np.ascontiguousarray(aux_all[sel])
    n = sel.size
    i = np.arange(n)
    Q[i % 6 == 0, 1:4] = 0.0
    Q[i % 6 == 1, 1:4] = -0.0
    Q[i % 6 == 2, 1:4] = np.array([0.0, -0.0, 0.0])
    Q[i % 6 == 3, 2] = -0.0
    rng = np.random.default_rng(20250612)
    nrm = rng.standard_normal((n, 3))
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    r = np.sqrt(aux[:, 0] ** 2 + aux[:, 1] ** 2 + aux[:, 2] ** 2)
    phi = np.arcsin(aux[:, 2] / r)
    der = np.ascontiguousarray(np.stack([np.sin(phi), np.cos(phi)], axis=1))
    host = np.full((n, 33), np.nan)
    hp = lambda x: x.ctypes.data_as(C.c_void_p)
    dpv = _pointwise(cm, law, 0, [Q, aux, nrm, der, host], n, hp)
    tq, ta, tn, td = (L._gpu(torch, x) for x in (Q, aux, nrm, der))
    dev_t = torch.full((n, 33), float("nan"), dtype=torch.float64, device="cuda:0")
    _pointwise(cm, law, 1, [tq, ta, tn, td, dev_t], n, lambda x: x.data_ptr())
    dev = dev_t.cpu().numpy()
    assert np.isfinite(host).all() and np.isfinite(dev).all()
    names = ["flux %d" % k for k in range(15)] + ["wavespeed %d" % k for k in range(5)] + \
            ["source %d" % k for k in range(5)] + ["gradient_argument %d" % k for k in range(8)]
    same = host.view(np.int64) == dev.view(np.int64)
    for c, name in enumerate(names):
        print("%-22s %d of %d points differ, max |diff| %.3e" % (name, (~same[:, c]).sum(), n,
                                                                 np.abs(host[:, c] - dev[:, c]).max()))
    # the sources are live: relaxation everywhere; Coriolis in the first two momentum sources wherever
    # the momentum was left alone; Rayleigh drag, the only vertical one, below sigma_b.  (The perturbation
    # keeps rho on the reference state, so gravity cancels.)
    moving = i % 6 >= 4
    assert np.count_nonzero(host[:, 24]) == n and np.all(host[moving, 21:23] != 0)
    assert 0 < np.count_nonzero(host[moving, 23]) < moving.sum()
    # signed zeros reach the outputs: u = rho u / rho of a -0 momentum is -0, and so is u rho e + u p
    assert (np.signbit(host[i % 6 == 1, 12:15]) & (host[i % 6 == 1, 12:15] == 0)).all()
    for c, name in enumerate(names):
        if c == 24:
            continue
        assert same[:, c].all(), name
    # SE_BOUND.  source 4 = -k_T rho cv_d (T - T_equil), T_equil = max(200, (315 - 60 s^2 - 10 log(sigma) c^2)
    # sigma^kappa).  Host and device agree on every operand but log and pow, each within 1 ulp of the
    # true value on either side (glibc, the device library's documented bound): T_equil <= 315 differs
    # by at most 2 * (1 + 1) ulp plus the roundings of the products that carry the difference on, say
    # 8 ulp(315) = 8 * 2^-44; k_T <= k_s = 1 / (4 day).
    k_s = 1.0 / (4 * dpv[9])
    se_bound = 8 * 2.0 ** -44 * k_s * Q[:, 0] * dpv[4]
    diff = np.abs(host[:, 24] - dev[:, 24])
    print("source 4: max |diff| / bound = %.3f" % (diff / se_bound).max())
    assert (diff <= se_bound).all()


# ---- two steps against the recorded parent ---------------------------------------------------

@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("case", list(CASES))
def test_two_steps_keep_the_bits_of_the_parent(cm, torch, golden, case):
    got, want = digests(cm, torch, case), golden[case]
    assert got.keys() == want.keys()
    for name in want:
        assert got[name] == want[name], name
