"""The dry atmosphere's parameter block carries quotients of its own members that the kernels used
to form per thread (csrc/physics_atmos.h, AtmosParams).  ``make_params`` must give them the bits of
the expressions the device code had: each is compared with ``==`` against that expression in numpy
float64 (an IEEE double division or product rounds the same way on the host and on the device).
No GPU: ``cmdg_atmos_host_constants`` runs ``make_params`` on the host.
"""
import ctypes as C

import numpy as np
import pytest

NAMES = ("k_a", "k_f", "k_s", "kappa", "gamma", "gamma_R", "R_ratio")


def _host_constants(cm, ip, dp):
    L = cm._lib.lib()
    ipa = (C.c_int32 * 16)(*[int(v) for v in ip])
    dpa = (C.c_double * 64)(*[float(v) for v in dp])
    out = (C.c_double * 7)()
    assert L.cmdg_atmos_host_constants(C.cast(ipa, C.c_void_p), C.cast(dpa, C.c_void_p),
                                       C.cast(out, C.c_void_p)) == 0
    return dict(zip(NAMES, (np.float64(v) for v in out)))


def _expected(dp):
    """The expressions of hs_coeffs, soundspeed and theta_v as they stood in the device code."""
    f = np.float64
    R_d, cp_d, cv_d, day = f(dp[2]), f(dp[3]), f(dp[4]), f(dp[9])
    gamma = cp_d / cv_d
    return {"k_a": f(1) / (f(40) * day), "k_f": f(1) / day, "k_s": f(1) / (f(4) * day),
            "kappa": R_d / cp_d, "gamma": gamma, "gamma_R": gamma * R_d, "R_ratio": R_d / R_d}


def _laws(cm):
    import argparse
    import bench
    from helpers import rising_bubble_setup
    args = argparse.Namespace(nhorz=None, nvert=8, scaling="weak", connectivity="full")
    hs = bench.build_workload(cm, "heldsuarez", 0, 1, 4, args, nhorz=2, nvert=2)[0]
    return {"heldsuarez": hs, "risingbubble": rising_bubble_setup(nx=2, ny=2, nz=2)[0]}


@pytest.mark.parametrize("name", ["heldsuarez", "risingbubble"])
def test_constants_of_the_shipped_laws(cm, name):
    ip, dp = _laws(cm)[name].descriptor()
    dp = np.concatenate([np.asarray(dp, dtype=np.float64), np.zeros(64)])[:64]
    got, want = _host_constants(cm, ip, dp), _expected(dp)
    for k in NAMES:
        assert got[k] == want[k], (k, got[k].hex(), want[k].hex())


def test_constants_whose_quotients_round(cm):
    """Parameters for which every quotient is inexact (a host compiler that folded, reassociated
    or multiplied by a reciprocal would show): random positive values, fixed seed."""
    rng = np.random.default_rng(20261018)
    ip = np.zeros(16, dtype=np.int32)
    for _ in range(64):
        dp = np.zeros(64)
        dp[:14] = rng.uniform(0.1, 1e5, 14)
        got, want = _host_constants(cm, ip, dp), _expected(dp)
        for k in NAMES:
            assert got[k] == want[k], (k, got[k].hex(), want[k].hex())
    assert _host_constants(cm, ip, dp)["R_ratio"] == 1.0


def test_null_arguments_are_refused(cm):
    L = cm._lib.lib()
    assert L.cmdg_atmos_host_constants(None, None, None) != 0
