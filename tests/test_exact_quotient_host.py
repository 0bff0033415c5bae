"""The shared-reciprocal quotient of csrc/exact_quotient.h on the host: its three steps
(``q0 = a y``, ``r = fma(-b, q0, a)``, ``q = fma(r, y, q0)`` with ``y = RN(1 / b)``) give the bits
of ``a / b``.  The stand-alone program tests/host/host_exact_quotient.cpp is built for the CPU with
``std::fma`` and run under AddressSanitizer and UndefinedBehaviorSanitizer as a process of its own
(nothing of it is loaded into Python).  Operands: the dry law's uniform divisors, 10^6 random normal
pairs with a fixed seed, divisors with all-ones and near-power-of-two significands, numerators
within one ulp of exact multiples.  Signed zeros, infinities and NaN belong to the device test
(tests/test_gpu_exact_quotient.py): on the host ``quot`` is ``/`` itself."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_three_steps_give_the_bits_of_the_division(tmp_path):
    exe = str(tmp_path / "host_exact_quotient")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-g", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           # (linked in: the program starts the same whatever the environment preloads)
                           "-static-libasan", "-static-libubsan",
                           "-I" + os.path.join(ROOT, "climatemachine.jl_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host", "host_exact_quotient.cpp"), "-o", exe])
    # the leak checker needs ptrace, which a container may withhold
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "host exact quotient: ok" in r.stdout, r.stdout
