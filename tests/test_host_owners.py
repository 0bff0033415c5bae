"""The order dispatch (csrc/with_constant.h) and the owner types (csrc/owned.h) on the host: the
stand-alone program tests/host/host_owners.cpp, built for the CPU against a stub of the HIP calls
the owners make and run under AddressSanitizer and UndefinedBehaviorSanitizer as a process of its
own (nothing of it is loaded into Python)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dispatch_and_owners_under_sanitizers(tmp_path):
    host = os.path.join(ROOT, "tests", "host")
    exe = str(tmp_path / "host_owners")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-g",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           # (linked in: the program starts the same whatever the environment preloads)
                           "-static-libasan", "-static-libubsan",
                           "-I" + os.path.join(host, "stub"),
                           "-I" + os.path.join(ROOT, "climatemachine.jl_amd", "csrc"),
                           os.path.join(host, "host_owners.cpp"), "-o", exe])
    # the stub counts what is still allocated itself; the leak checker needs ptrace, which a
    # container may withhold
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "host owners: ok" in r.stdout, r.stdout
