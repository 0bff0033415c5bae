"""The host half of direct stiffness summation (csrc/dss_tables.h: check the reference's tables,
flatten them into disjoint groups, lay the groups out in waves) on the host: the stand-alone program
tests/host/host_dss.cpp, built for the CPU and run under AddressSanitizer and
UndefinedBehaviorSanitizer as a process of its own (nothing of it is loaded into Python).  It
flattens the tables of the reference's two-element test, sums with them, and offers every malformed
table cmdg_dss_create must refuse."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flatten_and_validate_under_sanitizers(tmp_path):
    host = os.path.join(ROOT, "tests", "host")
    exe = str(tmp_path / "host_dss")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-g",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           # (linked in: the program starts the same whatever the environment preloads)
                           "-static-libasan", "-static-libubsan",
                           "-I" + os.path.join(ROOT, "climatemachine.jl_amd", "csrc"),
                           os.path.join(host, "host_dss.cpp"), "-o", exe])
    # the leak checker needs ptrace, which a container may withhold
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "host dss: ok" in r.stdout, r.stdout
