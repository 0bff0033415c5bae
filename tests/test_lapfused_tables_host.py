"""The host half of the fused Laplacian pass (csrc/lapfused_tables.h: for every lateral face node,
the neighbour's face task of the same mesh node and its other lateral face task there; which grids
are eligible) on the host: the stand-alone program tests/host/host_lapfused.cpp, built for the CPU
and run under AddressSanitizer and UndefinedBehaviorSanitizer as a process of its own (nothing of
it is loaded into Python).  It builds the tables for a 2 x 2 periodic patch, a hand-written
three-panel corner and a 3 x 3 periodic patch, checks the defining identities of tP / tE at every
face node, and offers the grids that must be reported ineligible."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tables_and_eligibility_under_sanitizers(tmp_path):
    host = os.path.join(ROOT, "tests", "host")
    exe = str(tmp_path / "host_lapfused")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-g",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           # (linked in: the program starts the same whatever the environment preloads)
                           "-static-libasan", "-static-libubsan",
                           "-I" + os.path.join(ROOT, "climatemachine.jl_amd", "csrc"),
                           os.path.join(host, "host_lapfused.cpp"), "-o", exe])
    # the leak checker needs ptrace, which a container may withhold
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "host lapfused: ok" in r.stdout, r.stdout
