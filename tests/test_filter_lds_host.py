"""The LDS budget of the element-filter kernels (csrc/filter_lds.h: static plus dynamic LDS per
kernel family, order and number of filtered states, and the chunk ``filter_apply`` launches with) on
the host: the stand-alone program tests/host/host_filter_lds.cpp, built for the CPU and run under
AddressSanitizer and UndefinedBehaviorSanitizer as a process of its own (nothing of it is loaded into
Python).  It checks the table at NQ = 2 .. 8 and that the rule which counted the dynamic buffers only
went over 64 KiB exactly once: mass preserving, N = 7, 7 states, 70 144 B."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_filter_lds_table_under_sanitizers(tmp_path):
    host = os.path.join(ROOT, "tests", "host")
    exe = str(tmp_path / "host_filter_lds")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-g",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           # (linked in: the program starts the same whatever the environment preloads)
                           "-static-libasan", "-static-libubsan",
                           "-I" + os.path.join(ROOT, "climatemachine.jl_amd", "csrc"),
                           os.path.join(host, "host_filter_lds.cpp"), "-o", exe])
    # the leak checker needs ptrace, which a container may withhold
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0 and "host filter lds: ok" in r.stdout, r.stdout
    rows = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("mass-preserving")]
    assert len(rows) == 7
    n7 = [w for w in rows if w[1] == "8"][0]
    assert (n7[3], n7[6], n7[8], n7[9]) == ("6", "61952", "7", "70144")
