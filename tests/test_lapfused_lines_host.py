"""The row condition of the fused Laplacian pass (csrc/lapfused_tables.h) on the host: the pass
lets the face lanes of one lateral face and one level hand each other the record of their plus
node, which is right only where those plus nodes are one row of one neighbour.  The stand-alone
program tests/host/host_lapfused_lines.cpp, built for the CPU and run under AddressSanitizer and
UndefinedBehaviorSanitizer as a process of its own (nothing of it is loaded into Python), checks
the condition on the 2 x 2 and 3 x 3 periodic patches and the three-panel corner with flipped
gluings, offers hand-made tables whose row straddles two levels, two neighbours or repeats an
index, which must come back ineligible with the reason, and checks the recorded second-ring index
idE = faceP[N][tE] and the edge-block slot at every task that has a tE."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_row_condition_and_edge_index_under_sanitizers(tmp_path):
    host = os.path.join(ROOT, "tests", "host")
    exe = str(tmp_path / "host_lapfused_lines")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-g",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           # (linked in: the program starts the same whatever the environment preloads)
                           "-static-libasan", "-static-libubsan",
                           "-I" + os.path.join(ROOT, "climatemachine.jl_amd", "csrc"),
                           os.path.join(host, "host_lapfused_lines.cpp"), "-o", exe])
    # the leak checker needs ptrace, which a container may withhold
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "host lapfused lines: ok" in r.stdout, r.stdout
