"""Host side of the moist IMEX path: AtmosAcousticGravityLinearModel of a MoistAtmosModel, the band
sizes of its column solver, and the registers of the compiled band solves (no GPU needed)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def moist_law(cm, **kw):
    MO, A = cm.moist, cm.atmos
    ps = MO.MoistParameters()
    ref = A.DecayingTemperatureProfile(ps, 290.0, 220.0, ps.R_d * 290.0 / ps.grav)
    return MO.MoistAtmosModel(None, ref, closure=MO.CLOSURE_CONSTANT, param_set=ps, **kw)


def test_moist_linear_mirror(cm):
    law = moist_law(cm)
    lin = cm.atmos.AtmosAcousticGravityLinearModel(law)
    assert lin.ns == 6 and lin.naux == 19
    assert lin.physics_id == 11 == cm.balancelaws.PHYSICS_MOIST_LINEAR_AG
    assert (lin.ngrad, lin.ngradflux, lin.ngradlap, lin.nhyper) == (0, 0, 0, 0)
    ip, dp = lin.descriptor()
    ipm, dpm = law.descriptor()
    assert np.array_equal(ip, ipm) and np.array_equal(dp, dpm)
    assert ip[4] == 0
    assert lin.state_names() == law.state_names()
    # the dry mirror keeps its id and five states
    dry = cm.atmos.AtmosAcousticGravityLinearModel(law._dry)
    assert (dry.ns, dry.physics_id) == (5, 10)


def test_moist_linear_mirror_refuses_no_orientation(cm):
    law = moist_law(cm, no_orientation=True)
    assert law.descriptor()[0][4] == 1
    with pytest.raises(ValueError, match="no_orientation"):
        cm.atmos.AtmosAcousticGravityLinearModel(law)


def test_six_state_band_sizes(cm):
    S = cm.systemsolvers
    assert S.lower_bandwidth(4, 6, 1) == 29
    assert S.lower_bandwidth(6, 6, 1) == 41
    # bench.py --workload bomex on one GPU: 16 x 16 x 32 elements at N = 6, stacks of 32
    N, ne, nz = 6, 16, 32
    p = S.lower_bandwidth(N, 6, 1)
    ncol = ne * ne * (N + 1) ** 2
    n = 6 * (N + 1) * nz
    b = S.band_bytes(ncol, n, p, p)
    assert b == 8192 * 343 * 6 * 83 * 8
    assert round(b / 1e9, 1) == 11.2


def _kernel_resources(obj):
    script = os.path.join(ROOT, "scripts", "kernel_resources.sh")
    out = subprocess.run(["bash", script, obj, "k_band_solve"], capture_output=True, text=True,
                         check=True).stdout
    res = {}
    for line in out.splitlines():
        m = re.match(r"\S*k_band_solveILi(\d+)ELi(\d+)E\S*\s+vgpr\s+(\d+).*scratch (\d+)", line)
        if m:
            res[(int(m.group(1)), int(m.group(2)))] = (int(m.group(3)), int(m.group(4)))
    return res


def test_band_solve_keeps_its_window_in_registers():
    """Every k_band_solve<Nq_v, nstate> of the built columnlu.o uses no scratch: the solution
    window (p + 1 doubles, 42 for N = 6 with six states) stays in registers."""
    obj = os.path.join(ROOT, "climatemachine.jl_amd", "csrc", "columnlu.o")
    if not os.path.exists(obj):
        pytest.skip("columnlu.o is not built")
    for tool in ("/opt/rocm/lib/llvm/bin/clang-offload-bundler", "/opt/rocm/lib/llvm/bin/llvm-readelf"):
        if not os.path.exists(tool):
            pytest.skip("%s is not installed" % tool)
    if shutil.which("objcopy") is None:
        pytest.skip("objcopy is not installed")
    res = _kernel_resources(obj)
    assert set(res) == {(5, 5), (6, 5), (5, 6), (7, 6)}, res
    for pair, (vgpr, scratch) in res.items():
        print("k_band_solve<%d, %d>: %d VGPRs, scratch %d" % (pair + (vgpr, scratch)))
        assert scratch == 0, (pair, scratch)
