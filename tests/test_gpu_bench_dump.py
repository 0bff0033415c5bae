"""bench.py --dump-outputs on the device: the files hold the state after exactly the timed steps,
and the same arguments give the same files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL_HS = ["--nhorz", "3", "--nvert", "2", "--no-parity", "--no-cpu", "--no-secondary", "--no-events"]


def _bench(outdir, *argv):
    e = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR"):
        e.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
                        "--dump-outputs", str(outdir)] + list(argv),
                       env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_dump_is_the_state_after_the_timed_steps(tmp_path):
    a = _bench(tmp_path / "a", "--steps", "2", "--warmup", "0", *SMALL_HS)
    b = _bench(tmp_path / "b", "--steps", "1", "--warmup", "1", *SMALL_HS)
    c = _bench(tmp_path / "c", "--steps", "1", "--warmup", "0", *SMALL_HS)
    d = _bench(tmp_path / "d", "--steps", "2", "--warmup", "0", *SMALL_HS)
    assert (a["steps"], b["steps"], c["steps"]) == (2, 1, 1)
    assert sorted(os.listdir(tmp_path / "a")) == ["state.npy"]
    qa = np.load(tmp_path / "a" / "state.npy")
    assert qa.dtype == np.float64 and qa.shape == (6 * 3 * 3 * 2, 5, 125)
    assert np.isfinite(qa).all()
    # warm-up + timed steps = 2 either way; the dump is taken before the event pass
    assert np.array_equal(qa, np.load(tmp_path / "b" / "state.npy"))
    assert np.array_equal(qa, np.load(tmp_path / "d" / "state.npy"))
    assert not np.array_equal(qa, np.load(tmp_path / "c" / "state.npy"))


@pytest.mark.gpu
def test_dump_of_the_split_explicit_ocean(tmp_path):
    args = ["--workload", "ocean-split-explicit", "--ocean-nx", "5", "--ocean-nz", "8",
            "--steps", "1", "--warmup", "0", "--no-cpu", "--no-events"]
    out = _bench(tmp_path / "a", *args)
    _bench(tmp_path / "b", *args)
    assert out["steps"] == 1
    assert sorted(os.listdir(tmp_path / "a")) == ["state_2d.npy", "state_3d.npy"]
    for name in ("state_3d.npy", "state_2d.npy"):
        q = np.load(tmp_path / "a" / name)
        assert q.dtype == np.float64 and np.isfinite(q).all()
        assert np.array_equal(q, np.load(tmp_path / "b" / name))
    assert np.load(tmp_path / "a" / "state_3d.npy").shape[0] == 5 * 5 * 8


@pytest.mark.gpu
def test_full_adds_the_extras_around_the_same_timed_steps(tmp_path):
    """A plain run prints the headline alone; ``--full`` adds the parity check, the event pass and
    the CPU baseline around the same timed steps, so it dumps the plain run's state."""
    small = ["--nhorz", "3", "--nvert", "2", "--steps", "2", "--warmup", "1"]
    plain = _bench(tmp_path / "plain", *small)
    full = _bench(tmp_path / "full", "--full", "--cpu-budget", "0.1", *small)
    extras = ("parity", "kernels_ms", "roofline", "cpu_baseline")
    assert not [k for k in extras if k in plain], sorted(plain)
    assert all(k in full for k in extras), sorted(full)
    assert full["parity"]["ok"] and plain["state_finite"] and full["state_finite"]
    for k in ("metric", "unit", "higher_is_better", "dtype", "steps", "warmup", "elements_total"):
        assert plain[k] == full[k], k
    assert np.array_equal(np.load(tmp_path / "plain" / "state.npy"),
                          np.load(tmp_path / "full" / "state.npy"))
