#!/usr/bin/env python3
"""scripts/make_golden_lsrk_bits.py OUTDIR: records the fixtures of
tests/test_gpu_lsrk_bits_vs_parent.py with the library of this tree (needs the GPU): per case, Q, dQ
and the two refreshed auxiliary columns after 3 LSRK54 steps through cmdg_lsrk_run, as float64
OUTDIR/lsrk_bits_<case>.npz.  Every case runs with the gradient-argument hand-off on and off; the
two must agree bit for bit (they do since the hand-off exists), and one array set is written."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from cmdg_loader import cm  # noqa: E402
import test_gpu_lsrk_bits_vs_parent as T  # noqa: E402


def main(outdir):
    os.makedirs(outdir, exist_ok=True)
    for case in T.CASES:
        on, used_on = T.run_case(cm, torch, case, 1)
        off, used_off = T.run_case(cm, torch, case, 0)
        assert used_off == 0
        for k in on:
            assert np.array_equal(on[k].view(np.int64), off[k].view(np.int64)), (case, k)
        path = os.path.join(outdir, "lsrk_bits_%s.npz" % case)
        np.savez(path, **on)
        print("%s: hand-off used %d / %d, %s, %d bytes" % (
            case, used_on, used_off, {k: v.shape for k, v in on.items()}, os.path.getsize(path)))


if __name__ == "__main__":
    main(sys.argv[1])
