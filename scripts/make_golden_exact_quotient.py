"""Record tests/golden/exact_quotient_bits.json: the sha256 of everything a caller can see after the
two-step runs of tests/test_gpu_exact_quotient.py (CASES there), taken with the package and the
libcmdg.so of a checkout of the commit BEFORE the shared-reciprocal quotient (csrc/exact_quotient.h).

    python scripts/make_golden_exact_quotient.py --root <built checkout of the parent commit> [--out FILE]

The package, the helpers and test_gpu_lapfused_lines.py (whose set-ups and run the cases use) come
from --root; only the table of cases comes from this tree.  Needs an MI355X."""
import argparse
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", required=True)
    ap.add_argument("--out", default=os.path.join(HERE, "tests", "golden", "exact_quotient_bits.json"))
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    sys.path[:0] = [os.path.join(root, "tests"), root]
    import torch
    from cmdg_loader import cm
    assert os.path.abspath(cm._lib.LIB_PATH).startswith(root), cm._lib.LIB_PATH
    spec = importlib.util.spec_from_file_location("cases", os.path.join(HERE, "tests", "test_gpu_exact_quotient.py"))
    cases = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cases)
    out = {case: cases.digests(cm, torch, case) for case in cases.CASES}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s: %s" % (args.out, {k: len(v) for k, v in out.items()}))


if __name__ == "__main__":
    main()
