"""Cost of one AtmosLESDefault collection (climatemachine.jl_amd/diagnostics.py, csrc/diagnostics.hip) on
the BOMEX benchmark grid (ne x ne x 2 ne elements, N = 6, as bench.py builds it) against two yardsticks
of the same run: one right-hand-side evaluation of the model, and a device-to-host copy of Q, the
auxiliary state and the gradient flux into pinned memory -- what the reference moves before its host
loops start, so its cost floor.  Prints one JSON line, writes it to --out and the medians into the
line of --design that carries the marker ``<!-- measure_les_diagnostics -->``:

  ms.collect, ms.rhs, ms.copy:  median (and minimum) over --runs runs after --warmup, HIP events on the
                                default stream around one call that returns when its work is done:
                                collect(Q, t, evaluate=False), dg(tendency, Q, t) + synchronize, and
                                the three copies
  ratio_rhs, ratio_copy:        ms.collect.median over the other two medians

No test depends on the figures.

Usage: python scripts/measure_les_diagnostics.py [--out profiles/les_diagnostics_bomex_measure.json --design DESIGN.md]"""
import argparse
import json
import re
import sys

sys.path.insert(0, ".")
sys.path.insert(0, "tests")

MARK = "<!-- measure_les_diagnostics -->"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ne", type=int, default=16)
    ap.add_argument("--N", type=int, default=6)
    ap.add_argument("--runs", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--design", default=None)
    args = ap.parse_args()
    assert args.runs >= 20, "report the median of at least 20 runs"
    import numpy as np
    import torch
    from cmdg_loader import cm
    assert torch.cuda.is_available(), "the measurement needs the GPU"
    M, ne = cm.mesh, args.ne
    rng = [np.linspace(0.0, 200.0 * ne, ne + 1), np.linspace(0.0, 200.0 * ne, ne + 1),
           np.linspace(0.0, 3000.0, 2 * ne + 1)]
    topl = M.StackedBrickTopology(rng, periodicity=(True, True, False), boundary=((0, 0), (0, 0), (1, 2)))
    grid = M.DiscontinuousSpectralElementGrid(topl, args.N)
    law = cm.moist.bomex_model(3000.0)
    dg = cm.dgmodel.DGModel(law, grid)
    Q = dg.init_ode_state(0.0)
    T = dg.create_state()
    diag = cm.diagnostics.AtmosLESDefault(dg).init()
    dg(T, Q, 0.0)
    dg.synchronize()
    arrays = [Q, dg.state_auxiliary, dg.state_gradient_flux]
    pinned = [torch.empty(a.shape, dtype=a.dtype, pin_memory=True) for a in arrays]
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    ms = {"collect": [], "rhs": [], "copy": []}
    for i in range(args.warmup + args.runs):
        torch.cuda.synchronize()
        ev[0].record()
        prof = diag.collect(Q, 0.0, evaluate=False)
        ev[1].record()
        dg(T, Q, 0.0)
        dg.synchronize()
        ev[2].record()
        for a, p in zip(arrays, pinned):
            p.copy_(a, non_blocking=True)
        ev[3].record()
        torch.cuda.synchronize()
        if i >= args.warmup:
            for k, (a, b) in (("collect", (0, 1)), ("rhs", (1, 2)), ("copy", (2, 3))):
                ms[k].append(ev[a].elapsed_time(ev[b]))
    assert np.isfinite(prof["avg_rho"]).all()
    res = {"workload": "BOMEX moist LES, stacked brick %dx%dx%d elements, N=%d" % (ne, ne, 2 * ne, args.N),
           "elements": int(grid.nelem), "levels": int(diag.nlevels), "runs": args.runs,
           "copy_bytes": int(sum(a.numel() * 8 for a in arrays)),
           "ms": {k: {"median": float(np.median(v)), "min": float(np.min(v))} for k, v in ms.items()}}
    res["ratio_rhs"] = res["ms"]["collect"]["median"] / res["ms"]["rhs"]["median"]
    res["ratio_copy"] = res["ms"]["collect"]["median"] / res["ms"]["copy"]["median"]
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if args.design:
        with open(args.design) as f:
            txt = f.read()
        new = ("%s Measured (scripts/measure_les_diagnostics.py, %s, median of %d): one collection %.3f ms, one "
               "right-hand-side evaluation %.3f ms (ratio %.2f), device-to-host copy of Q, aux and the gradient flux "
               "%.3f ms (ratio %.2f)." % (MARK, res["workload"], args.runs, res["ms"]["collect"]["median"],
                                        res["ms"]["rhs"]["median"], res["ratio_rhs"], res["ms"]["copy"]["median"],
                                        res["ratio_copy"]))
        assert MARK in txt, "no %s line in %s" % (MARK, args.design)
        with open(args.design, "w") as f:
            f.write(re.sub(re.escape(MARK) + r"[^\n]*", lambda m: new, txt, count=1))
    dg.close()


if __name__ == "__main__":
    main()
