"""Cost of one AtmosGCMDefault collection (climatemachine.jl_amd/diagnostics.py; csrc/kernels.h k_gcm_nodal,
csrc/interpolation.hip k_gcm_finish) on the Held-Suarez benchmark grid (6 x nhorz x nhorz x nvert elements,
N = 4, as bench.py builds it) with the reference's output resolution (experiments/AtmosGCM/heldsuarez.jl:
1 x 1 degree x 1000 m), against two yardsticks of the same run: one right-hand-side evaluation of the
model, and the device-to-host copy of Q and the auxiliary state into pinned memory -- what the reference
moves before its host loops start, so its cost floor.  Prints one JSON line, writes it to --out and the
medians into the line of --design that carries the marker ``<!-- measure_gcm_diagnostics -->``:

  ms.collect, ms.rhs, ms.copy:  median (and minimum) over --runs runs after --warmup, HIP events on the
                                default stream around one call that returns when its work is done:
                                collect(Q, t, copy=False) (the copy of the finished grid into the group's
                                pinned buffer included), dg(tendency, Q, t) + synchronize, and the two
                                copies
  ms.collect_private:           collect(Q, t) as a caller gets it by default, with private host arrays
  ratio_rhs, ratio_copy:        ms.collect.median over the other two medians

No test depends on the figures and no threshold is set on them.

Usage: python scripts/measure_gcm_diagnostics.py [--out profiles/gcm_diagnostics_heldsuarez_measure.json --design DESIGN.md]"""
import argparse
import json
import re
import sys
import time

sys.path.insert(0, ".")
sys.path.insert(0, "tests")

MARK = "<!-- measure_gcm_diagnostics -->"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nhorz", type=int, default=30)
    ap.add_argument("--nvert", type=int, default=8)
    ap.add_argument("--res", type=float, default=1.0, help="output resolution in degrees")
    ap.add_argument("--dz", type=float, default=1000.0, help="output level spacing in metres")
    ap.add_argument("--runs", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--design", default=None)
    args = ap.parse_args()
    assert args.runs >= 20, "report the median of at least 20 runs"
    import numpy as np
    import torch
    from cmdg_loader import cm
    from helpers import held_suarez_setup
    assert torch.cuda.is_available(), "the measurement needs the GPU"
    t0 = time.time()
    law, grid, direction, diffusion_direction = held_suarez_setup(n_horz=args.nhorz, n_vert=args.nvert, N=4)
    a, H = law.ps.planet_radius, 30e3
    lat = -90.0 + args.res * np.arange(int(round(180.0 / args.res)) + 1)
    lon = -180.0 + args.res * np.arange(int(round(360.0 / args.res)) + 1)
    rad = a + args.dz * np.arange(int(round(H / args.dz)) + 1)
    interpol = cm.mesh.interpolation.InterpolationCubedSphere(grid, np.linspace(a, a + H, args.nvert + 1), args.nhorz,
                                                             lat, lon, rad)
    dg = cm.dgmodel.DGModel(law, grid, direction=direction, diffusion_direction=diffusion_direction)
    Q = dg.init_ode_state(0.0)
    T = dg.create_state()
    diag = cm.diagnostics.AtmosGCMDefault(dg, interpol).init()
    setup_s = time.time() - t0
    dg(T, Q, 0.0)
    dg.synchronize()
    arrays = [Q, dg.state_auxiliary]
    pinned = [torch.empty(a_.shape, dtype=a_.dtype, pin_memory=True) for a_ in arrays]
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
    ms = {"collect": [], "rhs": [], "copy": [], "collect_private": []}
    for i in range(args.warmup + args.runs):
        torch.cuda.synchronize()
        ev[0].record()
        out = diag.collect(Q, 0.0, copy=False)
        ev[1].record()
        dg(T, Q, 0.0)
        dg.synchronize()
        ev[2].record()
        for a_, p in zip(arrays, pinned):
            p.copy_(a_, non_blocking=True)
        ev[3].record()
        diag.collect(Q, 0.0)
        ev[4].record()
        torch.cuda.synchronize()
        if i >= args.warmup:
            for k, (b, c) in (("collect", (0, 1)), ("rhs", (1, 2)), ("copy", (2, 3)), ("collect_private", (3, 4))):
                ms[k].append(ev[b].elapsed_time(ev[c]))
    assert np.isfinite(out["vort2"]).all() and (out["rho"] > 0).all()
    res = {"workload": "Held-Suarez dry GCM, stacked cubed sphere 6x%dx%dx%d elements, N=4, output %g x %g degree x "
                       "%g m" % (args.nhorz, args.nhorz, args.nvert, args.res, args.res, args.dz),
           "elements": int(grid.nelem), "output_points": int(interpol.Npl), "runs": args.runs,
           "grid_bytes": int(13 * interpol.Npl * 8), "copy_bytes": int(sum(a_.numel() * 8 for a_ in arrays)),
           "setup_seconds": setup_s,
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
        new = ("%s Measured (scripts/measure_gcm_diagnostics.py, %s, median of %d): one collection %.3f ms, one "
               "right-hand-side evaluation %.3f ms (ratio %.2f), device-to-host copy of Q and aux %.3f ms (ratio %.2f); "
               "a collection with private host arrays %.3f ms."
               % (MARK, res["workload"], args.runs, res["ms"]["collect"]["median"], res["ms"]["rhs"]["median"],
                  res["ratio_rhs"], res["ms"]["copy"]["median"], res["ratio_copy"],
                  res["ms"]["collect_private"]["median"]))
        assert MARK in txt, "no %s line in %s" % (MARK, args.design)
        with open(args.design, "w") as f:
            f.write(re.sub(re.escape(MARK) + r"[^\n]*", lambda m: new, txt, count=1))
    diag.close()
    dg.close()


if __name__ == "__main__":
    main()
