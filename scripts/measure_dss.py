"""Cost of the direct-stiffness-summation kernel (cmdg_dss_apply, csrc/dss.hip) on the benchmark
sphere (6 x 30 x 30 x 8 = 43 200 elements, N = 4, 5 states: the Held-Suarez grid as bench.py builds
it) against a device-to-device copy of the same array in the same run, which is the yardstick: the
summation reads and writes 98 of every 125 nodes, so it cannot be much cheaper than moving the array
once.  Prints one JSON line, writes it to --out and the two medians and their ratio into the line of
--design that carries the marker ``<!-- measure_dss -->``:

  ms.dss, ms.copy:  median (and minimum) over --runs runs after --warmup, HIP events on the default
                    stream around one cmdg_dss_apply(NULL, ...) and around one copy of the array;
                    the two alternate in one loop (the copy also restores the array, so the sums do
                    not grow from run to run)
  ratio:            ms.dss.median / ms.copy.median
  bytes:            needed = nodes touched x states x 8 B read and written, index = members x 8 B,
                    array = the whole array once; copy_TBs = 2 x array / ms.copy

Usage: python scripts/measure_dss.py [--out profiles/dss_heldsuarez_n30_measure.json --design DESIGN.md]"""
import argparse
import json
import re
import sys
import time

sys.path.insert(0, ".")
sys.path.insert(0, "tests")

MARK = "<!-- measure_dss -->"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-horz", type=int, default=30)
    ap.add_argument("--n-vert", type=int, default=8)
    ap.add_argument("--N", type=int, default=4)
    ap.add_argument("--nstate", type=int, default=5)
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
    M = cm.mesh
    a, H = cm.atmos.PlanetParameters().planet_radius, 30e3
    t0 = time.perf_counter()
    topl = M.StackedCubedSphereTopology(args.n_horz, np.linspace(a, a + H, args.n_vert + 1), boundary=(1, 2))
    grid = M.DiscontinuousSpectralElementGrid(topl, args.N, meshwarp=M.equiangular_cubed_sphere_warp)
    grid_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    obj = M.DSS(grid)
    tables_s = time.perf_counter() - t0
    ns = args.nstate
    src = torch.ones((grid.nelem, ns, grid.Np), dtype=torch.float64, device="cuda")
    Q = torch.empty_like(src)
    t0 = time.perf_counter()
    it = obj.device_object(Q.device)
    create_s = time.perf_counter() - t0
    groups, members, most, touched = obj.info(Q.device)
    L, check = cm._lib.lib(), cm._lib.check
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    ms = {"copy": [], "dss": []}
    for i in range(args.warmup + args.runs):
        torch.cuda.synchronize()
        ev[0].record()
        Q.copy_(src)
        ev[1].record()
        check(L.cmdg_dss_apply(None, it, Q.data_ptr(), ns))      # default stream; returns when done
        ev[2].record()
        torch.cuda.synchronize()
        if i >= args.warmup:
            ms["copy"].append(ev[0].elapsed_time(ev[1]))
            ms["dss"].append(ev[1].elapsed_time(ev[2]))
    got = Q[:, 0, :].cpu().numpy()
    assert got.max() == most and got.min() == 1.0                # dss(1): element counts
    array_b = grid.nelem * ns * grid.Np * 8
    res = {"workload": "Held-Suarez sphere 6x%dx%dx%d, N=%d, %d states" % (args.n_horz, args.n_horz, args.n_vert,
                                                                          args.N, ns),
           "elements": int(grid.nelem), "groups": groups, "members": members, "most_members": most,
           "nodes_touched_of_125": 125.0 * touched / (grid.nelem * grid.Np),
           "host_s": {"grid": grid_s, "tables": tables_s, "create": create_s}, "runs": args.runs,
           "ms": {k: {"median": float(np.median(v)), "min": float(np.min(v))} for k, v in ms.items()},
           "bytes": {"needed": 2 * touched * ns * 8, "index": members * 8, "array": array_b}}
    res["ratio"] = res["ms"]["dss"]["median"] / res["ms"]["copy"]["median"]
    res["copy_TBs"] = 2 * array_b / res["ms"]["copy"]["median"] / 1e9
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if args.design:
        with open(args.design) as f:
            txt = f.read()
        new = ("%s Measured (scripts/measure_dss.py, %s, median of %d): summation %.3f ms, device-to-device copy of "
               "the array %.3f ms, ratio %.2f." % (MARK, res["workload"], args.runs, res["ms"]["dss"]["median"],
                                                   res["ms"]["copy"]["median"], res["ratio"]))
        assert MARK in txt, "no %s line in %s" % (MARK, args.design)
        with open(args.design, "w") as f:
            f.write(re.sub(re.escape(MARK) + r"[^\n]*", lambda m: new, txt, count=1))
    obj.close()


if __name__ == "__main__":
    main()
