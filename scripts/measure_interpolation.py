"""Cost of interpolate + project + scatter on the benchmark sphere (6 x 30 x 30 x 8 = 43 200
elements, N = 4, 5 states, the Held-Suarez grid and model as bench.py builds them) onto
1 x 1 degree x 31 radii.  Prints one JSON line:

  ms:                 median (and minimum) over --runs runs, after --warmup: "device" = the three
                      kernels enqueued back to back on the model handle's compute stream through
                      the C entries and ONE cmdg_synchronize at the end, host clock around them
                      (each kernel alone the same way); "sync_api" = the three calls of the
                      Python front without a handle, each of which waits for its kernel -- wall
                      time of the synchronous interface, three host round trips included
  bytes:              what must move -- interpolate: state read once, 3 xi per point and the work
                      table read, v written; project: 2 int32 per point read, 3 columns of v read
                      and written; scatter: 3 int32 per point and v read, fiv written -- and that
                      as a fraction of the measured 6.29 TB/s copy rate over the "device" time
  ratio_to_step:      "device" total against one Held-Suarez step of the same build: ms_per_step of
                      the headline line of `python bench.py`, given with --bench-json FILE (or
                      --step-ms X)
  points_per_element: minimum / median / maximum over elements that own points (the polar skew),
                      work-groups launched and their mean fill out of 128 lanes

--kernel-stats CSV (with --combine RESULT.json): add the mean times of k_interpolate, k_project
and k_scatter from a `rocprofv3 --kernel-trace --stats` run of this script.

Usage: python bench.py --gpus 1 > bench.json; python scripts/measure_interpolation.py --bench-json bench.json"""
import argparse
import json
import sys
import time

sys.path.insert(0, ".")
sys.path.insert(0, "tests")

COPY_TBS = 6.29   # measured float4 copy rate of the MI355X


def add_kernel_stats(res, path):
    import csv
    out = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r.get("Name") or r.get("KernelName") or ""
            for k in ("k_interpolate", "k_project", "k_scatter"):
                if k in name:
                    out[k] = {"calls": int(r["Calls"]), "mean_us": float(r["AverageNs"]) / 1e3}
    res["kernel_stats"] = out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-horz", type=int, default=30)
    ap.add_argument("--n-vert", type=int, default=8)
    ap.add_argument("--res", type=float, default=1.0, help="degrees")
    ap.add_argument("--nrad", type=int, default=31)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--bench-json", default=None)
    ap.add_argument("--step-ms", type=float, default=None)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--combine", default=None)
    args = ap.parse_args()
    if args.combine:
        with open(args.combine) as f:
            res = json.loads(f.read().strip().splitlines()[-1])
        add_kernel_stats(res, args.kernel_stats)
        print(json.dumps(res))
        return
    assert args.runs >= 20, "report the median of at least 20 runs"
    import ctypes as C
    import numpy as np
    import torch
    from cmdg_loader import cm
    from helpers import held_suarez_setup
    assert torch.cuda.is_available(), "the measurement needs the GPU"
    I = cm.mesh.interpolation
    law, grid, d, dd = held_suarez_setup(n_horz=args.n_horz, n_vert=args.n_vert)
    dg = cm.dgmodel.DGModel(law, grid, direction=d, diffusion_direction=dd)
    a = cm.atmos.PlanetParameters().planet_radius
    vert_range = np.linspace(a, a + 30e3, args.n_vert + 1)
    lat = -90.0 + args.res * np.arange(int(round(180.0 / args.res)) + 1)
    lon = -180.0 + args.res * np.arange(int(round(360.0 / args.res)) + 1)
    rad = vert_range[0] + ((vert_range[-1] - vert_range[0]) / (args.nrad - 1)) * np.arange(args.nrad)
    t0 = time.perf_counter()
    it = I.InterpolationCubedSphere(grid, vert_range, args.n_horz, lat, lon, rad)
    setup_s = time.perf_counter() - t0
    dev = dg.device
    Q = dg.init_ode_state(0.0)
    ns = Q.shape[1]
    v = torch.zeros((ns, it.Npl), dtype=torch.float64, device=dev)
    fiv = torch.zeros((ns,) + it.dims[::-1], dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    L, h, obj = cm._lib.lib(), dg.handle, it.device_object(dev)
    cols = (C.c_int32 * 3)(2, 3, 4)
    objs, vs = (C.c_void_p * 1)(obj.value), (C.c_void_p * 1)(v.data_ptr())
    check = cm._lib.check
    enqueue = {     # with a handle: enqueued on its compute stream, no wait
        "interpolate": lambda: check(L.cmdg_interp_apply(h, obj, Q.data_ptr(), ns, Q.shape[0], v.data_ptr()), h),
        "project": lambda: check(L.cmdg_interp_project(h, obj, v.data_ptr(), ns, cols), h),
        "scatter": lambda: check(L.cmdg_interp_scatter(h, objs, 1, vs, ns, fiv.data_ptr()), h)}
    sync_api = [lambda: I.interpolate_local(it, Q, v), lambda: I.project_cubed_sphere(it, v, (2, 3, 4)),
                lambda: I.accumulate_interpolated_data(it, v, fiv)]

    def median_ms(fs, sync):
        ms = []
        for i in range(args.warmup + args.runs):
            sync()
            t = time.perf_counter()
            for f in fs:
                f()
            sync()
            if i >= args.warmup:
                ms.append(1e3 * (time.perf_counter() - t))
        return {"median": float(np.median(ms)), "min": float(np.min(ms))}

    res = {"workload": "Held-Suarez sphere 6x%dx%dx%d, N=4, %d states -> %g x %g deg x %d radii"
           % (args.n_horz, args.n_horz, args.n_vert, ns, args.res, args.res, args.nrad),
           "elements": int(grid.nreal), "points": it.Npl, "host_setup_s": setup_s, "runs": args.runs}
    per = np.diff(it.offset)
    per = per[per > 0]
    groups = int(np.sum((per + 127) // 128))
    res["points_per_element"] = {"min": int(per.min()), "median": float(np.median(per)), "max": int(per.max()),
                                 "elements_with_points": int(len(per)), "work_groups": groups,
                                 "mean_lanes_of_128": float(it.Npl / groups)}
    res["ms"] = {"device": {k: median_ms([f], dg.synchronize) for k, f in enqueue.items()}}
    res["ms"]["device"]["total"] = median_ms(list(enqueue.values()), dg.synchronize)
    res["ms"]["sync_api_total"] = median_ms(sync_api, lambda: None)
    npnt, Np = it.Npl, grid.Np
    b = {"interpolate": grid.nreal * Np * ns * 8 + npnt * 3 * 8 + groups * 16 + npnt * ns * 8,
         "project": npnt * 2 * 4 + npnt * 3 * 8 * 2,
         "scatter": npnt * 3 * 4 + npnt * ns * 8 + int(np.prod(it.dims)) * ns * 8}
    b["total"] = sum(b.values())
    res["bytes"] = dict(b)
    res["TBs"] = {k: b[k] / res["ms"]["device"][k]["median"] / 1e9 for k in b}
    res["fraction_of_copy_rate"] = {k: x / COPY_TBS for k, x in res["TBs"].items()}
    res["copy_rate_TBs"] = COPY_TBS
    res["ms_at_copy_rate"] = b["total"] / COPY_TBS / 1e9
    step_ms = args.step_ms
    if args.bench_json:
        with open(args.bench_json) as f:
            lines = [ln for ln in f.read().strip().splitlines() if ln.startswith("{")]
        step_ms = json.loads(lines[-1])["ms_per_step"]
    if step_ms:
        res["held_suarez_step_ms"] = step_ms
        res["ratio_to_step"] = res["ms"]["device"]["total"]["median"] / step_ms
    print(json.dumps(res))
    it.close()
    dg.close()


if __name__ == "__main__":
    main()
