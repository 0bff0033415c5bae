"""Time of the device reductions (cmdg_reduce, csrc/reductions.hip) on the bench-size Held-Suarez
state: 6 x 30 x 30 x 8 = 43 200 elements, N = 4, 5 states.  Prints one JSON line.

  call time:   host clock around cmdg_reduce, which ends in a device synchronise (both kernels,
               the copy of the partials and the host combine), median of --reps calls
  kernel time: from a rocprofv3 --kernel-trace --stats run of this script (--kernel-stats names
               its *_kernel_stats.csv); absent otherwise
  bytes:       what the op needs: (nstates + 1) * Np * nreal * 8 (the states and M), read once

Usage: python scripts/measure_reductions.py [--n-horz 30] [--reps 50] [--kernel-stats CSV]"""
import argparse
import csv
import json
import math
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
from cmdg_loader import cm            # noqa: E402
from helpers import held_suarez_setup  # noqa: E402

COPY_TBS = 6.29   # measured float4 copy rate of the MI355X (MI355X_MICROARCH: HBM)


def kernel_stats(path):
    """{kernel name: (calls, mean ns)} of the reduction kernels in a rocprofv3 stats file"""
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            if "k_reduce_" in name:
                out[name] = (int(row["Calls"]), float(row["AverageNs"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-horz", type=int, default=30)
    ap.add_argument("--n-vert", type=int, default=8)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--kernel-stats", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the measurement needs the GPU"
    R = cm.reductions
    law, grid, d, dd = held_suarez_setup(n_horz=args.n_horz, n_vert=args.n_vert)
    dg = cm.dgmodel.DGModel(law, grid, direction=d, diffusion_direction=dd)
    Q = dg.init_ode_state(0.0)
    ns, nodes = Q.shape[1], grid.nreal * grid.Np
    cases = {
        "weightedsum_all5": (lambda: R.weightedsum(dg, Q), ns + 1),
        "norm1_weighted_per_state": (lambda: R.norm(dg, Q, 1, True, (1, 3)), ns + 1),
        "norm2_weighted_per_state": (lambda: R.norm(dg, Q, 2, True, (1, 3)), ns + 1),
        "norm_inf": (lambda: R.norm(dg, Q, math.inf), ns),
        "maximum": (lambda: R.mapreduce(dg, "max", Q), ns),
    }
    res = {"workload": "Held-Suarez state 6x%dx%dx%d, N=4, %d elements, %d states, fp64"
           % (args.n_horz, args.n_horz, args.n_vert, grid.nreal, ns),
           "copy_rate_TBs": COPY_TBS, "ops": {}}
    for name, (fn, ncols) in cases.items():
        for _ in range(5):
            fn()                                  # warm-up: code objects, scratch
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            fn()                                  # ends in a synchronise of the compute stream
            ts.append(time.perf_counter() - t0)
        call = float(np.median(ts))
        nbytes = ncols * nodes * 8
        res["ops"][name] = {"needed_bytes": nbytes, "call_us_median": 1e6 * call,
                            "call_us_min": 1e6 * min(ts),
                            "call_TBs": nbytes / call / 1e12}
    # one Held-Suarez LSRK54 step, for the share a conservation check costs per step
    s = cm.odesolvers.LSRK54CarpenterKennedy(dg, Q, dt=0.2)
    s.dostep(Q, 2)
    dg.synchronize()
    t0 = time.perf_counter()
    s.dostep(Q, 10)
    dg.synchronize()
    step = (time.perf_counter() - t0) / 10
    res["heldsuarez_step_us"] = 1e6 * step
    res["ops"]["weightedsum_all5"]["call_share_of_step"] = \
        res["ops"]["weightedsum_all5"]["call_us_median"] / res["heldsuarez_step_us"]
    if args.kernel_stats:
        ks = kernel_stats(args.kernel_stats)
        res["kernel_stats"] = {k: {"calls": c, "mean_us": ns_ / 1e3} for k, (c, ns_) in ks.items()}
        # weightedsum_all5 is the only case here that launches the non-per-state sum kernels
        # (mangled or demangled names: template arguments <T_SUM = 0, per_state = false>)
        k1 = [v for k, v in ks.items() if "k_reduce_partialILi0ELb0E" in k or "k_reduce_partial<0, false>" in k]
        k2 = [v for k, v in ks.items() if "k_reduce_finalILi0E" in k or "k_reduce_final<0>" in k]
        if k1:
            kus = k1[0][1] / 1e3
            nb = res["ops"]["weightedsum_all5"]["needed_bytes"]
            res["weightedsum_all5_kernel"] = {
                "stage1_us": kus, "stage2_us": k2[0][1] / 1e3 if k2 else None,
                "stage1_TBs": nb / kus / 1e6, "fraction_of_copy_rate": nb / kus / 1e6 / COPY_TBS}
    dg.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
