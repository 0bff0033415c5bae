"""GMRES against the column LU as ARK2GKC's backward-Euler solver on the bench-size Held-Suarez state
(6 x 30 x 30 x 8 = 43 200 elements, N = 4, the full physics as bench.py builds it, the vertical
AtmosAcousticGravityLinearModel on the same auxiliary state), at the IMEX dt of scripts/measure_imex.py
(a tenth of the horizontal acoustic dt).  GeneralizedMinimalResidual(M = 20, rtol = 1e-8) by default.
Prints one JSON line.

  iterations:  of every solve of the timed steps (cmdg_gmres_step_info)
  step time:   host clock around --reps steps ending in a device synchronise, GMRES and column LU
  split:       one operator evaluation timed on its own (host clock around --reps evaluations and a
               synchronise) against the time of a solve per inner iteration
  bytes:       with --kernel-stats (the stats file of a rocprofv3 --kernel-trace --stats run of this
               script): k_gmres_mgs moves 3 state-sized arrays per launch (2 in a column's first
               launch), k_gmres_lincomb j + 2 for j vectors (the mean j of the run from the launch
               counts), against the 6.29 TB/s copy rate

Usage: python scripts/measure_gmres.py [--n-horz 30] [--reps 5] [--M 20] [--rtol 1e-8]
       python scripts/measure_gmres.py --combine RESULT.json --kernel-stats CSV   (no GPU)"""
import argparse
import csv
import json
import sys
import time

import torch

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
from cmdg_loader import cm            # noqa: E402
from helpers import held_suarez_setup  # noqa: E402

COPY_TBS = 6.29
VERTICAL, HORIZONTAL = 2, 1


def add_kernel_stats(res, path):
    state_bytes = res["state_bytes"]
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            if "k_gmres_" in name:
                out[name] = {"calls": int(row["Calls"]), "mean_us": float(row["AverageNs"]) / 1e3}
    res["kernel_stats"] = out
    calls = lambda key: sum(st["calls"] for name, st in out.items() if key in name)
    columns, dots, combos = calls("k_gmres_mgs<true>"), calls("k_gmres_mgs<false>"), calls("k_gmres_lincomb")
    for name, st in out.items():
        if "k_gmres_mgs<true>" in name or "k_gmres_scale" in name:
            arrays = 3.0                                  # read w, v, write w; read w, write v, copy
        elif "k_gmres_mgs<false>" in name:
            arrays = 3.0 - columns / max(dots, 1)         # a column's first launch reads two arrays only
        elif "k_gmres_lincomb" in name:
            arrays = columns / max(combos, 1) + 2.0       # the mean number of vectors, Q read and written
        else:
            continue
        st["state_arrays_per_launch"] = arrays
        st["TBs"] = arrays * state_bytes / st["mean_us"] / 1e6
        st["fraction_of_copy_rate"] = st["TBs"] / COPY_TBS


def timed(fn, reps, sync):
    fn()
    sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    sync()
    return (time.perf_counter() - t0) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-horz", type=int, default=30)
    ap.add_argument("--n-vert", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--M", type=int, default=20)
    ap.add_argument("--rtol", type=float, default=1e-8)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--combine", default=None)
    args = ap.parse_args()
    if args.combine:
        with open(args.combine) as f:
            res = json.loads(f.read().strip().splitlines()[-1])
        add_kernel_stats(res, args.kernel_stats)
        print(json.dumps(res))
        return
    assert torch.cuda.is_available(), "the measurement needs the GPU"
    ode = cm.odesolvers
    law, grid, d, dd = held_suarez_setup(n_horz=args.n_horz, n_vert=args.n_vert)
    dg = cm.dgmodel.DGModel(law, grid, direction=d, diffusion_direction=dd)
    lin = cm.dgmodel.DGModel(cm.atmos.AtmosAcousticGravityLinearModel(law), grid, direction=VERTICAL,
                             state_auxiliary=dg.state_auxiliary)
    Q0 = dg.init_ode_state(0.0)
    dt_h = 1 / dg.courant(cm.dgmodel.NONDIFFUSIVE_COURANT, Q0, 1.0, 0.0, HORIZONTAL)
    dt_v = 1 / dg.courant(cm.dgmodel.NONDIFFUSIVE_COURANT, Q0, 1.0, 0.0, VERTICAL)
    dt = 0.1 * dt_h
    sync = dg.synchronize
    res = {"workload": "Held-Suarez 6x%dx%dx%d, N=4, %d elements, fp64, ARK2GKC" %
           (args.n_horz, args.n_horz, args.n_vert, grid.nreal),
           "dt_s": dt, "vertical_acoustic_courant_of_dt": dt / dt_v, "copy_rate_TBs": COPY_TBS,
           "state_bytes": grid.nreal * 5 * grid.Np * 8,
           "gmres_M": args.M, "gmres_rtol": args.rtol}
    T, B = dg.create_state(), Q0.clone()
    op = timed(lambda: lin(T, B, 0.0, 1.0, 0.0), 4 * args.reps, sync)
    res["operator_evaluation_ms"] = 1e3 * op
    for kind in ("lu", "gmres"):
        Q = Q0.clone()
        if kind == "lu":
            be = ode.LinearBackwardEulerSolver(ode.ManyColumnLU())
        else:
            be = ode.LinearBackwardEulerSolver(ode.GeneralizedMinimalResidual(None, M=args.M, rtol=args.rtol))
        solver = ode.ARK2GiraldoKellyConstantinescu(dg, lin, be, Q, dt=dt)
        its = []

        def step():
            solver.dostep(Q, 1)
            its.extend(i.iterations for i in solver.solve_info)
        ms = 1e3 * timed(step, args.reps, sync)
        entry = {"ms_per_step": ms, "finite": bool(torch.isfinite(Q[:grid.nreal]).all())}
        if kind == "gmres":
            X = Q0.clone()
            n0 = len(its)
            solve = timed(lambda: its.append(solver.lu.solve(X, Q0).iterations) or X.copy_(Q0), args.reps,
                          lambda: None)
            per_solve = its[n0 + 1:]
            entry.update({"iterations": its[:n0], "mean_iterations_per_solve": sum(its[:n0]) / max(n0, 1),
                          "all_converged": all(i.converged for i in solver.solve_info),
                          "standalone_solve_ms": 1e3 * solve,
                          "standalone_solve_iterations": per_solve,
                          "ms_per_inner_iteration": 1e3 * solve / max(sum(per_solve) / max(len(per_solve), 1), 1),
                          "basis_bytes": (args.M + 1) * grid.nelem * 5 * grid.Np * 8})
            entry["operator_share_of_iteration"] = res["operator_evaluation_ms"] / entry["ms_per_inner_iteration"]
        res[kind] = entry
        solver.close()
    res["gmres_over_lu_step_time"] = res["gmres"]["ms_per_step"] / res["lu"]["ms_per_step"]
    if args.kernel_stats:
        add_kernel_stats(res, args.kernel_stats)
    lin.close()
    dg.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
