"""IMEX stepping on the bench-size Held-Suarez state: ARK2GiraldoKellyConstantinescu with
LinearBackwardEulerSolver(ManyColumnLU()) (csrc/columnlu.hip, the step in csrc/steppers.hip) against explicit LSRK54.
6 x 30 x 30 x 8 = 43 200 elements, N = 4; the full physics as bench.py builds it (hyperdiffusion,
Gravity, Coriolis, Held-Suarez forcing) and AtmosAcousticGravityLinearModel on the same auxiliary
state.  Prints one JSON line.

--workload bomex: the moist LES law as bench.py --workload bomex builds it (16 x 16 x 32
elements of 200 m x 200 m x 93.75 m at N = 6; --bomex-order 4 --bomex-dx 400 --bomex-nz 19 is
the reference's bomex_les.jl resolution, 100 m x 40 m node spacing) with the six-state linear law.
Each stepper runs at the dt the reference picks: IMEX at the horizontal Courant number 0.35
(bomex_les.jl:60, :91-92), LSRK54 at the every-direction Courant number 0.35.

  dt:          vertical and horizontal acoustic Courant dts, dg.courant(NONDIFFUSIVE, Q, 1, 0,
               direction) -> dt = 1 / courant (Courant number 1); the IMEX steps run at a tenth of
               the horizontal dt, LSRK54 is quoted at the every-direction dt
  step time:   host clock around --reps steps ending in a device synchronise, for both
               split_explicit_implicit values and for LSRK54
  solve time:  host clock around --reps cmdg_columnlu_solve calls (each ends in a synchronise);
               with --kernel-stats also the k_band_solve kernel mean from a rocprofv3
               --kernel-trace --stats run of this script
  bytes:       band bytes ncol n (p + q + 1) 8, read once per solve, plus the state read twice
               and written twice (forward then back substitution)

Usage: python scripts/measure_imex.py [--n-horz 30] [--reps 10] [--kernel-stats CSV]
       python scripts/measure_imex.py --combine RESULT.json --kernel-stats CSV   (no GPU: adds the
       kernel times of a rocprofv3 run of the first form to the JSON line it printed)"""
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

COPY_TBS = 6.29   # measured float4 copy rate of the MI355X (MI355X_MICROARCH: HBM)
VERTICAL, HORIZONTAL = 2, 1


def kernel_stats(path):
    """{kernel name: (calls, mean ns)} of the column-solver and ARK kernels in a rocprofv3 stats file"""
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            if any(k in name for k in ("k_band_", "k_probe_", "k_ark_", "k_add")):
                out[name] = (int(row["Calls"]), float(row["AverageNs"]))
    return out


def add_kernel_stats(res, path):
    ks = kernel_stats(path)
    res["kernel_stats"] = {k: {"calls": c, "mean_us": v / 1e3} for k, (c, v) in ks.items()}
    sol = [v for k, v in ks.items() if "k_band_solve" in k]
    if sol:
        us = sol[0][1] / 1e3
        nb = res["solve"]["bytes"]
        res["solve"]["kernel_us"] = us
        res["solve"]["kernel_TBs"] = nb / us / 1e6
        res["solve"]["kernel_fraction_of_copy_rate"] = nb / us / 1e6 / COPY_TBS


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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--combine", default=None)
    ap.add_argument("--workload", choices=["heldsuarez", "bomex"], default="heldsuarez")
    ap.add_argument("--bomex-ne", type=int, default=16)
    ap.add_argument("--bomex-nz", type=int, default=0, help="vertical elements (0: 2 ne)")
    ap.add_argument("--bomex-order", type=int, default=6)
    ap.add_argument("--bomex-dx", type=float, default=200.0, help="horizontal element size, m")
    args = ap.parse_args()
    if args.combine:
        with open(args.combine) as f:
            res = json.loads(f.read().strip().splitlines()[-1])
        add_kernel_stats(res, args.kernel_stats)
        print(json.dumps(res))
        return
    assert torch.cuda.is_available(), "the measurement needs the GPU"
    if args.workload == "bomex":
        return bomex(args)
    ode = cm.odesolvers
    law, grid, d, dd = held_suarez_setup(n_horz=args.n_horz, n_vert=args.n_vert)
    dg = cm.dgmodel.DGModel(law, grid, direction=d, diffusion_direction=dd)
    lin = cm.dgmodel.DGModel(cm.atmos.AtmosAcousticGravityLinearModel(law), grid, direction=VERTICAL,
                             state_auxiliary=dg.state_auxiliary)
    Q0 = dg.init_ode_state(0.0)
    c_v = dg.courant(cm.dgmodel.NONDIFFUSIVE_COURANT, Q0, 1.0, 0.0, VERTICAL)
    c_h = dg.courant(cm.dgmodel.NONDIFFUSIVE_COURANT, Q0, 1.0, 0.0, HORIZONTAL)
    c_e = dg.courant(cm.dgmodel.NONDIFFUSIVE_COURANT, Q0, 1.0, 0.0, 0)
    dt_v, dt_h, dt_e = 1 / c_v, 1 / c_h, 1 / c_e
    res = {"workload": "Held-Suarez 6x%dx%dx%d, N=4, %d elements, fp64, full physics as bench.py"
           % (args.n_horz, args.n_horz, args.n_vert, grid.nreal),
           "copy_rate_TBs": COPY_TBS,
           "acoustic_courant_dt_s": {"vertical": dt_v, "horizontal": dt_h, "every": dt_e,
                                     "ratio_horizontal_over_vertical": dt_h / dt_v}}
    sync = dg.synchronize
    # explicit LSRK54 at the bench's dt (its cost per step does not depend on dt)
    Q = Q0.clone()
    s = ode.LSRK54CarpenterKennedy(dg, Q, dt=0.15)
    lsrk = timed(lambda: s.dostep(Q, 1), args.reps, sync)
    res["lsrk54_ms_per_step"] = 1e3 * lsrk
    # IMEX at a tenth of the horizontal acoustic dt (the explicit part's limit; the reference's
    # heldsuarez.jl picks its dt from the horizontal Courant number)
    dt_imex = 0.1 * dt_h
    res["imex_dt_s"] = dt_imex
    for split in (False, True):
        Q = Q0.clone()
        t0 = time.perf_counter()
        solver = ode.ARK2GiraldoKellyConstantinescu(
            dg, lin, ode.LinearBackwardEulerSolver(ode.ManyColumnLU()), Q, dt=dt_imex,
            split_explicit_implicit=split)
        sync()
        setup = time.perf_counter() - t0
        step = timed(lambda: solver.dostep(Q, 1), args.reps, sync)
        ok = bool(torch.isfinite(Q[:grid.nreal]).all())
        key = "split" if split else "nosplit"
        res["imex_" + key] = {"ms_per_step": 1e3 * step, "finite": ok,
                              "create_assemble_factor_s": setup}
        lu = solver.lu
        if not split:
            res["band"] = {"ncol": lu.ncol, "n": lu.n, "p": lu.p, "q": lu.q, "bytes": lu.band_bytes}
            # one solve: band once, the state read twice and written twice
            X, B = dg.create_state(), Q0.clone()
            solve = timed(lambda: lu.solve(X, B), args.reps, lambda: None)
            nb = lu.band_bytes + 4 * grid.nreal * 5 * grid.Np * 8
            res["solve"] = {"call_ms": 1e3 * solve, "bytes": nb, "call_TBs": nb / solve / 1e12,
                            "call_fraction_of_copy_rate": nb / solve / 1e12 / COPY_TBS}
            t0 = time.perf_counter()
            lu.update(dt_imex * 0.29289321881345254)
            res["assemble_factor_s"] = time.perf_counter() - t0
        solver.close()
    # simulated seconds per wall second
    res["simulated_s_per_wall_s"] = {
        "lsrk54_at_every_direction_courant_1": dt_e / lsrk,
        "imex_nosplit": dt_imex / (res["imex_nosplit"]["ms_per_step"] / 1e3),
        "imex_split": dt_imex / (res["imex_split"]["ms_per_step"] / 1e3)}
    if args.kernel_stats:
        add_kernel_stats(res, args.kernel_stats)
    lin.close()
    dg.close()
    print(json.dumps(res))


def bomex(args):
    import numpy as np
    M, ode = cm.mesh, cm.odesolvers
    ne, N, dx = args.bomex_ne, args.bomex_order, args.bomex_dx
    nz = args.bomex_nz or 2 * ne
    rng = [np.linspace(0.0, dx * ne, ne + 1), np.linspace(0.0, dx * ne, ne + 1),
           np.linspace(0.0, 3000.0, nz + 1)]
    topl = M.StackedBrickTopology(rng, periodicity=(True, True, False), boundary=((0, 0), (0, 0), (1, 2)))
    grid = M.DiscontinuousSpectralElementGrid(topl, N)
    law = cm.moist.bomex_model(3000.0)
    dg = cm.dgmodel.DGModel(law, grid, direction=0)
    lin = cm.dgmodel.DGModel(cm.atmos.AtmosAcousticGravityLinearModel(law), grid, direction=VERTICAL,
                             state_auxiliary=dg.state_auxiliary)
    Q0 = dg.init_ode_state(0.0)
    c = {k: dg.courant(cm.dgmodel.NONDIFFUSIVE_COURANT, Q0, 1.0, 0.0, d)
         for k, d in (("vertical", VERTICAL), ("horizontal", HORIZONTAL), ("every", 0))}
    dt_imex, dt_lsrk = 0.35 / c["horizontal"], 0.35 / c["every"]
    res = {"workload": "BOMEX %dx%dx%d, N=%d, %d elements, element %g m x %g m x %g m, fp64, full "
                       "physics as bench.py --workload bomex" % (ne, ne, nz, N, grid.nreal, dx, dx, 3000.0 / nz),
           "copy_rate_TBs": COPY_TBS,
           "acoustic_courant_1_dt_s": {k: 1 / v for k, v in c.items()},
           "ratio_horizontal_over_vertical": c["vertical"] / c["horizontal"],
           "lsrk54_dt_s": dt_lsrk, "imex_dt_s": dt_imex,
           "imex_dt_over_vertical_acoustic_limit": dt_imex * c["vertical"]}
    sync = dg.synchronize
    Q = Q0.clone()
    s = ode.LSRK54CarpenterKennedy(dg, Q, dt=dt_lsrk)
    lsrk = timed(lambda: s.dostep(Q, 1), args.reps, sync)
    res["lsrk54_ms_per_step"] = 1e3 * lsrk
    res["lsrk54_finite"] = bool(torch.isfinite(Q[:grid.nreal]).all())
    for split in (False, True):
        Q = Q0.clone()
        t0 = time.perf_counter()
        solver = ode.ARK2GiraldoKellyConstantinescu(
            dg, lin, ode.LinearBackwardEulerSolver(ode.ManyColumnLU()), Q, dt=dt_imex,
            split_explicit_implicit=split)
        sync()
        setup = time.perf_counter() - t0
        step = timed(lambda: solver.dostep(Q, 1), args.reps, sync)
        key = "split" if split else "nosplit"
        res["imex_" + key] = {"ms_per_step": 1e3 * step, "finite": bool(torch.isfinite(Q[:grid.nreal]).all()),
                              "create_assemble_factor_s": setup}
        lu = solver.lu
        if not split:
            res["band"] = {"ncol": lu.ncol, "n": lu.n, "p": lu.p, "q": lu.q, "bytes": lu.band_bytes}
            X, B = dg.create_state(), Q0.clone()
            solve = timed(lambda: lu.solve(X, B), args.reps, lambda: None)
            nb = lu.band_bytes + 4 * grid.nreal * law.ns * grid.Np * 8
            res["solve"] = {"call_ms": 1e3 * solve, "bytes": nb, "call_TBs": nb / solve / 1e12,
                            "call_fraction_of_copy_rate": nb / solve / 1e12 / COPY_TBS}
            t0 = time.perf_counter()
            lu.update(dt_imex * 0.29289321881345254)
            sync()
            res["assemble_factor_s"] = time.perf_counter() - t0
        solver.close()
    res["simulated_s_per_wall_s"] = {
        "lsrk54": dt_lsrk / lsrk,
        "imex_nosplit": dt_imex / (res["imex_nosplit"]["ms_per_step"] / 1e3),
        "imex_split": dt_imex / (res["imex_split"]["ms_per_step"] / 1e3)}
    if args.kernel_stats:
        add_kernel_stats(res, args.kernel_stats)
    lin.close()
    dg.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
