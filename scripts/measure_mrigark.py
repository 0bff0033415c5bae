"""MRI-GARK stepping on the bench-size Held-Suarez state (6 x 30 x 30 x 8 = 43 200 elements,
N = 4, the full physics as bench.py builds it) against LSRK54 and ARK2GKC, rerun in the same
process.  Prints one JSON line.

  ERK45a:       MRIGARKERK45aSandu on the remainder (full minus the vertical acoustic-gravity
                linear law) over LSRK54 on the linear law at the vertical acoustic dt (Courant 1)
  ESDIRK24LSA:  MRIGARKESDIRK24LSA on the linear law (ManyColumnLU) over LSRK54 on the remainder
  LSRK54:       the full law at the every-direction acoustic dt
  ARK2GKC:      split and unsplit, at a tenth of the horizontal acoustic dt

Each (slow dt, fast dt) choice runs once, --steps slow steps from the initial state; the line
records whether the state stayed finite and the simulated seconds per wall second (host clock
around the steps, each ending in a device synchronise).

--kernel-stats CSV_OR_DB (with --combine RESULT.json): add the mean time of k_lsrk_mri_update and
k_mri_qhat from a rocprofv3 --kernel-trace --stats run of this script and their bytes, (4 + NR) 8
and (2 + NR) 8 per degree of freedom, over the copy rate.

Usage: python scripts/measure_mrigark.py [--n-horz 30] [--steps 5]
       python scripts/measure_mrigark.py --combine RESULT.json --kernel-stats CSV"""
import argparse
import csv
import json
import re
import sys
import time

sys.path.insert(0, ".")
sys.path.insert(0, "tests")

COPY_TBS = 6.29   # measured float4 copy rate of the MI355X
VERTICAL, HORIZONTAL = 2, 1


def _rows(path):
    """(kernel name, calls, mean ns) from a rocprofv3 kernel_stats.csv or a rocpd database."""
    if path.endswith(".db"):
        import sqlite3
        q = "select name, count(*), avg(end - start) from kernels where name like '%mri%' group by name"
        return sqlite3.connect(path).execute(q).fetchall()
    with open(path) as f:
        return [(r.get("Name") or r.get("KernelName") or "", int(r["Calls"]), float(r["AverageNs"]))
                for r in csv.DictReader(f)]


def add_kernel_stats(res, path):
    dofs = res["dofs"]
    out = {}
    for name, calls, ns in _rows(path):
        m = re.search(r"(k_lsrk_mri_update|k_mri_qhat)(?:ILi|<)(\d)", name)
        if not m:
            continue
        nr = int(m.group(2))
        per = (4 + nr) if m.group(1) == "k_lsrk_mri_update" else (2 + nr)
        us = float(ns) / 1e3
        nb = per * 8 * dofs
        out["%s<%d>" % (m.group(1), nr)] = {
            "calls": int(calls), "mean_us": us, "bytes": nb, "TBs": nb / us / 1e6,
            "fraction_of_copy_rate": nb / us / 1e6 / COPY_TBS}
    res["kernel_stats"] = out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-horz", type=int, default=30)
    ap.add_argument("--n-vert", type=int, default=8)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="one choice per scheme (for a profiler run)")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--combine", default=None)
    args = ap.parse_args()
    if args.combine:
        with open(args.combine) as f:
            res = json.loads(f.read().strip().splitlines()[-1])
        add_kernel_stats(res, args.kernel_stats)
        print(json.dumps(res))
        return
    import torch
    from cmdg_loader import cm
    from helpers import held_suarez_setup
    assert torch.cuda.is_available(), "the measurement needs the GPU"
    ode, dgm = cm.odesolvers, cm.dgmodel
    law, grid, d, dd = held_suarez_setup(n_horz=args.n_horz, n_vert=args.n_vert)
    dg = dgm.DGModel(law, grid, direction=d, diffusion_direction=dd)
    lin = dgm.DGModel(cm.atmos.AtmosAcousticGravityLinearModel(law), grid, direction=VERTICAL,
                      state_auxiliary=dg.state_auxiliary)
    rem = dgm.remainder_DGModel(dg, (lin,))
    Q0 = dg.init_ode_state(0.0)
    cour = lambda dr: dg.courant(dgm.NONDIFFUSIVE_COURANT, Q0, 1.0, 0.0, dr)
    dt_v, dt_h, dt_e = 1 / cour(VERTICAL), 1 / cour(HORIZONTAL), 1 / cour(0)
    nr = grid.nreal
    res = {"workload": "Held-Suarez 6x%dx%dx%d, N=4, %d elements, fp64, full physics as bench.py"
           % (args.n_horz, args.n_horz, args.n_vert, nr),
           "dofs": nr * 5 * grid.Np, "copy_rate_TBs": COPY_TBS, "slow_steps_per_run": args.steps,
           "acoustic_courant_dt_s": {"vertical": dt_v, "horizontal": dt_h, "every": dt_e}}

    def run(make, dt):
        Q = Q0.clone()
        solver = make(Q)
        dg.synchronize()
        solver.dostep(Q, 1)            # first step: warm-up (not timed)
        dg.synchronize()
        t0 = time.perf_counter()
        solver.dostep(Q, args.steps)
        dg.synchronize()
        wall = (time.perf_counter() - t0) / args.steps
        ok = bool(torch.isfinite(Q[:nr]).all())
        if hasattr(solver, "close"):
            solver.close()
        return {"dt_s": dt, "finite": ok, "ms_per_step": 1e3 * wall,
                "sim_s_per_wall_s": dt / wall if ok else 0.0}

    res["lsrk54"] = run(lambda Q: ode.LSRK54CarpenterKennedy(dg, Q, dt=dt_e), dt_e)
    for split in (False, True):
        res["ark2gkc_" + ("split" if split else "nosplit")] = run(
            lambda Q: ode.ARK2GiraldoKellyConstantinescu(
                dg, lin, ode.LinearBackwardEulerSolver(ode.ManyColumnLU()), Q, dt=0.1 * dt_h,
                split_explicit_implicit=split), 0.1 * dt_h)
    erk = [(10, 1.0), (20, 1.0), (40, 1.0)] if not args.quick else [(20, 1.0)]
    res["erk45a"] = []
    for slow, fast in erk:                       # multiples of the vertical acoustic dt
        r = run(lambda Q: ode.MRIGARKERK45aSandu(
            rem, ode.LSRK54CarpenterKennedy(lin, Q, dt=fast * dt_v), Q, dt=slow * dt_v), slow * dt_v)
        r.update(slow_over_vertical_dt=slow, fast_over_vertical_dt=fast)
        res["erk45a"].append(r)
    imp = ([(0.5, 0.25), (0.5, 0.5), (1.0, 0.5), (1.0, 1.0), (2.0, 1.0)] if not args.quick
           else [(0.5, 0.25)])
    res["esdirk24lsa"] = []
    for slow, fast in imp:                       # multiples of the horizontal acoustic dt
        r = run(lambda Q: ode.MRIGARKESDIRK24LSA(
            lin, ode.LinearBackwardEulerSolver(ode.ManyColumnLU()),
            ode.LSRK54CarpenterKennedy(rem, Q, dt=fast * dt_h), Q, dt=slow * dt_h), slow * dt_h)
        r.update(slow_over_horizontal_dt=slow, fast_over_horizontal_dt=fast)
        res["esdirk24lsa"].append(r)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
