"""What a tracer costs on the bench Held-Suarez sphere (6 x 30 x 30 x 8 = 43 200 elements, N = 4,
the full physics as bench.py builds it) with NT = 0, 1, 2 tracers (the reference's dummy
initialisation, heldsuarez.jl:99-100, 184-186).  Prints one JSON line.

  LSRK54:   ms per step through cmdg_lsrk_run (the fused path bench.py times)
  ARK2GKC:  ms per step at 0.1 of the horizontal acoustic Courant-1 dt, split and unsplit, with
            ManyColumnLU on the five-state linear model (its band does not grow with NT)

Timing follows DESIGN section 6: a warm-up run, then --repeat runs of --steps steps each between two
events on the handle's stream; the median run is reported.  The yardstick is the algorithmic-byte
model of SURVEY section 8(d): a tracer adds 8 (1 + 1 + 3) B to the gradient pass, 8 * 2 B to the
gradient-of-Laplacian pass and 8 (4 + 1 + 3) B to the tendency and update pass, 120 B on about
1 780 B per node update, +6.7 % per tracer.

Usage: python scripts/measure_tracers.py [--n-horz 30] [--steps 10] [--repeat 5] [--tracers 0 1 2]
Per-kernel figures: run it under ``rocprofv3 --kernel-trace --stats -- python scripts/measure_tracers.py
--no-imex --repeat 1`` and read the k_tendency / k_gradients / k_lapfused rows per law."""
import argparse
import json
import statistics
import sys

import torch

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
from cmdg_loader import cm            # noqa: E402
from helpers import held_suarez_setup  # noqa: E402

VERTICAL, HORIZONTAL = 2, 1
BYTES_PER_NODE_UPDATE, BYTES_PER_TRACER = 1780.0, 120.0


def timed(fn, steps, repeat, sync):
    """Median over ``repeat`` runs of the event time of ``steps`` calls, ms per call."""
    fn()
    sync()
    out = []
    for _ in range(repeat):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        sync()
        a.record()
        for _ in range(steps):
            fn()
        sync()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / steps)
    return statistics.median(out), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-horz", type=int, default=30)
    ap.add_argument("--n-vert", type=int, default=8)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--tracers", type=int, nargs="+", default=[0, 1, 2])
    ap.add_argument("--no-imex", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the measurement needs the GPU"
    A, ode = cm.atmos, cm.odesolvers
    res = {"byte_model_increase_per_tracer": BYTES_PER_TRACER / BYTES_PER_NODE_UPDATE, "cases": {}}
    for nt in args.tracers:
        law, grid, d, dd = held_suarez_setup(n_horz=args.n_horz, n_vert=args.n_vert)
        if nt:
            law = A.DryAtmosModel(law.init_state, orientation=law.orientation, ref_state=law.ref_state,
                                  viscosity=law.viscosity, dynamic_viscosity=law.dynamic_viscosity,
                                  hyperdiffusion_timescale=law.tau_hyper, sources=law.sources,
                                  boundary_conditions=law.boundary_conditions, param_set=law.ps,
                                  tracers=A.HeldSuarezSetup.tracers(nt))
        res["workload"] = ("Held-Suarez 6x%dx%dx%d, N=4, %d elements, fp64, full physics as bench.py"
                           % (args.n_horz, args.n_horz, args.n_vert, grid.nreal))
        dg = cm.dgmodel.DGModel(law, grid, direction=d, diffusion_direction=dd)
        Q0 = dg.init_ode_state(0.0)
        case = {"nstate": law.ns}
        Q, dQ = Q0.clone(), dg.create_state()
        s = ode.LSRK54CarpenterKennedy(dg, Q, dt=0.15)
        med, runs = timed(lambda: dg.lsrk_run(Q, dQ, 0.0, 0.15, 1, s.RKA, s.RKB, s.RKC), args.steps,
                          args.repeat, dg.synchronize)
        case["lsrk54_ms_per_step"], case["lsrk54_runs_ms"] = med, runs
        case["lsrk54_finite"] = bool(torch.isfinite(Q[:grid.nreal]).all())
        if not args.no_imex:
            lin = cm.dgmodel.DGModel(A.AtmosAcousticGravityLinearModel(law), grid, direction=VERTICAL,
                                     state_auxiliary=dg.state_auxiliary)
            dt = 0.1 / dg.courant(cm.dgmodel.NONDIFFUSIVE_COURANT, Q0, 1.0, 0.0, HORIZONTAL)
            case["imex_dt_s"] = dt
            for split in (False, True):
                Q = Q0.clone()
                solver = ode.ARK2GiraldoKellyConstantinescu(dg, lin, ode.LinearBackwardEulerSolver(ode.ManyColumnLU()),
                                                            Q, dt=dt, split_explicit_implicit=split)
                med, runs = timed(lambda: solver.dostep(Q, 1), max(1, args.steps // 2), args.repeat, dg.synchronize)
                key = "imex_split" if split else "imex_nosplit"
                case[key + "_ms_per_step"], case[key + "_runs_ms"] = med, runs
                case[key + "_finite"] = bool(torch.isfinite(Q[:grid.nreal]).all())
                case["band_bytes"] = solver.lu.band_bytes
                solver.close()
            lin.close()
        dg.close()
        res["cases"]["NT=%d" % nt] = case
    base = res["cases"].get("NT=0")
    if base:
        for k, c in res["cases"].items():
            nt = int(k[3:])
            if nt:
                c["increase_per_tracer_over_NT0"] = {
                    key: (c[key] / base[key] - 1) / nt for key in c if key.endswith("_ms_per_step") and key in base}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
