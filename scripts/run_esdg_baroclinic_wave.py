#!/usr/bin/env python
"""The reference's entropy-stable baroclinic wave (test/Numerics/ESDGMethods/DryAtmos/baroclinic_wave.jl,
``run(...)`` as ``main()`` calls it): N = 3, 8 x 8 elements per panel, 5 levels to 30 km,
``DecayingTemperatureProfile(290, 220, 8e3)``, sources ``(Coriolis(), Gravity())``, KG volume flux and
Rusanov surface flux, ``ARK2GiraldoKellyConstantinescu`` over the ESDGModel and the vertical
``DryAtmosAcousticGravityLinearModel`` with ``LinearBackwardEulerSolver(ManyColumnLU(); isadjustable =
false)``, ``split_explicit_implicit = false``, ``dt = 3 dx / soundspeed_air(330 K)`` from
``min_node_distance``, ten days, ``adjustfinalstep = false``.

    python scripts/run_esdg_baroclinic_wave.py [--days 10] [--chunk-steps 8000] [--timeout 600]

The run is cut into chunks of ``--chunk-steps`` steps; each chunk is a child process of its own under
``timeout -k 10 <--timeout>`` that reads the state the previous one left (float64, so the chunks
reproduce one uninterrupted run bit for bit: the stepper carries nothing but Q and t) and writes it
back.  A chunk that fails or runs out of time ends the run there.  A chunk also ends at every multiple of
``nt_freq = floor(timeend / (10 dt))`` steps, where the reference's StateCheck callback fires: the table
the reference checks is the callback's last record (step ``10 nt_freq``), not the state after the final step.

Written to profiles/esdg_baroclinic_wave.json: the StateCheck statistics of Q at the callback's last record
(minimum, maximum, mean, standard deviation with n - 1 over every node of the real elements, as
``scstats`` forms them) and after the final step, the
digits each agrees with the reference's table (tests/golden/esdg_baroclinic_wave_refvals.json; only
meaningful after the full ten days), ``norm(Q) / norm(Q0)`` and the wall time per step."""
import argparse
import json
import math
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

POLYNOMIALORDER, NUMELEM_HORZ, NUMELEM_VERT = 3, 8, 5
DOMAIN_HEIGHT = 30e3
CFL = 3
FIELDS = ("ρ", "ρu[1]", "ρu[2]", "ρu[3]", "ρe")


def setup():
    from cmdg_loader import cm
    M, A, E, ode = cm.mesh, cm.atmos, cm.esdg, cm.odesolvers
    ps = A.PlanetParameters()
    a = ps.planet_radius
    topl = M.StackedCubedSphereTopology(NUMELEM_HORZ, np.linspace(a, a + DOMAIN_HEIGHT, NUMELEM_VERT + 1),
                                        boundary=(1, 2))
    grid = M.DiscontinuousSpectralElementGrid(topl, POLYNOMIALORDER, meshwarp=E.cubedshellwarp)
    model = E.DryAtmosModel(E.SphericalOrientation(), E.BaroclinicWave(ps),
                            ref_state=E.DryReferenceState(A.DecayingTemperatureProfile(ps, 290.0, 220.0, 8e3)),
                            sources=(E.Coriolis(), E.Gravity()), param_set=ps)
    esdg = cm.dgmodel.ESDGModel(model, grid, volume_numerical_flux_first_order=E.KGVolumeFlux(),
                                surface_numerical_flux_first_order=E.RusanovNumericalFlux())
    lineardg = cm.dgmodel.DGModel(E.DryAtmosAcousticGravityLinearModel(model), grid,
                                  numerical_flux_first_order=0, direction=2,      # Rusanov, VerticalDirection
                                  state_auxiliary=esdg.state_auxiliary)
    acoustic_speed = math.sqrt(ps.cp_d / ps.cv_d * ps.R_d * 330.0)                # soundspeed_air(330 K)
    dt = CFL * esdg.min_node_distance() / acoustic_speed
    return cm, ode, grid, esdg, lineardg, dt


def scstats(a):
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    m = a.mean()
    return [float(a.min()), float(a.max()), float(m), float(np.sqrt(((a - m) ** 2).sum() / (a.size - 1)))]


def agreed_digits(value, ref):
    if value == ref:
        return 16
    if ref == 0:
        return 0
    return max(0, min(16, int(math.floor(-math.log10(abs(value - ref) / abs(ref))))))


def worker(args):
    import torch
    cm, ode, grid, esdg, lineardg, dt = setup()
    state = args.state
    if os.path.exists(state):
        with np.load(state) as z:
            Qh, t, steps, norm0 = z["Q"], float(z["t"]), int(z["steps"]), float(z["norm0"])
        Q = torch.from_numpy(Qh).to(esdg.device)
    else:
        Q = esdg.init_ode_state(0.0)
        t, steps, norm0 = 0.0, 0, esdg.norm(Q)
    solver = ode.ARK2GiraldoKellyConstantinescu(
        esdg, lineardg, ode.LinearBackwardEulerSolver(ode.ManyColumnLU(), isadjustable=False), Q, dt=dt, t0=t,
        split_explicit_implicit=False)
    esdg.synchronize()
    tic = time.perf_counter()
    nt_freq = int(math.floor(args.timeend / 10 / dt))          # floor(Int, 1 // 10 * timeend / dt)
    todo = min(args.chunk_steps, nt_freq - steps % nt_freq) if nt_freq > 0 else args.chunk_steps
    ode.solve(Q, solver, timeend=args.timeend, numberofsteps=todo, adjustfinalstep=False)
    esdg.synchronize()
    wall = time.perf_counter() - tic
    done = solver.steps
    Qh = Q.cpu().numpy()
    finite = bool(np.isfinite(Qh).all())
    np.savez(state, Q=Qh, t=np.float64(solver.t), steps=np.int64(steps + done), norm0=np.float64(norm0))
    info = dict(dt=dt, steps=steps + done, chunk_steps=done, t=solver.t, chunk_wall_s=wall, finite=finite,
                norm_ratio=esdg.norm(Q) / norm0, nreal=int(grid.nreal), nt_freq=nt_freq,
                stats=[scstats(Qh[:grid.nreal, s, :]) for s in range(5)])
    with open(state + ".json", "w") as f:
        json.dump(info, f)
    solver.close()
    lineardg.close()
    esdg.close()
    return 0 if finite else 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--days", type=float, default=10.0)
    ap.add_argument("--chunk-steps", type=int, default=8000)
    ap.add_argument("--timeout", type=int, default=600, help="seconds a chunk may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "esdg_baroclinic_wave.json"))
    ap.add_argument("--state", default=os.path.join(ROOT, "build", "esdg_baroclinic_wave_state.npz"),
                    help="where the chunks hand the state on (an ignored directory)")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--timeend", type=float, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        sys.exit(worker(args))
    timeend = args.days * 24 * 3600
    os.makedirs(os.path.dirname(args.state), exist_ok=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    for stale in (args.state, args.state + ".json"):
        if os.path.exists(stale):
            os.remove(stale)
    chunks, info, check, status = [], None, None, 0
    while info is None or info["t"] < timeend:
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--worker",
               "--timeend", repr(timeend), "--chunk-steps", str(args.chunk_steps), "--state", args.state]
        status = subprocess.run(cmd).returncode
        if status != 0:
            print("chunk %d ended with status %d: the run stops here" % (len(chunks) + 1, status), flush=True)
            break
        with open(args.state + ".json") as f:
            info = json.load(f)
        chunks.append(dict(steps=info["chunk_steps"], wall_s=info["chunk_wall_s"]))
        if info["nt_freq"] > 0 and info["steps"] % info["nt_freq"] == 0:
            check = info                      # what the StateCheck callback records
        print("t = %.1f s (%d steps), %.3f ms per step, norm(Q)/norm(Q0) = %.12f"
              % (info["t"], info["steps"], 1e3 * info["chunk_wall_s"] / max(info["chunk_steps"], 1),
                 info["norm_ratio"]), flush=True)
    if info is None:
        sys.exit(status or 1)
    with open(os.path.join(ROOT, "tests", "golden", "esdg_baroclinic_wave_refvals.json"), encoding="utf-8") as f:
        ref = json.load(f)["values"]
    check = check or info
    complete = status == 0 and args.days == 10.0 and check["steps"] == 10 * check["nt_freq"]
    per_step = [c["wall_s"] / c["steps"] for c in chunks if c["steps"] >= 100]
    if not per_step:
        per_step = [c["wall_s"] / c["steps"] for c in chunks if c["steps"] > 0]
    out = dict(
        config=dict(polynomialorder=POLYNOMIALORDER, numelem_horz=NUMELEM_HORZ, numelem_vert=NUMELEM_VERT,
                    domain_height=DOMAIN_HEIGHT, cfl=CFL, days=args.days, nreal=info["nreal"]),
        dt=info["dt"], steps=info["steps"], simtime=info["t"], chunk_status=status,
        comparable_with_reference_table=complete,
        statecheck_step=check["steps"], statecheck_simtime=check["t"], nt_freq=check["nt_freq"],
        statecheck={FIELDS[s]: dict(zip(("min", "max", "mean", "std"), check["stats"][s])) for s in range(5)},
        digits_agreed_with_reference={FIELDS[s]: dict(zip(("min", "max", "mean", "std"),
                                                          [agreed_digits(check["stats"][s][j], ref[s][2 + j])
                                                           for j in range(4)])) for s in range(5)},
        final_state={FIELDS[s]: dict(zip(("min", "max", "mean", "std"), info["stats"][s])) for s in range(5)},
        norm_ratio=info["norm_ratio"],
        wall_ms_per_step=dict(median=1e3 * float(np.median(per_step)), min=1e3 * min(per_step),
                              max=1e3 * max(per_step), chunks=len(per_step),
                              note="host wall time of the stepping loop of a chunk, one library call per step"))
    with open(args.out, "w", encoding="utf-8") as f:
        json.dump(out, f, indent=1, ensure_ascii=False)
        f.write("\n")
    print(json.dumps(out, ensure_ascii=False), flush=True)
    sys.exit(status)


if __name__ == "__main__":
    main()
