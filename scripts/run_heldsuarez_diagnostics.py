"""Steps the Held-Suarez set-up (experiments/AtmosGCM/heldsuarez.jl as tests/helpers.py and bench.py build
it) and writes the time series of the AtmosGCMDefault group (climatemachine.jl_amd/diagnostics.py): an
``.npz`` with ``time (nt,)``, the axes ``long``, ``lat``, ``level`` and one ``(nt, nlevel, nlat, nlong)``
array per variable (u, v, w, rho, temp, pres, thd, et, ei, ht, hi, vort, vort2).

Usage: python scripts/run_heldsuarez_diagnostics.py [--steps 20 --every 10 --out heldsuarez_gcm.npz]
                                                    [--nhorz 6 --nvert 4 --dt 1.0 --res 5 --dz 5000]"""
import argparse
import sys

sys.path.insert(0, ".")
sys.path.insert(0, "tests")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--every", type=int, default=10)
    ap.add_argument("--out", default="heldsuarez_gcm.npz")
    ap.add_argument("--nhorz", type=int, default=6)
    ap.add_argument("--nvert", type=int, default=4)
    ap.add_argument("--dt", type=float, default=1.0)
    ap.add_argument("--res", type=float, default=5.0, help="output resolution in degrees (the reference: 1)")
    ap.add_argument("--dz", type=float, default=5000.0, help="output level spacing in metres (the reference: 1000)")
    args = ap.parse_args()
    import numpy as np
    import torch
    from cmdg_loader import cm
    from helpers import held_suarez_setup
    assert torch.cuda.is_available(), "the run needs the GPU"
    law, grid, direction, diffusion_direction = held_suarez_setup(n_horz=args.nhorz, n_vert=args.nvert, N=4)
    a, H = law.ps.planet_radius, 30e3
    lat = -90.0 + args.res * np.arange(int(round(180.0 / args.res)) + 1)
    lon = -180.0 + args.res * np.arange(int(round(360.0 / args.res)) + 1)
    rad = a + args.dz * np.arange(int(round(H / args.dz)) + 1)
    interpol = cm.mesh.interpolation.InterpolationCubedSphere(grid, np.linspace(a, a + H, args.nvert + 1), args.nhorz,
                                                             lat, lon, rad)
    dg = cm.dgmodel.DGModel(law, grid, direction=direction, diffusion_direction=diffusion_direction)
    Q = dg.init_ode_state(0.0)
    solver = cm.odesolvers.LSRK54CarpenterKennedy(dg, Q, dt=args.dt)

    def show(t, p):
        print("t = %8.2f s  max |u| %.3f  max |w| %.3e  temp %.2f..%.2f  max |vort| %.3e  max |vort2| %.3e"
              % (t, np.abs(p["u"]).max(), np.abs(p["w"]).max(), p["temp"].min(), p["temp"].max(),
                 np.abs(p["vort"]).max(), np.abs(p["vort2"]).max()))
    cb = cm.diagnostics.AtmosGCMDefaultCallback(dg, interpol, sink=show)
    cm.odesolvers.solve(Q, solver, numberofsteps=args.steps, callbacks=[(args.every, cb)])
    shape = cb.records[0][1]["u"].shape if cb.records else ()
    print("wrote %s: %d records of a %s grid" % (cb.save(args.out), len(cb.records), "x".join(str(n) for n in shape)))
    cb.diag.close()
    dg.close()


if __name__ == "__main__":
    main()
