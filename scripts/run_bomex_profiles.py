"""Steps the BOMEX set-up (experiments/AtmosLES/bomex_les.jl as tests/helpers.py and bench.py build it)
and writes the time series of the AtmosLESDefault profiles (climatemachine.jl_amd/diagnostics.py): an
``.npz`` with ``time (nt,)``, ``z (L,)`` and one ``(nt, L)`` or ``(nt,)`` array per variable of the group.

Usage: python scripts/run_bomex_profiles.py [--steps 20 --every 10 --out bomex_profiles.npz]
                                            [--ne 4 --N 4 --dt 0.02]"""
import argparse
import sys

sys.path.insert(0, ".")
sys.path.insert(0, "tests")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--every", type=int, default=10)
    ap.add_argument("--out", default="bomex_profiles.npz")
    ap.add_argument("--ne", type=int, default=4, help="ne x ne x 2 ne elements of (200 m, 200 m, 3000 / (2 ne) m)")
    ap.add_argument("--N", type=int, default=4, help="polynomial order (4 or 6)")
    ap.add_argument("--dt", type=float, default=0.02)
    args = ap.parse_args()
    import numpy as np
    import torch
    from cmdg_loader import cm
    assert torch.cuda.is_available(), "the run needs the GPU"
    M, ne = cm.mesh, args.ne
    rng = [np.linspace(0.0, 200.0 * ne, ne + 1), np.linspace(0.0, 200.0 * ne, ne + 1),
           np.linspace(0.0, 3000.0, 2 * ne + 1)]
    topl = M.StackedBrickTopology(rng, periodicity=(True, True, False), boundary=((0, 0), (0, 0), (1, 2)))
    grid = M.DiscontinuousSpectralElementGrid(topl, args.N)
    dg = cm.dgmodel.DGModel(cm.moist.bomex_model(3000.0), grid)
    Q = dg.init_ode_state(0.0)
    solver = cm.odesolvers.LSRK54CarpenterKennedy(dg, Q, dt=args.dt)

    def show(t, p):
        print("t = %8.3f s  cld_cover %.3f  cld_base %7.1f  cld_top %7.1f  lwp %.3e  max tke %.3e"
              % (t, p["cld_cover"], p["cld_base"], p["cld_top"], p["lwp"], p["tke"].max()))
    cb = cm.diagnostics.AtmosLESDefaultCallback(dg, sink=show)
    cm.odesolvers.solve(Q, solver, numberofsteps=args.steps, callbacks=[(args.every, cb)])
    print("wrote %s: %d records of %d levels" % (cb.save(args.out), len(cb.records), cb.diag.nlevels))
    dg.close()


if __name__ == "__main__":
    main()
