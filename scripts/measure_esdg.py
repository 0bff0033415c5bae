#!/usr/bin/env python
"""Time one ESDGModel evaluation per volume flux with the library's profiling events
(``CMDG_K_ESDG_TENDENCY``), next to the Euler ``k_tendency`` of ``CMDG_PHYSICS_DRY_ATMOS`` on the
same grid, and append one JSON line per case to profiles/esdg_measure.jsonl.

    python scripts/measure_esdg.py [--grid brick|sphere|both] [--reps 7] [--evals 20]

Grids: a 24^3 warped periodic brick at N = 4; a 6 x 16 x 16 x 8 cubed sphere at N = 3.  Per case:
``reps`` repetitions of ``evals`` evaluations after a warm-up of the same length; the median time per
evaluation and the spread (max - min) / median over the repetitions are reported, with the two-point
fluxes per second (3 Nq per node and evaluation in the volume, one per face node) and the fraction
of the HBM peak (8 TB/s) the needed bytes -- state read, tendency written, metric terms and the
auxiliary columns read, once each -- would account for."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cmdg_loader import cm  # noqa: E402

HBM_PEAK = 8.0e12


def warp(x1, x2, x3):
    a = (4 / np.pi) * (1 - x1 ** 2) * (1 - x2 ** 2) * (1 - x3 ** 2)
    x1, x2 = np.cos(a) * x1 - np.sin(a) * x2, np.sin(a) * x1 + np.cos(a) * x2
    x1, x3 = np.cos(a) * x1 - np.sin(a) * x3, np.sin(a) * x1 + np.cos(a) * x3
    return x1, x2, x3


class Smooth:
    """A smooth positive state: the timing does not depend on it, the logarithms must be defined."""

    def init_state_prognostic(self, coord, aux):
        E = cm.esdg
        x, y, z = coord
        r = np.sqrt(x * x + y * y + z * z) + 1.0
        rho = 1.2 + 0.1 * np.sin(3 * x / r) * np.cos(2 * y / r)
        rhou = [rho * 0.1 * np.sin(2 * c / r) for c in (y, z, x)]
        p = 1.5 + 0.1 * np.cos(3 * z / r)
        return np.stack([rho] + rhou + [E.totalenergy(rho, rhou, p, E.gamma())], axis=1)


def grids(which):
    M, A = cm.mesh, cm.atmos
    if which in ("brick", "both"):
        rng = [np.linspace(-1.0, 1.0, 25)] * 3
        topl = M.BrickTopology(rng, periodicity=(True,) * 3, connectivity="face")
        yield "brick24_N4", M.DiscontinuousSpectralElementGrid(topl, 4, meshwarp=warp), False
    if which in ("sphere", "both"):
        ps = A.PlanetParameters()
        topl = M.StackedCubedSphereTopology(16, np.linspace(ps.planet_radius, ps.planet_radius + 30e3, 9),
                                            boundary=(1, 2))
        yield "sphere6x16x16x8_N3", M.DiscontinuousSpectralElementGrid(
            topl, 3, meshwarp=M.equiangular_cubed_sphere_warp), True


def time_evaluations(dg, Q, kernel, reps, evals):
    import torch
    T = torch.zeros_like(Q)
    for _ in range(evals):
        dg(T, Q, 0.0)
    dg.profile_enable(True)
    per = []
    for _ in range(reps):
        dg.profile_reset()
        for _ in range(evals):
            dg(T, Q, 0.0)
        ms, n = dg.profile_get(kernel)
        per.append(ms / max(n, 1))
    dg.profile_enable(False)
    per = np.array(per)
    return float(np.median(per)), float((per.max() - per.min()) / np.median(per))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", default="both", choices=("brick", "sphere", "both"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--evals", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "esdg_measure.jsonl"))
    args = ap.parse_args()
    E, A = cm.esdg, cm.atmos
    lines = []
    for name, grid, sphere in grids(args.grid):
        orient = E.SphericalOrientation() if sphere else E.FlatOrientation()
        law = E.DryAtmosModel(orient, Smooth(), sources=(E.Coriolis(), E.Gravity()) if sphere else ())
        Nq, nreal, Np = grid.Nq[0], grid.nreal, grid.Np
        pairs = nreal * (3 * Nq * Np + 6 * Nq * Nq)
        # Q read + tendency written (5 each), M + nine metric terms, grad Phi when gravity is on
        nbytes = 8.0 * nreal * Np * (5 + 5 + 10 + (3 if sphere else 0))
        for vname, vf in (("EntropyConservative", E.EntropyConservative()), ("CentralVolumeFlux", E.CentralVolumeFlux()),
                          ("KGVolumeFlux", E.KGVolumeFlux())):
            dg = cm.dgmodel.ESDGModel(law, grid, vf, E.RusanovNumericalFlux())
            Q = dg.init_ode_state(0.0)
            ms, spread = time_evaluations(dg, Q, "ESDG_TENDENCY", args.reps, args.evals)
            dg.close()
            lines.append(dict(grid=name, nelem=int(nreal), N=Nq - 1, kernel="k_esdg_tendency", volume_flux=vname,
                              surface_flux="Rusanov", ms_per_evaluation=ms, spread=spread,
                              two_point_fluxes_per_s=pairs / (ms * 1e-3),
                              hbm_fraction_needed_bytes=nbytes / (ms * 1e-3) / HBM_PEAK, reps=args.reps,
                              evals=args.evals))
            print(json.dumps(lines[-1]), flush=True)
        # the yardstick: the Euler k_tendency of the dry atmosphere law on the same grid
        ps = A.PlanetParameters()
        euler = A.DryAtmosModel(A.IsentropicVortexSetup(ps), orientation=A.ORIENT_NONE, ref_state=None, viscosity=0.0,
                                dynamic_viscosity=True, sources=0,
                                boundary_conditions=(A.BC_ATMOS_DEFAULT, A.BC_ATMOS_DEFAULT) if sphere else (),
                                param_set=ps)
        dg = cm.dgmodel.DGModel(euler, grid)
        import torch
        Q = torch.from_numpy(Smooth().init_state_prognostic([grid.vgeo[:, c, :] for c in (12, 13, 14)], None)).to(dg.device)
        ms, spread = time_evaluations(dg, Q, "TENDENCY", args.reps, args.evals)
        dg.close()
        lines.append(dict(grid=name, nelem=int(nreal), N=Nq - 1, kernel="k_tendency (CMDG_PHYSICS_DRY_ATMOS, Euler)",
                          ms_per_evaluation=ms, spread=spread, reps=args.reps, evals=args.evals))
        print(json.dumps(lines[-1]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
