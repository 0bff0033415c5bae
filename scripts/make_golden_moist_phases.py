"""Write tests/golden/moist_phase_cases.npz: inputs (rho, q_tot, e_int) of the moist law's saturation
adjustment in every phase regime and their answers from tests/moist_phase_restatement.py (mpmath,
40 digits), rounded to double.

    python scripts/make_golden_moist_phases.py [--out FILE]

CPU only, fixed seed, about a minute.  Every case is built from a target equilibrium temperature
T*, a density and a supersaturation s: q_tot = q_vs(T*, rho) (1 + s), e_int = the equilibrium energy
at T*.  rho is drawn in [0.3, 1.3]; a case with q_tot > 0.04 is drawn again (outside that box the
Newton recurrence of the law is no usable subject: it may still be iterating at step 40).

| group            | target                                               | cases |
| ice              | T* in 200 - 232.9 K                                  |  96   |
| mixed            | T* in 233.1 - 273.1 K                                | 128   |
| warm             | T* in 273.2 - 305 K                                  |  96   |
| near T_freeze    | T* within 1e-3 K of it                               |  48   |
| near T_icenuc    | T* within 1e-3 K of it                               |  48   |
| barely saturated | s in [1e-9, 1e-6], T* in 200 - 305 K                 |  32   |
| unsaturated      | relative humidity 0.2 - 0.999, T in 200 - 305 K      |  64   |
| clamped start    | T* in 200 - 225 K with so much ice that the all-vapour temperature, from which the
|                  | recurrence starts, lies below T_min = 150 K          |  16   |
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(HERE, "tests"), HERE]

SEED = 20240611
Q_TOT_MAX = 0.04
COUNTS = (96, 128, 96, 48, 48, 32, 64, 16)


def main():
    import mpmath as mp
    import moist_phase_restatement as R
    from cmdg_loader import cm
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=R.FIXTURE)
    args = ap.parse_args()
    k = R.constants(cm.moist.MoistParameters())
    rng = np.random.default_rng(SEED)
    Tf, Ti = k["T_freeze"], k["T_icenuc"]
    saturated = lambda: 10.0 ** rng.uniform(-3.0, -0.3)        # noqa: E731
    draw = [lambda: (rng.uniform(200.0, 232.9), saturated()),
            lambda: (rng.uniform(233.1, 273.1), saturated()),
            lambda: (rng.uniform(273.2, 305.0), saturated()),
            lambda: (Tf + rng.uniform(-1e-3, 1e-3), saturated()),
            lambda: (Ti + rng.uniform(-1e-3, 1e-3), saturated()),
            lambda: (rng.uniform(200.0, 305.0), 10.0 ** rng.uniform(-9.0, -6.0)),
            lambda: (rng.uniform(200.0, 305.0), rng.uniform(0.2, 0.999) - 1.0),
            lambda: (rng.uniform(200.0, 225.0), None)]
    cols = {n: [] for n in ("group",) + R.INPUTS + R.OUTPUTS}
    redrawn = 0
    with mp.workdps(R.DIGITS):
        c = R.exact(k)
        for g, n in enumerate(COUNTS):
            done = 0
            while done < n:
                Ts, s = draw[g]()
                rho = rng.uniform(0.3, 1.3)
                Tm, rm = mp.mpf(float(Ts)), mp.mpf(float(rho))
                if s is None:
                    q_tot = float(rng.uniform(0.02, Q_TOT_MAX))
                else:
                    q_tot = float(R.q_vs(c, Tm, rm) * (1 + mp.mpf(float(s))))
                if q_tot > Q_TOT_MAX:
                    redrawn += 1
                    continue
                e_int = float(R.e_int_equil(c, Tm, rm, mp.mpf(q_tot)))
                if s is None and not R.T_all_vapour(c, mp.mpf(e_int), mp.mpf(q_tot)) < k["T_min"] - 1:
                    redrawn += 1
                    continue
                out = R.answers(k, rho, q_tot, e_int)
                assert abs(out["T"] - Ts) < 1e-9, (g, Ts, out["T"])
                cols["group"].append(g)
                for name, v in zip(R.INPUTS, (rho, q_tot, e_int)):
                    cols[name].append(v)
                for name in R.OUTPUTS:
                    cols[name].append(out[name])
                done += 1
            print("%-17s %4d cases" % (R.GROUPS[g], n), flush=True)
    arrays = {n: np.asarray(v, dtype=np.int8 if n == "group" else np.float64) for n, v in cols.items()}
    np.savez(args.out, **arrays)
    print("wrote %s: %d cases (%d draws discarded), %d bytes" % (
        args.out, len(cols["group"]), redrawn, os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
