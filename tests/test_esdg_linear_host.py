"""The restatement of the entropy-stable IMEX chain (tests/esdg_linear_restatement.py) and the host
mirror (climatemachine.jl_amd/esdg.py) pinned to the reference's definitions: the linear law is the
derivative of the full law at the resting reference state, the operator is linear, the horizontal
operator carries no source, the wall reflects, an ARK2 step without a linear part is the explicit
tableau's step, the BaroclinicWave state is what its formulas say, and the stored table parses."""
import json
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from cmdg_loader import cm
import esdg_linear_restatement as LR
import esdg_restatement as R
from esdg_imex_cases import STATE_SCALE, brick, per_state_max_rel, random_state, sphere

E = cm.esdg
EPS = np.finfo(np.float64).eps
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rest_state(nodes=400, seed=5):
    """A resting reference state per node (DecayingTemperatureProfile at random altitudes) with random
    unit gradients of Phi, and its auxiliary columns."""
    ps = cm.atmos.PlanetParameters()
    rng = np.random.default_rng(seed)
    z = rng.uniform(0.0, 30e3, nodes)
    T, p = cm.atmos.DecayingTemperatureProfile(ps, 290.0, 220.0, 8e3)(z)
    rho = p / (ps.R_d * T)
    g = ps.cp_d / ps.cv_d
    k = rng.standard_normal((3, nodes))
    k /= np.sqrt((k * k).sum(axis=0))
    aux = [ps.grav * z, ps.grav * k[0], ps.grav * k[1], ps.grav * k[2], T, p, rho, p / (g - 1)]
    zero = np.zeros(nodes)
    return ps, [rho, zero, zero, zero, p / (g - 1)], aux, rng


def test_linear_law_is_the_derivative_of_the_full_law_at_rest():
    """Centred differences of the full law's ``flux_first_order!`` and Gravity source around the resting
    reference state, in random directions, against the linear law's flux and source.

    The bound is the finite-difference error, from the step alone.  Scale the state by (rho_0, rho_0 c_0,
    rho_0 c_0^2) with c_0 the reference sound speed; the perturbation direction has entries of at most 1
    in those units and the step is h.  Every flux entry is a product of the entries (1 + h r) and of
    1 / (1 + h r_rho), so its third derivative along the direction is bounded by 3! times the number of
    such products, at most 4 (rho u (rho e + p) / rho with p's kinetic part), times the largest
    coefficient gamma + 1 < 3: the centred difference is off by at most h^2 / 6 * 72 = 12 h^2 of the
    entry's scale.  Rounding adds (eps / h) times the entry of the unperturbed flux, which is at most
    gamma / (gamma - 1) + 1 < 5 scales (the enthalpy): 5 eps / h.  With h = 1e-5 that is 1.2e-9 + 1.1e-10."""
    ps, q0, aux, rng = _rest_state()
    g = ps.cp_d / ps.cv_d
    full = R.Law(ps.cp_d, ps.cv_d, sources=(R.GRAVITY,))
    lin = LR.LinearLaw(ps.cp_d, ps.cv_d)
    rho0, p0 = q0[0], aux[5]
    c0 = np.sqrt(g * p0 / rho0)
    unit = [rho0, rho0 * c0, rho0 * c0, rho0 * c0, rho0 * c0 * c0]
    r = rng.uniform(-1.0, 1.0, (5, len(rho0)))
    dq = [unit[s] * r[s] for s in range(5)]
    h = 1e-5
    bound = 12 * h * h + 5 * EPS / h
    qp = [q0[s] + h * dq[s] for s in range(5)]
    qm = [q0[s] - h * dq[s] for s in range(5)]
    Fp, Fm = full.flux_first_order(qp), full.flux_first_order(qm)
    FL = lin.flux_first_order(dq, aux)
    # the scale of a flux of state s: the state's unit times c_0
    worst = 0.0
    for d in range(3):
        for s in range(5):
            fd = (Fp[d][s] - Fm[d][s]) / (2 * h)
            err = np.max(np.abs(fd - FL[d][s]) / (unit[s] * c0))
            worst = max(worst, err)
            assert err <= bound, (d, s, err, bound)
    Sp, Sm = full.source(qp, aux), full.source(qm, aux)
    SL = lin.source(dq, aux, LR.VERTICAL)
    for s in range(5):
        fd = (Sp[s] - Sm[s]) / (2 * h)
        # a source of state s: the state's unit times grav (|grad Phi| = grav here)
        err = np.max(np.abs(fd - SL[s]) / (unit[s] * ps.grav))
        worst = max(worst, err)
        assert err <= bound, (s, err, bound)
    assert np.array_equal(np.stack(SL), np.stack(lin.source(dq, aux, LR.EVERY)))
    print("linearisation: worst scaled difference %.2e, bound %.2e" % (worst, bound))


def _operator(case, direction, nf=LR.RUSANOV, N=3, nvert=2):
    law, grid = case(N, nvert)
    aux = law.init_state_auxiliary(grid)
    ps = law.param_set
    return LR.DGRestatement(LR.LinearLaw(ps.cp_d, ps.cv_d), grid, aux, direction, nf), law, grid, aux


@pytest.mark.parametrize("case", [sphere, brick], ids=["sphere", "brick"])
@pytest.mark.parametrize("direction", [LR.VERTICAL, LR.HORIZONTAL, LR.EVERY])
def test_operator_is_linear(case, direction):
    """``L(a Q1 + b Q2) = a L(Q1) + b L(Q2)`` to rounding, per state.  A node's tendency is a sum of at most
    3 Nq volume terms, six face terms and the source, each a product of a handful of factors: fewer than
    64 roundings, each of at most eps times the sum of the magnitudes, which for these random fields is
    the size of |a| |L Q1| + |b| |L Q2| at its largest node -- 64 eps of that maximum, per state."""
    op, _, grid, _ = _operator(case, direction)
    Q1, Q2 = random_state(grid, 1), random_state(grid, 2)
    a, b = 0.75, -1.625
    T1, T2, T12 = np.zeros_like(Q1), np.zeros_like(Q1), np.zeros_like(Q1)
    op(T1, Q1)
    op(T2, Q2)
    op(T12, a * Q1 + b * Q2)
    size = np.max(abs(a) * np.abs(T1) + abs(b) * np.abs(T2), axis=(0, 2))
    err = np.max(np.abs(T12 - (a * T1 + b * T2)), axis=(0, 2))
    print("linearity: error / size per state", err / size)
    assert np.all(err <= 64 * EPS * size), err / size


def test_horizontal_operator_has_no_source():
    """``source!`` acts for the vertical and every-direction operators only: the horizontal one ignores the
    geopotential altogether."""
    op, law, grid, aux = _operator(sphere, LR.HORIZONTAL)
    ps = law.param_set
    q = [random_state(grid, 3)[:, s, :] for s in range(5)]
    a = [aux[:, c, :] for c in range(8)]
    L = LR.LinearLaw(ps.cp_d, ps.cv_d)
    assert all(np.all(S == 0) for S in L.source(q, a, LR.HORIZONTAL))
    assert any(np.any(S != 0) for S in L.source(q, a, LR.VERTICAL))
    aux2 = aux.copy()
    aux2[:, 0:4, :] *= 3.0
    op2 = LR.DGRestatement(L, grid, aux2, LR.HORIZONTAL)
    Q = random_state(grid, 3)
    T, T2 = np.zeros_like(Q), np.zeros_like(Q)
    op(T, Q)
    op2(T2, Q)
    assert np.array_equal(T, T2)


def test_wall_reflects_the_normal_momentum():
    rng = np.random.default_rng(4)
    n = rng.standard_normal((3, 50))
    n = list(n / np.sqrt((n * n).sum(axis=0)))
    qM = list(rng.standard_normal((5, 50)))
    qP = LR.LinearLaw(1004.0, 717.0).boundary_state(n, qM)
    mn = sum(qM[1 + d] * n[d] for d in range(3))
    pn = sum(qP[1 + d] * n[d] for d in range(3))
    assert np.allclose(pn, -mn, rtol=0, atol=8 * EPS * np.abs(mn).max())
    for d in range(3):      # the tangential part is the minus side's
        assert np.allclose(qP[1 + d] - pn * n[d], qM[1 + d] - mn * n[d], rtol=0, atol=16 * EPS * np.abs(qM[1 + d]).max())
    assert np.array_equal(qP[0], qM[0]) and np.array_equal(qP[4], qM[4])


@pytest.mark.parametrize("split", [False, True])
def test_ark2_step_without_a_linear_part_is_the_explicit_step(split):
    """With L = 0 the implicit solve is the identity and the low-storage stage vectors must collapse to
    ``Q + dt sum_j a_ij R_j``.  The operator here is the every-direction linear DG (any operator serves);
    dt makes ``dt |F|`` the size of the state for the stiffest state, so nothing hides behind a small step.  The stage
    vector is formed from O(1) multiples of Q that cancel: a few eps of |Q| per stage, carried through
    one more evaluation of size |Q| / dt: 64 eps of each state's maximum covers the three stages."""
    op, _, grid, _ = _operator(brick, LR.EVERY)
    Q0 = random_state(grid, 6)
    T = np.zeros_like(Q0)
    op(T, Q0)
    dt = float(np.min(np.max(np.abs(Q0), axis=(0, 2)) / np.max(np.abs(T), axis=(0, 2))))
    tab = LR.ark2gkc_tableau()
    want = LR.explicit_tableau_step(op, Q0, 0.0, dt, tab)
    got = LR.ark_step(op, None, None, Q0.copy(), 0.0, dt, tab, split)
    moved = per_state_max_rel(want, Q0)
    err = per_state_max_rel(got, want)
    print("moved", moved, "error", err)
    assert np.all(moved > 0.01)     # the step moves every state by far more than the bound
    assert np.all(err <= 64 * EPS), err


def test_baroclinic_wave_initial_state():
    """``p`` from the state is the analytic ``p``, ``rho = p / (R_d T_v)``, and the momentum carries the
    perturbation inside ``0 < d < d_0`` only.  4 x 4 elements per panel put nodes inside d_0 = a / 6.
    The pressure from the state subtracts a kinetic energy of at most 1e-2 of rho e: 16 eps relative."""
    problem = E.BaroclinicWave()
    law, grid = sphere(3, nvert=1, nhorz=4, problem=problem)
    ps = law.param_set
    aux = law.init_state_auxiliary(grid)
    Q = law.init_state_prognostic(grid, aux)
    assert Q.shape == (grid.nelem, 5, grid.Np) and np.isfinite(Q).all()
    coord = [grid.vgeo[:, c, :] for c in (12, 13, 14)]
    lam, phi, z, T_v, p, u_ref = problem.base_state(coord)
    g = ps.cp_d / ps.cv_d
    p_state = E.pressure(Q[:, 0], [Q[:, 1], Q[:, 2], Q[:, 3]], Q[:, 4], g)
    assert np.max(np.abs(p_state / p - 1)) <= 16 * EPS
    assert np.max(np.abs(Q[:, 0] * (ps.R_d * T_v) / p - 1)) <= 4 * EPS
    # the analytic fields are the test case's: surface pressure MSLP, equatorial surface temperature T_E
    surface = np.abs(z) < 1e-6
    assert np.allclose(p[surface], ps.MSLP, rtol=1e-12)
    up, vp, d = problem.perturbation(lam, phi, z)
    d_0 = ps.planet_radius / 6
    inside = (d > 0) & (d < d_0)
    assert inside.any() and (~inside).any()
    assert np.all(up[~inside] == 0) and np.all(vp[~inside] == 0)
    assert np.any(up[inside] != 0) and np.max(np.abs(up)) <= 1.0 and np.max(np.abs(vp)) <= 1.0
    # outside d_0 the flow is the zonal base flow: no meridional, no radial momentum
    rhat = [c / np.sqrt(coord[0] ** 2 + coord[1] ** 2 + coord[2] ** 2) for c in coord]
    radial = sum(Q[:, 1 + i] * rhat[i] for i in range(3))
    assert np.max(np.abs(radial)) <= 1e-12 * np.max(np.abs(Q[:, 1:4]))
    zonal = [-np.sin(lam), np.cos(lam), 0 * lam]
    speed = sum(Q[:, 1 + i] * zonal[i] for i in range(3)) / Q[:, 0]
    assert np.allclose(speed[~inside], u_ref[~inside], rtol=0, atol=1e-12 * np.abs(u_ref).max())


def test_python_surface():
    """The linear model refuses a model without a reference state (the reference's message), shares the
    full model's parameter block and auxiliary count; ``cubedshellwarp`` is DryAtmos.jl:827-860."""
    bare = E.DryAtmosModel(E.SphericalOrientation(), E.BaroclinicWave())
    with pytest.raises(ValueError, match="DryAtmosAcousticGravityLinearModel needs a model with a reference state"):
        E.DryAtmosAcousticGravityLinearModel(bare)
    law, _ = sphere(3, nvert=1)
    lin = E.DryAtmosAcousticGravityLinearModel(law)
    assert (lin.ns, lin.naux, lin.physics_id) == (5, 8, 14)
    assert all(np.array_equal(a, b) for a, b in zip(lin.descriptor(), law.descriptor()))

    def warp(a, b, c):          # the reference's scalar function, branch for branch
        R_ = max(abs(a), abs(b), abs(c))

        def f(sR, xi, eta):
            X, Y = math.tan(math.pi * xi / 4), math.tan(math.pi * eta / 4)
            x1 = sR / math.sqrt(X ** 2 + Y ** 2 + 1)
            return x1, X * x1, Y * x1

        fdim = int(np.argmax([abs(a), abs(b), abs(c)]))
        if fdim == 0 and a < 0:
            x1, x2, x3 = f(-R_, b / a, c / a)
        elif fdim == 1 and b < 0:
            x2, x1, x3 = f(-R_, a / b, c / b)
        elif fdim == 0 and a > 0:
            x1, x2, x3 = f(R_, b / a, c / a)
        elif fdim == 1 and b > 0:
            x2, x1, x3 = f(R_, a / b, c / b)
        elif fdim == 2 and c > 0:
            x3, x2, x1 = f(R_, b / c, a / c)
        else:
            x3, x2, x1 = f(-R_, b / c, a / c)
        return x1, x2, x3

    rng = np.random.default_rng(8)
    pts = rng.uniform(-1.0, 1.0, (60, 3))
    pts[np.arange(60), rng.integers(0, 3, 60)] = rng.choice([-1.0, 1.0], 60)     # on the cube's faces
    got = E.cubedshellwarp(pts[:, 0], pts[:, 1], pts[:, 2])
    want = np.array([warp(*p) for p in pts]).T
    assert np.allclose(np.stack(got), want, rtol=4 * EPS, atol=0)


def test_kernels_of_the_linear_law_use_no_scratch():
    """The built engine_esdg_linear.o: every ``k_tendency`` of the law and the column solver's substitution
    at its own order, ``k_band_solve<4, 5>`` (a window of 20 doubles per lane), keep to registers."""
    obj = os.path.join(ROOT, "climatemachine.jl_amd", "csrc", "engine_esdg_linear.o")
    tools = ("/opt/rocm/lib/llvm/bin/clang-offload-bundler", "/opt/rocm/lib/llvm/bin/llvm-readelf")
    if not os.path.exists(obj) or not all(os.path.exists(t) for t in tools) or shutil.which("objcopy") is None:
        pytest.skip("engine_esdg_linear.o is not built, or the code-object tools are not installed")
    out = subprocess.run(["bash", os.path.join(ROOT, "scripts", "kernel_resources.sh"), obj], capture_output=True,
                         text=True, check=True).stdout
    rows = [ln for ln in out.splitlines() if "k_tendency" in ln or "k_band_solve" in ln]
    assert sum("k_band_solveILi4ELi5E" in ln for ln in rows) == 1
    assert sum("k_tendency" in ln for ln in rows) >= 2
    for ln in rows:
        assert ln.rstrip().endswith("scratch 0"), ln


def test_reference_table_parses():
    with open(os.path.join(ROOT, "tests", "golden", "esdg_baroclinic_wave_refvals.json"), encoding="utf-8") as f:
        ref = json.load(f)
    assert [r[1] for r in ref["values"]] == ["ρ", "ρu[1]", "ρu[2]", "ρu[3]", "ρe"]
    assert len(ref["values"]) == 5 and all(len(r) == 6 for r in ref["values"])
    assert all(isinstance(v, float) for r in ref["values"] for v in r[2:])
    assert [r[:2] for r in ref["precision"]] == [r[:2] for r in ref["values"]]
    assert all(r[2:] == [12, 12, 12, 12] for r in ref["precision"])
    for r in ref["values"]:          # min <= mean <= max, std > 0
        assert r[2] <= r[4] <= r[3] and r[5] > 0
