"""Cases shared by the tests that pin the ocean laws and the column operators at every compiled
polynomial order (tests/test_integrals_orders_host.py, tests/test_ocean_orders_host.py,
tests/test_gpu_integrals_orders.py, tests/test_gpu_ocean_orders.py) and the bodies the N = 4 tests
of tests/test_gpu_ocean.py and tests/test_gpu_split_explicit.py share with them.

Two kinds of things live here.  (1) Inputs with closed forms, built in ``np.longdouble`` from the
grid's node coordinates alone: a column integrand whose antiderivative is a polynomial, and an
ocean state whose ``w``, ``wz0`` and ``pkin`` follow from hydrostatic_boussinesq_model.jl by hand.
Nothing of the oracle or of the kernels enters them.  (2) Comparison bodies, which take ``cm``,
``oracle`` and ``torch`` from the caller: this module imports neither at module level."""
import numpy as np

from helpers import (ocean_gyre_setup, ocean_spindown_setup, ocean_windstress_setup, rel_linf,
                     split_explicit_setup)

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
TOL = 1e-12

# ---- column integrals from exact antiderivatives --------------------------------------------------
INTEGRAL_ORDERS = (1, 2, 3, 4, 5, 6, 7)
INTEGRAL_NVERT = (1, 2, 5)
INTEGRAL_BOUND = 64 * EPS       # x max|exact|; 4 x the oracle's worst on these inputs (16.1 eps)
_THICKNESS = (0.30, 0.45, 0.45, 0.70, 0.45)     # cumulative 0.30, 0.75, 1.20, 1.90, 2.35
Z_BOTTOM, Z_TOP = -1.0, 2.0


def stacks_per_block(N):
    """SPB of csrc/columns.h: a 256-thread block walks 256 // Nq^2 stacks side by side."""
    return 256 // (N + 1) ** 2


def integral_stack_counts(N):
    """One short of a block, one over a block (the second block holds a single stack), and two
    full blocks."""
    spb = stacks_per_block(N)
    return (spb - 1, spb + 1, 2 * spb)


def column_grid(cm, N, nvert, nstacks, rank=0, size=1):
    """``nstacks`` x 1 x ``nvert`` elements, periodic laterally, walls in the vertical; layers of
    uneven thickness between z = -1 and z = 2."""
    M = cm.mesh
    cum = np.concatenate([[0.0], np.cumsum(_THICKNESS[:nvert])])
    z = Z_BOTTOM + (Z_TOP - Z_BOTTOM) * cum / cum[-1]
    z[0], z[-1] = Z_BOTTOM, Z_TOP
    rng = [np.linspace(0.0, 3.0, nstacks + 1), np.linspace(0.0, 3.0, 2), z]
    topl = M.StackedBrickTopology(rng, periodicity=(True, True, False),
                                  boundary=((0, 0), (0, 0), (1, 2)), rank=rank, size=size)
    return M.DiscontinuousSpectralElementGrid(topl, N)


def column_law(cm):
    """Any law compiled at N = 1..7 serves as the handle's: AdvectionDiffusion."""
    BL = cm.balancelaws
    return BL.AdvectionDiffusion(3, BL.Pseudo1D(np.ones(3) / np.sqrt(3), 1.0, 1 / 100, -1 / 2, 1 / 10),
                                 (BL.InhomogeneousBC(0), BL.InhomogeneousBC(1)))


def _poly(c, s):
    out = np.zeros_like(s)
    for p in range(len(c) - 1, -1, -1):
        out = out * s + c[p]
    return out


def _antiderivative(c):
    """coefficients of int_0^s sum_p c_p s^p"""
    return np.concatenate([[LD(0)], np.asarray(c, dtype=LD) / np.arange(1, len(c) + 1).astype(LD)])


def polynomial_column_case(grid, N):
    """f = (sum_p c_p z^p) (1 + sin(x) y), of degree exactly N in z, with
    c = default_rng(N).uniform(-1, 1, N + 1); evaluated in long double at the grid's nodes and
    rounded once.  Returns (f, upward integral, reverse integral) as float64 arrays (nelem, Np):
    (F(z) - F(z_bottom)) g and (F(z_top) - F(z)) g with F the antiderivative."""
    c = np.random.default_rng(N).uniform(-1, 1, N + 1).astype(LD)
    x, y, z = (np.asarray(grid.vgeo[:, 12 + d, :], dtype=LD) for d in range(3))
    g = 1 + np.sin(x) * y
    F = _antiderivative(c)
    Fz, Fb, Ft = _poly(F, z), _poly(F, np.asarray(LD(Z_BOTTOM))), _poly(F, np.asarray(LD(Z_TOP)))
    f = _poly(c, z) * g
    return (np.asarray(f, dtype=np.float64), np.asarray((Fz - Fb) * g, dtype=np.float64),
            np.asarray((Ft - Fz) * g, dtype=np.float64))


# aux columns of the one-output cases: upward integral, reverse integral, integrand, three that
# nothing may touch
COL_UP, COL_REV, COL_F, NAUX1 = 0, 1, 2, 6


def one_output_aux(grid, f):
    aux = np.full((grid.nelem, NAUX1, grid.Np), np.nan)
    aux[:, COL_F] = f
    return aux


def one_output_fields():
    """(src, scale, dst, rsrc, rdst) of the one-output cases"""
    return [(0, COL_F)], [1.0], [COL_UP], [COL_UP], [COL_REV]


def integral_errors(aux, nreal, up, rev):
    """(upward, reverse) largest error over the real elements in units of eps x max|exact|"""
    eu = np.abs(aux[:nreal, COL_UP] - up[:nreal]).max() / (EPS * np.abs(up[:nreal]).max())
    er = np.abs(aux[:nreal, COL_REV] - rev[:nreal]).max() / (EPS * np.abs(rev[:nreal]).max())
    return float(eu), float(er)


# many outputs: state and auxiliary integrands, a negative scale and 1e-3 among the first two, the
# second output integrated in place (its integrand's column is its destination), the first reversed
# in place
MANY_NS, MANY_NAUX = 3, 14
MANY_SRC = [(1, 0), (0, 1), (0, 13), (1, 1), (0, 12), (1, 2)]
MANY_SCALE = [-2.0, 1e-3, 0.5, 3.0, 1.0, 1.0]
MANY_DST = [0, 1, 2, 3, 4, 5]
MANY_RDST = [0, 7, 8, 9, 10, 11]


def many_output_case(grid, nout, seed=1):
    """(Q, aux, src, scale, dst, rdst, untouched aux columns): everything that is no integrand is
    NaN before the call."""
    rng = np.random.default_rng(seed)
    Q = rng.standard_normal((grid.nelem, MANY_NS, grid.Np))
    aux = np.full((grid.nelem, MANY_NAUX, grid.Np), np.nan)
    src, dst, rdst = MANY_SRC[:nout], MANY_DST[:nout], MANY_RDST[:nout]
    for st, col in src:
        if not st:
            aux[:, col] = rng.standard_normal((grid.nelem, grid.Np))
    used = set(dst) | set(rdst) | {col for st, col in src if not st}
    untouched = [c for c in range(MANY_NAUX) if c not in used]
    return Q, aux, src, MANY_SCALE[:nout], dst, rdst, untouched


# ---- the ocean's column composition against closed forms -------------------------------------------
ANALYTIC_ORDERS = (2, 3, 4, 5)
W_ORACLE_BOUND = 1e-11          # x max|w| on the centre stack: 17 x the oracle's worst (6.0e-13)
PKIN_BOUND = 64 * EPS           # x max|pkin|: the two kernels of the column integrals above, on an
                                # integrand that does not depend on z


def walled_box(name, N):
    """The 3 x 3 x 2 gyre / windstress box: the stack in the middle has interior lateral faces only."""
    setup = {"gyre": ocean_gyre_setup, "windstress": ocean_windstress_setup}[name]
    return setup(Nx=3, Ny=3, Nz=2, N=N)


def centre_stack(grid, L=1e6):
    """element indices of the stack in the middle of a 3 x 3 x nvert box of side L"""
    x, y = grid.vgeo[:grid.nreal, 12, :], grid.vgeo[:grid.nreal, 13, :]
    xm, ym = x.mean(axis=1), y.mean(axis=1)
    e = np.nonzero((xm > L / 3) & (xm < 2 * L / 3) & (ym > L / 3) & (ym < 2 * L / 3))[0]
    assert len(e) == grid.topology.stacksize
    return e


def analytic_ocean_case(law, grid, N):
    """u = p1(x/L) q1(z/H), v = p2(y/L) q2(z/H), eta = 0, theta = theta(x, y): p of degree N, q of
    degree max(N - 2, 0) (what CutoffFilter(grid, N - 1) keeps in the vertical), theta without
    vertical structure (what the exponential filter keeps).  With D.div_h u = du/dx + dv/dy,
    A.w = -div_h u integrated upwards from z = -H, pkin the integral of -alpha_T theta from z up to
    the surface, and wz0 the surface w through the column (hydrostatic_boussinesq_model.jl,
    update_auxiliary_state_gradient! and the integral_* / reverse_integral_* methods):
        w = -(p1'(x/L)/L int_{-H}^{z} q1 + p2'(y/L)/L int_{-H}^{z} q2),
        pkin = alpha_T theta z,     wz0 = w(x, y, 0).
    Returns (Q, w, wz0, pkin) as float64 arrays; the closed forms are evaluated in long double."""
    L, H = LD(law.problem.Lx), LD(law.problem.H)
    rng = np.random.default_rng(N)
    nq = max(N - 2, 0) + 1
    p1, p2 = (rng.uniform(-1, 1, N + 1).astype(LD) for _ in range(2))
    q1, q2 = (rng.uniform(-1, 1, nq).astype(LD) for _ in range(2))
    x, y, z = (np.asarray(grid.vgeo[:, 12 + d, :], dtype=LD) for d in range(3))
    xs, ys, zs = x / L, y / L, z / H
    deriv = lambda p: p[1:] * np.arange(1, len(p)).astype(LD)
    Q = np.zeros((grid.nelem, 4, grid.Np))
    Q[:, 0] = np.asarray(_poly(p1, xs) * _poly(q1, zs), dtype=np.float64)
    Q[:, 1] = np.asarray(_poly(p2, ys) * _poly(q2, zs), dtype=np.float64)
    theta = 9 + 2 * np.sin(2 * LD(np.pi) * xs) + np.cos(2 * LD(np.pi) * ys)
    Q[:, 3] = np.asarray(theta, dtype=np.float64)
    bottom = np.asarray(LD(-1))

    def w_at(s):
        I1 = H * (_poly(_antiderivative(q1), s) - _poly(_antiderivative(q1), bottom))
        I2 = H * (_poly(_antiderivative(q2), s) - _poly(_antiderivative(q2), bottom))
        return -(_poly(deriv(p1), xs) / L * I1 + _poly(deriv(p2), ys) / L * I2)

    w, wz0 = w_at(zs), w_at(np.zeros_like(zs))
    pkin = LD(law.alpha_T) * np.asarray(Q[:, 3], dtype=LD) * z
    f64 = lambda a: np.asarray(a, dtype=np.float64)
    return Q, f64(w), f64(wz0), f64(pkin)


def analytic_errors(aux, stack, w, wz0, pkin):
    """errors of aux columns w (1), pkin (2), wz0 (3) on ``stack`` relative to max|w| / max|pkin|"""
    sw = np.abs(w[stack]).max()
    out = {"w": float(np.abs(aux[stack, 1] - w[stack]).max() / sw),
           "wz0": float(np.abs(aux[stack, 3] - wz0[stack]).max() / sw)}
    sp = np.abs(pkin[stack]).max()
    if sp > 0:
        out["pkin"] = float(np.abs(aux[stack, 2] - pkin[stack]).max() / sp)
    return out


# ---- comparison bodies: the device against the oracle ----------------------------------------------
def to_gpu(torch, a):
    x = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return x


def perturbed_ocean_state(law, grid, aux, seed=5):
    Q = law.init_state_prognostic(grid, aux, 3600.0)
    rng = np.random.default_rng(seed)
    Q[:, 0:2] += 0.05 * rng.standard_normal(Q[:, 0:2].shape)
    Q[:, 3] = 10.0 + rng.standard_normal(Q[:, 3].shape)
    return Q


def oracle_ocean_model(cm, oracle, law, grid):
    """the oracle's operator with the hooks of the ocean driver: CutoffFilter(grid, N - 1) on u,
    ExponentialFilter(grid, 1, 8) on theta"""
    F = cm.mesh.filters
    odg = oracle.OracleDGModel(law, grid)
    oracle.hydrostatic_boussinesq_hooks(odg, F.CutoffFilter(grid, grid.N[-1] - 1),
                                        F.ExponentialFilter(grid, 1, 8))
    return odg


def close_ocean_model(dg, keep):
    dg.set_rhs_hooks()
    for f in keep:
        f.close()
    dg.close()


def check_ocean_tendency_and_aux(cm, oracle, torch, variant, N=4, alpha_beta=((1.0, 1.0),)):
    """One evaluation of the periodic 3 x 2 x 3 box with the law's hooks per (alpha, beta): Q after
    the in-place filters bit for bit, w / pkin / wz0, the tendency per state and the gradient flux
    at TOL."""
    O = cm.ocean
    law, grid = ocean_spindown_setup(Nx=3, Ny=2, Nz=3, N=N)
    law0 = law            # the analytic state is restated for the non-rotating box only
    if variant == "advection_rotating":
        law = O.HydrostaticBoussinesqModel(
            O.SimpleBox(1e6, 1e6, 400.0, rotation=O.ROTATING,
                        BC=(O.OceanBC(O.IMPENETRABLE_NOSLIP), O.OceanBC(O.PENETRABLE_FREESLIP))),
            momentum_advection=True, tracer_advection=True, c_h=1.0, c_z=0.1)
    odg = oracle_ocean_model(cm, oracle, law, grid)
    dg = cm.dgmodel.DGModel(law, grid)
    keep = O.install_hydrostatic_boussinesq_hooks(dg)
    Q0 = perturbed_ocean_state(law0, grid, odg.state_auxiliary)
    T0 = np.random.default_rng(1).standard_normal(Q0.shape)
    for alpha, beta in alpha_beta:
        Qo, To = Q0.copy(), T0.copy()
        odg(To, Qo, 0.0, alpha, beta)
        Qg, Tg = to_gpu(torch, Q0), to_gpu(torch, T0)
        dg(Tg, Qg, 0.0, alpha, beta)
        # the filters of update_auxiliary_state! act on Q itself
        assert np.array_equal(Qg.cpu().numpy(), Qo) and not np.array_equal(Qo, Q0)
        auxg = dg.state_auxiliary.cpu().numpy()
        for c, name in ((1, "w"), (2, "pkin"), (3, "wz0")):
            sc = max(np.abs(odg.state_auxiliary[:, c]).max(), 1e-300)
            assert np.abs(auxg[:, c] - odg.state_auxiliary[:, c]).max() / sc < TOL, name
        Tn = Tg.cpu().numpy()
        for s in range(4):
            assert rel_linf(Tn[:, s], To[:, s]) < TOL, s
        assert rel_linf(dg.state_gradient_flux.cpu().numpy(), odg.state_gradient_flux) < TOL
    close_ocean_model(dg, keep)


def check_ocean_courant(cm, oracle, torch, law, grid):
    """src/Ocean/HydrostaticBoussinesq/Courant.jl: the four local Courant numbers in the
    directions calculate_dt uses them, and the resulting time step."""
    dg = cm.dgmodel.DGModel(law, grid)
    odg = oracle.OracleDGModel(law, grid)
    Q0 = law.init_state_prognostic(grid, odg.state_auxiliary, 0.0)
    rng = np.random.default_rng(4)
    Q0[:, 0:2] = 0.05 * rng.standard_normal(Q0[:, 0:2].shape)
    w = 1e-3 * rng.standard_normal(Q0[:, 0].shape)
    odg.state_auxiliary[:, 1] = w
    dg.state_auxiliary[:, 1] = to_gpu(torch, w)
    Qg = to_gpu(torch, Q0)
    for kind in (0, 1, 2, 3):
        for d in (0, 1, 2):
            o = oracle.courant(kind, odg, Q0, 7.0, 0.0, d)
            g = dg.courant(kind, Qg, 7.0, 0.0, d)
            assert abs(g - o) <= 1e-13 * abs(o), (kind, d, g, o)
    dt_o = law.calculate_dt(lambda k, d: oracle.courant(k, odg, Q0, 1.0, 0.0, d), 0.4)
    dt_g = law.calculate_dt(lambda k, d: dg.courant(k, Qg, 1.0, 0.0, d), 0.4)
    assert abs(dt_g - dt_o) <= 1e-13 * dt_o
    dg.close()


def check_fused_columns_equal_sequence(cm, torch, monkeypatch, setups):
    """CMDG_FUSED_COLUMNS = 0 (the recorded operations one by one) against 2 (k_column_chain,
    k_flow_deviation, the paired vertical filter): three LSRK144 steps, state and every auxiliary
    column bit for bit.  ``setups``: callables returning (law, grid)."""
    O = cm.ocean
    for setup in setups:
        res = []
        for fused in ("0", "2"):
            monkeypatch.setenv("CMDG_FUSED_COLUMNS", fused)
            law, grid = setup()
            dg = cm.dgmodel.DGModel(law, grid)
            keep = O.install_hydrostatic_boussinesq_hooks(dg)
            rng = np.random.default_rng(9)
            Q0 = law.init_state_prognostic(grid, dg.state_auxiliary.cpu().numpy(), 0.0)
            Q0[:, 0:2] += 0.05 * rng.standard_normal(Q0[:, 0:2].shape)
            Q0[:, 3] += 0.1 * rng.standard_normal(Q0[:, 3].shape)
            Q = to_gpu(torch, Q0)
            solver = cm.odesolvers.LSRK144NiegemannDiehlBusch(dg, Q, dt=60.0)
            solver.dostep(Q, nsteps=3)
            dg.synchronize()
            res.append((Q.cpu().numpy().copy(), dg.state_auxiliary.cpu().numpy().copy()))
            close_ocean_model(dg, keep)
        nr = grid.nreal
        assert np.isfinite(res[0][0][:nr]).all()
        assert np.array_equal(res[0][0][:nr], res[1][0][:nr])
        assert np.array_equal(res[0][1][:nr], res[1][1][:nr])


def check_ocean_multirank_matches_single_rank(cm, torch, N=4, size=3):
    """Two LSRK144 steps of the periodic 4 x 3 x 3 box on ``size`` local ranks against one rank, at
    1e-11 per state."""
    O = cm.ocean
    RKA, RKB, RKC = cm.odesolvers.LSRK144_COEFFICIENTS
    law, grid = ocean_spindown_setup(Nx=4, Ny=3, Nz=3, N=N)
    dg1 = cm.dgmodel.DGModel(law, grid)
    k1 = O.install_hydrostatic_boussinesq_hooks(dg1)
    Q1h = perturbed_ocean_state(law, grid, dg1.state_auxiliary.cpu().numpy())
    gl1 = grid.topology.globalelems
    byglobal = {int(g): Q1h[i] for i, g in enumerate(gl1[:grid.nreal])}
    Q1 = to_gpu(torch, Q1h)
    dQ1 = torch.zeros_like(Q1)
    dg1.lsrk_run(Q1, dQ1, 0.0, 60.0, 2, RKA, RKB, RKC)
    dg1.synchronize()
    ref = {int(g): Q1[i].cpu().numpy() for i, g in enumerate(gl1[:grid.nreal])}
    dgs, Qs, grids, keeps = [], [], [], []
    for r in range(size):
        lawr, gridr = ocean_spindown_setup(Nx=4, Ny=3, Nz=3, N=N, rank=r, size=size)
        d = cm.dgmodel.DGModel(lawr, gridr)
        keeps.append(O.install_hydrostatic_boussinesq_hooks(d))
        q = np.full((gridr.nelem, 4, gridr.Np), np.nan)
        for i, g in enumerate(gridr.topology.globalelems[:gridr.nreal]):
            q[i] = byglobal[int(g)]
        dgs.append(d)
        grids.append(gridr)
        Qs.append(to_gpu(torch, q))
    cm.dgmodel.connect_local(dgs)
    dQs = [torch.zeros_like(q) for q in Qs]
    torch.cuda.synchronize()
    cm.dgmodel.group_lsrk_run(dgs, Qs, dQs, 0.0, 60.0, 2, RKA, RKB, RKC)
    for d in dgs:
        d.synchronize()
    for gr, q in zip(grids, Qs):
        qn = q.cpu().numpy()
        for i, g in enumerate(gr.topology.globalelems[:gr.nreal]):
            for s in range(4):
                sc = max(np.abs(ref[int(g)][s]).max(), 1e-6)
                assert np.abs(qn[i, s] - ref[int(g)][s]).max() / sc < 1e-11, (s, i)
    for d in dgs + [dg1]:
        d.set_rhs_hooks()
        d.close()
    return grids


# ---- split-explicit --------------------------------------------------------------------------------
def split_explicit_device_pair(cm, law3, g3, law2, g2):
    O = cm.ocean
    dg3 = cm.dgmodel.DGModel(law3, g3)
    keep = O.install_hydrostatic_boussinesq_hooks(dg3)
    dg2 = cm.dgmodel.DGModel(law2, g2, numerical_flux_first_order=cm.balancelaws.CentralNumericalFluxFirstOrder)
    return dg3, dg2, keep


def split_explicit_oracle_pair(cm, oracle, law3, g3, law2, g2):
    o3 = oracle_ocean_model(cm, oracle, law3, g3)
    o2 = oracle.OracleDGModel(law2, g2, nf_first=1)
    return o3, o2


def close_split_explicit_pair(dg3, dg2, keep):
    close_ocean_model(dg3, keep)
    dg2.close()


def scaled_linf(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def check_exchange_functions(cm, oracle, torch, N=4):
    """initialize_states! + tendency_from_slow_to_fast! and reconcile_from_fast_to_slow!
    (src/Ocean/SplitExplicit/Communication.jl) on the coupled 3 x 2 x 3 box."""
    law3, g3, law2, g2 = split_explicit_setup(True, Nx=3, Ny=2, Nz=3, N=N)
    o3, o2 = split_explicit_oracle_pair(cm, oracle, law3, g3, law2, g2)
    dg3, dg2, keep = split_explicit_device_pair(cm, law3, g3, law2, g2)
    rng = np.random.default_rng(7)
    Q3 = law3.init_state_prognostic(g3, o3.state_auxiliary, 1800.0)
    Q3[:, 0:2] += 0.05 * rng.standard_normal(Q3[:, 0:2].shape)
    Q2 = law2.init_state_prognostic(g2, o2.state_auxiliary, 1800.0)
    Q2[:, 1:3] += 5.0 * rng.standard_normal((g2.nelem, 2, 1, g2.Nq[0] * g2.Nq[1])).repeat(
        g2.Nq[2], axis=2).reshape(g2.nelem, 2, -1)
    dQ = rng.standard_normal(Q3.shape) * 1e-6
    Q3g, Q2g = to_gpu(torch, Q3), to_gpu(torch, Q2)
    se_o = oracle.SplitExplicitOracle(o3, o2, Q3, Q2, 1800.0, 300.0)
    se = cm.ocean.SplitExplicitSolver(dg3, dg2, Q3g, Q2g, 1800.0, 300.0)
    # initialize_states! + tendency_from_slow_to_fast!
    o3.state_auxiliary[:, 6:8] = 1.0
    dg3.state_auxiliary[:, 6:8] = 1.0
    torch.cuda.synchronize()
    se.initialize_states()
    se.tendency_from_slow_to_fast(to_gpu(torch, dQ))
    dg3.synchronize()
    o3.state_auxiliary[:, 6:8] = -0.0
    top = o3.integrate_velocity(dQ)
    se_o._v2(o2.state_auxiliary)[:, 1:3] = top[:, :, None, :]
    se_o._v3(o3.state_auxiliary)[:, :, 6:8] -= (top / se_o.H)[:, None, :, None, :]
    assert scaled_linf(dg2.state_auxiliary.cpu().numpy()[:, 1:3], o2.state_auxiliary[:, 1:3]) < TOL
    assert scaled_linf(dg3.state_auxiliary.cpu().numpy()[:, 6:8], o3.state_auxiliary[:, 6:8]) < TOL
    # reconcile_from_fast_to_slow!
    se.reconcile_from_fast_to_slow(Q3g, Q2g)
    dg3.synchronize()
    top = o3.integrate_velocity(Q3)
    du = 1 / se_o.H * (se_o._v2(Q2)[:, 1:3, 0, :] - top)
    se_o._v2(o2.state_auxiliary)[:, 3:5] = du[:, :, None, :]
    se_o._v3(Q3)[:, :, 0:2] += du[:, None, :, None, :]
    se_o._v3(Q3)[:, :, 2] = se_o._v2(Q2)[:, 0, 0, :][:, None, None, :]
    assert scaled_linf(dg2.state_auxiliary.cpu().numpy()[:, 3:5], o2.state_auxiliary[:, 3:5]) < TOL
    Qn = Q3g.cpu().numpy()
    assert scaled_linf(Qn[:, 0:2], Q3[:, 0:2]) < TOL
    assert np.array_equal(Qn[:, 2], Q3[:, 2]) and np.array_equal(Qn[:, 3], Q3[:, 3])
    # after the reconciliation the vertical mean of u is U / H
    top = o3.integrate_velocity(Qn)
    assert scaled_linf(top / se_o.H, se_o._v2(Q2)[:, 1:3, 0, :] / se_o.H) < 1e-11
    close_split_explicit_pair(dg3, dg2, keep)


def check_split_explicit_steps(cm, oracle, torch, coupled, dt_slow, N=4):
    """Three slow steps of the 3 x 2 x 3 box through cmdg_split_explicit_step against the oracle's
    SplitExplicitSolver."""
    law3, g3, law2, g2 = split_explicit_setup(coupled, Nx=3, Ny=2, Nz=3, N=N)
    o3, o2 = split_explicit_oracle_pair(cm, oracle, law3, g3, law2, g2)
    dg3, dg2, keep = split_explicit_device_pair(cm, law3, g3, law2, g2)
    Q3 = law3.init_state_prognostic(g3, o3.state_auxiliary, 0.0)
    Q2 = law2.init_state_prognostic(g2, o2.state_auxiliary, 0.0)
    Q3g, Q2g = to_gpu(torch, Q3), to_gpu(torch, Q2)
    se_o = oracle.SplitExplicitOracle(o3, o2, Q3, Q2, dt_slow, 300.0)
    se = cm.ocean.SplitExplicitSolver(dg3, dg2, Q3g, Q2g, dt_slow, 300.0)
    t = 0.0
    for _ in range(3):
        se_o.dostep(Q3, Q2, t)
        t += dt_slow
    se.dostep(Q3g, Q2g, 3)
    assert se.t == t and se.steps == 3
    A3, A2 = dg3.state_auxiliary.cpu().numpy(), dg2.state_auxiliary.cpu().numpy()
    Qn3, Qn2 = Q3g.cpu().numpy(), Q2g.cpu().numpy()
    for s in (0, 2):                      # u, eta (v stays at rounding level, theta is zero)
        assert scaled_linf(Qn3[:, s], Q3[:, s]) < TOL, s
    assert np.abs(Qn3[:, 1]).max() < 1e-12 and not Qn3[:, 3].any()
    for s in (0, 1):                      # eta, U
        assert scaled_linf(Qn2[:, s], Q2[:, s]) < TOL, s
    cols3 = (1, 3, 4, 6) if coupled else (1, 3)     # w, wz0, u_d, dG_u
    for c in cols3:
        tol = 1e-9 if c == 6 else TOL               # dG_u: see test_split_explicit_oracle.py
        assert scaled_linf(A3[:, c], o3.state_auxiliary[:, c]) < tol, c
    if coupled:
        assert scaled_linf(A2[:, 1], o2.state_auxiliary[:, 1]) < 1e-9      # G_U
        assert scaled_linf(A2[:, 3], o2.state_auxiliary[:, 3]) < 1e-9      # Delta_u, a difference
    close_split_explicit_pair(dg3, dg2, keep)
