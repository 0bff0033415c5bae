"""Orders other than N = 4 on a partition and under the fused LSRK update (``-m gpu``).

The pass kernels change shape with the order: from N = 5 up two elements share a work-group
(``TendencyShape::EPB == 2``: thread-to-element split through ``NTE``, no LDS staging of the minus
side, a dead second sub-element at the end of an odd list, ``send_nodes`` striding by ``NTE``); below
N = 3 the face-task threads outnumber the nodes; for ``NQ != NQV`` the face tables and the ghost
slots (``(eP - nreal) * Np + vidP``) use other strides.  Every case here runs such an order on a
partition of one process (local transport) and makes three comparisons:

1. ``group_lsrk_run`` with the default direct exchange against the same run with
   ``OPT_REFERENCE_HALO``: the same bits, ghost elements of Q never read (NaN) where the law
   receives directly, and the pack / unpack launch counts of the N = 4 tests;
2. the direct run against the CPU oracle on the whole, unpartitioned grid, element by element
   through ``topology.globalelems``, per state column;
3. ``group_rhs`` with ``alpha, beta = 0.5, 2.0`` and a random old tendency against the oracle, with
   ``state_gradient_flux`` where the law forms it.

Tolerances: 1e-12 for tendencies, gradient fluxes and advection-diffusion steps; 1e-11 for the
atmosphere laws after LSRK steps (as test_gpu_orders.py grants at N = 6).  The Smagorinsky law's
gradient flux is compared with the oracle's operator applied to the theta_v the device holds, and
that theta_v with the oracle's in units in the last place (``_Case.oracle_gradient_flux``): the N^2
column differentiates theta_v, and the last place of theta_v alone is worth 1e-12 of it.  The observed maxima are
recorded with ``helpers.observe``.  Each case asserts, before anything is launched, the elements per
work-group its order compiles to and the interior / exterior list lengths that make it hit the
edge (an empty interior list, odd lists, a last work-group with one live element).
"""
import numpy as np
import pytest

from helpers import (bomex_setup, held_suarez_setup, observe, pseudo1d_setup, rel_linf,
                     rising_bubble_setup, variable_degree_setup)
from test_gpu_halo_direct import _run_group
from test_gpu_split_explicit import _partitioned_pair_against_single_rank

pytestmark = pytest.mark.gpu
TOL = 1e-12          # tendencies, gradient fluxes, advection-diffusion steps
TOL_ATMOS = 1e-11    # atmosphere laws after LSRK steps
ALPHA, BETA = 0.5, 2.0
# theta_v = R_m / R_d * T / (p / p_0)^kappa on the device against the host: ``pow`` comes from two
# libraries, each within a unit in the last place of the exact value (two between them); T reaches it
# through a difference and a quotient that one compiler may contract into fused multiply-adds and
# the other not (one unit for T, one for the quotient by the Exner function)
THETA_V_ULPS = 4


def _gpu(torch, a):
    x = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return x


def _epb(N):
    return 2 if N >= 5 else 1


class _Case:
    """One law at one order on ``size`` ranks.  ``setup(rank, size) -> (law, grid)``;
    ``lists[rank] = (len(interiorelems), len(exteriorelems))``; ``Q0`` and ``T0`` live on the whole
    grid and are scattered to the ranks by global element number, ghosts included."""

    def __init__(self, cm, oracle, torch, tag, setup, size, lists, epb, modes=(1, 1),
                 gradflux=True, model_kw=None, perturb=None, t_rhs=0.2, theta_v=False, flux=None):
        self.cm, self.oracle, self.torch, self.tag = cm, oracle, torch, tag
        self.setup, self.size, self.lists, self.epb, self.modes = setup, size, lists, epb, modes
        self.gradflux, self.kw, self.t_rhs = gradflux, dict(model_kw or {}), t_rhs
        self.theta_v = theta_v        # the gradient pass differentiates aux.moisture.theta_v
        # the first-order numerical flux, where it is not the default: the two models name it differently
        self.okw = dict(self.kw, **({} if flux is None else {"nf_first": flux}))
        self.dkw = dict(self.kw, **({} if flux is None else {"numerical_flux_first_order": flux}))
        self.law, self.grid = setup(0, 1)
        assert self.grid.nreal == self.grid.nelem
        self.odg = oracle.OracleDGModel(self.law, self.grid, **self.okw)
        rng = np.random.default_rng(self.grid.N[0] + 10 * self.grid.N[-1])
        self.Q0 = self.law.init_state_prognostic(self.grid, self.odg.state_auxiliary, 0.0)
        if perturb is not None:
            perturb(self.Q0, rng)
        self.T0 = rng.standard_normal(self.Q0.shape)
        self.pos = {int(g): i for i, g in enumerate(self.grid.topology.globalelems)}
        assert sum(setup(r, size)[1].nreal for r in range(size)) == self.grid.nreal

    def rows(self, grid, real_only=True):
        """Rows of a whole-grid array that hold the elements of a rank's grid, in its order."""
        gl = grid.topology.globalelems
        return np.array([self.pos[int(g)] for g in (gl[:grid.nreal] if real_only else gl)])

    def make(self, rank, size):
        """The rank's handle, its preconditions asserted on the host."""
        law, grid = self.setup(rank, size)
        assert (len(grid.interiorelems), len(grid.exteriorelems)) == self.lists[rank], self.tag
        dg = self.cm.dgmodel.DGModel(law, grid, **self.dkw)
        assert dg.query("TENDENCY_ELEMS_PER_GROUP") == self.epb, self.tag
        return law, grid, dg

    def initial(self, grid, dg=None):
        """The case's initial state on a rank's elements, ghosts included (``_run_group``'s ``init``)."""
        return _gpu(self.torch, self.Q0[self.rows(grid, real_only=False)])

    def oracle_gradient_flux(self, parts):
        """The oracle's gradient flux for comparison 3.  For the Smagorinsky law column 9 is
        N^2 = grad(theta_v) . grad(Phi) / theta_v, and theta_v, about 300 K, varies by hundredths of
        a kelvin from node to node: one unit in its last place (5.7e-14 K) at the nodes of a line
        moves the derivative by up to ulp * ||D||_inf * 2 / h, 9e-13 of the column's maximum at
        N = 6 here.  Against the oracle's own theta_v the device's N^2 is 1.008e-12 off at N = 6 and
        6.0e-13 at N = 5, the other nine columns bit-equal.  So the two halves are pinned
        separately: the theta_v the device's nodal refresh leaves is within THETA_V_ULPS of the
        oracle's, and the oracle evaluates its gradient pass once more on that theta_v (it reads
        the column of the auxiliary state, as the reference does) -- what the kernel adds to its
        input is then held to 1e-12 like every other column.  Observed: theta_v differs by at most
        one unit in the last place at both orders; N^2 on the device's theta_v 3.2e-13 (N = 5) and
        5.0e-13 (N = 6).  The rest is not traced: the device's gradient pass evaluates theta_v
        from (Q, aux) itself instead of reading the column, and may round it differently there."""
        odg = self.odg
        if not self.theta_v:
            return odg.state_gradient_flux.copy()
        col = self.law.off_moist
        own = odg.state_auxiliary[:, col].copy()
        held = np.full_like(own, np.nan)
        for _, grid, dg in parts:
            held[self.rows(grid)] = dg.state_auxiliary[:grid.nreal, col].cpu().numpy()
        ulps = np.abs(held - own) / np.spacing(np.abs(own))
        assert self.observe("theta_v, units in the last place", ulps.max()) <= THETA_V_ULPS

        def refresh(dgm, Q, t, which):
            dgm.update_auxiliary_state_hook = None
            dgm.update_auxiliary_state(Q, t, which)
            dgm.update_auxiliary_state_hook = refresh
            dgm.state_auxiliary[:, col] = held

        odg.update_auxiliary_state_hook = refresh
        odg(self.T0.copy(), self.Q0.copy(), self.t_rhs, ALPHA, BETA)
        odg.update_auxiliary_state_hook = None
        return odg.state_gradient_flux.copy()

    def observe(self, what, value):
        return observe("orders_partitioned %s size=%d: %s" % (self.tag, self.size, what), value)

    def check_group_rhs(self):
        """Comparison 3; the handles answer DIRECT_SEND / DIRECT_RECV before the launch."""
        cm, torch, odg = self.cm, self.torch, self.odg
        To = self.T0.copy()
        odg(To, self.Q0.copy(), self.t_rhs, ALPHA, BETA)
        parts = [self.make(r, self.size) for r in range(self.size)]
        dgs = [p[2] for p in parts]
        Qs, Ts = [], []
        for _, grid, dg in parts:
            q = self.initial(grid)
            if self.modes[1]:
                q[grid.nreal:] = float("nan")
            Qs.append(q)
            Ts.append(_gpu(torch, self.T0[self.rows(grid, real_only=False)]))
        torch.cuda.synchronize()
        cm.dgmodel.connect_local(dgs)
        for dg in dgs:
            assert (dg.query("DIRECT_SEND"), dg.query("DIRECT_RECV")) == self.modes, self.tag
            assert bool(dg.query("GRADFLUX_LIVE")) == self.gradflux, self.tag
        cm.dgmodel.group_rhs(dgs, Ts, Qs, self.t_rhs, ALPHA, BETA)
        gfo = self.oracle_gradient_flux(parts) if self.gradflux else None
        for (law, grid, dg), T in zip(parts, Ts):
            nr, rows = grid.nreal, self.rows(grid)
            Tn = T[:nr].cpu().numpy()
            assert np.isfinite(Tn).all()
            for s in range(law.ns):
                assert self.observe("group_rhs", rel_linf(Tn[:, s], To[rows, s])) < TOL, s
            if self.gradflux:
                gf = dg.state_gradient_flux[:nr].cpu().numpy()
                for s in range(law.ngradflux):
                    assert self.observe("gradient flux", rel_linf(gf[:, s], gfo[rows, s])) < TOL, s
        for dg in dgs:
            dg.close()

    def oracle_steps(self, nsteps, dt):
        Qo, dQo = self.Q0.copy(), np.zeros_like(self.Q0)
        for i in range(nsteps):
            self.oracle.lsrk54_step(self.odg, Qo, dQo, i * dt, dt)
        return Qo

    def check_steps(self, nsteps, dt, tol, Qo=None):
        """Comparisons 1 and 2."""
        cm, torch = self.cm, self.torch
        nan = bool(self.modes[1])
        direct, gh_d, modes_d, n_d = _run_group(cm, torch, self.make, self.size, nsteps, dt,
                                                reference=False, nan_ghosts=nan, init=self.initial)
        ref, _, modes_r, n_r = _run_group(cm, torch, self.make, self.size, nsteps, dt,
                                          reference=True, nan_ghosts=nan, init=self.initial)
        assert modes_d == self.modes and modes_r == (0, 0), self.tag
        for a, b in zip(direct, ref):
            assert np.isfinite(a).all()
            assert np.array_equal(a, b)
        assert n_d["PACK"] == 1, n_d
        if self.modes[1]:
            assert n_d["UNPACK"] == 0, n_d
            assert all(np.isnan(g).all() for g in gh_d)          # nothing unpacked
        else:
            assert n_d["UNPACK"] == n_r["UNPACK"] == n_r["PACK"], (n_d, n_r)
        assert n_r["PACK"] == n_r["UNPACK"] > 1 and n_d["TRANSPORT"] == n_r["TRANSPORT"], (n_d, n_r)
        Qo = self.oracle_steps(nsteps, dt) if Qo is None else Qo
        for r, q in enumerate(direct):
            rows = self.rows(self.setup(r, self.size)[1])
            for s in range(self.law.ns):
                assert self.observe("%d steps" % nsteps, rel_linf(q[:, s], Qo[rows, s])) < tol, (r, s)


# ---- A. advection-diffusion -----------------------------------------------------------------
@pytest.mark.parametrize("N,size", [(1, 2), (2, 2), (3, 2), (5, 2), (6, 2), (7, 2), (5, 3), (7, 3)])
def test_advection_diffusion_orders_on_a_partition(cm, oracle, torch, N, size):
    """Size 2: real / interior / exterior = 12 / 3 / 9 and 15 / 0 / 15 (an empty interior list, odd
    exterior lists, at EPB = 2 a last work-group with one live element); size 3: 9 / 0 / 9 on all
    ranks.  N = 1, 2: more face-task threads than nodes."""
    dt = pseudo1d_setup(Ne=3, N=N)[2]
    case = _Case(cm, oracle, torch, "advdiff N=%d" % N,
                 lambda r, s: pseudo1d_setup(Ne=3, N=N, direction=0, rank=r, size=s)[:2], size,
                 lists={2: [(3, 9), (0, 15)], 3: [(0, 9)] * 3}[size], epb=_epb(N),
                 model_kw=dict(direction=0),
                 perturb=lambda Q, rng: Q.__iadd__(1e-3 * rng.standard_normal(Q.shape)))
    case.check_group_rhs()
    case.check_steps(3, dt, TOL)


# ---- B. Held-Suarez with hyperdiffusion -----------------------------------------------------
def _perturb_winds(scale):
    def perturb(Q, rng):
        Q[:, 1:4] += Q[:, 0:1] * scale * rng.standard_normal(Q[:, 1:4].shape)
    return perturb


@pytest.mark.parametrize("N", [2, 3, 5, 6])
def test_held_suarez_orders_fused_update_and_partition(cm, oracle, torch, N):
    """``k_tendency<DryAtmos<true,true,true>, NQ, NQ, LSRK = true>``: first the single-rank
    ``lsrk_run`` against the oracle (the fused update, at EPB = 2 for N >= 5, where the gradient
    arguments are not handed on), then three ranks of the cubed sphere with interior / exterior lists
    of 5 / 13, 1 / 17 and 6 / 12 elements: grids of 1 to 17 work-groups (fewer than 8 and no
    multiple of 8 for the XCD remap), both lists odd on one rank; four exchanges per stage."""
    nsteps, dt = 2, 2.0
    case = _Case(cm, oracle, torch, "heldsuarez N=%d" % N,
                 lambda r, s: held_suarez_setup(3, 1, N=N, rank=r, size=s)[:2], 3,
                 lists=[(5, 13), (1, 17), (6, 12)], epb=_epb(N), gradflux=False,
                 model_kw=dict(direction=0, diffusion_direction=1), perturb=_perturb_winds(2.0))
    Qo = case.oracle_steps(nsteps, dt)
    dg = cm.dgmodel.DGModel(case.law, case.grid, **case.kw)
    assert dg.query("TENDENCY_ELEMS_PER_GROUP") == _epb(N)
    Q = _gpu(torch, case.Q0)
    dQ = torch.zeros_like(Q)
    dg.lsrk_run(Q, dQ, 0.0, dt, nsteps, oracle.RKA, oracle.RKB, oracle.RKC)
    dg.synchronize()
    if N >= 5:
        assert dg.query("GRADARG_HANDOFF") == 0                   # the hand-off is for EPB = 1 only
    Qn = Q.cpu().numpy()
    for s in range(5):
        assert observe("orders_partitioned heldsuarez N=%d size=1: %d steps" % (N, nsteps),
                       rel_linf(Qn[:, s], Qo[:, s])) < TOL_ATMOS, s
    dg.close()
    case.check_group_rhs()
    case.check_steps(nsteps, dt, TOL_ATMOS, Qo=Qo)


# ---- C. Smagorinsky bubble --------------------------------------------------------------------
@pytest.mark.parametrize("N", [5, 6])
def test_smagorinsky_bubble_orders_on_a_partition(cm, oracle, torch, N):
    """The gradient flux is live, exchanged, and read on the plus side from the receive buffer at
    EPB = 2; exterior lists of 12 and 15 elements, empty interior lists.  The N^2 column of the
    gradient flux is compared on the theta_v the device holds (``_Case.oracle_gradient_flux``)."""
    case = _Case(cm, oracle, torch, "bubble N=%d" % N,
                 lambda r, s: rising_bubble_setup(nx=3, ny=3, nz=3, N=N, rank=r, size=s), 2,
                 lists=[(0, 12), (0, 15)], epb=2, perturb=_perturb_winds(3.0), theta_v=True)
    case.check_group_rhs()
    case.check_steps(2, 0.02, TOL_ATMOS)


# ---- D. BOMEX -----------------------------------------------------------------------------------
def test_bomex_order_six_on_a_partition(cm, oracle, torch):
    """The moist law at its other order: direct send, unpacked receive (its nodal refresh runs on
    the ghost elements, which therefore keep their values), exterior lists of 9 and 9 elements.
    The saturation adjustment is iterated to convergence, as in test_gpu_moist.py."""
    def setup(r, s):
        law, grid = bomex_setup(nx=3, ny=2, nz=3, N=6, rank=r, size=s)
        law.maxiter, law.tolerance = 40, 1e-11
        return law, grid

    def perturb(Q, rng):
        Q[:, 1:4] += Q[:, 0:1] * 0.5 * rng.standard_normal(Q[:, 1:4].shape)
        Q[:, 5] *= 1 + 0.05 * rng.random(Q[:, 5].shape)          # some cloud

    case = _Case(cm, oracle, torch, "bomex N=6", setup, 2, lists=[(0, 9), (0, 9)], epb=2,
                 modes=(1, 0), perturb=perturb)
    case.check_group_rhs()
    case.check_steps(2, 0.01, TOL_ATMOS)


# ---- E. mixed orders ----------------------------------------------------------------------------
@pytest.mark.parametrize("orders", [(4, 2), (2, 4)])
def test_mixed_order_ghosts_on_a_partition(cm, oracle, torch, orders):
    """polynomialorder = (N_h, N_v) on two ranks (16 interior and 16 exterior elements each): the
    three-branch face task, face tables whose stride differs from the per-face counts, and ghost
    slots of a mixed-order element."""
    def setup(r, s):
        law, grid, _ = variable_degree_setup(1, orders, "horizontal", rank=r, size=s)
        law.problem.n = np.ones(3) / np.sqrt(3)                  # flow across every face
        return law, grid

    dt = variable_degree_setup(1, orders, "horizontal")[2]
    case = _Case(cm, oracle, torch, "advdiff N=(%d,%d)" % orders, setup, 2,
                 lists=[(16, 16), (16, 16)], epb=1,
                 perturb=lambda Q, rng: Q.__iadd__(1e-2 * rng.standard_normal(Q.shape)))
    case.check_group_rhs()
    case.check_steps(3, dt, TOL)


def test_split_explicit_barotropic_two_node_extrusion_on_a_partition(cm, torch, monkeypatch):
    """The (4, 1) barotropic handle on two ranks.  The oracle has no stepper for the partitioned
    split-explicit pair, so the reference here is the single-rank device pair, with the comparison
    and the tolerance of test_partitioned_split_explicit_matches_single_rank."""
    monkeypatch.setenv("CMDG_HALO_PRIORITY", "0")

    def before_launch(rank, slow, fast):
        assert tuple(fast.grid.N) == (4, 4, 1)
        assert (len(slow.grid.interiorelems), len(slow.grid.exteriorelems)) == (0, 18)
        assert (len(fast.grid.interiorelems), len(fast.grid.exteriorelems)) == (0, 6)
        assert slow.query("TENDENCY_ELEMS_PER_GROUP") == 1 and fast.query("TENDENCY_ELEMS_PER_GROUP") == 1
        assert (slow.query("DIRECT_SEND"), slow.query("DIRECT_RECV")) == (1, 0)      # hooks: unpacked
        assert (fast.query("DIRECT_SEND"), fast.query("DIRECT_RECV")) == (1, 1)

    _partitioned_pair_against_single_rank(cm, torch, 2, N_extrusion=1, before_launch=before_launch)
