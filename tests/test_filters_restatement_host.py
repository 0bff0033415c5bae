"""The independent restatement of the element filters (tests/filters_restatement.py) on the host:
  * the host's filter matrices (mesh/filters.py) against the 40-digit ones at N = 1 .. 7, inside the
    entrywise bound ``c eps |V| |Sigma| |V^-1|`` with ``c`` the operation count of the host construction,
    and ``grid.xi`` against the 40-digit LGL nodes to 1 ulp;
  * the twin oracle (oracle/filter_oracle.c) against the restatement on the whole case table that
    tests/test_gpu_filters_orders.py runs on the device: every node inside its bound, and the largest
    error / bound ratio at most 0.5 (a bound the oracle fills further than that is a bound derived wrongly).
The case table lives here (``CASES``, ``build_case``) so that host and device run the same cases.  CPU only."""
import functools
import math

import numpy as np
import pytest

import filters_restatement as R
from cmdg_loader import cm
from helpers import held_suarez_setup, observe

M = cm.mesh
F = cm.mesh.filters
BL = cm.balancelaws
EVERY, HORZ, VERT = 0, 1, 2
EPS = float(np.finfo(np.float64).eps)
ATMOS_ENGINE_ORDERS = (2, 3, 4, 5, 6)       # the dry-atmosphere engine is compiled at these orders


# ---- filter matrices ------------------------------------------------------------------------------------
def _one_element(N):
    topl = M.BrickTopology([np.linspace(-1.0, 1.0, 2)] * 3, periodicity=(True,) * 3)
    return M.DiscontinuousSpectralElementGrid(topl, N)


@functools.lru_cache(maxsize=None)
def _nodes(N):
    grid = _one_element(N)
    return grid, R.lgl_nodes(N, grid.xi[0])


def _matrix_cases():
    out = []
    for N in range(1, 8):
        for Nc, s in sorted({(0, 32), (0, 4), (min(1, N - 1), 8), (N - 1, 2)}):
            out.append(("ExponentialFilter", N, Nc, s))
        for Nc, s in sorted({(0, 32), (N - 1, 4)}):
            out.append(("BoydVandevenFilter", N, Nc, s))
        for Nc in sorted({0, N // 2, N - 1, N}):
            out.append(("CutoffFilter", N, Nc, None))
        for Nc in sorted({0, N - 1, N, N + 1, N + 3}):
            out.append(("MassPreservingCutoffFilter", N, Nc, None))
    return out


# roundings on the way to one entry of the host matrix: the orthonormal recurrence (a division and a
# square root for its coefficient, two products, a difference, a quotient per degree), sigma, the
# scaling of V by Sigma, and the solve (factorisation, forward and back substitution: three dot
# products of N + 1 terms)
SIGMA_OPS = {"ExponentialFilter": 4, "BoydVandevenFilter": 12, "CutoffFilter": 0, "MassPreservingCutoffFilter": 0}


def _host_op_count(cls, N):
    return 6 * N + SIGMA_OPS[cls] + 1 + 3 * (N + 1)


@pytest.mark.parametrize("N", range(1, 8))
def test_reference_points_are_the_lgl_nodes(N):
    grid, x = _nodes(N)
    want = R.to_float64(x)
    for d in range(3):
        xi = np.asarray(grid.xi[d])
        assert np.all(np.diff(xi) > 0)
        assert np.all(np.abs(xi - want) <= np.spacing(np.abs(want))), (xi - want)


@pytest.mark.parametrize("cls,N,Nc,s", _matrix_cases())
def test_host_filter_matrix_within_entrywise_bound(cls, N, Nc, s):
    grid, x = _nodes(N)
    filt = getattr(F, cls)(grid, Nc) if s is None else getattr(F, cls)(grid, Nc, s)
    sigma = {"ExponentialFilter": lambda: R.sigma_exponential(s, -math.log(EPS)),
             "BoydVandevenFilter": lambda: R.sigma_boyd_vandeven(s)}.get(cls, lambda: R.sigma_cutoff)()
    W, B = R.filter_matrix(x, Nc, sigma, modified=cls == "MassPreservingCutoffFilter")
    W, B = R.to_float64(W), R.to_float64(B)
    c = _host_op_count(cls, N)
    for A in filt.filter_matrices:
        err = np.abs(np.asarray(A) - W)
        assert np.all(err <= c * EPS * B + np.spacing(np.abs(W)) / 2), (err / EPS).max()   # (+ rounding W to double)
        observe("filter matrix |host - 40 digits| / eps, N = %d" % N, err.max() / EPS)
    if Nc > N:
        assert np.array_equal(filt.filter_matrices[0], np.eye(N + 1))


def test_restatement_rejects_what_the_reference_rejects():
    _, x = _nodes(3)
    with pytest.raises(AssertionError):
        R.filter_matrix(x, 4, R.sigma_cutoff)             # spectral_filter_matrix: 0 <= Nc <= N
    with pytest.raises(TypeError):
        R.filter_matrix(x, 3, R.sigma_exponential(4, 36.0))   # eta = 0 / 0 has no exponential


# ---- the case table -------------------------------------------------------------------------------------
class ReferenceColumns:
    """A perturbation target on two named columns of the auxiliary state: what
    ``AtmosFilterPerturbations`` / ``AtmosSpecificFilterPerturbations`` hand to the library
    (``target_id``, ``indices``, ``aux_offsets()``), for a handle whose law is not the dry atmosphere."""
    indices = (1, 2, 3, 4, 5)

    def __init__(self, target_id, c_rho, c_rhoe):
        self.target_id, self._cols = target_id, (c_rho, c_rhoe)

    def aux_offsets(self):
        return self._cols


@functools.lru_cache(maxsize=None)
def brick_setup(N):
    """A 3 x 1 x 3 brick, periodic in x and y, with unequal element widths: 9 elements (not a multiple
    of 8), masses that differ between elements.  Returns ``(law, grid, aux, targets)``: at the orders of
    the dry-atmosphere engine the rising-bubble law and its hydrostatic reference state, with the
    library's own target classes; at N = 1 and 7 the advection-diffusion law, two columns of whose
    auxiliary state are filled with smooth positive fields of physical size (rho ~ 1, rho e ~ 2e5), and
    ``ReferenceColumns`` targets naming them."""
    rng = [np.array([0.0, 300.0, 1000.0, 1500.0]), np.array([0.0, 500.0]), np.array([0.0, 200.0, 700.0, 1500.0])]
    topl = M.StackedBrickTopology(rng, periodicity=(True, True, False), boundary=((0, 0), (0, 0), (1, 2)))
    grid = M.DiscontinuousSpectralElementGrid(topl, N)
    if N in ATMOS_ENGINE_ORDERS:
        A = cm.atmos
        ps = A.PlanetParameters()
        law = A.DryAtmosModel(A.RisingBubbleSetup(ps, xc=750.0, zc=300.0, rc=300.0), orientation=A.ORIENT_FLAT,
                              ref_state=A.DryAdiabaticProfile(ps, 300.0, 0.0), smagorinsky=ps.C_smag,
                              sources=A.SRC_GRAVITY, boundary_conditions=(A.BC_ATMOS_DEFAULT, A.BC_ATMOS_DEFAULT),
                              param_set=ps)
        aux = law.init_state_auxiliary(grid)
        targets = {"pert": F.AtmosFilterPerturbations(law), "specific": F.AtmosSpecificFilterPerturbations(law)}
    else:
        law = BL.AdvectionDiffusion(3, BL.Pseudo1D(np.ones(3) / np.sqrt(3), 1.0, 1 / 100, -1 / 2, 1 / 10),
                                    (BL.InhomogeneousBC(0), BL.InhomogeneousBC(1)))
        aux = law.init_state_auxiliary(grid)
        assert aux.shape[1] >= 2
        x, z = grid.vgeo[:, 12, :], grid.vgeo[:, 14, :]
        c_rho, c_rhoe = aux.shape[1] - 1, 0
        aux[:, c_rho] = 1.0 + 0.1 * np.sin(2 * np.pi * x / 1500.0) * np.cos(np.pi * z / 1500.0) - 2e-4 * z
        aux[:, c_rhoe] = 2e5 * (1.0 + 0.05 * np.cos(2 * np.pi * x / 1500.0 + z / 700.0))
        targets = {"pert": ReferenceColumns(1, c_rho, c_rhoe), "specific": ReferenceColumns(2, c_rho, c_rhoe)}
    aux = np.ascontiguousarray(aux)
    c_rho, c_rhoe = targets["pert"].aux_offsets()
    assert aux[:, c_rho].min() > 0.5 and aux[:, c_rhoe].min() > 1e4
    return law, grid, aux, targets


@functools.lru_cache(maxsize=None)
def sphere_setup(N):
    """``held_suarez_setup(n_horz=2, n_vert=2, N=N)``: curved metrics, 48 elements."""
    law, grid, d, dd = held_suarez_setup(n_horz=2, n_vert=2, N=N)
    aux = np.ascontiguousarray(law.init_state_auxiliary(grid))
    targets = {"pert": F.AtmosFilterPerturbations(law), "specific": F.AtmosSpecificFilterPerturbations(law)}
    return (law, d, dd), grid, aux, targets


def make_filter(kind, grid):
    """Horizontal and vertical cutoffs differ wherever the order allows it, so that the two matrices do."""
    N = grid.N[0]
    if kind == "exponential":
        return F.ExponentialFilter(grid, (1, 0) if N >= 2 else 0, 4)
    if kind == "boydvandeven":
        return F.BoydVandevenFilter(grid, (0, 1) if N >= 2 else 0, 4)
    if kind == "cutoff":
        return F.CutoffFilter(grid, (max(1, N - 2), N))                  # vertical: Nc == N
    if kind == "masspreserving":                                          # N = 1: vertical Nc > N, the identity
        return F.MassPreservingCutoffFilter(grid, (max(1, N - 2), N) if N >= 2 else (1, 2))
    assert kind == "tmar"
    return F.TMARFilter()


FAMILY = {"exponential": "k_apply_filter", "boydvandeven": "k_apply_filter", "cutoff": "k_apply_filter",
          "masspreserving": "k_apply_mp_filter", "tmar": "k_apply_tmar_filter"}


def _cases():
    """(grid name, N, kind, target name, directions, nstate, FilterIndices or None)"""
    out = []
    subset = (4, 1, 4)                                 # a strict subset of five states, one index twice
    for kind in ("exponential", "boydvandeven", "cutoff"):
        for N in (1, 2, 5, 7):
            for tg in ("indices", "pert", "specific"):
                out.append(("brick", N, kind, tg, (EVERY, HORZ, VERT), 5, subset))
    for N in (1, 2, 4, 5, 7):
        for tg in ("indices", "pert", "specific"):
            out.append(("brick", N, "masspreserving", tg, (EVERY, HORZ, VERT), 5, subset))
    for N in (1, 2, 5, 7):
        out.append(("brick", N, "tmar", "indices", (EVERY,), 3, (2, 1)))
    for N in (2, 5):
        for tg in ("indices", "pert", "specific"):
            out.append(("sphere", N, "masspreserving", tg, (EVERY, HORZ, VERT) if tg == "indices" else (EVERY,), 5, subset))
        out.append(("sphere", N, "tmar", "indices", (EVERY,), 3, (2, 1)))
    # more filtered states than one launch stages (csrc/filter_lds.h: 6 mass-preserving and 7 spectral
    # states at N = 7, 10 mass-preserving states at N = 6)
    out.append(("brick", 7, "masspreserving", "indices", (EVERY,), 11, (1, 2, 3, 5, 6, 7, 9, 10, 11)))
    out.append(("brick", 7, "exponential", "indices", (EVERY,), 17, tuple(range(1, 18))))
    out.append(("brick", 6, "masspreserving", "indices", (EVERY,), 11, tuple(range(1, 12))))
    return out


CASES = _cases()


def case_id(c):
    return "%s-N%d-%s-%s-%dof%d" % (c[0], c[1], c[2], c[3], len(set(c[6])), c[5])


@functools.lru_cache(maxsize=None)
def build_case(c):
    """``(setup, grid, aux, target, filt, Q0)`` of a case; ``Q0`` is shared and must not be written."""
    gname, N, kind, tname, _, nstate, idx = c
    setup, grid, aux, targets = brick_setup(N) if gname == "brick" else sphere_setup(N)
    rng = np.random.default_rng(1000 * N + len(kind) + 10 * nstate)
    filt = make_filter(kind, grid)
    if tname == "indices":
        target = F.FilterIndices(*idx)
        if kind == "tmar":
            # mostly positive, some negative nodes: the clipped sum stays well away from zero; the
            # second state is negative all over element 0, which must come back as zeros
            Q0 = 1.0 + 0.6 * rng.standard_normal((grid.nelem, nstate, grid.Np))
            Q0[0, 1] = -np.abs(Q0[0, 1]) - 0.1
            Mass = grid.vgeo[:, 9, :]
            num = (Mass[:, None] * Q0).sum(axis=2)
            den = (Mass[:, None] * np.maximum(Q0, 0)).sum(axis=2)
            live = np.ones_like(num, dtype=bool)
            live[0, 1] = False
            assert np.all(num[live] > 0.25 * den[live]) and np.all(den[live] > 0) and num[0, 1] < 0
        else:
            Q0 = 3.0 + rng.standard_normal((grid.nelem, nstate, grid.Np))
    else:
        # within 1 % of the reference columns, momenta O(5): the near cancellation the targets exist for
        target = targets[tname]
        c_rho, c_rhoe = target.aux_offsets()
        Q0 = np.empty((grid.nelem, 5, grid.Np))
        Q0[:, 0] = aux[:, c_rho] * (1 + 0.01 * rng.uniform(-1, 1, aux[:, 0].shape))
        Q0[:, 4] = aux[:, c_rhoe] * (1 + 0.01 * rng.uniform(-1, 1, aux[:, 0].shape))
        Q0[:, 1:4] = 5.0 * rng.standard_normal(Q0[:, 1:4].shape)
    Q0 = np.ascontiguousarray(Q0)
    Q0.setflags(write=False)
    return setup, grid, aux, target, filt, Q0


def restate(c, direction):
    """``(value, bound)`` of the restatement for a case and direction."""
    _, grid, aux, target, filt, Q0 = build_case(c)
    return R.apply(Q0, target, grid, filt.kind, filt.filter_matrices, direction, aux)


def check_against_restatement(name, c, direction, Q, limit=1.0):
    """Every node of ``Q`` inside the restatement's bound; returns the largest error / bound ratio."""
    value, bound = restate(c, direction)
    assert np.isfinite(Q).all() and np.isfinite(bound.astype(np.float64)).all()
    r = R.ratio(Q, value, bound)
    observe("filters restatement: %s error / bound, %s, %s" % (name, FAMILY[c[2]], c[3]), r)
    assert r <= limit, (case_id(c), direction, r)
    return r


def is_identity(c, direction):
    """The one application of the table whose matrix is the identity (``Nc > N``)."""
    return c[2] == "masspreserving" and c[1] == 1 and direction == VERT


def untouched_states(c):
    """0-based states a FilterIndices case does not list (bit-identical afterwards), else none."""
    return [s for s in range(c[5]) if s + 1 not in c[6]] if c[3] == "indices" else []


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_oracle_within_restatement_bounds(oracle, c):
    _, grid, aux, target, filt, Q0 = build_case(c)
    for direction in c[4]:
        Q = Q0.copy()
        oracle.apply_filter(Q, target, grid, filt, direction=direction, state_auxiliary=aux)
        # a ratio above 0.5 would mean the bound's derivation is wrong, not that the oracle is
        check_against_restatement("oracle", c, direction, Q, limit=0.5)
        assert is_identity(c, direction) or not np.array_equal(Q, Q0)
        for s in untouched_states(c):
            assert np.array_equal(Q[:, s], Q0[:, s]), s
        if c[2] == "tmar":
            assert Q[:, [i - 1 for i in c[6]]].min() >= 0 and not Q[0, 1].any()


def test_mass_preserving_restatement_preserves_mass():
    """The restatement on its own: element means of every state survive to the long double's rounding,
    and the plain cutoff does not keep them."""
    c = ("sphere", 2, "masspreserving", "indices", (EVERY,), 5, (4, 1, 4))
    _, grid, aux, target, filt, Q0 = build_case(c)
    Mass = grid.vgeo[:, 9, :].astype(R.LD)[:, None]
    before = (Mass * Q0).sum(axis=2)
    v, _ = R.apply(Q0, target, grid, R.K_MASS_PRESERVING, filt.filter_matrices, EVERY)
    assert np.abs((Mass * v).sum(axis=2) - before).max() <= 1e-16 * np.abs(before).max()
    v, _ = R.apply(Q0, target, grid, R.K_SPECTRAL, filt.filter_matrices, EVERY)
    assert np.abs((Mass * v).sum(axis=2) - before).max() >= 1e-6 * np.abs(before).max()
