"""Direct stiffness summation on the device (csrc/dss.hip through ``mesh.dss``, ``mesh.dss_apply``,
``mesh.group_dss``) against the NumPy restatement of the reference's host loops
(tests/dss_restatement.py), bit for bit: sums of the same doubles in the same order.  ``-m gpu``.

Shapes are the smallest that hold every branch: the reference's two-element (4, 4, 5) brick (orders no
engine is compiled for, NULL handle, -1 padding in the edge and face maps, one wave that is not
full), its three-rank brick (ghost exchange, groups of 2, 4 and 8 members, several work-groups), the
3 x 3 x 2 cubed sphere on three ranks (flipped faces, swapped edges, groups of 3 and 6) and a
two-rank brick of orders (4, 2)."""
import ctypes as C

import numpy as np
import pytest

import dss_restatement as R
from helpers import held_suarez_setup, pseudo1d_setup, variable_degree_setup

pytestmark = pytest.mark.gpu


def _gpu(torch, a):
    x = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return x


def _brick_grid(cm, rng, N, rank=0, size=1):
    M = cm.mesh
    topl = M.StackedBrickTopology([np.asarray(r, dtype=np.float64) for r in rng], periodicity=(False,) * 3,
                                  boundary=((1, 2),) * 3, connectivity="full", rank=rank, size=size)
    return M.DiscontinuousSpectralElementGrid(topl, N)


MPI_RANGE = (range(0, 5), range(5, 10), range(0, 4))      # DSS_mpi.jl: brickrange (0:4, 5:9, 0:3)


class _Ranks:
    """The models of every rank of one partitioned set-up, connected in one process."""

    def __init__(self, cm, setup, size, **model_kw):
        self.cm, self.size = cm, size
        self.grids, self.dgs = [], []
        for r in range(size):
            law, grid = setup(r, size)
            self.grids.append(grid)
            self.dgs.append(cm.dgmodel.DGModel(law, grid, **model_kw))
        cm.dgmodel.connect_local(self.dgs)

    def run(self, torch, Q0s):
        """``group_dss`` on copies of ``Q0s``; returns the host arrays."""
        Qs = [_gpu(torch, q) for q in Q0s]
        self.cm.mesh.group_dss(self.dgs, Qs)
        return [q.cpu().numpy() for q in Qs]

    def restated(self, Q0s):
        Qs = [q.copy() for q in Q0s]
        R.dss(self.grids, Qs)
        return Qs

    def random(self, nstate, seed):
        rng = np.random.default_rng(seed)
        return [rng.standard_normal((g.nelem, nstate, g.Np)) for g in self.grids]

    def close(self):
        for g in self.grids:
            if getattr(g, "_dss_object", None) is not None:
                g._dss_object.close()
        for dg in self.dgs:
            dg.close()


@pytest.fixture(scope="module")
def brick3(cm, torch):
    law = pseudo1d_setup()[0]
    case = _Ranks(cm, lambda r, s: (law, _brick_grid(cm, MPI_RANGE, 4, r, s)), 3, direction=0)
    yield case
    case.close()


@pytest.fixture(scope="module")
def sphere3(cm, torch):
    case = _Ranks(cm, lambda r, s: held_suarez_setup(3, 2, rank=r, size=s)[:2], 3, direction=0,
                  diffusion_direction=1)
    yield case
    case.close()


def _same_on_real(case, got, want):
    for r, (g, a, b) in enumerate(zip(case.grids, got, want)):
        assert np.array_equal(a[:g.nreal], b[:g.nreal]), r


# ---- bit for bit against the restatement -----------------------------------------------------------
@pytest.mark.parametrize("nstate", [1, 17])
def test_two_element_brick_without_a_handle(cm, torch, nstate):
    """Orders (4, 4, 5): no engine is compiled for them, the summation needs none.  Nodes in no group
    keep their bits; the flattened tables are the 30 pairs of the shared face."""
    grid = _brick_grid(cm, (range(0, 3), range(5, 7), range(0, 2)), (4, 4, 5))
    obj = cm.mesh.DSS(grid)
    Q0 = np.random.default_rng(nstate).standard_normal((grid.nelem, nstate, grid.Np))
    want = R.dss3d_cpu(Q0.copy(), grid)
    Q = _gpu(torch, Q0)
    cm.mesh.dss_apply(Q, obj)
    got = Q.cpu().numpy()
    assert np.array_equal(got, want)
    assert obj.info(Q.device) == (30, 60, 2, 60)
    touched = np.zeros((grid.nelem, grid.Np), dtype=bool)
    touched[0, np.arange(grid.Np).reshape(grid.Nq, order="F")[-1].reshape(-1)] = True
    touched[1, np.arange(grid.Np).reshape(grid.Nq, order="F")[0].reshape(-1)] = True
    assert touched.sum() == 60
    untouched = ~touched
    assert np.array_equal(got.transpose(0, 2, 1)[untouched].view(np.int64),
                          Q0.transpose(0, 2, 1)[untouched].view(np.int64))
    assert (got.transpose(0, 2, 1)[touched] != Q0.transpose(0, 2, 1)[touched]).all()
    if nstate == 1:                       # the reference's own test, on the device
        ldof = (np.arange(1, grid.Np + 1, dtype=np.float64)[None, None, :]
                + grid.Np * np.arange(2, dtype=np.float64)[:, None, None])
        Q = _gpu(torch, ldof)
        cm.mesh.dss_apply(Q, grid)        # (the grid's own object, made and kept at first use)
        R.check_dss_jl(grid, ldof, Q.cpu().numpy())
        grid._dss_object.close()
    obj.close()


def test_three_rank_brick_through_group_dss(cm, torch, brick3):
    """nstate 3 is the most the exchange buffers of an AdvectionDiffusion handle hold."""
    Q0s = brick3.random(3, 1)
    _same_on_real(brick3, brick3.run(torch, Q0s), brick3.restated(Q0s))
    for g in brick3.grids:                # the flattened tables hold what the reference's tables say
        t = g.topology
        shared = np.diff(t.vtconnoff) > 0
        groups = 9 * t.fcconn.shape[1] + 3 * (len(t.edgconnoff) - 1) + int(shared.sum())
        members = 18 * t.fcconn.shape[1] + len(t.edgconn) + len(t.vtconn) // 2
        assert g._dss_object.info("cuda") == (groups, members, 8, members)
        assert groups > 256 and groups % 64 != 0                     # several work-groups, a ragged tail


def test_dss_mpi_jl_literals_on_the_device(cm, torch, brick3):
    """test/Numerics/Mesh/DSS_mpi.jl at N = 4 (the counts do not depend on the order)."""
    Q0s = []
    for g in brick3.grids:
        Q = np.zeros((g.nelem, 3, g.Np))
        Q[:g.nreal] = 1.0
        Q0s.append(Q)
    for r, (g, Q) in enumerate(zip(brick3.grids, brick3.run(torch, Q0s))):
        R.check_dss_mpi_jl(g, r, Q)


def test_held_suarez_sphere_on_three_ranks(cm, torch, sphere3):
    Q0s = sphere3.random(5, 2)
    _same_on_real(sphere3, sphere3.run(torch, Q0s), sphere3.restated(Q0s))
    orders = set()
    for g in sphere3.grids:
        orders |= set(g.topology.fcconn[4].tolist())
    assert orders == {1, 3}


def test_orders_4_2_on_two_ranks(cm, torch):
    case = _Ranks(cm, lambda r, s: variable_degree_setup(1, (4, 2), rank=r, size=s)[:2], 2)
    try:
        assert (case.grids[0].edgemap == -1).any() and (case.grids[0].facemap == -1).any()
        Q0s = case.random(2, 3)
        _same_on_real(case, case.run(torch, Q0s), case.restated(Q0s))
    finally:
        case.close()


# ---- partition invariance --------------------------------------------------------------------------
def _integers(case, whole, nstate, seed):
    """Integer-valued data on the whole grid and its rows on every rank (sums of integers are exact,
    so the order of a group's members, which differs between partitions, does not matter)."""
    Qw = np.random.default_rng(seed).integers(-1000, 1000, (whole.nelem, nstate, whole.Np)).astype(np.float64)
    pos = {int(g): i for i, g in enumerate(whole.topology.globalelems)}
    rows = [np.array([pos[int(g)] for g in grid.topology.globalelems]) for grid in case.grids]
    return Qw, rows


@pytest.mark.parametrize("which", ["brick", "sphere"])
def test_partition_invariance(cm, torch, brick3, sphere3, which):
    if which == "brick":
        case, whole, ns = brick3, _brick_grid(cm, MPI_RANGE, 4), 3
    else:
        case, whole, ns = sphere3, held_suarez_setup(3, 2)[1], 5
    Qw, rows = _integers(case, whole, ns, 4)
    one = _gpu(torch, Qw)
    cm.mesh.dss_apply(one, whole)
    one = one.cpu().numpy()
    whole._dss_object.close()
    assert not np.array_equal(one, Qw)
    for g, row, got in zip(case.grids, rows, case.run(torch, [Qw[r] for r in rows])):
        assert np.array_equal(got[:g.nreal], one[row[:g.nreal]])


# ---- ordering on the handle's stream ---------------------------------------------------------------
def test_dss_apply_is_ordered_behind_a_filter_on_the_same_handle(cm, torch):
    F = cm.mesh.filters
    law = pseudo1d_setup()[0]
    grid = _brick_grid(cm, MPI_RANGE, 4)
    dg = cm.dgmodel.DGModel(law, grid, direction=0)
    ns = 8
    f = F.make_device_filter(dg, F.ExponentialFilter(grid, 0, 4), F.FilterIndices(range(1, ns + 1)), nstate=ns)
    Q0 = np.random.default_rng(6).standard_normal((grid.nelem, ns, grid.Np))
    A, B = _gpu(torch, Q0), _gpu(torch, Q0)
    f.apply(A)
    dg.synchronize()
    cm.mesh.dss_apply(A, grid, dg)
    dg.synchronize()
    f.apply(B)                            # enqueued ...
    cm.mesh.dss_apply(B, grid, dg)        # ... and the summation directly behind it
    dg.synchronize()
    a, b = A.cpu().numpy(), B.cpu().numpy()
    assert np.array_equal(a, b)
    Qf = _gpu(torch, Q0)
    f.apply(Qf)
    dg.synchronize()
    assert np.array_equal(a, R.dss3d_cpu(Qf.cpu().numpy(), grid))
    # dss!(Q, grid) on an unpartitioned handle: no exchange, the same sums
    D = _gpu(torch, Qf.cpu().numpy())
    cm.mesh.dss(D, dg)
    assert np.array_equal(D.cpu().numpy(), a)
    f.close()
    grid._dss_object.close()
    dg.close()


# ---- refusals --------------------------------------------------------------------------------------
def test_more_states_than_the_exchange_buffers_hold(cm, torch, brick3):
    Q0s = brick3.random(4, 7)
    with pytest.raises(cm._lib.CmdgError, match="halo: nstate too large for the buffers"):
        brick3.run(torch, Q0s)
    Q0s = brick3.random(3, 8)             # the handles serve the next call
    _same_on_real(brick3, brick3.run(torch, Q0s), brick3.restated(Q0s))


def _create(cm, obj, spoil):
    L = cm._lib.lib()
    spoil(obj)
    d = obj.descriptor()
    h = C.c_void_p()
    status = L.cmdg_dss_create(None, C.byref(d), C.byref(h))
    return status, L.cmdg_last_error(None).decode(), h


def test_create_refuses_broken_tables(cm, torch):
    grid = _brick_grid(cm, (range(0, 3), range(5, 7), range(0, 2)), (4, 4, 5))

    def twice(o):                         # vertex 2 of element 1 at a second unique vertex
        o.vtconn[4] = 2

    def beyond(o):
        o.edgconn[2] = o.nelem + 1

    for spoil, reason in ((twice, "is in two groups"), (beyond, "names element 3, outside 1..2")):
        status, msg, h = _create(cm, cm.mesh.DSS(grid), spoil)
        assert status == -1 and reason in msg and not h.value, (status, msg)


def test_dss_needs_a_handle(cm, torch):
    grid = _brick_grid(cm, (range(0, 3), range(5, 7), range(0, 2)), (4, 4, 5))
    obj = cm.mesh.DSS(grid)
    Q = _gpu(torch, np.zeros((grid.nelem, 1, grid.Np)))
    L = cm._lib.lib()
    assert L.cmdg_dss(None, obj.device_object(Q.device), Q.data_ptr(), 1) == -1
    assert "needs a handle" in L.cmdg_last_error(None).decode()
    obj.close()


def test_dss_desc_struct_matches_header_field_order(cm):
    from test_abi_symbols import _header_fields
    fields = _header_fields("cmdg_dss_desc")
    assert fields == [f[0] for f in cm.mesh.CmdgDssDesc._fields_], fields
