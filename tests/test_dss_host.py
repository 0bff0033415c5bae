"""Direct stiffness summation on the host: the topology's DSS tables (Topologies.jl:810-988,
:1687-1850), the grid's vertex, edge and face maps (Grids.jl:640-745) and the NumPy restatement
of ``dss3d_CPU!`` built on them reproduce the reference's own tests (test/Numerics/Mesh/DSS.jl,
DSS_mpi.jl) and pair the right nodes on the cubed sphere and on a fully periodic brick.  No GPU."""
import numpy as np
import pytest

from cmdg_loader import cm
import dss_restatement as R

M = cm.mesh


def _brick(rng, N, rank=0, size=1, periodicity=(False,) * 3, connectivity="full"):
    topl = M.StackedBrickTopology([np.asarray(r) for r in rng], periodicity=periodicity,
                                  boundary=((1, 2), (3, 4), (5, 6)), connectivity=connectivity,
                                  rank=rank, size=size)
    return M.DiscontinuousSpectralElementGrid(topl, N)


def test_laziness_building_a_grid_builds_no_tables():
    g = _brick((range(0, 3), range(5, 7), range(0, 2)), (4, 4, 5))
    assert g.topology._dss is None and getattr(g, "_vefmaps", None) is None
    assert g.topology.elemtovert is not None              # the base topology's, kept
    assert g.topology.vtconnoff is not None and g.topology._dss is not None
    assert g.vertmap is not None and g._vefmaps is not None


def test_reference_dss_jl():
    """test/Numerics/Mesh/DSS.jl: brickrange (0:2, 5:6, 0:1), N = (4, 4, 5), values ldof + (e-1) Np."""
    g = _brick((range(0, 3), range(5, 7), range(0, 2)), (4, 4, 5))
    assert (g.topology.nreal, g.topology.nghost, g.Np) == (2, 0, 150)
    Q = (np.arange(1, g.Np + 1, dtype=np.float64)[None, None, :]
         + g.Np * np.arange(2, dtype=np.float64)[:, None, None])
    pre = Q.copy()
    R.dss([g], [Q])
    R.check_dss_jl(g, pre, Q)
    t = g.topology
    # the tables themselves: four shared vertices, four shared edges, one shared face
    assert t.vtconnoff[-1] - 1 == len(t.vtconn) == 16 and len(t.edgconnoff) - 1 == 4
    assert t.fcconn.shape == (5, 1) and t.fcconn[:, 0].tolist() == [2, 1, 1, 2, 1]
    assert g.edgemap.shape == (2, 12, 4) and g.facemap.shape == (2, 6, 12)
    assert (g.edgemap[:, :8, 3] == -1).all() and (g.facemap[:, 4:, 9:] == -1).all()


def test_reference_dss_mpi_jl():
    """test/Numerics/Mesh/DSS_mpi.jl: three ranks, brickrange (0:4, 5:9, 0:3), three states of ones."""
    grids = [_brick((range(0, 5), range(5, 10), range(0, 4)), (4, 4, 5), rank=r, size=3) for r in range(3)]
    Qs = []
    for g in grids:
        Q = np.zeros((g.nelem, 3, g.Np))
        Q[:g.nreal] = 1.0
        Qs.append(Q)
    R.dss(grids, Qs)
    for r, (g, Q) in enumerate(zip(grids, Qs)):
        R.check_dss_mpi_jl(g, r, Q)


def _point_ids(grids):
    """An integer id per geometric point over all ranks (coordinates rounded to 1e-7 of the radius:
    the copies of a node differ by rounding errors of 1e-16, distinct nodes by 1e-2 and more), and
    the number of real elements that contain each point."""
    keys = []
    for g in grids:
        x = np.stack([g.vgeo[:, c, :] for c in (12, 13, 14)], axis=-1)       # (nelem, Np, 3)
        keys.append(np.round(x / 1e-7).astype(np.int64))
    allk = np.concatenate([k.reshape(-1, 3) for k in keys])
    uniq, inv = np.unique(allk, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    ids, count, at = [], np.zeros(len(uniq), dtype=np.int64), 0
    for g, k in zip(grids, keys):
        n = k.shape[0] * k.shape[1]
        i = inv[at:at + n].reshape(k.shape[0], k.shape[1])
        at += n
        ids.append(i + 1)
        np.add.at(count, i[:g.nreal].reshape(-1), 1)
    return ids, count


@pytest.mark.parametrize("N", [3, (4, 4, 2)])
@pytest.mark.parametrize("size", [1, 3])
def test_cubed_sphere_pairs_the_right_nodes(N, size):
    grids = []
    for r in range(size):
        topl = M.StackedCubedSphereTopology(3, np.array([1.0, 1.5, 2.0]), rank=r, size=size)
        grids.append(M.DiscontinuousSpectralElementGrid(topl, N, meshwarp=M.equiangular_cubed_sphere_warp))
    ids, count = _point_ids(grids)
    Qs = []
    for g, i in zip(grids, ids):
        Q = np.zeros((g.nelem, 2, g.Np))
        Q[:g.nreal, 0] = 1.0
        Q[:g.nreal, 1] = i[:g.nreal]
        Qs.append(Q)
    R.dss(grids, Qs)
    valences, face_ordr, edge_ordr = set(), set(), set()
    for g, i, Q in zip(grids, ids, Qs):
        nr = g.nreal
        assert np.array_equal(Q[:nr, 0], count[i[:nr] - 1].astype(np.float64))
        assert np.array_equal(Q[:nr, 1], Q[:nr, 0] * i[:nr])
        valences |= set(Q[:nr, 0][:, g.vertmap - 1].reshape(-1).tolist())
        face_ordr |= set(g.topology.fcconn[4].tolist())
        edge_ordr |= set(g.topology.edgconn[1::3].tolist())
    # what the case is for: flipped faces, swapped edges, every vertex valence of the stacked sphere
    assert face_ordr == {1, 3} and edge_ordr == {1, 2}
    assert valences == {3.0, 4.0, 6.0, 8.0}


@pytest.mark.parametrize("size", [1, 2])
def test_fully_periodic_brick(size):
    rng = (np.arange(3.0), np.arange(4.0), np.arange(3.0))                  # 2 x 3 x 2 elements
    grids = [_brick(rng, (2, 2, 3), rank=r, size=size, periodicity=(True,) * 3) for r in range(size)]
    assert all(g.topology.periodicstack for g in grids)
    Qs = []
    for g in grids:
        Q = np.zeros((g.nelem, 1, g.Np))
        Q[:g.nreal] = 1.0
        Qs.append(Q)
    R.dss(grids, Qs)
    seen = set()
    for g, Q in zip(grids, Qs):
        seen |= set(Q[:g.nreal].reshape(-1).tolist())
        nodes = np.arange(g.Np).reshape(g.Nq, order="F")
        assert (Q[:g.nreal, 0][:, nodes[1:-1, 1:-1, 1:-1].reshape(-1)] == 1.0).all()
        assert (Q[:g.nreal, 0][:, g.vertmap - 1] == 8.0).all()               # every corner: eight elements
        assert (Q[:g.nreal, 0][:, g.facemap[0][g.facemap[0] != -1] - 1] == 2.0).all()
    assert seen == {1.0, 2.0, 4.0, 8.0}


def test_tables_are_none_where_the_reference_has_nothing():
    rng3 = (range(0, 3), range(5, 7), range(0, 2))
    face = _brick(rng3, 4, connectivity="face").topology
    assert face.elemtovert is None and face.elemtouvert is None
    assert all(getattr(face, a) is None for a in ("vtconn", "vtconnoff", "fcconn", "edgconn", "edgconnoff"))
    flat = M.BrickTopology([np.arange(3.0), np.arange(3.0)], connectivity="full")
    assert flat.elemtouvert is not None and flat.vtconn is None and flat.fcconn is None and flat.edgconn is None
    assert M.grids.init_vertex_edge_face_mappings((4, 4)) == (None, None, None)
    assert M.grids.init_vertex_edge_face_mappings((4, 4, 1)) == (None, None, None)
    vm, em, fm = M.grids.init_vertex_edge_face_mappings((1, 1, 2))
    assert vm is not None and em is not None and fm is None


def test_refused_grids_raise_value_error():
    rng3 = (range(0, 3), range(5, 7), range(0, 2))
    with pytest.raises(ValueError, match='connectivity = "face"'):
        M.DSS(_brick(rng3, 4, connectivity="face"))
    with pytest.raises(ValueError, match="vertical polynomial order 1"):
        M.DSS(_brick(rng3, (4, 4, 1)))
    with pytest.raises(ValueError, match="vertical polynomial order 0"):
        M.DSS(_brick(rng3, (4, 4, 0)))                                       # a DGFVModel grid
    with pytest.raises(ValueError, match="no interior face node"):
        M.DSS(_brick(rng3, (1, 1, 2)))
    topl2 = M.StackedBrickTopology([np.arange(3.0), np.arange(3.0)], connectivity="face")
    with pytest.raises(ValueError, match="3-D grids only"):
        M.DSS(M.DiscontinuousSpectralElementGrid(topl2, 4))
    flat = M.BrickTopology([np.arange(3.0)] * 3, connectivity="face")
    with pytest.raises(ValueError, match="stacked topology"):
        M.DSS(M.DiscontinuousSpectralElementGrid(flat, 4))
    # a supported grid builds its descriptor without touching the library
    d = M.DSS(_brick(rng3, (4, 4, 5)))
    assert d.descriptor().nvt == len(d.vtconnoff) - 1 and d.descriptor().nfc == 1


def test_dss_desc_struct_matches_header_field_order():
    from test_abi_symbols import _header_fields
    fields = _header_fields("cmdg_dss_desc")
    assert fields == [f[0] for f in M.CmdgDssDesc._fields_], fields


def test_group_dss_refuses_bad_handle_lists():
    """As every entry that takes several handles (tests/test_group_entries_host.py): a NULL list,
    n < 1 and a NULL member are refused before anything else is looked at."""
    from test_group_entries_host import INVALID, _arr, _handle_lists
    L = cm._lib.lib()
    for h, n, why in _handle_lists():
        assert L.cmdg_group_dss(h, n, _arr(), _arr(), 1) == INVALID, why
