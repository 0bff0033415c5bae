"""NumPy restatement of the reference's direct stiffness summation on the host, ``dss3d_CPU!``
(src/Numerics/Mesh/DSS.jl:128-165) with ``dss_vertex!`` :190-214, ``dss_edge!`` :244-278 and
``dss_face!`` :296-316: the three loops as written, every sum started from ``-0.0`` and taken in the
tables' order, so that a device result can be held to it bit for bit.  Also the ghost exchange of
``dss!`` (:29-31) for ranks held in one process, through ``vmapsend`` / ``vmaprecv`` and the
neighbour ranges, as tests/test_halo_fixture.py does it, and the assertions of the reference's two
DSS tests (test/Numerics/Mesh/DSS.jl, DSS_mpi.jl) for the host and the device test to share.

Arrays are numpy views of the reference's layout: ``Q[e, ivar, n]`` is ``data[n + 1, ivar + 1, e + 1]``.
"""
import numpy as np


def dss3d_cpu(Q, grid):
    """``dss3d_CPU!`` in place on ``Q (nelem, nvars, Np)`` with the tables of ``grid``."""
    t = grid.topology
    vertmap, edgemap, facemap = grid.vertmap, grid.edgemap, grid.facemap
    vtconn, vtconnoff = t.vtconn, t.vtconnoff
    edgconn, edgconnoff = t.edgconn, t.edgconnoff
    fcconn = t.fcconn                                     # (5, nfc)
    nvt, nedg, nfc = len(vtconnoff) - 1, len(edgconnoff) - 1, fcconn.shape[1]
    Nemax, Nfmax = edgemap.shape[2], facemap.shape[2]
    for ivar in range(Q.shape[1]):
        data = Q[:, ivar, :]                              # data[lelem - 1, loc - 1]
        for vx in range(nvt):                             # dss_vertex!
            st = vtconnoff[vx] - 1
            nlvt = (vtconnoff[vx + 1] - vtconnoff[vx]) // 2
            sumv = -0.0
            for j in range(nlvt):
                lvt, lelem = vtconn[st + 2 * j], vtconn[st + 2 * j + 1]
                sumv = sumv + data[lelem - 1, vertmap[lvt - 1] - 1]
            for j in range(nlvt):
                lvt, lelem = vtconn[st + 2 * j], vtconn[st + 2 * j + 1]
                data[lelem - 1, vertmap[lvt - 1] - 1] = sumv
        for ex in range(nedg):                            # dss_edge!
            st = edgconnoff[ex] - 1
            nledg = (edgconnoff[ex + 1] - edgconnoff[ex]) // 3
            for k in range(Nemax):
                sume = -0.0
                for j in range(nledg):
                    ledg, lor, lelem = edgconn[st + 3 * j:st + 3 * j + 3]
                    loc = edgemap[lor - 1, ledg - 1, k]
                    if loc != -1:
                        sume = sume + data[lelem - 1, loc - 1]
                for j in range(nledg):
                    ledg, lor, lelem = edgconn[st + 3 * j:st + 3 * j + 3]
                    loc = edgemap[lor - 1, ledg - 1, k]
                    if loc != -1:
                        data[lelem - 1, loc - 1] = sume
        for fx in range(nfc):                             # dss_face!
            lfc, lel, nabrlfc, nabrlel, ordr = fcconn[:, fx]
            ordr = 2 if ordr == 3 else 1
            for j in range(Nfmax):
                loc1 = facemap[ordr - 1, lfc - 1, j]
                loc2 = facemap[0, nabrlfc - 1, j]
                if loc1 != -1 and loc2 != -1:
                    sumf = data[lel - 1, loc1 - 1] + data[nabrlel - 1, loc2 - 1]
                    data[lel - 1, loc1 - 1] = sumf
                    data[nabrlel - 1, loc2 - 1] = sumf
    return Q


def ghost_exchange(grids, Qs):
    """``begin_ghost_exchange!`` / ``end_ghost_exchange!`` for the ranks of one process:
    ``grids[r]``, ``Qs[r]`` belong to rank ``r``; the send buffer is ``(nvmap, nvars)`` with
    ``(e, n) = fldmod1(vmap, Np)``, and a neighbour owns a contiguous range of both maps."""
    sends = []
    for g, Q in zip(grids, Qs):
        vs = np.asarray(g.vmapsend, dtype=np.int64) - 1
        sends.append(Q[vs // g.Np, :, vs % g.Np].copy() if len(vs) else np.zeros((0, Q.shape[1])))
    for r, (g, Q) in enumerate(zip(grids, Qs)):
        vr = np.asarray(g.vmaprecv, dtype=np.int64) - 1
        recv = np.zeros((len(vr), Q.shape[1]))
        for n, nbr in enumerate(g.nabrtorank):
            a, b = g.nabrtovmaprecv[n]
            k = list(grids[nbr].nabrtorank).index(r)
            sa, sb = grids[nbr].nabrtovmapsend[k]
            assert sb - sa == b - a
            recv[a - 1:b] = sends[nbr][sa - 1:sb]
        if len(vr):
            Q[vr // g.Np, :, vr % g.Np] = recv


def dss(grids, Qs):
    """``dss!`` on every rank: exchange, then the summation."""
    ghost_exchange(grids, Qs)
    for g, Q in zip(grids, Qs):
        dss3d_cpu(Q, g)


# ---- the assertions of the reference's tests -----------------------------------------------------
def _nodes(grid):
    return np.arange(grid.Np).reshape(grid.Nq, order="F")


def check_dss_jl(grid, pre, post):
    """Every ``@test`` of test/Numerics/Mesh/DSS.jl: two elements side by side in x1, one state."""
    Nq = grid.Nq
    interior = _nodes(grid)[1:Nq[0] - 1, 1:Nq[1] - 1, 1:Nq[2] - 1].flatten(order="F")
    vm = grid.vertmap - 1
    em, fm = grid.edgemap[0], grid.facemap[0]             # orientation 1: (12, Nemax), (6, Nfmax)
    ne = [max(q - 2, 0) for q in Nq]
    nf = [ne[1] * ne[2], ne[0] * ne[2], ne[0] * ne[1]]

    def same(el, i, m, n):
        idx = m[i - 1, :n] - 1
        assert np.array_equal(post[el - 1, 0, idx], pre[el - 1, 0, idx]), (el, i)

    def shared(el1, i1, el3, i3, m, n):
        assert np.array_equal(post[el1 - 1, 0, m[i1 - 1, :n] - 1],
                              pre[el1 - 1, 0, m[i1 - 1, :n] - 1] + pre[el3 - 1, 0, m[i3 - 1, :n] - 1]), (el1, i1)

    for el, other, own_side, other_side in ((1, 2, 1, 0), (2, 1, 0, 1)):
        assert np.array_equal(pre[el - 1, 0, interior], post[el - 1, 0, interior])
        # vertices: those with x1 on the shared side take the neighbour's opposite vertex
        exp = [pre[el - 1, 0, vm[v]] + (pre[other - 1, 0, vm[v ^ 1]] if (v & 1) == own_side else 0.0)
               for v in range(8)]
        assert np.array_equal(post[el - 1, 0, vm], np.array(exp)), el
        for i in (1, 2, 3, 4):
            same(el, i, em, ne[0])
        # edges along x2 (5..8) and x3 (9..12): the odd ones lie at x1 = -1, the even ones at x1 = +1
        for base, n in ((5, ne[1]), (9, ne[2])):
            for q in range(4):
                i = base + q
                if (q & 1) == own_side:
                    shared(el, i, other, i - 1 if own_side else i + 1, em, n)
                else:
                    same(el, i, em, n)
        mine, theirs = (2, 1) if own_side else (1, 2)
        shared(el, mine, other, theirs, fm, nf[0])
        same(el, theirs, fm, nf[0])
        for i, n in ((3, nf[1]), (4, nf[1]), (5, nf[2]), (6, nf[2])):
            same(el, i, fm, n)


DSS_MPI_EXPECTED = {        # rank: (vertices, edges 1..12, faces 1..6) of local element 1, DSS_mpi.jl:74-165
    0: ([1, 2, 2, 4, 2, 4, 4, 8], [1, 2, 2, 4, 1, 2, 2, 4, 1, 2, 2, 4], [1, 2, 1, 2, 1, 2]),
    1: ([2, 4, 1, 2, 4, 8, 2, 4], [2, 1, 4, 2, 1, 2, 2, 4, 2, 4, 1, 2], [1, 2, 2, 1, 1, 2]),
    2: ([4, 2, 2, 1, 8, 4, 4, 2], [2, 1, 4, 2, 2, 1, 4, 2, 4, 2, 2, 1], [2, 1, 2, 1, 1, 2]),
}


def check_dss_mpi_jl(grid, rank, data):
    """Every ``@test`` of test/Numerics/Mesh/DSS_mpi.jl for ``rank``: ``data`` is the rank's array
    after ``dss!`` of ones on the real and zeros on the ghost elements."""
    Nq = grid.Nq
    interior = _nodes(grid)[1:Nq[0] - 1, 1:Nq[1] - 1, 1:Nq[2] - 1].flatten(order="F")
    verts, edges, faces = DSS_MPI_EXPECTED[rank]
    lel = 0
    for ivar in range(data.shape[1]):
        assert np.unique(data[lel, ivar, interior]).tolist() == [1.0]
        assert data[lel, ivar, grid.vertmap - 1].tolist() == [float(v) for v in verts]
        for m, exp in ((grid.edgemap[0], edges), (grid.facemap[0], faces)):
            for i, want in enumerate(exp):
                idx = m[i][m[i] != -1] - 1
                assert np.unique(data[lel, ivar, idx]).tolist() == [float(want)], (rank, ivar, i + 1)
