// The row condition of the fused Laplacian pass and its second-ring index (csrc/lapfused_tables.h) on
// the host.  The pass lets the NQ face lanes of one lateral face and one level hand each other the
// record of their plus node, which is right only if those plus nodes are one row of one neighbour:
// one element, one level, one face of it, indices along that face a permutation of 0 .. NQ-1.
// lapfused_build must accept the periodic patch and the three-panel corner (flipped gluings
// included) with that property at every row, refuse hand-made tables whose row straddles two
// levels, two neighbours, or repeats an index -- each with a reason and without a crash --, and
// record idE = faceP[N][tE] at every task with a tE.  Built by tests/test_lapfused_lines_host.py
// with -fsanitize=address,undefined and run as a process of its own.
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "lapfused_tables.h"

using namespace cmdg;

static int failures = 0;
#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++failures;                                           \
        }                                                         \
    } while (0)

namespace {
// a grid as cmdg_create digests it: faceP (NFT, nreal), elemtobndy (6, nreal); top and bottom walls
struct Grid {
    int NQ, NQV, Np, Nfph, NL, NFT;
    int64_t nreal;
    std::vector<int32_t> faceP;
    std::vector<int64_t> bndy;
    Grid(int nq, int nqv, int64_t n) : NQ(nq), NQV(nqv), nreal(n)
    {
        Np = NQ * NQ * NQV, Nfph = NQ * NQV, NL = 4 * Nfph, NFT = NL + 2 * NQ * NQ;
        faceP.assign((size_t)(NFT * nreal), 0);
        bndy.assign((size_t)(6 * nreal), 0);
        for (int64_t e = 0; e < nreal; ++e) {
            bndy[4 + 6 * e] = 1, bndy[5 + 6 * e] = 2;
            for (int n = 0; n < NQ * NQ; ++n) {
                faceP[NFT * e + NL + n] = (int32_t)(e * Np + n);
                faceP[NFT * e + NL + NQ * NQ + n] = (int32_t)(e * Np + n + NQ * NQ * (NQV - 1));
            }
        }
    }
    int node(int i, int j, int k) const { return i + NQ * (j + NQ * k); }
    int face_node(int f, int a, int k) const
    {
        const int E = NQ - 1;
        return f == 0 ? node(0, a, k) : f == 1 ? node(E, a, k) : f == 2 ? node(a, 0, k) : node(a, E, k);
    }
    int task(int f, int a, int k) const { return f * Nfph + a + NQ * k; }
    // one face node of e1 against one of e2, both ways
    void pair(int64_t e1, int f1, int a1, int k1, int64_t e2, int f2, int a2, int k2)
    {
        faceP[NFT * e1 + task(f1, a1, k1)] = (int32_t)(e2 * Np + face_node(f2, a2, k2));
        faceP[NFT * e2 + task(f2, a2, k2)] = (int32_t)(e1 * Np + face_node(f1, a1, k1));
    }
    // glue face f1 of e1 to face f2 of e2, position a on the first meeting a (or E - a) on the second
    void glue(int64_t e1, int f1, int64_t e2, int f2, bool flip)
    {
        for (int k = 0; k < NQV; ++k)
            for (int a = 0; a < NQ; ++a) pair(e1, f1, a, k, e2, f2, flip ? NQ - 1 - a : a, k);
    }
};

Grid periodic_patch(int NQ, int NQV, int nx, int ny)
{
    Grid g(NQ, NQV, (int64_t)nx * ny);
    for (int ey = 0; ey < ny; ++ey)
        for (int ex = 0; ex < nx; ++ex) {
            const int64_t e = ex + nx * ey;
            g.glue(e, 1, (ex + 1) % nx + nx * ey, 0, false);
            g.glue(e, 3, ex + nx * ((ey + 1) % ny), 2, false);
        }
    return g;
}

// three elements round a corner: face 1 of each meets face 3 of the next, face 0 of each meets face 2
// of the next with the positions reversed
Grid three_panel_corner(int NQ, int NQV)
{
    Grid g(NQ, NQV, 3);
    for (int e = 0; e < 3; ++e) {
        g.glue(e, 1, (e + 1) % 3, 3, false);
        g.glue(e, 0, (e + 1) % 3, 2, true);
    }
    return g;
}

// the row property, checked here from faceP and tP alone, and idE at every task with a tE
void rows_and_edges(const Grid &g)
{
    LapFusedTables t;
    lapfused_build(g.NQ, g.NQV, g.nreal, g.faceP.data(), g.bndy.data(), t);
    CHECK(t.eligible);
    CHECK((int64_t)t.idE.size() == g.NL * g.nreal && (int64_t)t.tE.size() == g.NL * g.nreal);
    if (!t.eligible || (int64_t)t.idE.size() != g.NL * g.nreal) return;
    int64_t edges = 0;
    for (int64_t e = 0; e < g.nreal; ++e)
        for (int f = 0; f < 4; ++f)
            for (int k = 0; k < g.NQV; ++k) {
                std::vector<int> seen((size_t)g.NQ, 0);
                int slots[2] = {0, 0};
                const int t0 = g.task(f, 0, k);
                const int64_t N0 = g.faceP[g.NFT * e + t0] / g.Np;
                const int k0 = (int)(g.faceP[g.NFT * e + t0] % g.Np) / (g.NQ * g.NQ), f0 = t.tP[(size_t)(g.NL * e + t0)] / g.Nfph;
                for (int a = 0; a < g.NQ; ++a) {
                    const int tt = g.task(f, a, k);
                    const int64_t idP = g.faceP[g.NFT * e + tt], N = idP / g.Np;
                    const int vidP = (int)(idP - N * g.Np), fS = t.tP[(size_t)(g.NL * e + tt)] / g.Nfph;
                    CHECK(N == N0 && vidP / (g.NQ * g.NQ) == k0 && fS == f0);
                    const int idx = lapfused_index_in_face(g.NQ, fS, vidP);
                    CHECK(idx >= 0 && idx < g.NQ);
                    if (idx < 0 || idx >= g.NQ) continue;
                    CHECK(g.face_node(fS, idx, k0) == vidP);  // the index is the position along N's face
                    ++seen[(size_t)idx];
                    const int tE = t.tE[(size_t)(g.NL * e + tt)], idE = t.idE[(size_t)(g.NL * e + tt)];
                    if (tE >= 0) {
                        CHECK(idE == g.faceP[g.NFT * N + tE]);
                        CHECK(idx == 0 || idx == g.NQ - 1);  // y at an end of N's row
                        const int slot = lapfused_edge_slot(g.NQV, f, k, idx == g.NQ - 1);
                        CHECK(slot == 2 * (tt / g.NQ) + (idx == g.NQ - 1 ? 1 : 0) && slot < 8 * g.NQV);
                        ++slots[idx == g.NQ - 1 ? 1 : 0];
                        ++edges;
                    } else {
                        CHECK(idE == -1);
                        CHECK(idx != 0 && idx != g.NQ - 1);
                    }
                }
                for (int n = 0; n < g.NQ; ++n) CHECK(seen[(size_t)n] == 1);
                CHECK(slots[0] == 1 && slots[1] == 1);  // every slot of the edge block has one owner
            }
    CHECK(edges == g.nreal * 8 * g.NQV);
}

void ineligible(const char *what, const Grid &g, const char *reason)
{
    LapFusedTables t;
    lapfused_build(g.NQ, g.NQV, g.nreal, g.faceP.data(), g.bndy.data(), t);
    if (t.eligible || t.why.find(reason) == std::string::npos || !t.tP.empty() || !t.tE.empty() || !t.idE.empty()) {
        printf("FAILED: %s: eligible = %d, reason \"%s\" (wanted \"%s\")\n", what, (int)t.eligible, t.why.c_str(), reason);
        ++failures;
    }
}
}  // namespace

int main()
{
    for (int NQ = 3; NQ <= 5; ++NQ) {
        const int NQV = NQ == 5 ? 3 : NQ;  // (one mixed order)
        rows_and_edges(periodic_patch(NQ, NQV, 2, 2));
        rows_and_edges(periodic_patch(NQ, NQV, 3, 3));
        rows_and_edges(three_panel_corner(NQ, NQV));
    }
    // The hand-made tables below keep every face node seen exactly once from the other side (tP
    // exists and is unique): only the row condition can refuse them.
    {
        // element 0's face 1 against element 1's face 0 on a 3 x 3 patch: position 1 of levels 0 and 1
        // exchanged on the far side
        Grid g = periodic_patch(4, 4, 3, 3);
        g.pair(0, 1, 1, 0, 1, 0, 1, 1);
        g.pair(0, 1, 1, 1, 1, 0, 1, 0);
        ineligible("a row across two levels", g, "straddles two levels");
    }
    {
        // position 2 of faces 1 of elements 0 and 3 (level 0) exchanged between their neighbours 1 and 4
        Grid g = periodic_patch(4, 4, 3, 3);
        g.pair(0, 1, 2, 0, 4, 0, 2, 0);
        g.pair(3, 1, 2, 0, 1, 0, 2, 0);
        ineligible("a row across two neighbours", g, "straddles two neighbours");
    }
    {
        // Two tasks of a row face one node of the neighbour: a vertical edge of it, reached through its
        // two lateral faces.  Position 1 of element 0's row takes element 1's corner column through
        // element 1's face 2; the two face nodes this leaves without a partner (position 1 of element
        // 1's face 0, position 0 of element 7's face 3) face each other.
        Grid g = periodic_patch(4, 4, 3, 3);
        g.pair(0, 1, 1, 0, 1, 2, 0, 0);
        g.pair(1, 0, 1, 0, 7, 3, 0, 0);
        ineligible("a row that repeats an index", g, "repeats an index");
    }
    if (failures) return 1;
    printf("host lapfused lines: ok\n");
    return 0;
}
