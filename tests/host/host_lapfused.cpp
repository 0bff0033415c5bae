// The create-time index tables of the fused Laplacian pass (csrc/lapfused_tables.h) on the host:
// for a 2 x 2 periodic patch and a hand-written three-panel corner (with flipped gluings) the
// defining identities of tP / tE must hold at every lateral face node; a grid with one wall face, a
// neighbour seen through two of its faces at one node, and a plus side outside the real elements
// must come back ineligible, with a reason and without a crash.  Built by
// tests/test_lapfused_tables_host.py with -fsanitize=address,undefined and run as a process of its own.
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
// a grid as cmdg_create digests it: faceP (NFT, nreal), elemtobndy (6, nreal)
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
        // top and bottom are walls: the plus side is the minus node itself
        for (int64_t e = 0; e < nreal; ++e) {
            bndy[4 + 6 * e] = 1, bndy[5 + 6 * e] = 2;
            for (int n = 0; n < NQ * NQ; ++n) {
                faceP[NFT * e + NL + n] = (int32_t)(e * Np + n);
                faceP[NFT * e + NL + NQ * NQ + n] = (int32_t)(e * Np + n + NQ * NQ * (NQV - 1));
            }
        }
    }
    int node(int i, int j, int k) const { return i + NQ * (j + NQ * k); }
    // node of lateral face f at position a along the face, level k
    int face_node(int f, int a, int k) const
    {
        const int E = NQ - 1;
        return f == 0 ? node(0, a, k) : f == 1 ? node(E, a, k) : f == 2 ? node(a, 0, k) : node(a, E, k);
    }
    // glue face f1 of e1 to face f2 of e2, position a on the first meeting a (or E - a) on the second
    void glue(int64_t e1, int f1, int64_t e2, int f2, bool flip)
    {
        for (int k = 0; k < NQV; ++k)
            for (int a = 0; a < NQ; ++a) {
                const int b = flip ? NQ - 1 - a : a;
                faceP[NFT * e1 + f1 * Nfph + a + NQ * k] = (int32_t)(e2 * Np + face_node(f2, b, k));
                faceP[NFT * e2 + f2 * Nfph + b + NQ * k] = (int32_t)(e1 * Np + face_node(f1, a, k));
            }
    }
};

// the defining identities of tP / tE at every lateral face node; returns the number of nodes with a tE
int64_t identities(const Grid &g, const LapFusedTables &t)
{
    int64_t edges = 0;
    CHECK(t.eligible);
    CHECK((int64_t)t.tP.size() == g.NL * g.nreal && (int64_t)t.tE.size() == g.NL * g.nreal);
    if (!t.eligible || (int64_t)t.tP.size() != g.NL * g.nreal) return -1;
    for (int64_t e = 0; e < g.nreal; ++e)
        for (int tt = 0; tt < g.NL; ++tt) {
            const int64_t idP = g.faceP[g.NFT * e + tt], N = idP / g.Np;
            const int vidP = (int)(idP - N * g.Np), vidM = lapfused_face_vid(g.NQ, g.NQV, tt);
            const int tP = t.tP[(size_t)(g.NL * e + tt)], tE = t.tE[(size_t)(g.NL * e + tt)];
            CHECK(tP >= 0 && tP < g.NL);
            if (tP < 0 || tP >= g.NL) continue;
            CHECK(lapfused_face_vid(g.NQ, g.NQV, tP) == vidP);        // its minus node is our plus node
            CHECK(g.faceP[g.NFT * N + tP] == e * g.Np + vidM);         // its plus node is our minus node
            const int i = vidP % g.NQ, j = (vidP / g.NQ) % g.NQ;
            const bool on1 = i == 0 || i == g.NQ - 1, on2 = j == 0 || j == g.NQ - 1;
            CHECK(on1 || on2);
            if (on1 && on2) {  // y on a vertical edge of N: the other lateral face of N at y
                CHECK(tE >= 0 && tE < g.NL && tE != tP);
                if (tE < 0 || tE >= g.NL) continue;
                CHECK(lapfused_face_vid(g.NQ, g.NQV, tE) == vidP);
                CHECK((tE / g.Nfph) / 2 != (tP / g.Nfph) / 2);          // one xi1 face, one xi2 face
                CHECK(g.faceP[g.NFT * N + tE] != e * g.Np + vidM);
                ++edges;
            } else {
                CHECK(tE == -1);
            }
        }
    return edges;
}

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

// three elements round a corner: face 1 of each meets face 3 of the next (the corner at i = j = E
// of all three), face 0 of each meets face 2 of the next with the positions reversed
Grid three_panel_corner(int NQ, int NQV)
{
    Grid g(NQ, NQV, 3);
    for (int e = 0; e < 3; ++e) {
        g.glue(e, 1, (e + 1) % 3, 3, false);
        g.glue(e, 0, (e + 1) % 3, 2, true);
    }
    return g;
}

void ineligible(const char *what, const Grid &g, const char *reason)
{
    LapFusedTables t;
    lapfused_build(g.NQ, g.NQV, g.nreal, g.faceP.data(), g.bndy.data(), t);
    if (t.eligible || t.why.find(reason) == std::string::npos || !t.tP.empty() || !t.tE.empty()) {
        printf("FAILED: %s: eligible = %d, reason \"%s\" (wanted \"%s\")\n", what, (int)t.eligible, t.why.c_str(), reason);
        ++failures;
    }
}
}  // namespace

int main()
{
    for (int NQ = 2; NQ <= 5; ++NQ) {
        const int NQV = NQ == 5 ? 3 : NQ;  // (one mixed order)
        {
            const Grid g = periodic_patch(NQ, NQV, 2, 2);
            LapFusedTables t;
            lapfused_build(g.NQ, g.NQV, g.nreal, g.faceP.data(), g.bndy.data(), t);
            // every element: 4 faces x 2 ends x NQV levels face nodes on a vertical edge of the neighbour
            CHECK(identities(g, t) == 4 * 8 * NQV);
        }
        {
            const Grid g = three_panel_corner(NQ, NQV);
            LapFusedTables t;
            lapfused_build(g.NQ, g.NQV, g.nreal, g.faceP.data(), g.bndy.data(), t);
            CHECK(identities(g, t) == 3 * 8 * NQV);
        }
        {
            const Grid g = periodic_patch(NQ, NQV, 3, 3);  // neighbours across opposite faces differ
            LapFusedTables t;
            lapfused_build(g.NQ, g.NQV, g.nreal, g.faceP.data(), g.bndy.data(), t);
            CHECK(identities(g, t) == 9 * 8 * NQV);
        }
    }
    {
        Grid g = periodic_patch(5, 5, 2, 2);  // one wall face: plus side = minus side, tagged
        g.bndy[1 + 6 * 2] = 1;
        for (int n = 0; n < g.Nfph; ++n) g.faceP[g.NFT * 2 + g.Nfph + n] = (int32_t)(2 * g.Np + g.face_node(1, n % 5, n / 5));
        ineligible("one wall face", g, "lateral face 2 of element 3 is a boundary face");
    }
    {
        // one element whose face 0 is glued to its own face 2 and face 1 to its face 3: the corner
        // node (0, 0) is its own neighbour through both faces
        Grid g(5, 5, 1);
        g.glue(0, 0, 0, 2, false);
        g.glue(0, 1, 0, 3, false);
        ineligible("a neighbour seen through two faces at one node", g, "is seen twice");
    }
    {
        Grid g = periodic_patch(4, 4, 2, 2);  // a plus side that is not the other side of anything
        g.faceP[g.NFT * 1 + 3] = g.faceP[g.NFT * 1 + 2];
        ineligible("a face node nobody faces", g, "is not seen");
    }
    {
        Grid g = periodic_patch(4, 4, 2, 2);  // plus sides outside the real elements
        g.faceP[g.NFT * 0 + 7] = (int32_t)(g.nreal * g.Np);
        ineligible("a ghost on the plus side", g, "no real element");
        g.faceP[g.NFT * 0 + 7] = -5;
        ineligible("a negative plus side", g, "no real element");
    }
    {
        LapFusedTables t;
        lapfused_build(5, 5, 0, nullptr, nullptr, t);
        CHECK(!t.eligible && t.tP.empty());
    }
    if (failures) return 1;
    printf("host lapfused: ok\n");
    return 0;
}
