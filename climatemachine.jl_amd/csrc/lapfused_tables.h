// Fused Laplacian pass (kernels.h k_lapfused): the host half of its create-time tables.  The pass
// forms, in the lanes of an element's lateral face nodes, the gradient the NEIGHBOUR holds at the
// plus-side node y -- the neighbour's volume gradient at y plus the lifts of the neighbour's own
// lateral faces that contain y.  What it needs to know of the neighbour N per lateral face task t
// of element e (minus node vidM, plus node faceP[e][t] = N * Np + vidP) is found here, from the
// digested face table (GridDev::faceP) alone:
//   tP[e][t]  the face task of N that is the same mesh node seen from the other side: its minus
//             node is vidP and faceP[N][tP] == e * Np + vidM;
//   tE[e][t]  N's other lateral face task whose minus node is vidP (y on a vertical edge of N), or
//             -1.  Its plus side is the one datum of the second ring of neighbours the pass reads:
//   idE[e][t] faceP[N][tE], the global node id of that datum, or -1.  The pass is handed idE in the
//             place of tE, so that it can ask for the datum together with N's own records.
// A grid is eligible only if every lateral face of every real element is interior, every plus side
// is a real element, tP exists and is unique for every lateral face node (a neighbour reached
// through two of its faces at one node -- a one-element-wide periodic direction -- has two), and
// every row of face nodes -- the NQ tasks of one lateral face and one level -- faces one row of one
// neighbour: its plus nodes lie in one element, on one level and on one face of it, and their
// indices along that face are a permutation of 0 .. NQ-1.  The pass relies on the last rule: of N's
// two lines of nodes through y the one in the shared face consists of the plus nodes of the sibling
// tasks of the row, which hand their records to each other (kernels.h, the exchange of k_lapfused).
//
// No HIP in this file: tests/host/host_lapfused.cpp builds it with the host compiler and sanitizers.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

// (the two index helpers below are also called by the kernel that fills the tables, cmdg.hip)
#ifdef __HIPCC__
#define CMDG_LAPFUSED_HD __host__ __device__
#else
#define CMDG_LAPFUSED_HD
#endif

namespace cmdg {

struct LapFusedTables {
    int NQ = 0, NQV = 0;
    int64_t nreal = 0;
    bool eligible = false;
    std::string why;               // why not, when not eligible
    std::vector<int32_t> tP, tE;   // (NL, nreal), NL = 4 NQ NQV lateral face tasks
    std::vector<int32_t> idE;      // (NL, nreal)
};

// Where a task with a tE finds N's normal and lift weight at tE (the edge block behind lapT): y is
// the first or the last node of N's row, and every row has exactly one of each.  f, b: the task's
// own face and level; last: y is the last node (index NQ-1 along N's face), not the first.
CMDG_LAPFUSED_HD inline int lapfused_edge_slot(int NQV, int f, int b, bool last)
{
    return 2 * (f * NQV + b) + (last ? 1 : 0);
}
// the index of node vid along lateral face f of its element (the position n % NQ of its face task)
CMDG_LAPFUSED_HD inline int lapfused_index_in_face(int NQ, int f, int vid)
{
    return f < 2 ? (vid / NQ) % NQ : vid % NQ;
}

// volume node of lateral face task t (kernels.h face_vid; Grids.jl:586-594)
inline int lapfused_face_vid(int NQ, int NQV, int t)
{
    const int Nfph = NQ * NQV, f = t / Nfph, n = t % Nfph, a = n % NQ, b = n / NQ;
    switch (f) {
    case 0: return NQ * (a + NQ * b);
    case 1: return (NQ - 1) + NQ * (a + NQ * b);
    case 2: return a + NQ * NQ * b;
    default: return a + NQ * ((NQ - 1) + NQ * b);
    }
}

// the (at most two) lateral face tasks whose minus node is `vid`: one of a xi1 face, one of a xi2
// face; -1 where the node is not on such a face
inline void lapfused_tasks_of(int NQ, int NQV, int vid, int out[2])
{
    const int Nfph = NQ * NQV, i = vid % NQ, j = (vid / NQ) % NQ, k = vid / (NQ * NQ);
    out[0] = i == 0 ? j + NQ * k : (i == NQ - 1 ? Nfph + j + NQ * k : -1);
    out[1] = j == 0 ? 2 * Nfph + i + NQ * k : (j == NQ - 1 ? 3 * Nfph + i + NQ * k : -1);
}

// faceP: (NFT, nreal) as GridDev::faceP, elemtobndy: (6, nelem) as the reference's.  Never fails:
// a grid the pass cannot take comes back with eligible == false and the reason.
inline void lapfused_build(int NQ, int NQV, int64_t nreal, const int32_t *faceP, const int64_t *elemtobndy,
                           LapFusedTables &out)
{
    out = LapFusedTables();
    out.NQ = NQ;
    out.NQV = NQV;
    out.nreal = nreal;
    auto no = [&](const std::string &m) {
        out.eligible = false;
        out.why = m;
        out.tP.clear();
        out.tE.clear();
        out.idE.clear();
    };
    if (NQ < 2 || NQV < 1 || nreal < 1 || !faceP || !elemtobndy) return no("empty grid");
    const int Np = NQ * NQ * NQV, Nfph = NQ * NQV, NL = 4 * Nfph, NFT = NL + 2 * NQ * NQ;
    auto str = [](int64_t v) { return std::to_string(v); };
    for (int64_t e = 0; e < nreal; ++e)
        for (int f = 0; f < 4; ++f)
            if (elemtobndy[f + 6 * e] != 0)
                return no("lateral face " + str(f + 1) + " of element " + str(e + 1) + " is a boundary face");
    out.tP.assign((size_t)(NL * nreal), -1);
    out.tE.assign((size_t)(NL * nreal), -1);
    out.idE.assign((size_t)(NL * nreal), -1);
    for (int64_t e = 0; e < nreal; ++e)
        for (int t = 0; t < NL; ++t) {
            const int64_t idP = faceP[NFT * e + t];
            const int64_t me = e * Np + lapfused_face_vid(NQ, NQV, t);
            if (idP < 0 || idP >= nreal * Np)
                return no("face task " + str(t) + " of element " + str(e + 1) + " has no real element on its plus side");
            const int64_t N = idP / Np;
            int cand[2];
            lapfused_tasks_of(NQ, NQV, (int)(idP - N * Np), cand);
            int found = -1, other = -1, matches = 0;
            for (int c = 0; c < 2; ++c) {
                if (cand[c] < 0) continue;
                if (faceP[NFT * N + cand[c]] == me) {
                    if (matches++ == 0) found = cand[c];
                } else {
                    other = cand[c];
                }
            }
            if (matches != 1)
                return no("face task " + str(t) + " of element " + str(e + 1) + (matches == 0 ? " is not seen" : " is seen twice") +
                          " from its neighbour " + str(N + 1));
            out.tP[(size_t)(NL * e + t)] = found;
            out.tE[(size_t)(NL * e + t)] = other;
            if (other >= 0) out.idE[(size_t)(NL * e + t)] = faceP[NFT * N + other];
        }
    // the rows: the NQ tasks of lateral face f at level b against the first of them
    for (int64_t e = 0; e < nreal; ++e)
        for (int r = 0; r < 4 * NQV; ++r) {
            const int f = r / NQV, b = r % NQV, t0 = f * Nfph + NQ * b;
            const std::string row = "the row of face " + str(f + 1) + ", level " + str(b + 1) + " of element " + str(e + 1);
            const int64_t N0 = faceP[NFT * e + t0] / Np;
            const int k0 = (int)(faceP[NFT * e + t0] - N0 * Np) / (NQ * NQ), f0 = out.tP[(size_t)(NL * e + t0)] / Nfph;
            unsigned seen = 0;
            for (int a = 0; a < NQ; ++a) {
                const int64_t idP = faceP[NFT * e + t0 + a], N = idP / Np;
                const int vidP = (int)(idP - N * Np);
                if (N != N0) return no(row + " straddles two neighbours");
                if (vidP / (NQ * NQ) != k0) return no(row + " straddles two levels of its neighbour");
                // (two tasks at one node of N can each have their tP, on N's two faces there: the
                // repeated index is what names that, so it is looked for first)
                const unsigned bit = 1u << lapfused_index_in_face(NQ, f0, vidP);
                if (seen & bit) return no(row + " repeats an index along its neighbour's face");
                seen |= bit;
                if (out.tP[(size_t)(NL * e + t0 + a)] / Nfph != f0) return no(row + " straddles two faces of its neighbour");
            }
        }
    out.eligible = true;
}

}  // namespace cmdg
