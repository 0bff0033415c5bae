// Fused Laplacian pass (kernels.h k_lapfused): the host half of its create-time tables.  The pass
// forms, in the lanes of an element's lateral face nodes, the gradient the NEIGHBOUR holds at the
// plus-side node y -- the neighbour's volume gradient at y plus the lifts of the neighbour's own
// lateral faces that contain y.  What it needs to know of the neighbour N per lateral face task t
// of element e (minus node vidM, plus node faceP[e][t] = N * Np + vidP) is found here, from the
// digested face table (GridDev::faceP) alone:
//   tP[e][t]  the face task of N that is the same mesh node seen from the other side: its minus
//             node is vidP and faceP[N][tP] == e * Np + vidM;
//   tE[e][t]  N's other lateral face task whose minus node is vidP (y on a vertical edge of N), or
//             -1.  Its plus side is the one datum of the second ring of neighbours the pass reads.
// A grid is eligible only if every lateral face of every real element is interior, every plus side
// is a real element, and tP exists and is unique for every lateral face node (a neighbour reached
// through two of its faces at one node -- a one-element-wide periodic direction -- has two).
//
// No HIP in this file: tests/host/host_lapfused.cpp builds it with the host compiler and sanitizers.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

namespace cmdg {

struct LapFusedTables {
    int NQ = 0, NQV = 0;
    int64_t nreal = 0;
    bool eligible = false;
    std::string why;               // why not, when not eligible
    std::vector<int32_t> tP, tE;   // (NL, nreal), NL = 4 NQ NQV lateral face tasks
};

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
        }
    out.eligible = true;
}

}  // namespace cmdg
