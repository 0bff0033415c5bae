// What the pass kernels and the nodal kernels share: the arguments of a pass, the face and volume
// helpers, the launch shape of the tendency pass and the hand-off of the gradient arguments.
#pragma once
#include "cmdg_common.h"
#include "law_defaults.h"

// minimum waves per SIMD requested from the register allocator (tuning knobs)
#ifndef CMDG_TEND_MINW
#define CMDG_TEND_MINW 1
#endif
// elements per work-group of k_tendency for N >= 5 (see TendencyShape)
#ifndef CMDG_TEND_EPB_LARGE
#define CMDG_TEND_EPB_LARGE 2
#endif
// ... and for N <= 4 (one: 192 threads, minus side of the faces staged in LDS; two measured
// slower on Held-Suarez and on the rising bubble, profiles/r03_ab_two_elements_n4.txt)
#ifndef CMDG_TEND_EPB_SMALL
#define CMDG_TEND_EPB_SMALL 1
#endif
// k_gradients: the Held-Suarez instantiation needs 130 VGPRs unconstrained (3 waves/SIMD);
// asking for 4 gives 128 without scratch and 9 % less time per launch (profiles/r01_ab_*.txt)
#ifndef CMDG_GRAD_MINW
#define CMDG_GRAD_MINW 4
#endif
#ifndef CMDG_GRAD_BOUND_LARGE
#define CMDG_GRAD_BOUND_LARGE 1024
#endif
#ifndef CMDG_LAP_MINW
#define CMDG_LAP_MINW 1
#endif
// k_lapfused: 4 waves per SIMD keep five work-groups of N = 4 resident (<= 128 VGPRs)
#ifndef CMDG_LAPFUSED_MINW
#define CMDG_LAPFUSED_MINW 4
#endif

namespace cmdg {

// ---------------------------------------------------------------------------------
template <class P>
struct PassArgs {
    typename P::Params prm;
    GridDev g;
    const int64_t *elems;  // 1-based element list (interior or exterior)
    int64_t nelems;
    // state arrays
    const double *Q;
    const double *aux;
    double *aux_rw;         // same array, for the fused auxiliary refresh
    const double *derived;  // handle-owned time-invariant per-node fields of the law (P::NDER)
    double *gf;        // state_gradient_flux (written by gradients, read by tendency)
    double *hypgrad;   // Qhypervisc_grad
    double *hypdiv;    // Qhypervisc_div
    double *tendency;  // tendency (== dQ when the LSRK update is fused)
    double *Qout;      // LSRK: updated state
    double *garg;      // gradient arguments handed from a fused update to the next stage (GradArgHandoff)
    double *lapr;      // Laplacian records of a ring-ordered evaluation (k_divgrad / k_gradlap RING)
    int hypdiv_out;    // k_divgrad<RING>: write the caller's Qhypervisc_div as well (uniform)
    double t, alpha, beta;
    const double *tptr;  // time of the evaluation in device memory (a captured step is replayed
                         // with the time a one-thread kernel of the graph advances); NULL: t
    double rkb_dt, rka_next;
    int direction;     // direction of this pass (dg.direction or dg.diffusion_direction)
    int model_dir;     // dg.direction handed to the pointwise fluxes
    int nf_first;
    HaloDev h;         // ghost exchange without pack / unpack launches (cmdg_common.h)
};

struct FacePt {
    double n[3], sM, vMI;
    double w;  // vMI * sM out of the digest (LIFTW passes, which then load neither factor)
    int64_t eP;
    int vidM, vidP, bctag;
};

// Volume node of face node n of face f: faces 1..6 = xi1-, xi1+, xi2-, xi2+, xi3-, xi3+, the
// remaining two indices in order, lower axis fastest (Grids.jl:586-594).  This is vmap- minus
// the element offset; cmdg_create checks the caller's vmap- against it.
template <int NQ, int NQV = NQ>
__host__ __device__ __forceinline__ constexpr int face_vid(int f, int n)
{
    const int a = n % NQ, b = n / NQ;
    switch (f) {
    case 0: return NQ * (a + NQ * b);
    case 1: return (NQ - 1) + NQ * (a + NQ * b);
    case 2: return a + NQ * NQ * b;
    case 3: return a + NQ * ((NQ - 1) + NQ * b);
    case 4: return n;
    default: return n + NQ * NQ * (NQV - 1);
    }
}

// index half of face_setup: issued at kernel start so that the plus-side gathers do not wait
// for a dependent table load when the interface phase begins
template <int NQ, int NQV = NQ>
__device__ __forceinline__ void face_index(const GridDev &g, int64_t e, int t, int f, int32_t &idP,
                                           int &bctag)
{
    idP = g.faceP[(int64_t)KDims<NQ, NQV>::NFT * e + t];
    bctag = (int)g.elemtobndy[f + 6 * e];
}
// LIFTW: the lift weight vMI * sM comes from GridDev::faceW (the gradient, Laplacian and
// gradient-of-Laplacian passes, whose face phase uses the two factors only in that product)
template <int NQ, int NQV = NQ, bool LIFTW = false>
__device__ __forceinline__ void face_geometry(const GridDev &g, int64_t e, int t, int f, int n,
                                              int32_t idP, int bctag, FacePt &fp)
{
    constexpr int Np = KDims<NQ, NQV>::Np, NFT = KDims<NQ, NQV>::NFT;
    const double *sg = g.faceG + (int64_t)4 * NFT * e + t;
    fp.n[0] = sg[0];
    fp.n[1] = sg[NFT];
    fp.n[2] = sg[2 * NFT];
    fp.vidM = face_vid<NQ, NQV>(f, n);
    if constexpr (LIFTW) {
        fp.w = g.faceW[(int64_t)NFT * e + t];
    } else {
        fp.sM = sg[3 * NFT];
        fp.vMI = g.vgeo[fp.vidM + (int64_t)Np * (VMI + (int64_t)g.nvgeo * e)];
    }
    fp.bctag = bctag;
    fp.eP = idP / Np;
    fp.vidP = idP - (int)fp.eP * Np;
}
template <int NQ, int NQV = NQ, bool LIFTW = false>
__device__ __forceinline__ void face_setup(const GridDev &g, int64_t e, int t, int f, int n,
                                           FacePt &fp)
{
    int32_t idP;
    int bctag;
    face_index<NQ, NQV>(g, e, t, f, idP, bctag);
    face_geometry<NQ, NQV, LIFTW>(g, e, t, f, n, idP, bctag, fp);
}

// The optional members of a law functor P, their defaults and what each stands for: law_defaults.h.

// is the law's state_gradient_flux kept node-major (P::GF_NODE_MAJOR, and there is one)
template <class P>
inline constexpr bool gf_node_major = P::GF_NODE_MAJOR && P::NGF > 0;
template <class P, int Np>
__device__ __forceinline__ int64_t gf_at(int n, int s, int64_t e)
{
    return col_at<gf_node_major<P>, P::NGF, Np>(n, s, e);
}
template <class P, int Np>
__device__ __forceinline__ void load_gf(Vec<P::NGF> &dst, const double *__restrict__ arr, int n, int64_t e)
{
#pragma unroll
    for (int s = 0; s < P::NGF; ++s) dst[s] = arr[gf_at<P, Np>(n, s, e)];
}
template <class P, int Np>
__device__ __forceinline__ void load_plus_gf(Vec<P::NGF> &dst, const double *__restrict__ arr,
                                             const double *__restrict__ recv, int gslot, int vidP, int64_t eP)
{
    if (gslot >= 0) {
#pragma unroll
        for (int s = 0; s < P::NGF; ++s) dst[s] = recv[s + (int64_t)P::NGF * gslot];
    } else {
        load_gf<P, Np>(dst, arr, vidP, eP);
    }
}

// numerical_flux_first_order!  NumericalFluxes.jl:223-285 (Rusanov) / :300-340 (central)
template <class P>
__device__ __forceinline__ void nf_first_order(const typename P::Params &prm, int nf,
                                               Vec<P::NS> &fluxn, const double *n,
                                               const double *QM, const double *auxM,
                                               const double *QP, const double *auxP, double t,
                                               int facedir)
{
    constexpr int NS = P::NS;
    if constexpr (P::LAW_NF) {
        if (nf >= NF_ROE) {
            P::numerical_flux_law(prm, nf, fluxn, n, QM, auxM, QP, auxP, t, facedir);
            return;
        }
    }
    Vec<3 * NS> FM, FP;
    Vec<NS> wM, wP;
    FM.negzero();
    FP.negzero();
    if constexpr (P::HAS_FLUX_WAVESPEED) {
        if (nf == NF_RUSANOV) {
            P::flux_wavespeed(prm, FM, wM, n, QM, auxM, t, facedir);
            P::flux_wavespeed(prm, FP, wP, n, QP, auxP, t, facedir);
        } else {
            P::flux_first_order(prm, FM, QM, auxM, t, facedir);
            P::flux_first_order(prm, FP, QP, auxP, t, facedir);
        }
    } else {
        P::flux_first_order(prm, FM, QM, auxM, t, facedir);
        P::flux_first_order(prm, FP, QP, auxP, t, facedir);
    }
    const double nh0 = n[0] / 2, nh1 = n[1] / 2, nh2 = n[2] / 2;
#pragma unroll
    for (int s = 0; s < NS; ++s)
        fluxn[s] += (FM[3 * s] + FP[3 * s]) * nh0 + (FM[3 * s + 1] + FP[3 * s + 1]) * nh1 +
                    (FM[3 * s + 2] + FP[3 * s + 2]) * nh2;
    if (nf == NF_RUSANOV) {
        if constexpr (!P::HAS_FLUX_WAVESPEED) {
            P::wavespeed(prm, wM, n, QM, auxM, t, facedir);
            P::wavespeed(prm, wP, n, QP, auxP, t, facedir);
        }
        Vec<NS> pen;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const double mw = wM[s] > wP[s] ? wM[s] : wP[s];
            pen[s] = mw * (QM[s] - QP[s]);
        }
        if constexpr (P::HAS_PENALTY) P::update_penalty(prm, pen, n, QM, QP);  // (:266-279)
#pragma unroll
        for (int s = 0; s < NS; ++s) fluxn[s] += pen[s] / 2;
    }
}

// ---------------------------------------------------------------------------------
// Index of a surface node among the element's surface nodes (-1: interior node).  The
// minus-side face data of the interface phases is staged in LDS for surface nodes only.
template <int NQ, int NQV = NQ>
__device__ __forceinline__ int surf_index(int ijk)
{
    constexpr int NI = NQ - 2, NIV = NQV > 2 ? NQV - 2 : 0;
    const int i = ijk % NQ, j = (ijk / NQ) % NQ, k = ijk / (NQ * NQ);
    const bool ii = i >= 1 && i <= NI, jj = j >= 1 && j <= NI, kk = k >= 1 && k <= NIV;
    if (ii && jj && kk) return -1;
    auto clampi = [](int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); };
    int before = NI * NI * clampi(k - 1, NIV);
    if (kk) {
        before += NI * clampi(j - 1, NI);
        if (jj) before += clampi(i - 1, NI);
    }
    return ijk - before;
}
template <int NQ, int NQV = NQ>
struct SurfDims {
    static constexpr int NSURF =
        NQ * NQ * NQV - (NQ - 2) * (NQ - 2) * (NQV > 2 ? NQV - 2 : 0);
};

// compute_gradient_flux! of a node whose gradient ARGUMENT G is at hand (P::HAS_GRADIENT_FLUX_G)
template <class P>
__device__ __forceinline__ void law_gradient_flux(const typename P::Params &prm, double *gf,
                                                  const double *g, const double *Q, const double *aux,
                                                  double t, const double *G)
{
    if constexpr (P::HAS_GRADIENT_FLUX_G)
        P::gradient_flux_g(prm, gf, g, Q, aux, t, G);
    else
        P::gradient_flux(prm, gf, g, Q, aux, t);
}

// the register budget of the gradient pass: the law's own (P::GRAD_MIN_WAVES) or the library's
template <class P>
inline constexpr int grad_min_waves = P::GRAD_MIN_WAVES > 0 ? P::GRAD_MIN_WAVES : CMDG_GRAD_MINW;

// ---------------------------------------------------------------------------------
// Launch shape of the tendency pass.  N <= 4: one element per work-group, 192 threads.  Larger
// elements: 343 nodes are six waves, which the four SIMDs of a CU take as 2-1-2-1 -- two of them
// carry twice the work and a second six-wave work-group does not become resident above 128
// VGPRs (profiles/r02_lds_occupancy.jsonl).  Two elements per work-group (686 threads, eleven
// waves, 3-3-3-2) even that out; the minus side of the faces is then read from memory instead
// of being staged, so that both elements' flux buffers fit the LDS of a CU.  The other shapes
// measured -- the pass in two launches (volume, then interface + update), paired work-groups that
// keep a shared xi1 face on chip, four-wave work-groups for large elements -- lost and were removed
// (DESIGN.md Appendix A).
template <class P, int NQ, int NQV>
struct TendencyShape {
    using KD = KDims<NQ, NQV>;
    static constexpr int EPB = KD::Np > 125 ? CMDG_TEND_EPB_LARGE : CMDG_TEND_EPB_SMALL;
    static constexpr bool STAGE_M = EPB == 1;  // minus side of the faces staged in LDS
    static constexpr int NTE = EPB == 1 ? KD::NT : (KD::Np > KD::NFT ? KD::Np : KD::NFT);  // threads per element
    static constexpr int NT = EPB == 1 ? KD::NT : ((EPB * NTE + 63) / 64) * 64;
    static int64_t blocks(int64_t nelems) { return (nelems + EPB - 1) / EPB; }
};

// ---------------------------------------------------------------------------------
// Hand-off of the gradient arguments inside cmdg_lsrk_run.  The input of stage s+1 is the Q+ the
// fused update of stage s holds in LDS, and P::gradient_argument is a pure function of the node's
// (Q, aux) whose time argument is unused.  A law that says so (P::GRADARG_HANDOFF, law_defaults.h)
// gets two more instantiations: k_tendency<..., GARG_OUT> evaluates the argument of Q+ once
// per node, stores the entries the USE_GF = false gradient pass consumes (those of
// gradient_argument_mask<P, false>(), entry s = G[hv_indexmap(s)]) as one record per node in a
// library-owned array, node-major like Qhypervisc_grad -- (NGL, Np, nelem) -- and does the nodal
// auxiliary refresh for Q+; k_gradients<..., GARG_IN> of the next stage reads and gathers those
// records instead of 9 columns of Q / aux per node and per interior face node.  Same expressions on
// the same operands: every bit downstream is unchanged.  One element per work-group only.
// An evaluation that reads the records also keeps its Laplacians as records of NGL doubles in the
// face-contiguous order (cmdg_common.h ring_slot; PassArgs::lapr): k_divgrad<..., RING> writes them,
// k_gradlap<..., RING> reads its own and gathers the plus side from them -- one 32-byte record out
// of one contiguous run per face instead of four columns of Qhypervisc_div.  That launch is handed
// GridDev::facePr as faceP, so its FacePt's vidP is the ring slot of the plus-side node.  The
// records themselves and grad G stay in the natural node order: ring-ordered they measured no
// faster in any pass (profiles/ab_face_contiguous.txt).
// A run's hand-off launches follow one another with no hook, filter, exchange or caller in between,
// so the columns the refresh writes are seen by somebody only after the last of them (it leaves the
// auxiliary state of the final evaluation's input, as every run promises).  The other hand-off
// launches of a law that says P::GRADARG_REFRESH_UNREAD run k_tendency<..., GARG_OUT, false>, which
// neither calls update_aux nor stores the columns.
template <class P, int NQ, int NQV>
struct GradArgHandoff {
    static constexpr bool value = P::GRADARG_HANDOFF && P::NGL > 0 && P::HAS_UPDATE_AUX && P::FUSE_UPDATE_AUX &&
                                  TendencyShape<P, NQ, NQV>::EPB == 1;
    // may the refresh be left out of the hand-off launches nobody can observe
    static constexpr bool elide_refresh = value && P::GRADARG_REFRESH_UNREAD;
};
template <int NGL, int Np>
__device__ __forceinline__ int64_t garg_at(int n, int64_t e)
{
    return (int64_t)NGL * (n + (int64_t)Np * e);
}


}  // namespace cmdg
