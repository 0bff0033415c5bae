// Hand-written gfx950 kernels of the DG hot path.  One workgroup per element (the tendency pass
// of elements above N = 4 takes two, see TendencyShape):
//   phase 1  thread = volume node: pointwise physics, contravariant fluxes / gradient
//            arguments staged in LDS;
//   phase 2  thread = volume node: (N+1)-point contractions with D out of LDS, result
//            into an LDS accumulator;
//   phase 3  thread = face node (6 faces x Nfp tasks at once): numerical / boundary
//            fluxes, lifted into the LDS accumulator one opposite-face pair at a time
//            (race free, reference order);
//   phase 4  thread = volume node: one coalesced store per output field (for the
//            tendency kernel with the LSRK update fused in).
// Each kernel replaces a *group* of reference kernels (horizontal + vertical volume
// kernel and the per-direction interface launches) of
// src/Numerics/DGMethods/DGModel_kernels.jl; the accumulation order of the reference
// is kept term by term (see DESIGN.md "summation order").
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

// ---------------------------------------------------------------------------------
// Tendency pass: volume_tendency! (:64-548) + dgsem_interface_tendency! (:588-901),
// optionally fused with the LSRK update! (LowStorageRungeKuttaMethod.jl:146-158).
// RECV: the plus side of ghost neighbours comes from the receive buffers (exterior launches of a
// handle whose exchanges are not unpacked).  A variant of its own: the second addressing mode
// costs the Held-Suarez instantiation 24 VGPRs (128 -> 150, one wave per SIMD less), which the
// interior launches and single-rank handles do not pay.
// The pass is bound by its chain of dependent loads, not by bytes, so its memory round trips are
// issued as early as registers allow: the metric rows go out with the state, before the flux
// arithmetic (METRICS_FIRST), and the old tendency of all states in one batch ahead of the
// contraction instead of one dependent load per state inside it (profiles/r04_ab_tendency_hoist.txt;
// gathering every plus-side value of a face node before the first-order flux lost).
// GARG_OUT: the fused update also forms the next stage's gradient arguments and refreshes the
// nodal auxiliary state for Q+ (GradArgHandoff).  The auxiliary columns both need are dead in
// registers by then: they are loaded again after the face phase, in flight across the lift.
// GARG_REFRESH = false: the records alone (GradArgHandoff::elide_refresh).
template <class P, int NQ, int NQV, bool LSRK, bool USE_GF, bool RECV = false, bool GARG_OUT = false,
          bool GARG_REFRESH = true>
__device__ __forceinline__ void tendency_body(const PassArgs<P> &a)
{
    static_assert(!GARG_OUT || (LSRK && !USE_GF && !RECV && TendencyShape<P, NQ, NQV>::EPB == 1),
                  "the hand-off rides in the fused update of single-rank handles");
    static_assert(GARG_REFRESH || (GARG_OUT && GradArgHandoff<P, NQ, NQV>::elide_refresh),
                  "only a hand-off launch of a law that opts in may leave the refresh out");
    using KD = KDims<NQ, NQV>;
    const double a_t = a.tptr ? *a.tptr : a.t;  // (uniform: one scalar load)
    using SH = TendencyShape<P, NQ, NQV>;
    constexpr int EPB = SH::EPB;
    constexpr bool STAGE_M = SH::STAGE_M;
    constexpr int Np = KD::Np, NS = P::NS, NAUX = P::NAUX, NGF = P::NGF,
                  NHYP = P::NHYP, NHG = 3 * P::NGL, NFA = P::NFAUX,
                  NSURF = SurfDims<NQ, NQV>::NSURF, NGFS = USE_GF ? NGF : 0,
                  NMF = STAGE_M ? NFA + NGFS + NHYP : 0;
    // LDS: sD derivative matrices; sF_ contravariant flux [d][s][ijk], later the accumulator; sM_ minus
    // side, surface nodes [field][sidx]; sQ_ the prognostic state of every node (minus side of the
    // faces, and the "Q" of the fused update at the end: re-reading it from memory 20 us after the
    // first read misses L2).  (Reached through pointers, and the body kept out of the kernel: either
    // change alters the generated code, though not the results.)
    __shared__ double aD[NQ * NQ + (NQV == NQ ? 0 : NQV * NQV)], aF[EPB * 3 * NS * Np],
        aM[EPB * (NMF > 0 ? NMF : 1) * (NMF > 0 ? NSURF : 1)], aQ[EPB * NS * Np];
    double *sD = aD, *sF_ = aF, *sM_ = aM, *sQ_ = aQ;
    const double *const sDv = sD + (NQV == NQ ? 0 : NQ * NQ);  // vertical derivative matrix
    // this thread's element of the work-group and its index there
    const int sub = EPB == 1 ? 0 : (int)threadIdx.x / SH::NTE;
    const int tid = EPB == 1 ? (int)threadIdx.x : (int)threadIdx.x - sub * SH::NTE;
    const int64_t li = (int64_t)EPB * xcd_remap(blockIdx.x, gridDim.x) + sub;
    const bool live = EPB == 1 || (sub < EPB && li < a.nelems);
    const int64_t e = live ? a.elems[li] - 1 : 0;
    const int lsub = live ? sub : 0;
    double *const sF = sF_ + lsub * (3 * NS * Np);
    double *const sM = sM_ + lsub * ((NMF > 0 ? NMF : 1) * (NMF > 0 ? NSURF : 1));
    double *const sQ = sQ_ + lsub * (NS * Np);
    double *const sT = sF;              // tendency accumulator [s][ijk] (aliases sF after phase 2)
    if (threadIdx.x < NQ * NQ) sD[threadIdx.x] = a.g.D[threadIdx.x];
    if constexpr (NQV != NQ) {
        if (threadIdx.x < NQV * NQV) sD[NQ * NQ + threadIdx.x] = a.g.Dv[threadIdx.x];
    }
    const bool hz = a.direction != DIR_VERTICAL, vt = a.direction != DIR_HORIZONTAL;
    // USE_GF: does flux_second_order depend on the gradient-flux state at all?  With zero
    // viscosity (Held-Suarez) tau = -2*0*S and D_t = 0: the 9 fields only ever multiply
    // zeros, so the host picks the instantiation that does not read them (identical results).
    constexpr bool use_gf = NGF > 0 && USE_GF;
    // the hyperdiffusive inviscid instantiation at N <= 4 (Held-Suarez): 126 VGPRs, five work-groups
    // per CU, and its SIMDs issue fp64 VALU work 60 % of the time
    constexpr bool HS_SHAPE = NHYP > 0 && !use_gf && Np <= 125 && NS >= 5;
    int32_t f_idP = 0;
    int f_bctag = 0, f_f = 0, f_n = 0;
    KD::face_task(tid, f_f, f_n);
    const bool face_on = live && tid < KD::NFT && (f_f < 4 ? hz : vt);
    if (face_on) face_index<NQ, NQV>(a.g, e, tid, f_f, f_idP, f_bctag);
    Vec<NS> S;
    double MI = 0;
    if (live && tid < Np) {
        const double *vg = a.g.vgeo + (int64_t)Np * a.g.nvgeo * e + tid;
        const double M = vg[VM * Np];
        MI = vg[VMI * Np];
        Vec<NS> lQ;
        Vec<NAUX> laux;
        Vec<NGF> lgf;
        Vec<NHYP> lhyp;
        double x11 = 0, x12 = 0, x13 = 0, x21 = 0, x22 = 0, x23 = 0, x31 = 0, x32 = 0, x33 = 0;
        // the metric rows with the first batch of loads -- unless that costs a work-group of
        // residency: the hyperdiffusive inviscid instantiation at N <= 4 (Held-Suarez) sits at 126
        // VGPRs, five work-groups per CU; with nine more doubles live across the flux arithmetic it
        // takes 148 and runs on four (661 us against 636; rising bubble 132 -> 124 us, BOMEX 589 -> 578)
        constexpr bool METRICS_FIRST = !HS_SHAPE;
        if constexpr (METRICS_FIRST) {
            if (hz) {
                x11 = vg[XI1X1 * Np], x12 = vg[XI1X2 * Np], x13 = vg[XI1X3 * Np];
                x21 = vg[XI2X1 * Np], x22 = vg[XI2X2 * Np], x23 = vg[XI2X3 * Np];
            }
            if (vt) x31 = vg[XI3X1 * Np], x32 = vg[XI3X2 * Np], x33 = vg[XI3X3 * Np];
        }
        load_state<NS, Np>(lQ, a.Q, tid, e);
        load_state<NAUX, Np>(laux, a.aux, tid, e);
#pragma unroll
        for (int s = 0; s < NGF; ++s) lgf[s] = 0.0;
        if (use_gf) load_gf<P, Np>(lgf, a.gf, tid, e);
#pragma unroll
        for (int s = 0; s < NHYP; ++s)
            lhyp[s] = a.hypgrad[hg_at<NHG, Np>(tid, s, e)];
        if constexpr (METRICS_FIRST) __builtin_amdgcn_sched_barrier(0);  // (all of them in flight here)
        const int sidx = surf_index<NQ, NQV>(tid);
#pragma unroll
        for (int s = 0; s < NS; ++s) sQ[s * Np + tid] = lQ[s];
        if (STAGE_M && sidx >= 0) {  // stage the minus side of the interface phase
#pragma unroll
            for (int s = 0; s < NFA; ++s) sM[s * NSURF + sidx] = laux[P::face_aux(s)];
            if (use_gf) {
#pragma unroll
                for (int s = 0; s < NGF; ++s) sM[(NFA + s) * NSURF + sidx] = lgf[s];
            }
#pragma unroll
            for (int s = 0; s < NHYP; ++s) sM[(NFA + NGFS + s) * NSURF + sidx] = lhyp[s];
        }
        Vec<3 * NS> F, F2;
        F.negzero();
        P::flux_first_order(a.prm, F, lQ, laux, a_t, a.model_dir);
        F2.negzero();
        P::flux_second_order(a.prm, F2, lQ, lgf, lhyp, laux, a_t);
#pragma unroll
        for (int q = 0; q < 3 * NS; ++q) F[q] += F2[q];
        if (hz) {
            if constexpr (!METRICS_FIRST) {
                x11 = vg[XI1X1 * Np], x12 = vg[XI1X2 * Np], x13 = vg[XI1X3 * Np];
                x21 = vg[XI2X1 * Np], x22 = vg[XI2X2 * Np], x23 = vg[XI2X3 * Np];
            }
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const double F1 = F[3 * s], F2_ = F[3 * s + 1], F3 = F[3 * s + 2];
                sF[(0 * NS + s) * Np + tid] = M * (x11 * F1 + x12 * F2_ + x13 * F3);
                sF[(1 * NS + s) * Np + tid] = M * (x21 * F1 + x22 * F2_ + x23 * F3);
            }
        }
        if (vt) {
            // (both directions' rows in ONE late batch were tried too: nine doubles live across the two
            // blocks cost the same 24 VGPRs as the early batch)
            if constexpr (!METRICS_FIRST) x31 = vg[XI3X1 * Np], x32 = vg[XI3X2 * Np], x33 = vg[XI3X3 * Np];
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const double F1 = F[3 * s], F2_ = F[3 * s + 1], F3 = F[3 * s + 2];
                sF[(2 * NS + s) * Np + tid] = M * (x31 * F1 + x32 * F2_ + x33 * F3);
            }
        }
        S.negzero();
        if constexpr (P::HAS_SOURCE) {
            Vec<P::NDER> lder;
            load_state<P::NDER, Np>(lder, a.derived, tid, e);
            P::source(a.prm, S, lQ, lgf, laux, lder, a_t, a.model_dir);
        }
    }
    __syncthreads();
    Vec<NS> Tv;
    if (live && tid < Np) {
        const int i = tid % NQ, j = (tid / NQ) % NQ, k = tid / (NQ * NQ);
        Vec<NS> Tprev;  // the old tendency, one batch of loads
#pragma unroll
        for (int s = 0; s < NS; ++s) Tprev[s] = 0.0;
        if (a.beta != 0) {
#pragma unroll
            for (int s = 0; s < NS; ++s) Tprev[s] = a.tendency[tid + (int64_t)Np * (s + (int64_t)NS * e)];
        }
        // MI * D does not depend on the state, but the compiler forms it (and reads D) once per
        // state: it does not merge across the per-state direction tests.  Where the instruction
        // stream is a bound (HS_SHAPE) the 15 products are formed once -- (MI * D) * F as before; the
        // other instantiations keep their code and their registers (30 more VGPRs would move some).
        double mDi[NQ], mDj[NQ], mDk[NQV];
#pragma unroll
        for (int n = 0; n < NQ; ++n) mDi[n] = mDj[n] = 0.0;
#pragma unroll
        for (int kk = 0; kk < NQV; ++kk) mDk[kk] = 0.0;
        if constexpr (HS_SHAPE) {
            if (hz) {
#pragma unroll
                for (int n = 0; n < NQ; ++n) {
                    mDi[n] = MI * sD[n + NQ * i];
                    mDj[n] = MI * sD[n + NQ * j];
                }
            }
            if (vt) {
#pragma unroll
                for (int kk = 0; kk < NQV; ++kk) mDk[kk] = MI * sDv[kk + NQV * k];
            }
        }
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            double T = 0.0;
            const double Told = Tprev[s];
            if (hz) {  // generic kernel called with HorizontalDirection() (:64-309)
                double lt = 0.0;
                if (a.direction == DIR_HORIZONTAL && P::HAS_SOURCE) lt += S[s];
#pragma unroll
                for (int n = 0; n < NQ; ++n) {
                    lt += (HS_SHAPE ? mDi[n] : MI * sD[n + NQ * i]) * sF[(0 * NS + s) * Np + n + NQ * (j + NQ * k)];
                    lt += (HS_SHAPE ? mDj[n] : MI * sD[n + NQ * j]) * sF[(1 * NS + s) * Np + i + NQ * (n + NQ * k)];
                }
                T = a.beta != 0 ? a.alpha * lt + a.beta * Told : a.alpha * lt;
            }
            if (vt) {  // ::VerticalDirection kernel (:312-548); beta = true after the
                       // horizontal call in EveryDirection (SpaceDiscretization.jl:1192)
                double lt = 0.0;
#pragma unroll
                for (int kk = 0; kk < NQV; ++kk) {
                    lt += (HS_SHAPE ? mDk[kk] : MI * sDv[kk + NQV * k]) * sF[(2 * NS + s) * Np + i + NQ * (j + NQ * kk)];
                    if (kk == k && P::HAS_SOURCE) lt += S[s];
                }
                if (hz)
                    T = a.alpha * lt + T;
                else
                    T = a.beta != 0 ? a.alpha * lt + a.beta * Told : a.alpha * lt;
            }
            Tv[s] = T;
        }
    }
    __syncthreads();  // every read of sF is done: it becomes the accumulator sT
    if (live && tid < Np) {
#pragma unroll
        for (int s = 0; s < NS; ++s) sT[s * Np + tid] = Tv[s];
    }
    // ---- faces: dgsem_interface_tendency! ------------------------------------------
    Vec<NS> lift;
    int vidM = 0, fpair = -1;
    if (tid < KD::NFT) {
        int f, n;  // recomputed: cheaper than two registers live across the volume phases
        KD::face_task(tid, f, n);
        if (face_on) {
            const int facedir = f < 4 ? DIR_HORIZONTAL : DIR_VERTICAL;
            FacePt fp;
            face_geometry<NQ, NQV>(a.g, e, tid, f, n, f_idP, f_bctag, fp);
            Vec<NS> QM, QPn, QPd, flux;
            Vec<NAUX> auxM, auxPn, auxPd;
            Vec<NGF> gfM, gfP;
            Vec<NHYP> hypM, hypP;
            const int sidx = surf_index<NQ, NQV>(fp.vidM);
#pragma unroll
            for (int s = 0; s < NAUX; ++s) auxM[s] = 0;
#pragma unroll
            for (int s = 0; s < NS; ++s) QM[s] = sQ[s * Np + fp.vidM];
#pragma unroll
            for (int s = 0; s < NFA; ++s)
                auxM[P::face_aux(s)] =
                    STAGE_M ? sM[s * NSURF + sidx]
                            : a.aux[fp.vidM + (int64_t)Np * (P::face_aux(s) + (int64_t)NAUX * e)];
#pragma unroll
            for (int s = 0; s < NGF; ++s) gfM[s] = gfP[s] = 0.0;
            const int gslot = RECV ? ghost_slot<Np>(a.h, fp.eP, fp.vidP) : -1;
            if (use_gf) {
                if constexpr (STAGE_M) {
#pragma unroll
                    for (int s = 0; s < NGF; ++s) gfM[s] = sM[(NFA + s) * NSURF + sidx];
                } else {
                    load_gf<P, Np>(gfM, a.gf, fp.vidM, e);
                }
            }
#pragma unroll
            for (int s = 0; s < NHYP; ++s)
                hypM[s] = STAGE_M ? sM[(NFA + NGFS + s) * NSURF + sidx]
                                  : a.hypgrad[hg_at<NHG, Np>(fp.vidM, s, e)];
#pragma unroll
            for (int s = 0; s < NAUX; ++s) auxPn[s] = 0;
            if (use_gf) load_plus_gf<P, Np>(gfP, a.gf, a.h.recvGF, gslot, fp.vidP, fp.eP);
            load_plus<NS, Np, NS>(QPn, a.Q, a.h.recvQ, gslot, fp.vidP, fp.eP);
#pragma unroll
            for (int s = 0; s < NFA; ++s)
                auxPn[P::face_aux(s)] = a.aux[fp.vidP + (int64_t)Np * (P::face_aux(s) + (int64_t)NAUX * fp.eP)];
            load_plus_hg<NHG, Np, NHYP>(hypP, a.hypgrad, a.h.recvHG, gslot, fp.vidP, fp.eP);
#pragma unroll
            for (int s = 0; s < NS; ++s) QPd[s] = QPn[s];
#pragma unroll
            for (int s = 0; s < NAUX; ++s) auxPd[s] = auxPn[s];
            flux.negzero();
            if (fp.bctag == 0) {
                nf_first_order<P>(a.prm, a.nf_first, flux, fp.n, QM, auxM, QPn, auxPn, a_t, facedir);
                // CentralNumericalFluxSecondOrder  NumericalFluxes.jl:670-715
                Vec<3 * NS> FM, FP;
                FM.negzero();
                P::flux_second_order(a.prm, FM, QM, gfM, hypM, auxM, a_t);
                FP.negzero();
                P::flux_second_order(a.prm, FP, QPd, gfP, hypP, auxPd, a_t);
                const double nh0 = fp.n[0] / 2, nh1 = fp.n[1] / 2, nh2 = fp.n[2] / 2;
#pragma unroll
                for (int s = 0; s < NS; ++s)
                    flux[s] += (FM[3 * s] + FP[3 * s]) * nh0 +
                               (FM[3 * s + 1] + FP[3 * s + 1]) * nh1 +
                               (FM[3 * s + 2] + FP[3 * s + 2]) * nh2;
            } else {
                // boundary: the plus side is a copy of the minus side (e+ = e-, :686-692)
                // and the full minus-side auxiliary state may be needed by the law
                load_state<NAUX, Np>(auxM, a.aux, fp.vidM, e);
#pragma unroll
                for (int s = 0; s < NAUX; ++s) auxPn[s] = auxPd[s] = auxM[s];
                Vec<NS> Q1;
                Vec<NAUX> aux1;
                Vec<NGF> gf1;
                for (int s = 0; s < NS; ++s) Q1[s] = 0;
                for (int s = 0; s < NAUX; ++s) aux1[s] = 0;
                for (int s = 0; s < NGF; ++s) gf1[s] = 0;
                if (f == 4) {  // bottom face: first interior node (:786-816)
                    load_state<NS, Np>(Q1, a.Q, n + NQ * NQ, e);
                    load_state<NAUX, Np>(aux1, a.aux, n + NQ * NQ, e);
                    if (use_gf) load_gf<P, Np>(gf1, a.gf, n + NQ * NQ, e);
                }
                // numerical_boundary_flux_first_order!  NumericalFluxes.jl:163-205
                P::boundary_state(a.prm, BS_FIRST, fp.bctag, QPn, auxPn, fp.n, QM, auxM, a_t, Q1,
                                  aux1);
                nf_first_order<P>(a.prm, a.nf_first, flux, fp.n, QM, auxM, QPn, auxPn, a_t, facedir);
                // normal_boundary_flux_second_order!  NumericalFluxes.jl:872-918
                Vec<3 * NS> FP;
                FP.negzero();
                P::boundary_flux_second_order(a.prm, fp.bctag, FP, QPd, gfP, hypP, auxPd, fp.n, QM,
                                              gfM, hypM, auxM, a_t, Q1, gf1, aux1);
#pragma unroll
                for (int s = 0; s < NS; ++s)
                    flux[s] +=
                        FP[3 * s] * fp.n[0] + FP[3 * s + 1] * fp.n[1] + FP[3 * s + 2] * fp.n[2];
            }
#pragma unroll
            for (int s = 0; s < NS; ++s) lift[s] = a.alpha * fp.vMI * fp.sM * flux[s];
            vidM = fp.vidM;
            fpair = f / 2;
        }
    }
    Vec<NAUX> gaux;  // (the compiler drops the columns neither function reads)
    if constexpr (GARG_OUT) {
        if (live && tid < Np) load_state<NAUX, Np>(gaux, a.aux, tid, e);
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < 3; ++p) {  // opposite faces touch disjoint nodes (:898-899)
        if (fpair == p) {
#pragma unroll
            for (int s = 0; s < NS; ++s) sT[s * Np + vidM] -= lift[s];
        }
        __syncthreads();
    }
    if (live && tid < Np) {
        Vec<NS> Qn;  // the updated state of this node
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int64_t o = tid + (int64_t)Np * (s + (int64_t)NS * e);
            const double T = sT[s * Np + tid];
            if constexpr (LSRK) {  // update!: Q += rkb*dt*dQ; dQ *= rka
                Qn[s] = sQ[s * Np + tid] + a.rkb_dt * T;
                a.Qout[o] = Qn[s];
                a.tendency[o] = T * a.rka_next;
            } else {
                a.tendency[o] = T;
            }
        }
        if constexpr (GARG_OUT) {
            Vec<P::NGRAD> G;
            G.negzero();
            P::gradient_argument(a.prm, G, Qn, gaux, a_t);
            double *rec = a.garg + garg_at<P::NGL, Np>(tid, e);
#pragma unroll
            for (int s = 0; s < P::NGL; ++s) rec[s] = G[P::hv_indexmap(s)];
            if constexpr (GARG_REFRESH) {
                // kernel_nodal_update_auxiliary_state! for the next evaluation's input
                P::update_aux(a.prm, Qn, gaux, a_t);
#pragma unroll
                for (int s = 0; s < P::NUPD; ++s)
                    a.aux_rw[tid + (int64_t)Np * (P::upd_aux(s) + (int64_t)NAUX * e)] = gaux[P::upd_aux(s)];
            }
        }
    }
    if constexpr (LSRK) {  // the updated state of the nodes of vmapsend, straight to the send buffer
        if (live)
            send_nodes<NS, NS>(a.h, 0, e, tid, EPB == 1 ? (int)SH::NT : (int)SH::NTE, [&](int s, int n) {
                return sQ[s * Np + n] + a.rkb_dt * sT[s * Np + n];
            });
    }
}
template <class P, int NQ, int NQV, bool LSRK, bool USE_GF, bool RECV = false, bool GARG_OUT = false,
          bool GARG_REFRESH = true>
__global__ void __launch_bounds__((TendencyShape<P, NQ, NQV>::NT), CMDG_TEND_MINW) k_tendency(const PassArgs<P> a)
{
    tendency_body<P, NQ, NQV, LSRK, USE_GF, RECV, GARG_OUT, GARG_REFRESH>(a);
}

// ---------------------------------------------------------------------------------
// Gradient pass: volume_gradients! (:934-1328) + dgsem_interface_gradients! (:1365-1651)
// USE_GF = false: the law's second-order flux does not read the gradient-flux state (zero
// viscosity): only the gradients the hyperdiffusion passes consume are formed and stored, and
// state_gradient_flux is left untouched (cmdg_set_option(CMDG_OPT_KEEP_GRADFLUX) restores it).
template <class P, bool USE_GF>
__host__ __device__ constexpr unsigned gradient_argument_mask()
{
    if (USE_GF) return ~0u;
    unsigned m = 0;
    for (int s = 0; s < P::NGL; ++s) m |= 1u << P::hv_indexmap(s);
    return m;
}

// ---- the per-node and per-face-node expressions of the hyperdiffusion passes: one text for
// k_gradients, k_divgrad and k_lapfused, which must agree bit for bit ----------------------------
// Horizontal volume gradient of one field at node (i, j, .): line1(n) = G(n, j, k), line2(n) =
// G(i, n, k); added to gh[0..2], xi1 terms first.
template <int NQ, class Line>
__device__ __forceinline__ double line_derivative(const double *sD, int i, Line line)
{
    double G = 0.0;
#pragma unroll
    for (int n = 0; n < NQ; ++n) G += sD[i + NQ * n] * line(n);
    return G;
}
__device__ __forceinline__ void metric_gradient(double x11, double x12, double x13, double x21, double x22,
                                                double x23, double G1, double G2, double *gh)
{
    gh[0] += x11 * G1;
    gh[1] += x12 * G1;
    gh[2] += x13 * G1;
    gh[0] += x21 * G2;
    gh[1] += x22 * G2;
    gh[2] += x23 * G2;
}
template <int NQ, class Line1, class Line2>
__device__ __forceinline__ void grad_volume_h(const double *sD, int i, int j, Line1 line1, Line2 line2, double x11,
                                              double x12, double x13, double x21, double x22, double x23,
                                              double *gh)
{
    const double G1 = line_derivative<NQ>(sD, i, line1), G2 = line_derivative<NQ>(sD, j, line2);
    metric_gradient(x11, x12, x13, x21, x22, x23, G1, G2, gh);
}
// CentralNumericalFluxGradient (NumericalFluxes.jl:67-83), one component of one field
__device__ __forceinline__ double central_gradient_flux(double nd, double GP, double GM)
{
    return nd * (GP + GM) / 2;
}
// ... and what a face node adds to the gradient of its minus node
__device__ __forceinline__ double gradient_lift(double w, double tg, double nGM)
{
    return w * (tg - nGM);
}
// M * (xi_d . grad G) of one field
__device__ __forceinline__ double contravariant(double M, double xa, double xb, double xc, double G1, double G2,
                                                double G3)
{
    return M * (xa * G1 + xb * G2 + xc * G3);
}
// horizontal volume divergence of one field at node (i, j, k): c1 / c2 = the xi1 / xi2 products [ijk]
template <int NQ>
__device__ __forceinline__ double div_volume_h(double MI, const double *sD, const double *c1, const double *c2, int i,
                                               int j, int k)
{
    double dh = 0.0;
#pragma unroll
    for (int n = 0; n < NQ; ++n) {
        dh -= MI * sD[n + NQ * i] * c1[n + NQ * (j + NQ * k)];
        dh -= MI * sD[n + NQ * j] * c2[i + NQ * (n + NQ * k)];
    }
    return dh;
}
// CentralNumericalFluxDivergence (NumericalFluxes.jl:720-730) of one field: gP / gM its three components
__device__ __forceinline__ double central_divergence_flux(const double *gP, const double *gM, double nh0, double nh1,
                                                          double nh2)
{
    return (gP[0] + gM[0]) * nh0 + (gP[1] + gM[1]) * nh1 + (gP[2] + gM[2]) * nh2;
}

// GARG_IN (GradArgHandoff): the arguments of the volume nodes and of the plus side of interior
// faces are read from the records the previous stage's fused update left; boundary faces keep
// boundary_state on the element's own Q / aux; no auxiliary refresh (the update did it).
template <class P, int NQ, int NQV = NQ, bool USE_GF = true, bool GARG_IN = false>
// (six-wave work-groups of the large elements share a CU only at <= 128 VGPRs, see TendencyShape;
// a launch bound of 1024 threads is the hard form of that request)
__global__ void __launch_bounds__((KDims<NQ, NQV>::Np > 125 ? CMDG_GRAD_BOUND_LARGE : KDims<NQ, NQV>::NT),
                                   (NQ == 5 && NQV == 5 ? grad_min_waves<P> : 1)) k_gradients(const PassArgs<P> a)
{
    using KD = KDims<NQ, NQV>;
    const double a_t = a.tptr ? *a.tptr : a.t;  // (uniform: one scalar load)
    constexpr int Np = KD::Np, NS = P::NS, NAUX = P::NAUX, NGRAD = P::NGRAD,
                  NGF = USE_GF ? P::NGF : 0, NGL = P::NGL, NHG = 3 * NGL, NACC = NGF + NHG;
    constexpr unsigned GMASK = gradient_argument_mask<P, USE_GF>();
    static_assert(!GARG_IN || (!USE_GF && NGL > 0), "the hand-off feeds the USE_GF = false pass");
    __shared__ double sD[NQ * NQ + (NQV == NQ ? 0 : NQV * NQV)];
    const double *const sDv = sD + (NQV == NQ ? 0 : NQ * NQ);  // vertical derivative matrix
    __shared__ double sG[(NGRAD > 0 ? NGRAD : 1) * Np];
    __shared__ double sA[(NACC > 0 ? NACC : 1) * Np];  // [gf..., hypgrad...][ijk]
    const int tid = threadIdx.x;
    const int64_t e = a.elems[xcd_remap(blockIdx.x, gridDim.x)] - 1;
    if (tid < NQ * NQ) sD[tid] = a.g.D[tid];
    if constexpr (NQV != NQ) {
        if (tid < NQV * NQV) sD[NQ * NQ + tid] = a.g.Dv[tid];
    }
    const bool hz = a.direction != DIR_VERTICAL, vt = a.direction != DIR_HORIZONTAL;
    Vec<NS> lQ;
    Vec<NAUX> laux;
    if constexpr (GARG_IN) {
        if (tid < Np) {
            const double *rec = a.garg + garg_at<NGL, Np>(tid, e);
#pragma unroll
            for (int s = 0; s < NGL; ++s) sG[P::hv_indexmap(s) * Np + tid] = rec[s];
        }
    } else if (tid < Np) {
        load_state<NS, Np>(lQ, a.Q, tid, e);
        load_state<NAUX, Np>(laux, a.aux, tid, e);
        if constexpr (P::HAS_UPDATE_AUX && P::FUSE_UPDATE_AUX) {
            // kernel_nodal_update_auxiliary_state! of the real elements, fused: the refreshed
            // entries are read by no kernel of this evaluation (see P::FUSE_UPDATE_AUX)
            P::update_aux(a.prm, lQ, laux, a_t);
#pragma unroll
            for (int s = 0; s < P::NUPD; ++s)
                a.aux_rw[tid + (int64_t)Np * (P::upd_aux(s) + (int64_t)NAUX * e)] =
                    laux[P::upd_aux(s)];
        }
        Vec<NGRAD> G;
        G.negzero();
        P::gradient_argument(a.prm, G, lQ, laux, a_t);
#pragma unroll
        for (int s = 0; s < NGRAD; ++s)
            if (GMASK >> s & 1) sG[s * Np + tid] = G[s];
    }
    __syncthreads();
    if (tid < Np) {
        const int i = tid % NQ, j = (tid / NQ) % NQ, k = tid / (NQ * NQ);
        const double *vg = a.g.vgeo + (int64_t)Np * a.g.nvgeo * e + tid;
        Vec<3 * NGRAD> gh, gv;
        gh.negzero();
        gv.negzero();
        if (hz) {
            const double x11 = vg[XI1X1 * Np], x12 = vg[XI1X2 * Np], x13 = vg[XI1X3 * Np];
            const double x21 = vg[XI2X1 * Np], x22 = vg[XI2X2 * Np], x23 = vg[XI2X3 * Np];
#pragma unroll
            for (int s = 0; s < NGRAD; ++s) {
                if (!(GMASK >> s & 1)) continue;
                grad_volume_h<NQ>(
                    sD, i, j, [&](int n) { return sG[s * Np + n + NQ * (j + NQ * k)]; },
                    [&](int n) { return sG[s * Np + i + NQ * (n + NQ * k)]; }, x11, x12, x13, x21, x22, x23,
                    &gh[3 * s]);
            }
        }
        if (vt) {
            const double x31 = vg[XI3X1 * Np], x32 = vg[XI3X2 * Np], x33 = vg[XI3X3 * Np];
#pragma unroll
            for (int s = 0; s < NGRAD; ++s) {
                if (!(GMASK >> s & 1)) continue;
                double G3 = -0.0;
#pragma unroll
                for (int n = 0; n < NQV; ++n)
                    G3 += sDv[k + NQV * n] * sG[s * Np + i + NQ * (j + NQ * n)];
                gv[3 * s + 0] += x31 * G3;
                gv[3 * s + 1] += x32 * G3;
                gv[3 * s + 2] += x33 * G3;
            }
        }
        // hyperdiffusion gradients: "=" by the first kernel, "+=" by the vertical one
#pragma unroll
        for (int s = 0; s < NGL; ++s)
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const int q = d + 3 * P::hv_indexmap(s);
                sA[(NGF + 3 * s + d) * Np + tid] = hz ? (vt ? gh[q] + gv[q] : gh[q]) : gv[q];
            }
        if constexpr (NGF > 0) {
            Vec<NGF> o1, o2;
            o1.negzero();
            o2.negzero();
            Vec<NGRAD> Gn;  // this node's gradient argument (every entry is staged when NGF > 0)
#pragma unroll
            for (int s = 0; s < NGRAD; ++s) Gn[s] = (GMASK >> s & 1) ? sG[s * Np + tid] : 0.0;
            if (hz) law_gradient_flux<P>(a.prm, o1, gh, lQ, laux, a_t, Gn);
            if (vt) law_gradient_flux<P>(a.prm, o2, gv, lQ, laux, a_t, Gn);
#pragma unroll
            for (int s = 0; s < NGF; ++s)
                sA[s * Np + tid] = hz ? (vt ? o1[s] + o2[s] : o1[s]) : o2[s];
        }
    }
    __syncthreads();
    Vec<NACC> corr;
    int vidM = 0, fpair = -1;
    if (tid < KD::NFT) {
        int f, n;
        KD::face_task(tid, f, n);
        const bool on = f < 4 ? hz : vt;
        if (on) {
            FacePt fp;
            face_setup<NQ, NQV, true>(a.g, e, tid, f, n, fp);
            Vec<NS> QM, QP;
            Vec<NAUX> auxM, auxP;
            Vec<NGRAD> GM, GP;
            if constexpr (!GARG_IN) {
                load_state<NS, Np>(QM, a.Q, fp.vidM, e);       // only kept if the law reads them
                load_state<NAUX, Np>(auxM, a.aux, fp.vidM, e);  // (gradient_flux / boundary_state)
            }
#pragma unroll
            for (int s = 0; s < NGRAD; ++s)
                GM[s] = (GMASK >> s & 1) ? sG[s * Np + fp.vidM] : 0.0;  // == G(Q-, aux-)
            GP.negzero();
            Vec<NGF> lgf;
            lgf.negzero();
            Vec<3 * NGRAD> tg, nGM;
            if (fp.bctag == 0) {  // CentralNumericalFluxGradient  NumericalFluxes.jl:67-83
                // the plus side is read inside the branch that uses it: of the neighbour's
                // auxiliary columns only those the law's gradient argument touches are gathered
                if constexpr (GARG_IN) {
                    const double *rec = a.garg + garg_at<NGL, Np>(fp.vidP, fp.eP);
#pragma unroll
                    for (int s = 0; s < NGL; ++s) GP[P::hv_indexmap(s)] = rec[s];
                } else {
                    load_plus<NS, Np, NS>(QP, a.Q, a.h.recvQ, ghost_slot<Np>(a.h, fp.eP, fp.vidP), fp.vidP,
                                          fp.eP);
                    load_state<NAUX, Np>(auxP, a.aux, fp.vidP, fp.eP);
                    P::gradient_argument(a.prm, GP, QP, auxP, a_t);
                }
#pragma unroll
                for (int s = 0; s < NGRAD; ++s)
#pragma unroll
                    for (int d = 0; d < 3; ++d) tg[d + 3 * s] = central_gradient_flux(fp.n[d], GP[s], GM[s]);
            } else {  // numerical_boundary_flux_gradient!  NumericalFluxes.jl:85-123
                // e+ = e-, vid+ = vid- on boundary faces (:686-692): the plus side starts as
                // a copy of the minus side, already loaded
                if constexpr (GARG_IN) {
                    load_state<NS, Np>(QM, a.Q, fp.vidM, e);
                    load_state<NAUX, Np>(auxM, a.aux, fp.vidM, e);
                }
#pragma unroll
                for (int s = 0; s < NS; ++s) QP[s] = QM[s];
#pragma unroll
                for (int s = 0; s < NAUX; ++s) auxP[s] = auxM[s];
                Vec<NS> Q1;
                Vec<NAUX> aux1;
                for (int s = 0; s < NS; ++s) Q1[s] = 0;
                for (int s = 0; s < NAUX; ++s) aux1[s] = 0;
                if (f == 4) {
                    load_state<NS, Np>(Q1, a.Q, n + NQ * NQ, e);
                    load_state<NAUX, Np>(aux1, a.aux, n + NQ * NQ, e);
                }
                P::boundary_state(a.prm, BS_GRADIENT, fp.bctag, QP, auxP, fp.n, QM, auxM, a_t, Q1,
                                  aux1);
                P::gradient_argument(a.prm, GP, QP, auxP, a_t);
#pragma unroll
                for (int s = 0; s < NGRAD; ++s)
#pragma unroll
                    for (int d = 0; d < 3; ++d) tg[d + 3 * s] = fp.n[d] * GP[s];
            }
            if constexpr (NGF > 0) law_gradient_flux<P>(a.prm, lgf, tg, QM, auxM, a_t, GM);
#pragma unroll
            for (int s = 0; s < NGRAD; ++s)
#pragma unroll
                for (int d = 0; d < 3; ++d) nGM[d + 3 * s] = fp.n[d] * GM[s];
#pragma unroll
            for (int s = 0; s < NGL; ++s)
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    const int q = d + 3 * P::hv_indexmap(s);
                    corr[NGF + 3 * s + d] = gradient_lift(fp.w, tg[q], nGM[q]);
                }
            if constexpr (NGF > 0) {
                Vec<NGF> visc;
                for (int s = 0; s < NGF; ++s) visc[s] = 0;
                law_gradient_flux<P>(a.prm, visc, nGM, QM, auxM, a_t, GM);
#pragma unroll
                for (int s = 0; s < NGF; ++s) corr[s] = fp.w * (lgf[s] - visc[s]);
            }
            vidM = fp.vidM;
            fpair = f / 2;
        }
    }
#pragma unroll
    for (int p = 0; p < 3; ++p) {
        if (fpair == p) {
#pragma unroll
            for (int s = 0; s < NACC; ++s) sA[s * Np + vidM] += corr[s];
        }
        __syncthreads();
    }
    if (tid < Np) {
        if constexpr (!gf_node_major<P>) {
#pragma unroll
            for (int s = 0; s < NGF; ++s)
                a.gf[tid + (int64_t)Np * (s + (int64_t)P::NGF * e)] = sA[s * Np + tid];
        }
    }
    if constexpr (gf_node_major<P> && NGF > 0)
        store_node_major<P::NGF, Np, NGF>(a.gf, e, tid, (int)blockDim.x, sA);
    if constexpr (NHG > 0)
        store_node_major<NHG, Np, NHG>(a.hypgrad, e, tid, (int)blockDim.x, sA + NGF * Np);
    if constexpr (NGF > 0)
        send_nodes<P::NGF, NGF>(a.h, 0, e, tid, (int)blockDim.x, [&](int s, int n) { return sA[s * Np + n]; });
    if constexpr (NHG > 0)
        send_nodes<NHG, NHG>(a.h, 1, e, tid, (int)blockDim.x,
                             [&](int s, int n) { return sA[(NGF + s) * Np + n]; });
}

// ---------------------------------------------------------------------------------
// Laplacian pass: volume_divergence_of_gradients! (:2132-2329) +
// interface_divergence_of_gradients! (:2360-2494)
// RING (an evaluation of a hand-off run that reads the records, GradArgHandoff): the Laplacians are
// left as ring-ordered records in PassArgs::lapr for k_gradlap<..., RING>; the caller's
// Qhypervisc_div is written only where PassArgs::hypdiv_out says so.
template <class P, int NQ, int NQV = NQ, bool RING = false>
__global__ void __launch_bounds__((KDims<NQ, NQV>::NT)) k_divgrad(const PassArgs<P> a)
{
    using KD = KDims<NQ, NQV>;
    const double a_t = a.tptr ? *a.tptr : a.t;  // (uniform: one scalar load)
    constexpr int Np = KD::Np, NAUX = P::NAUX, NGL = P::NGL, NHG = 3 * NGL,
                  NHYP = P::NHYP, NG = NGL > 0 ? NGL : 1;
    __shared__ double sD[NQ * NQ + (NQV == NQ ? 0 : NQV * NQV)];
    const double *const sDv = sD + (NQV == NQ ? 0 : NQ * NQ);  // vertical derivative matrix
    __shared__ double sC[3 * NG * Np];  // M * (xi_d . grad) [d][s][ijk]
    __shared__ double sA[NG * Np];
    constexpr int NSURF = SurfDims<NQ, NQV>::NSURF;
    __shared__ double sM[(NHG > 0 ? NHG : 1) * NSURF];  // minus-side gradients, surface nodes
    const int tid = threadIdx.x;
    const int64_t e = a.elems[xcd_remap(blockIdx.x, gridDim.x)] - 1;
    if (tid < NQ * NQ) sD[tid] = a.g.D[tid];
    if constexpr (NQV != NQ) {
        if (tid < NQV * NQV) sD[NQ * NQ + tid] = a.g.Dv[tid];
    }
    const bool hz = a.direction != DIR_VERTICAL, vt = a.direction != DIR_HORIZONTAL;
    double MI = 0;
    if (tid < Np) {
        const double *vg = a.g.vgeo + (int64_t)Np * a.g.nvgeo * e + tid;
        const double M = vg[VM * Np];
        MI = vg[VMI * Np];
        // only the metric rows of the directions this pass differentiates in are read (a
        // horizontal diffusion_direction, Held-Suarez, never touches xi3)
        double x11 = 0, x12 = 0, x13 = 0, x21 = 0, x22 = 0, x23 = 0, x31 = 0, x32 = 0, x33 = 0;
        if (hz) {
            x11 = vg[XI1X1 * Np], x12 = vg[XI1X2 * Np], x13 = vg[XI1X3 * Np];
            x21 = vg[XI2X1 * Np], x22 = vg[XI2X2 * Np], x23 = vg[XI2X3 * Np];
        }
        if (vt) x31 = vg[XI3X1 * Np], x32 = vg[XI3X2 * Np], x33 = vg[XI3X3 * Np];
        Vec<NHG> G;  // (all of them in flight before the first LDS store: -17 % on this pass)
#pragma unroll
        for (int q = 0; q < NHG; ++q) G[q] = a.hypgrad[hg_at<NHG, Np>(tid, q, e)];
#pragma unroll
        for (int s = 0; s < NGL; ++s) {
            const double G1 = G[3 * s + 0], G2 = G[3 * s + 1], G3 = G[3 * s + 2];
            if (hz) {
                sC[(0 * NG + s) * Np + tid] = contravariant(M, x11, x12, x13, G1, G2, G3);
                sC[(1 * NG + s) * Np + tid] = contravariant(M, x21, x22, x23, G1, G2, G3);
            }
            if (vt) sC[(2 * NG + s) * Np + tid] = contravariant(M, x31, x32, x33, G1, G2, G3);
            const int sidx = surf_index<NQ, NQV>(tid);
            if (sidx >= 0) {
                sM[(3 * s + 0) * NSURF + sidx] = G1;
                sM[(3 * s + 1) * NSURF + sidx] = G2;
                sM[(3 * s + 2) * NSURF + sidx] = G3;
            }
        }
    }
    __syncthreads();
    if (tid < Np) {
        const int i = tid % NQ, j = (tid / NQ) % NQ, k = tid / (NQ * NQ);
#pragma unroll
        for (int s = 0; s < NGL; ++s) {
            double dh = 0.0, dv = 0.0;
            if (hz) dh = div_volume_h<NQ>(MI, sD, sC + (0 * NG + s) * Np, sC + (1 * NG + s) * Np, i, j, k);
            if (vt) {
#pragma unroll
                for (int kk = 0; kk < NQV; ++kk)
                    dv -= MI * sDv[kk + NQV * k] * sC[(2 * NG + s) * Np + i + NQ * (j + NQ * kk)];
            }
            sA[s * Np + tid] = hz ? (vt ? dh + dv : dh) : dv;
        }
    }
    __syncthreads();
    Vec<NGL> corr;
    int vidM = 0, fpair = -1;
    if (tid < KD::NFT) {
        int f, n;
        KD::face_task(tid, f, n);
        const bool on = f < 4 ? hz : vt;
        if (on) {
            FacePt fp;
            face_setup<NQ, NQV, true>(a.g, e, tid, f, n, fp);
            Vec<NHG> gM, gP;
            const int sidx = surf_index<NQ, NQV>(fp.vidM);
#pragma unroll
            for (int q = 0; q < NHG; ++q) gM[q] = sM[q * NSURF + sidx];
            load_plus_hg<NHG, Np, NHG>(gP, a.hypgrad, a.h.recvHG, ghost_slot<Np>(a.h, fp.eP, fp.vidP),
                                    fp.vidP, fp.eP);
            if (fp.bctag != 0) {  // numerical_boundary_flux_divergence!  :732-763
                Vec<NAUX> auxM, auxP;
                load_state<NAUX, Np>(auxM, a.aux, fp.vidM, e);
                load_state<NAUX, Np>(auxP, a.aux, fp.vidP, fp.eP);
                P::boundary_state_divergence(a.prm, fp.bctag, gP, auxP, fp.n, gM, auxM, a_t);
            }
            // CentralNumericalFluxDivergence  NumericalFluxes.jl:720-730
            const double nh0 = fp.n[0] / 2, nh1 = fp.n[1] / 2, nh2 = fp.n[2] / 2;
#pragma unroll
            for (int s = 0; s < NGL; ++s) {
                const double ldiv = central_divergence_flux(&gP[3 * s], &gM[3 * s], nh0, nh1, nh2);
                corr[s] = fp.w * ldiv;
            }
            vidM = fp.vidM;
            fpair = f / 2;
        }
    }
#pragma unroll
    for (int p = 0; p < 3; ++p) {
        if (fpair == p) {
#pragma unroll
            for (int s = 0; s < NGL; ++s) sA[s * Np + vidM] += corr[s];
        }
        __syncthreads();
    }
    // (the records go out of LDS in memory order: one record per lane at its ring slot measured
    // 13 us per launch slower, profiles/ab_face_contiguous.txt)
    if constexpr (RING) store_ring_major<NG, NQ, NQV>(a.lapr, e, tid, (int)blockDim.x, sA);
    if (tid < Np) {
        if (!RING || a.hypdiv_out) {
#pragma unroll
            for (int s = 0; s < NGL; ++s)
                a.hypdiv[tid + (int64_t)Np * (s + (int64_t)NHYP * e)] = sA[s * Np + tid];
        }
    }
    // (the NGL columns this pass writes are all the next one reads of Qhypervisc_div)
    if constexpr (NGL > 0)
        send_nodes<NGL, NGL>(a.h, 0, e, tid, (int)blockDim.x, [&](int s, int n) { return sA[s * Np + n]; });
}

// ---------------------------------------------------------------------------------
// Gradient and Laplacian pass of a hand-off evaluation in one launch: what k_gradients<..., false,
// GARG_IN> followed by k_divgrad<..., RING> leave in PassArgs::lapr (and Qhypervisc_div), bit for
// bit, without grad G going to memory and back.  For a horizontal diffusion_direction on a grid
// whose lateral faces are all interior (lapfused_tables.h): k_divgrad needs the neighbour's grad G
// only at the shared lateral face nodes, and the neighbour N's value at such a node y is
//   N's volume gradient at y   two NQ-point contractions over N's own records, along N's xi1 and
//                              xi2 lines through y, with N's metric rows at y (lapT);
//   + the lift of N's face that is shared with this element: N's normal and weight there (lapT),
//     plus side = this element's own record, held in LDS;
//   + where y is on a vertical edge of N, the lift of N's other lateral face at y (its normal
//     and weight: the edge block), whose plus side is one record of N's neighbour (lapI's idE) --
// added in N's own order: volume, then the face of the pair xi1 (N's faces 0 / 1), then xi2.  Every
// term is the text k_gradients evaluates for N (line_derivative, metric_gradient,
// central_gradient_flux, gradient_lift), so the sum is the value N would have stored.
// Of N's two lines through y one is normal to the shared face and one lies in it.  The records of the
// in-face line are the plus nodes of the row of sibling tasks (same face, same level: create checks
// this of every row, lapfused_tables.h), so a face lane gathers the normal line alone -- NQ records,
// y among them -- and the lanes of a row hand each other their y through LDS (sX), each slot under
// the index of its y along N's face; line_derivative then sums the same values in the same order.
// The create-time tables, per lateral face task t = 0 .. NL-1 (NL = 4 Nfph), about the neighbour N
// on the plus side, whose node y = vidP the task faces:
//   lapI[e][c][t]  int32: c = 0 tP, N's face task of the same mesh node; c = 1 idE, the global node
//                  faced by N's other lateral face task at y (tE), or -1
//   lapT[e][c][t]  c = 0..5 N's horizontal metric rows at y (xi1x1, xi1x2, xi1x3, xi2x1, xi2x2,
//                  xi2x3), c = 6..9 N's n1, n2, n3 and lift weight at tP
//   edge[e][c][r]  behind lapT[e]: N's n1, n2, n3 and lift weight at tE, r = 2 (row of t) + (y is the
//                  last node of N's row, not the first): the 2 of the NQ tasks of a row that have a tE
// 88 B per lateral face node and 32 B per edge slot (8 NQV of them): a digest of grid geometry like faceG, not of caller state.  This
// launch is handed lapI as GridDev::facePr and lapT as PassArgs::derived, neither of which a
// Laplacian pass reads (as k_gradlap<..., RING> is handed facePr as faceP): the argument block of
// every other pass kernel, and with it their code, stays what it was.
// A face lane reads in three dependent trips: elems; its own tables (faceP, faceG, faceW, lapI);
// N's records.  What only the neighbour's gradient gP needs (lapT, edge, the record at idE) is
// asked for behind the barrier that ends the own-gradient phase and gP formed while the volume
// lanes contract the Laplacian: gP is first used by the Laplacian's own face phase.
// Lanes: the volume nodes are threads 0 .. Np-1, the 4 Nfph lateral face tasks the LAST threads of
// the group, so that the gathers of the face lanes and the contractions of the volume lanes fall
// into different waves where the group has more than one.
template <class P, int NQ, int NQV = NQ>
__global__ void __launch_bounds__((KDims<NQ, NQV>::NT), CMDG_LAPFUSED_MINW) k_lapfused(const PassArgs<P> a)
{
    using KD = KDims<NQ, NQV>;
    constexpr int Np = KD::Np, NGL = P::NGL, NHG = 3 * NGL, NHYP = P::NHYP, NG = NGL > 0 ? NGL : 1,
                  NL = 4 * KD::Nfph, NT = KD::NT, NE = 8 * NQV, LT = 10 * NL + 4 * NE;
    static_assert(NT >= NL && NGL > 0, "one lane per lateral face task");
    __shared__ double sD[NQ * NQ];
    __shared__ double sG[NG * Np];      // gradient arguments [s][ijk]
    __shared__ double sA[3 * NG * Np];  // grad G [3 s + d][ijk]
    __shared__ double sC[2 * NG * Np];  // M * (xi_d . grad) [d][s][ijk], d = 0, 1
    __shared__ double sL[NG * Np];      // Laplacians [s][ijk]
    __shared__ double sX[NG * NL];      // the exchange: N's argument at y [s][row of the task][index of y in N's row]
    static_assert(sizeof(double) * (NQ * NQ + 7 * NG * Np + NG * NL) <= 32768,
                  "LDS of k_lapfused: five work-groups per CU");
    const int tid = threadIdx.x;
    const int64_t e = a.elems[xcd_remap(blockIdx.x, gridDim.x)] - 1;
    const int ft = tid - (NT - NL);  // lateral face task of this lane (< 0: none)
    if (tid < NQ * NQ) sD[tid] = a.g.D[tid];
    // Everything a lane can ask for knowing the element alone, in one trip: the volume lanes their
    // record and metric terms, the face lanes their own tables.
    Vec<NGL> r;
    double M = 0, MI = 0, x11 = 0, x12 = 0, x13 = 0, x21 = 0, x22 = 0, x23 = 0;
#pragma unroll
    for (int s = 0; s < NGL; ++s) r[s] = 0;
    if (tid < Np) {
        const double *rec = a.garg + garg_at<NGL, Np>(tid, e);
#pragma unroll
        for (int s = 0; s < NGL; ++s) r[s] = rec[s];
        const double *vg = a.g.vgeo + (int64_t)Np * a.g.nvgeo * e + tid;
        M = vg[VM * Np];
        MI = vg[VMI * Np];
        x11 = vg[XI1X1 * Np], x12 = vg[XI1X2 * Np], x13 = vg[XI1X3 * Np];
        x21 = vg[XI2X1 * Np], x22 = vg[XI2X2 * Np], x23 = vg[XI2X3 * Np];
    }
    FacePt fp = {};
    int32_t idE = -1;
    int tP = 0;
    if (ft >= 0) {
        int f, n;
        KD::face_task(ft, f, n);
        face_setup<NQ, NQV, true>(a.g, e, ft, f, n, fp);
        tP = a.g.facePr[((int64_t)2 * e + 0) * NL + ft];
        idE = a.g.facePr[((int64_t)2 * e + 1) * NL + ft];
    }
    // (A use of all of it on every path: these values are loaded and used under the same conditions
    // in separate blocks, and what the compiler knows of a load's completion is lost where paths
    // join.  Without this, every later use waits for all the loads the lane has issued since -- the
    // volume lanes of the middle wave for the gathers of its face lanes.)
    asm volatile("" ::"v"(M), "v"(MI), "v"(x11), "v"(x12), "v"(x13), "v"(x21), "v"(x22), "v"(x23), "v"(r[0]),
                 "v"(r[NGL - 1]), "v"(fp.vidP), "v"(fp.w), "v"(fp.n[0]), "v"(fp.n[1]), "v"(fp.n[2]), "v"(tP), "v"(idE));
    if (tid < Np) {
#pragma unroll
        for (int s = 0; s < NGL; ++s) sG[s * Np + tid] = r[s];
    }
    // of the neighbour its normal line of records through y: in flight across the barrier
    int idx = 0, xrow = 0;  // index of y along N's face; first exchange slot of the lane's row
    bool x1 = true, far = false;  // N's normal line at y is its xi1 line; y is the last node of it
    double rn[NQ][NG] = {};
    if (ft >= 0) {
        int fS, nn;
        KD::face_task(tP, fS, nn);
        x1 = fS < 2, far = fS & 1;
        const int iP = fp.vidP % NQ, jP = (fp.vidP / NQ) % NQ, kP = fp.vidP / (NQ * NQ);
        idx = x1 ? jP : iP;
        xrow = ft - ft % NQ;
        const double *line = a.garg + garg_at<NGL, Np>(x1 ? NQ * (jP + NQ * kP) : iP + NQ * NQ * kP, fp.eP);
        const int step = x1 ? NGL : NGL * NQ;
#pragma unroll
        for (int m = 0; m < NQ; ++m)
#pragma unroll
            for (int s = 0; s < NGL; ++s) rn[m][s] = line[m * step + s];
    }
    __syncthreads();
    // ---- own volume gradient (k_gradients, horizontal)
    if (tid < Np) {
        const int i = tid % NQ, j = (tid / NQ) % NQ, k = tid / (NQ * NQ);
        Vec<NHG> gh;
        gh.negzero();
#pragma unroll
        for (int s = 0; s < NGL; ++s)
            grad_volume_h<NQ>(
                sD, i, j, [&](int n) { return sG[s * Np + n + NQ * (j + NQ * k)]; },
                [&](int n) { return sG[s * Np + i + NQ * (n + NQ * k)]; }, x11, x12, x13, x21, x22, x23, &gh[3 * s]);
#pragma unroll
        for (int q = 0; q < NHG; ++q) sA[q * Np + tid] = gh[q];
    }
    // ---- face lanes: the lift of the own gradient; N's argument at y into the exchange; N's
    // derivative along its normal line at y
    Vec<NHG> corr;
    Vec<NGL> Gn;
    int fpair = -1;
    if (ft >= 0) {
        fpair = ft / (2 * KD::Nfph);
        Vec<NGL> GY, GM;  // N's argument at y (an end of the normal line), this element's at the face node
#pragma unroll
        for (int s = 0; s < NGL; ++s) GY[s] = far ? rn[NQ - 1][s] : rn[0][s];
#pragma unroll
        for (int s = 0; s < NGL; ++s) sX[s * NL + xrow + idx] = GY[s];
#pragma unroll
        for (int s = 0; s < NGL; ++s) GM[s] = sG[s * Np + fp.vidM];
#pragma unroll
        for (int s = 0; s < NGL; ++s)
            Gn[s] = line_derivative<NQ>(sD, far ? NQ - 1 : 0, [&](int m) { return rn[m][s]; });
        // own lift (k_gradients' interface phase, interior face)
#pragma unroll
        for (int s = 0; s < NGL; ++s)
#pragma unroll
            for (int d = 0; d < 3; ++d)
                corr[3 * s + d] =
                    gradient_lift(fp.w, central_gradient_flux(fp.n[d], GY[s], GM[s]), fp.n[d] * GM[s]);
    }
    __syncthreads();
    // (as above, of the gathered line: the registers it arrived in are used again by the volume lanes)
#pragma unroll
    for (int m = 0; m < NQ; ++m) asm volatile("" ::"v"(rn[m][0]), "v"(rn[m][NGL - 1]));
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        if (fpair == p) {
#pragma unroll
            for (int q = 0; q < NHG; ++q) sA[q * Np + fp.vidM] += corr[q];
        }
        __syncthreads();
    }
    // what the neighbour's gradient needs besides the two lines: in flight while the
    // volume lanes form the contravariant products
    double T[10], nE[3] = {0, 0, 0}, wE = 0;
    Vec<NGL> GE;
    if (ft >= 0) {
        const double *lapT = a.derived + (int64_t)LT * e;
#pragma unroll
        for (int c = 0; c < 10; ++c) T[c] = lapT[c * NL + ft];
        if (idE >= 0) {
            const double *edge = lapT + 10 * NL + 2 * (ft / NQ) + (idx == NQ - 1 ? 1 : 0);
            nE[0] = edge[0], nE[1] = edge[NE], nE[2] = edge[2 * NE];
            wE = edge[3 * NE];
            const double *rec = a.garg + (int64_t)NGL * idE;
#pragma unroll
            for (int s = 0; s < NGL; ++s) GE[s] = rec[s];
        }
    }
    // ---- Laplacian (k_divgrad, horizontal): the own gradient is complete in sA
    if (tid < Np) {
#pragma unroll
        for (int s = 0; s < NGL; ++s) {
            const double G1 = sA[(3 * s + 0) * Np + tid], G2 = sA[(3 * s + 1) * Np + tid],
                         G3 = sA[(3 * s + 2) * Np + tid];
            sC[(0 * NG + s) * Np + tid] = contravariant(M, x11, x12, x13, G1, G2, G3);
            sC[(1 * NG + s) * Np + tid] = contravariant(M, x21, x22, x23, G1, G2, G3);
        }
    }
    __syncthreads();
    if (tid < Np) {
        const int i = tid % NQ, j = (tid / NQ) % NQ, k = tid / (NQ * NQ);
#pragma unroll
        for (int s = 0; s < NGL; ++s)
            sL[s * Np + tid] = div_volume_h<NQ>(MI, sD, sC + (0 * NG + s) * Np, sC + (1 * NG + s) * Np, i, j, k);
    }
    Vec<NGL> corrL;
    if (ft >= 0) {
        // the neighbour's gradient at y, as it forms it: volume (xi1 line, then xi2 line), then the
        // lifts of its lateral faces at y in its own order, the face of the pair xi1 first -- the one
        // shared with this element, and at a vertical edge of N its other one
        Vec<NGL> GY, GM, Gf;
#pragma unroll
        for (int s = 0; s < NGL; ++s) GY[s] = sX[s * NL + xrow + idx];
#pragma unroll
        for (int s = 0; s < NGL; ++s) GM[s] = sG[s * Np + fp.vidM];
#pragma unroll
        for (int s = 0; s < NGL; ++s)
            Gf[s] = line_derivative<NQ>(sD, idx, [&](int m) { return sX[s * NL + xrow + m]; });
        Vec<NHG> gP;
        gP.negzero();
#pragma unroll
        for (int s = 0; s < NGL; ++s)
            metric_gradient(T[0], T[1], T[2], T[3], T[4], T[5], x1 ? Gn[s] : Gf[s], x1 ? Gf[s] : Gn[s], &gP[3 * s]);
        const bool edge_first = !x1;  // (the other face is of the other pair)
#pragma unroll
        for (int s = 0; s < NGL; ++s)
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const double lS = gradient_lift(T[9], central_gradient_flux(T[6 + d], GM[s], GY[s]), T[6 + d] * GY[s]);
                if (idE >= 0) {
                    const double lE = gradient_lift(wE, central_gradient_flux(nE[d], GE[s], GY[s]), nE[d] * GY[s]);
                    gP[3 * s + d] += edge_first ? lE : lS;
                    gP[3 * s + d] += edge_first ? lS : lE;
                } else {
                    gP[3 * s + d] += lS;
                }
            }
        Vec<NHG> gM;
#pragma unroll
        for (int q = 0; q < NHG; ++q) gM[q] = sA[q * Np + fp.vidM];
        const double nh0 = fp.n[0] / 2, nh1 = fp.n[1] / 2, nh2 = fp.n[2] / 2;
#pragma unroll
        for (int s = 0; s < NGL; ++s) {
            const double ldiv = central_divergence_flux(&gP[3 * s], &gM[3 * s], nh0, nh1, nh2);
            corrL[s] = fp.w * ldiv;
        }
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        if (fpair == p) {
#pragma unroll
            for (int s = 0; s < NGL; ++s) sL[s * Np + fp.vidM] += corrL[s];
        }
        __syncthreads();
    }
    store_ring_major<NG, NQ, NQV>(a.lapr, e, tid, (int)blockDim.x, sL);
    if (tid < Np && a.hypdiv_out) {
#pragma unroll
        for (int s = 0; s < NGL; ++s) a.hypdiv[tid + (int64_t)Np * (s + (int64_t)NHYP * e)] = sL[s * Np + tid];
    }
}

// ---------------------------------------------------------------------------------
// Gradient-of-Laplacian pass: volume_gradients_of_laplacians! (:2525-2824) +
// interface_gradients_of_laplacians! (:2859-3026)
// RING: the Laplacians are read and gathered as the ring-ordered records k_divgrad<..., RING> left.
template <class P, int NQ, int NQV = NQ, bool RING = false>
__global__ void __launch_bounds__((KDims<NQ, NQV>::NT), CMDG_LAP_MINW) k_gradlap(const PassArgs<P> a)
{
    using KD = KDims<NQ, NQV>;
    const double a_t = a.tptr ? *a.tptr : a.t;  // (uniform: one scalar load)
    constexpr int Np = KD::Np, NS = P::NS, NAUX = P::NAUX, NGL = P::NGL,
                  NHG = 3 * NGL, NHYP = P::NHYP, NG = NGL > 0 ? NGL : 1,
                  NH = NHYP > 0 ? NHYP : 1;
    __shared__ double sD[NQ * NQ + (NQV == NQ ? 0 : NQV * NQV)];
    const double *const sDv = sD + (NQV == NQ ? 0 : NQ * NQ);  // vertical derivative matrix
    __shared__ double sL[NG * Np];
    __shared__ double sA[NH * Np];
    const int tid = threadIdx.x;
    const int64_t e = a.elems[xcd_remap(blockIdx.x, gridDim.x)] - 1;
    if (tid < NQ * NQ) sD[tid] = a.g.D[tid];
    if constexpr (NQV != NQ) {
        if (tid < NQV * NQV) sD[NQ * NQ + tid] = a.g.Dv[tid];
    }
    const bool hz = a.direction != DIR_VERTICAL, vt = a.direction != DIR_HORIZONTAL;
    if (tid < Np) {
        Vec<NGL> l;  // (all loads in flight before the first LDS store, as in k_divgrad)
        if constexpr (RING) {
            const double *rec = a.lapr + garg_at<NG, Np>(ring_slot<NQ, NQV>(tid), e);
#pragma unroll
            for (int s = 0; s < NGL; ++s) l[s] = rec[s];
        } else {
#pragma unroll
            for (int s = 0; s < NGL; ++s) l[s] = a.hypdiv[tid + (int64_t)Np * (s + (int64_t)NHYP * e)];
        }
#pragma unroll
        for (int s = 0; s < NGL; ++s) sL[s * Np + tid] = l[s];
    }
    __syncthreads();
    if (tid < Np) {
        const int i = tid % NQ, j = (tid / NQ) % NQ, k = tid / (NQ * NQ);
        const double *vg = a.g.vgeo + (int64_t)Np * a.g.nvgeo * e + tid;
        Vec<NS> lQ;
        Vec<NAUX> laux;
        load_state<NS, Np>(lQ, a.Q, tid, e);
        load_state<NAUX, Np>(laux, a.aux, tid, e);
        Vec<NHG> lh, lv;
        lh.negzero();
        lv.negzero();
        if (hz) {
            const double x11 = vg[XI1X1 * Np], x12 = vg[XI1X2 * Np], x13 = vg[XI1X3 * Np];
            const double x21 = vg[XI2X1 * Np], x22 = vg[XI2X2 * Np], x23 = vg[XI2X3 * Np];
#pragma unroll
            for (int s = 0; s < NGL; ++s) {
                double l1 = 0.0, l2 = 0.0;
#pragma unroll
                for (int n = 0; n < NQ; ++n) {
                    l1 += sD[i + NQ * n] * sL[s * Np + n + NQ * (j + NQ * k)];
                    l2 += sD[j + NQ * n] * sL[s * Np + i + NQ * (n + NQ * k)];
                }
                lh[3 * s + 0] = x11 * l1;
                lh[3 * s + 1] = x12 * l1;
                lh[3 * s + 2] = x13 * l1;
                lh[3 * s + 0] += x21 * l2;
                lh[3 * s + 1] += x22 * l2;
                lh[3 * s + 2] += x23 * l2;
            }
        }
        if (vt) {
            const double x31 = vg[XI3X1 * Np], x32 = vg[XI3X2 * Np], x33 = vg[XI3X3 * Np];
#pragma unroll
            for (int s = 0; s < NGL; ++s) {
                double l3 = -0.0;
#pragma unroll
                for (int n = 0; n < NQV; ++n)
                    l3 += sDv[k + NQV * n] * sL[s * Np + i + NQ * (j + NQ * n)];
                lv[3 * s + 0] += x31 * l3;
                lv[3 * s + 1] += x32 * l3;
                lv[3 * s + 2] += x33 * l3;
            }
        }
        Vec<NHYP> h1, h2;
        h1.negzero();
        h2.negzero();
        if (hz) P::post_gradient_laplacian(a.prm, h1, lh, lQ, laux, a_t);
        if (vt) P::post_gradient_laplacian(a.prm, h2, lv, lQ, laux, a_t);
#pragma unroll
        for (int s = 0; s < NHYP; ++s) sA[s * Np + tid] = hz ? (vt ? h1[s] + h2[s] : h1[s]) : h2[s];
    }
    __syncthreads();
    Vec<NHYP> corr;
    int vidM = 0, fpair = -1;
    if (tid < KD::NFT) {
        int f, n;
        KD::face_task(tid, f, n);
        const bool on = f < 4 ? hz : vt;
        if (on) {
            FacePt fp;
            face_setup<NQ, NQV, true>(a.g, e, tid, f, n, fp);
            Vec<NS> QM, QP;
            Vec<NAUX> auxM, auxP;
            Vec<NGL> lapM, lapP;
            load_state<NS, Np>(QM, a.Q, fp.vidM, e);
            load_state<NAUX, Np>(auxM, a.aux, fp.vidM, e);
            if constexpr (RING) {
                // fp.vidP is the ring slot of the plus-side node (facePr).  Q+ / aux+ are read by the
                // boundary state alone, where e+ = e-, vid+ = vid-: copies of the minus side
#pragma unroll
                for (int s = 0; s < NS; ++s) QP[s] = QM[s];
#pragma unroll
                for (int s = 0; s < NAUX; ++s) auxP[s] = auxM[s];
#pragma unroll
                for (int s = 0; s < NGL; ++s) lapM[s] = sL[s * Np + fp.vidM];
                const double *rec = a.lapr + garg_at<NG, Np>(fp.vidP, fp.eP);
#pragma unroll
                for (int s = 0; s < NGL; ++s) lapP[s] = rec[s];
            } else {
                const int gslot = ghost_slot<Np>(a.h, fp.eP, fp.vidP);
                load_plus<NS, Np, NS>(QP, a.Q, a.h.recvQ, gslot, fp.vidP, fp.eP);
                load_state<NAUX, Np>(auxP, a.aux, fp.vidP, fp.eP);
#pragma unroll
                for (int s = 0; s < NGL; ++s) lapM[s] = sL[s * Np + fp.vidM];
                load_plus<NHYP, Np, NGL, NGL>(lapP, a.hypdiv, a.h.recvHD, gslot, fp.vidP, fp.eP);
            }
            if (fp.bctag != 0)  // numerical_boundary_flux_higher_order!  :792-832
                P::boundary_state_higher_order(a.prm, fp.bctag, QP, auxP, lapP, fp.n, QM, auxM,
                                               lapM, a_t);
            // CentralNumericalFluxHigherOrder  NumericalFluxes.jl:768-790
            Vec<NHG> G;
#pragma unroll
            for (int s = 0; s < NGL; ++s)
#pragma unroll
                for (int d = 0; d < 3; ++d) G[d + 3 * s] = fp.n[d] * (lapP[s] - lapM[s]) / 2;
            Vec<NHYP> lh;
            for (int s = 0; s < NHYP; ++s) lh[s] = 0;
            P::post_gradient_laplacian(a.prm, lh, G, QM, auxM, a_t);
#pragma unroll
            for (int s = 0; s < NHYP; ++s) corr[s] = fp.w * lh[s];
            vidM = fp.vidM;
            fpair = f / 2;
        }
    }
#pragma unroll
    for (int p = 0; p < 3; ++p) {
        if (fpair == p) {
#pragma unroll
            for (int s = 0; s < NHYP; ++s) sA[s * Np + vidM] += corr[s];
        }
        __syncthreads();
    }
    if constexpr (NHYP > 0) store_node_major<NHG, Np, NHYP>(a.hypgrad, e, tid, (int)blockDim.x, sA);
    if constexpr (NHYP > 0)
        send_nodes<NHG, NHYP>(a.h, 0, e, tid, (int)blockDim.x, [&](int s, int n) { return sA[s * Np + n]; });
}

// ---------------------------------------------------------------------------------
// kernel_nodal_update_auxiliary_state!  (:1769-1825); elements [e0, e1)
template <class P, int NQ, int NQV = NQ>
__global__ void k_update_aux(typename P::Params prm, const double *Q, double *aux,
                             const uint8_t *activedofs, double t, int64_t e0, int64_t e1)
{
    constexpr int Np = KDims<NQ, NQV>::Np, NS = P::NS, NAUX = P::NAUX;
    const int64_t I = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t e = e0 + I / Np;
    const int n = (int)(I % Np);
    if (e >= e1) return;
    if (activedofs && !activedofs[n + e * Np]) return;
    Vec<NS> lQ;
    Vec<NAUX> laux;
    load_state<NS, Np>(lQ, Q, n, e);
    load_state<NAUX, Np>(laux, aux, n, e);
    P::update_aux(prm, lQ, laux, t);
    if constexpr (P::NUPD > 0) {  // the law names the entries its refresh rewrites
#pragma unroll
        for (int s = 0; s < P::NUPD; ++s)
            aux[n + (int64_t)Np * (P::upd_aux(s) + (int64_t)NAUX * e)] = laux[P::upd_aux(s)];
    } else {
#pragma unroll
        for (int s = 0; s < NAUX; ++s) aux[n + (int64_t)Np * (s + (int64_t)NAUX * e)] = laux[s];
    }
}

// one-time: time-invariant per-node fields the law would otherwise recompute every call
template <class P, int NQ, int NQV = NQ>
__global__ void k_init_derived(typename P::Params prm, const double *aux, double *derived,
                               int64_t nelem)
{
    constexpr int Np = KDims<NQ, NQV>::Np, NAUX = P::NAUX, NDER = P::NDER;
    const int64_t I = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t e = I / Np;
    const int n = (int)(I % Np);
    if (e >= nelem) return;
    Vec<NAUX> laux;
    load_state<NAUX, Np>(laux, aux, n, e);
    Vec<NDER> d;
    P::init_derived(prm, d, laux);
#pragma unroll
    for (int s = 0; s < NDER; ++s) derived[n + (int64_t)Np * (s + (int64_t)NDER * e)] = d[s];
}

// ---- courant(local_courant, dg, m, Q, dt, t, direction)  SpaceDiscretization.jl:307-365 ----
// One block per real element: node coordinates staged in LDS, the minimum neighbour distance
// (kernel_min_neighbor_distance!, Grids.jl:1228-1333) and the law's local Courant number
// (kernel_local_courant!, DGModel_kernels.jl:3028-3096) evaluated per node, then a block-wide
// extremum.  MODE 0: out[e] = min distance of the element, MODE 1: out[e] = max Courant.
template <class P, int NQ, int NQV, int MODE>
__global__ __launch_bounds__((KDims<NQ, NQV>::Np <= 128 ? 128 : 256)) void k_courant(
    typename P::Params prm, const double *__restrict__ vgeo, int nvgeo,
    const double *__restrict__ Q, const double *__restrict__ aux, const double *__restrict__ gf,
    int kind, double dt, double t, int direction, double *__restrict__ out)
{
    constexpr int Np = KDims<NQ, NQV>::Np, NT = Np <= 128 ? 128 : 256;
    __shared__ double sx[3][Np], sred[NT];
    const int tid = threadIdx.x;
    const int64_t e = blockIdx.x;
    constexpr int X1 = 12;  // _x1 (Grids.jl:76-92), 0-based column
    for (int n = tid; n < Np; n += NT)
#pragma unroll
        for (int d = 0; d < 3; ++d) sx[d][n] = vgeo[n + (int64_t)Np * (X1 + d + (int64_t)nvgeo * e)];
    __syncthreads();
    double val = MODE == 0 ? INFINITY : -INFINITY;
    for (int n = tid; n < Np; n += NT) {
        const int i = n % NQ, j = (n / NQ) % NQ, k = n / (NQ * NQ);
        double md = INFINITY;
        auto dist = [&](int m) {
            const double d0 = sx[0][n] - sx[0][m], d1 = sx[1][n] - sx[1][m], d2 = sx[2][n] - sx[2][m];
            return sqrt(d0 * d0 + d1 * d1 + d2 * d2);
        };
        if (direction != DIR_VERTICAL) {
            if (i > 0) md = fmin(md, dist(n - 1));
            if (i < NQ - 1) md = fmin(md, dist(n + 1));
            if (j > 0) md = fmin(md, dist(n - NQ));
            if (j < NQ - 1) md = fmin(md, dist(n + NQ));
        }
        if (direction != DIR_HORIZONTAL) {
            if (k > 0) md = fmin(md, dist(n - NQ * NQ));
            if (k < NQV - 1) md = fmin(md, dist(n + NQ * NQ));
        }
        if constexpr (MODE == 0) {
            val = fmin(val, md);
        } else {
            Vec<P::NS> lQ;
            Vec<P::NAUX> lA;
            Vec<P::NGF> lG;
            load_state<P::NS, Np>(lQ, Q, n, e);
            load_state<P::NAUX, Np>(lA, aux, n, e);
            if constexpr (P::NGF > 0) load_gf<P, Np>(lG, gf, n, e);
            val = fmax(val, P::courant(prm, kind, lQ, lA, lG, md, dt, t, direction));
        }
    }
    sred[tid] = val;
    __syncthreads();
    for (int h = NT / 2; h > 0; h >>= 1) {
        if (tid < h) sred[tid] = MODE == 0 ? fmin(sred[tid], sred[tid + h]) : fmax(sred[tid], sred[tid + h]);
        __syncthreads();
    }
    if (tid == 0) out[e] = sred[0];
}

// ---- AtmosLESDefault diagnostics, nodal pass (src/Diagnostics/atmos_les_default.jl:629-636) ----
// compute_thermo! and the two sub-grid terms at every node of the real elements: one thread per
// node, D[n, s, e] in the layout of the auxiliary state; the level reductions that read D are
// law-independent (diagnostics.hip).  has_gf = 0: the handle forms no gradient flux (its diffusivity
// is zero) and the law is handed zeros.
template <class P, int NQ, int NQV>
__global__ __launch_bounds__(256) void k_les_nodal(typename P::Params prm, const double *__restrict__ Q,
                                                   const double *__restrict__ aux, const double *__restrict__ gf,
                                                   int has_gf, double t, int64_t nreal, double *__restrict__ D)
{
    constexpr int Np = KDims<NQ, NQV>::Np, ND = P::NDIAG;
    const int64_t I = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t e = I / Np;
    const int n = (int)(I - e * Np);
    if (e >= nreal) return;
    Vec<P::NS> lQ;
    Vec<P::NAUX> lA;
    Vec<P::NGF> lG;
    Vec<ND> d;
    load_state<P::NS, Np>(lQ, Q, n, e);
    load_state<P::NAUX, Np>(lA, aux, n, e);
    if constexpr (P::NGF > 0) {
        if (has_gf) {
            load_gf<P, Np>(lG, gf, n, e);
        } else {
#pragma unroll
            for (int s = 0; s < P::NGF; ++s) lG[s] = 0.0;
        }
    }
    P::les_diagnostics(prm, d, lQ, lA, lG, t);
#pragma unroll
    for (int s = 0; s < ND; ++s) D[n + (int64_t)Np * (s + (int64_t)ND * e)] = d[s];
}

// ---- AtmosGCMDefault diagnostics: VectorGradients, Vorticity and the nodal pass -------------------
// (src/Diagnostics/diagnostic_fields.jl:129-298, :382-396; atmos_gcm_default.jl:337-357).  The
// reference's vector_gradients_kernel! gives an element to (Nq, Nq) threads, reduces every line of
// nodes serially through LDS in three phases and keeps the nine reference-space derivatives in a
// global array g.  Here a work-group of Np threads owns an element: u = rho u / rho is staged in LDS
// and thread n forms its own nine sums in registers -- each the sum, left to right in ascending node
// index, of the rounded products D[i, r] u[r], the first product being the initial value, as
// `s_U[i, 1] += s_U[i, r]` sums them -- then the metric combination, left to right.  The units that
// instantiate this are compiled without contraction (Makefile), so the result has the reference's bits.
constexpr int GCM_NCOL = 14;  // rho, rho u[3], rho e | temp, pres, theta_dry, e_int, h_tot, h_int | Omega[3]

// sU: (3, Np) velocity of the element; sD (NQ, NQ) / sDv (NQV, NQV) column-major; vg: the element's
// vgeo at node n; out[3 c + m] = d u_c / d x_m (the reference's column order)
template <int NQ, int NQV>
__device__ __forceinline__ void vgrad_node(const double *sU, const double *sD, const double *sDv,
                                           const double *__restrict__ vg, int n, double *out)
{
    constexpr int Np = NQ * NQ * NQV, Nij = NQ * NQ;
    const int i = n % NQ, j = (n / NQ) % NQ, k = n / Nij;
    double x[3][3];  // x[d][m] = d xi_d / d x_m
#pragma unroll
    for (int d = 0; d < 3; ++d)
#pragma unroll
        for (int m = 0; m < 3; ++m) x[d][m] = vg[(XI1X1 + d + 3 * m) * Np];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double *u = sU + c * Np;
        double g1 = sD[i] * u[NQ * (j + NQ * k)];
#pragma unroll
        for (int r = 1; r < NQ; ++r) g1 += sD[i + NQ * r] * u[r + NQ * (j + NQ * k)];
        double g2 = sD[j] * u[i + Nij * k];
#pragma unroll
        for (int s = 1; s < NQ; ++s) g2 += sD[j + NQ * s] * u[i + NQ * s + Nij * k];
        double g3 = sDv[k] * u[i + NQ * j];
#pragma unroll
        for (int t = 1; t < NQV; ++t) g3 += sDv[k + NQV * t] * u[i + NQ * j + Nij * t];
#pragma unroll
        for (int m = 0; m < 3; ++m) out[3 * c + m] = g1 * x[0][m] + g2 * x[1][m] + g3 * x[2][m];
    }
}

// vorticity_kernel! (:393-395) from the nine columns of a node
__device__ __forceinline__ void vorticity_node(const double *vg9, double *om)
{
    om[0] = vg9[7] - vg9[5];  // d2 u3 - d3 u2
    om[1] = vg9[2] - vg9[6];  // d3 u1 - d1 u3
    om[2] = vg9[3] - vg9[1];  // d1 u2 - d2 u1
}

// stages the derivative matrices and the element's velocity; returns after the barrier
template <int NQ, int NQV>
__device__ __forceinline__ void stage_velocity(double *sU, double *sD, double *sDv, const double *__restrict__ D,
                                               const double *__restrict__ Dv, int n, const double u[3])
{
    constexpr int Np = NQ * NQ * NQV;
    for (int q = n; q < NQ * NQ; q += Np) sD[q] = D[q];
    for (int q = n; q < NQV * NQV; q += Np) sDv[q] = Dv[q];
#pragma unroll
    for (int c = 0; c < 3; ++c) sU[c * Np + n] = u[c];
    __syncthreads();
}

// VectorGradients(dg, Q): vgrad (nreal, 9, Np); ns = columns of Q (rho, rho u[3] lead)
template <int NQ, int NQV>
__global__ __launch_bounds__(NQ *NQ *NQV) void k_vector_gradients(const double *__restrict__ Q, int ns,
                                                                   const double *__restrict__ vgeo, int nvgeo,
                                                                   const double *__restrict__ D,
                                                                   const double *__restrict__ Dv,
                                                                   double *__restrict__ vgrad)
{
    constexpr int Np = NQ * NQ * NQV;
    __shared__ double sU[3 * Np], sD[NQ * NQ], sDv[NQV * NQV];
    const int64_t e = blockIdx.x;
    const int n = threadIdx.x;
    const double *q = Q + n + (int64_t)Np * ns * e;
    const double rho = q[0];
    const double u[3] = {q[Np] / rho, q[2 * Np] / rho, q[3 * Np] / rho};
    stage_velocity<NQ, NQV>(sU, sD, sDv, D, Dv, n, u);
    double out[9];
    vgrad_node<NQ, NQV>(sU, sD, sDv, vgeo + n + (int64_t)Np * nvgeo * e, n, out);
#pragma unroll
    for (int c = 0; c < 9; ++c) vgrad[n + (int64_t)Np * (c + 9 * e)] = out[c];
}

// The group's nodal pass: Q, the auxiliary state and the nine metric columns are read once per node;
// G (nelem, 14, Np) takes the five prognostic columns, the law's gcm_thermo and Omega, and the three u
// columns go to the auxiliary array of the group's VorticityModel handle, u (nelem, 3, Np).  Every column
// has the bits of the separate calls: the same device functions in the same order.
template <class P, int NQ, int NQV>
__global__ __launch_bounds__(NQ *NQ *NQV) void k_gcm_nodal(typename P::Params prm, const double *__restrict__ Q,
                                                            const double *__restrict__ aux,
                                                            const double *__restrict__ vgeo, int nvgeo,
                                                            const double *__restrict__ D,
                                                            const double *__restrict__ Dv, double *__restrict__ G,
                                                            double *__restrict__ uout)
{
    constexpr int Np = NQ * NQ * NQV;
    static_assert(P::NS >= 5, "rho, rho u[3], rho e");
    __shared__ double sU[3 * Np], sD[NQ * NQ], sDv[NQV * NQV];
    const int64_t e = blockIdx.x;
    const int n = threadIdx.x;
    Vec<P::NS> lQ;
    Vec<P::NAUX> lA;
    load_state<P::NS, Np>(lQ, Q, n, e);
    load_state<P::NAUX, Np>(lA, aux, n, e);
    const double rho = lQ[0];
    const double u[3] = {lQ[1] / rho, lQ[2] / rho, lQ[3] / rho};
    stage_velocity<NQ, NQV>(sU, sD, sDv, D, Dv, n, u);
    double out[9], om[3];
    vgrad_node<NQ, NQV>(sU, sD, sDv, vgeo + n + (int64_t)Np * nvgeo * e, n, out);
    vorticity_node(out, om);
    Vec<6> th;
    P::gcm_thermo(prm, th, lQ, lA);
    double *g = G + n + (int64_t)Np * GCM_NCOL * e;
#pragma unroll
    for (int s = 0; s < 5; ++s) g[s * Np] = lQ[s];
#pragma unroll
    for (int s = 0; s < 6; ++s) g[(5 + s) * Np] = th[s];
#pragma unroll
    for (int s = 0; s < 3; ++s) g[(11 + s) * Np] = om[s];
#pragma unroll
    for (int c = 0; c < 3; ++c) uout[n + (int64_t)Np * (c + 3 * e)] = u[c];
}

}  // namespace cmdg
