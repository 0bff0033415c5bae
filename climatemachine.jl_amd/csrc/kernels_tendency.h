// The tendency pass (kernels.h has the phases every pass kernel goes through).
#pragma once
#include "kernels_common.h"

namespace cmdg {

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

}  // namespace cmdg
