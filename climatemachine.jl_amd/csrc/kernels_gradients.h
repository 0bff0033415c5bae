// The gradient pass and the passes of the hyperdiffusion: Laplacian, fused gradient + Laplacian,
// gradient of Laplacian (kernels.h has the phases every pass kernel goes through).
#pragma once
#include "kernels_common.h"

namespace cmdg {

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

}  // namespace cmdg
