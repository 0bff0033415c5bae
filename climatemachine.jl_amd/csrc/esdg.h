// Tendency of an ESDGModel handle (cmdg_create_esdg): entropy-stable flux-differencing DG.
// k_esdg_tendency replaces, per element list, the three esdg_volume_tendency! launches
// (src/Numerics/DGMethods/ESDGModel_kernels.jl:30-228) and the four dgsem_interface_tendency!
// launches of (esdg::ESDGModel)(tendency, Q, _, t, alpha, beta) (ESDGModel.jl:110-316).
//
// One work-group per element:
//   phase 1  thread = volume node: what a partner's two-point flux needs of this node (EsdgNode) and
//            M * xi_d,x for the three directions into LDS; beta * tendency + alpha * source;
//   phase 2  thread = volume node: for d = 1, 2, 3 and l = 1 .. Nq the two-point flux H against the
//            l-th node of the xi_d line, - (alpha / M) D[id, l] (G . H), then
//            + (alpha / M) (H . G[ild]) D[l, id]  (ESDGModel_kernels.jl:196-220, same order);
//   phase 3  thread = face node, all six faces at once: the surface flux, lifted into the LDS
//            accumulator one opposite-face pair at a time, faces 1..6 as the DG tendency pass;
//   phase 4  thread = volume node: one store per state.
// The pass is bound by the fp64 instruction stream (3 Nq two-point fluxes per node, two logarithmic
// means each for the entropy-conservative flux), not by HBM: the loops over d and l are kept rolled
// so that one copy of the flux code is resident.  Ghost neighbours are read from the ghost elements
// of Q: an ESDG handle unpacks its exchange as the reference does.
#pragma once
#include "kernels_common.h"
#include "physics_esdg_dryatmos.h"

namespace cmdg {

template <class P>
struct EsdgArgs {
    typename P::Params prm;
    GridDev g;
    const int64_t *elems;  // 1-based element list (interior or exterior)
    int64_t nelems;
    const double *Q;
    const double *aux;
    int naux;  // columns of aux (4, or 8 with a reference state); the kernels read the first 4
    double *tendency;
    double t, alpha, beta;
};

// LDS slots of a node record (EsdgNode members a flux does not read are never stored)
enum { EN_RHO = 0, EN_U = 1, EN_A = 4, EN_P = 5, EN_B = 6, EN_USQ = 7, EN_NSLOT = 8 };

template <class P, int NQ, int VF, int SF>
__global__ void __launch_bounds__((KDims<NQ, NQ>::NT)) k_esdg_tendency(const EsdgArgs<P> a)
{
    using KD = KDims<NQ, NQ>;
    constexpr int Np = KD::Np, NS = P::NS, NAUX = P::NAUX;
    constexpr bool UINV = VF == ESDG_CENTRAL;
    __shared__ double sD[NQ * NQ], sN[EN_NSLOT * Np], sG[9 * Np], sT[NS * Np];
    const int tid = (int)threadIdx.x;
    const int64_t e = a.elems[xcd_remap(blockIdx.x, gridDim.x)] - 1;
    if (tid < NQ * NQ) sD[tid] = a.g.D[tid];
    int32_t f_idP = 0;
    int f_bctag = 0, f_f = 0, f_n = 0;
    KD::face_task(tid, f_f, f_n);
    const bool face_on = SF != ESDG_NONE && tid < KD::NFT;
    if (face_on) face_index<NQ, NQ>(a.g, e, tid, f_f, f_idP, f_bctag);
    Vec<NS> T;
    double MIa = 0;
    EsdgNode n1{};
    if (tid < Np) {
        const double *vg = a.g.vgeo + (int64_t)Np * a.g.nvgeo * e + tid;
        const double M = vg[VM * Np];
        Vec<NS> lQ;
        Vec<NAUX> laux;
        load_state<NS, Np>(lQ, a.Q, tid, e);
#pragma unroll
        for (int s = 0; s < NAUX; ++s)  // (the columns the sources do not read are dropped)
            laux[s] = a.aux[tid + (int64_t)Np * (s + (int64_t)a.naux * e)];
        if constexpr (VF != ESDG_NONE) {
#pragma unroll
            for (int d = 0; d < 3; ++d)
#pragma unroll
                for (int c = 0; c < 3; ++c) sG[(3 * d + c) * Np + tid] = M * vg[(XI1X1 + d + 3 * c) * Np];
            P::template node<UINV>(a.prm, n1, lQ);
            sN[EN_RHO * Np + tid] = n1.rho;
#pragma unroll
            for (int d = 0; d < 3; ++d) sN[(EN_U + d) * Np + tid] = n1.u[d];
            sN[EN_P * Np + tid] = n1.p;
            if constexpr (VF == ESDG_EC) {
                sN[EN_B * Np + tid] = n1.b;
                sN[EN_USQ * Np + tid] = n1.usq;
            } else {
                sN[EN_A * Np + tid] = VF == ESDG_KG ? n1.e : n1.rhoe;
            }
        }
        // Build ode scaling into mass matrix (ESDGModel_kernels.jl:109-120)
        MIa = a.alpha / M;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            T[s] = a.beta != 0 ? a.tendency[tid + (int64_t)Np * (s + (int64_t)NS * e)] : -0.0;
            T[s] *= a.beta;
        }
        Vec<NS> S;
        S.negzero();
        P::source(a.prm, S, lQ, nullptr, laux, nullptr, a.t, DIR_EVERY);
#pragma unroll
        for (int s = 0; s < NS; ++s) T[s] += a.alpha * S[s];
    }
    __syncthreads();
    if constexpr (VF != ESDG_NONE) {
        if (tid < Np) {
#pragma unroll 1
            for (int d = 0; d < 3; ++d) {
                const int stride = d == 0 ? 1 : (d == 1 ? NQ : NQ * NQ);
                const int id = (tid / stride) % NQ;
                const int base = tid - id * stride;
                const double *G = sG + 3 * d * Np;
                const double g1 = G[tid], g2 = G[Np + tid], g3 = G[2 * Np + tid];
#pragma unroll 1
                for (int l = 0; l < NQ; ++l) {
                    const int ild = base + l * stride;
                    EsdgNode n2;
                    n2.rho = sN[EN_RHO * Np + ild];
#pragma unroll
                    for (int c = 0; c < 3; ++c) n2.u[c] = sN[(EN_U + c) * Np + ild];
                    n2.p = sN[EN_P * Np + ild];
                    if constexpr (VF == ESDG_EC) {
                        n2.b = sN[EN_B * Np + ild];
                        n2.usq = sN[EN_USQ * Np + ild];
                    } else if constexpr (VF == ESDG_KG) {
                        n2.e = sN[EN_A * Np + ild];
                    } else {
                        n2.rhoe = sN[EN_A * Np + ild];
                    }
                    double H[3][NS];
                    P::template volume_flux<VF>(a.prm, H, n1, n2);
                    const double Dil = sD[id + NQ * l], Dli = sD[l + NQ * id];
                    const double h1 = G[ild], h2 = G[Np + ild], h3 = G[2 * Np + ild];
#pragma unroll
                    for (int s = 0; s < NS; ++s) {
                        T[s] -= MIa * Dil * (g1 * H[0][s] + g2 * H[1][s] + g3 * H[2][s]);
                        T[s] += MIa * (H[0][s] * h1 + H[1][s] * h2 + H[2][s] * h3) * Dli;
                    }
                }
            }
        }
    }
    if (tid < Np) {
#pragma unroll
        for (int s = 0; s < NS; ++s) sT[s * Np + tid] = T[s];
    }
    // ---- faces: dgsem_interface_tendency! (DGModel_kernels.jl:588-901), no second-order terms ----
    if constexpr (SF != ESDG_NONE) {
        Vec<NS> lift;
        int vidM = 0, fpair = -1;
        if (face_on) {
            const int facedir = f_f < 4 ? DIR_HORIZONTAL : DIR_VERTICAL;
            FacePt fp;
            face_geometry<NQ, NQ>(a.g, e, tid, f_f, f_n, f_idP, f_bctag, fp);
            Vec<NS> QM, QP, flux;
            Vec<NAUX> auxM, auxP;
            load_state<NS, Np>(QM, a.Q, fp.vidM, e);
            load_state<NS, Np>(QP, a.Q, fp.vidP, fp.eP);
#pragma unroll
            for (int s = 0; s < NAUX; ++s) auxM[s] = auxP[s] = 0;
            if (fp.bctag != 0)  // the plus side enters as a copy of the minus side (:686-692)
                P::boundary_state(a.prm, BS_FIRST, fp.bctag, QP, auxP, fp.n, QM, auxM, a.t, nullptr, nullptr);
            flux.negzero();
            if constexpr (SF == ESDG_EC)
                P::surface_ec(a.prm, flux, fp.n, QM, QP);
            else if constexpr (SF == ESDG_EC_PENALTY)
                P::surface_ec_penalty(a.prm, flux, fp.n, QM, QP);
            else if constexpr (SF == ESDG_MATRIX)
                P::surface_matrix(a.prm, flux, fp.n, QM, QP);
            else
                nf_first_order<P>(a.prm, NF_RUSANOV, flux, fp.n, QM, auxM, QP, auxP, a.t, facedir);
#pragma unroll
            for (int s = 0; s < NS; ++s) lift[s] = a.alpha * fp.vMI * fp.sM * flux[s];
            vidM = fp.vidM;
            fpair = f_f / 2;
        }
        __syncthreads();
#pragma unroll
        for (int p = 0; p < 3; ++p) {  // opposite faces touch disjoint nodes
            if (fpair == p) {
#pragma unroll
                for (int s = 0; s < NS; ++s) sT[s * Np + vidM] -= lift[s];
            }
            __syncthreads();
        }
    }
    if (tid < Np) {
#pragma unroll
        for (int s = 0; s < NS; ++s) a.tendency[tid + (int64_t)Np * (s + (int64_t)NS * e)] = sT[s * Np + tid];
    }
}

// state_to_entropy_variables! and state_to_entropy of every node of the real elements:
// beta (Np, 6, nelem) and eta (Np, 1, nelem), either may be NULL
template <class P, int Np>
__global__ void k_esdg_entropy(typename P::Params prm, const double *__restrict__ Q, const double *__restrict__ aux,
                               int naux, double *__restrict__ beta, double *__restrict__ eta, int64_t nreal)
{
    const int64_t I = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (I >= nreal * Np) return;
    const int64_t e = I / Np;
    const int n = (int)(I - e * Np);
    Vec<P::NS> lQ;
    load_state<P::NS, Np>(lQ, Q, n, e);
    const double Phi[1] = {aux[n + (int64_t)Np * naux * e]};
    if (beta) {
        double ent[P::NENT];
        P::state_to_entropy_variables(prm, ent, lQ, Phi);
#pragma unroll
        for (int s = 0; s < P::NENT; ++s) beta[n + (int64_t)Np * (s + (int64_t)P::NENT * e)] = ent[s];
    }
    if (eta) eta[n + (int64_t)Np * e] = P::state_to_entropy(prm, lQ, Phi);
}

}  // namespace cmdg
