// The nodal kernels: one thread per node or one work-group per element, no face terms.  What the
// law layer of the engine (engine_law.h) launches.
#pragma once
#include "kernels_common.h"

namespace cmdg {

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
