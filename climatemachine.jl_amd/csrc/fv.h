// Vertical finite-volume passes of a DGFVModel handle (polynomialorder = (N_h, 0)): gfx950 kernels
// that replace vert_fvm_interface_tendency! and vert_fvm_interface_gradients!
// (src/Numerics/DGMethods/DGFVModel_kernels.jl:47-739, :741-944).
//
// The reference walks a stack serially, one thread per horizontal node (Nq^2 = 25 threads per
// stack).  Here the work of a stack is laid out over (horizontal node, cell): the node index is the
// fastest thread index, so every global access is a run of Nq^2 consecutive doubles, and the cells
// of a stack are worked on side by side.  One work-group owns one whole stack; stacks are never
// split across ranks, so nothing outside the group's stack is read.
//   phase 1  thread = (node, cell): prognostic -> primitive, primitives and cell weights 2 JcV of
//            the whole stack into LDS;
//   phase 2  thread = (node, face): the two cells next to the face are reconstructed from their
//            stencils in LDS, first-order numerical flux on the reconstructed face states,
//            second-order numerical flux on the cell states, boundary fluxes at the two ends; the
//            face flux goes to LDS;
//   phase 3  thread = (node, cell): bottom-face term, then source, then top-face term -- the
//            reference's summation order per cell -- and its write rules (:597-613, :634-643,
//            :720-734).
// LDS: Nq^2 * (NS * nvertelem + NS * (nvertelem + 1) + nvertelem) doubles (fv_lds_bytes: primitives,
// fluxes of nvertelem + 1 faces, weights).  Up to FV_LDS_DEFAULT a launch asks for it as it is; up to
// FV_LDS_MAX the handle raises the kernel's dynamic-LDS limit when it is created (engine_fv.h).
#pragma once
#include "kernels_common.h"

namespace cmdg {

enum { FV_RECON_CONSTANT = 0, FV_RECON_LINEAR = 1 };
enum { FV_LIMITER_VANLEER = 0, FV_LIMITER_NONE = 1 };

// ---- law hooks with the reference's defaults (src/BalanceLaws/prog_prim_conversion.jl) ----------
// A law that converts says so (HAS_PRIM_CONVERSION, HAS_FACE_AUX_STATE, law_defaults.h) and defines
// prognostic_to_primitive / primitive_to_prognostic (prm, out, in, aux) or
// construct_face_auxiliary_state (prm, aux_face, aux_cell, dz); the defaults are the identity and
// the copy.
template <class P>
__device__ __forceinline__ void law_prognostic_to_primitive(const typename P::Params &prm, double *prim,
                                                            const double *prog, const double *aux)
{
    if constexpr (P::HAS_PRIM_CONVERSION) {
        P::prognostic_to_primitive(prm, prim, prog, aux);
    } else {
#pragma unroll
        for (int s = 0; s < P::NS; ++s) prim[s] = prog[s];
    }
}
template <class P>
__device__ __forceinline__ void law_primitive_to_prognostic(const typename P::Params &prm, double *prog,
                                                            const double *prim, const double *aux)
{
    if constexpr (P::HAS_PRIM_CONVERSION) {
        P::primitive_to_prognostic(prm, prog, prim, aux);
    } else {
#pragma unroll
        for (int s = 0; s < P::NS; ++s) prog[s] = prim[s];
    }
}
template <class P>
__device__ __forceinline__ void law_face_auxiliary_state(const typename P::Params &prm, double *aux_face,
                                                         const double *aux_cell, double dz)
{
    if constexpr (P::HAS_FACE_AUX_STATE) {
        P::construct_face_auxiliary_state(prm, aux_face, aux_cell, dz);
    } else {
#pragma unroll
        for (int s = 0; s < P::NAUX; ++s) aux_face[s] = aux_cell[s];
    }
}

template <class P>
struct FvArgs {
    typename P::Params prm;
    GridDev g;
    const int64_t *elems;  // 1-based element list of whole stacks, bottom element first
    int64_t nelems;
    int nvert;
    const double *Q, *aux, *derived;
    double *gf;
    double *tendency;
    double t, alpha, beta;
    int increment;   // dg.direction isa EveryDirection: after the horizontal passes
    int add_source;  // dg.direction isa VerticalDirection
    int model_dir, nf_first;
    int recon, limiter;
    int hydrostatic;  // HBFVReconstruction around the reconstruction (laws with P::PRIM_P >= 0)
};

// slope of the limited linear reconstruction (FVReconstructions.jl:168-192)
__device__ __forceinline__ double fv_limited_slope(int limiter, double d_top, double d_bot)
{
    if (limiter == FV_LIMITER_NONE) return (d_top + d_bot) / 2;
    return d_top * d_bot > 0 ? 2 * d_top * d_bot / (d_top + d_bot) : 0.0;
}

// Half-width of the stencil of cell k (0-based) of a stack of nv cells: the full width W in the
// interior and on a periodic stack; next to a non-periodic end it shrinks symmetrically
// (:475-516), and the bottom cell, reconstructed before the walk starts, uses itself alone (:304-311).
template <int W, bool PERIODIC>
__device__ __forceinline__ int fv_half_width(int k, int nv)
{
    if (PERIODIC || W == 0) return W;
    const int eV = k + 1;
    if (eV == 1) return 0;
    if (W < eV && eV < nv - W + 1) return W;
    if (eV <= W) return eV - 1;
    return nv - eV;
}

// Face primitives of cell k from the 2 hw + 1 cells around it (neighbours taken modulo the stack
// height, as the reference loads them).  FVConstant and a one-cell range copy the cell; FVLinear on
// a wider range works on its middle three cells (FVReconstructions.jl:103-143).
// hb (laws that name a pressure primitive, P::PRIM_P >= 0; hb_g their g): HBFVReconstruction around it
// (src/Atmos/Model/reconstructions.jl:15-73) -- the hydrostatic reference pressures of the stencil,
// built outward from the centre cell with rho g dz / 2 of the cell weights, leave p before the
// reconstruction, and p_ref +- rho g dz / 2 of the centre cell joins the two face values after it.
// Cells further out than the middle three never reach the inner reconstruction, so their
// reference pressures are not formed.
template <class P, int W, bool PERIODIC>
__device__ __forceinline__ void fv_reconstruct(const double *sP, const double *sW, int Nh, int nv, int n, int k,
                                               int recon, int limiter, bool hb, double hb_g, double *bot,
                                               double *top)
{
    constexpr int NS = P::NS;
    constexpr bool CAN_HB = P::PRIM_P >= 0;
    constexpr int PP = CAN_HB ? P::PRIM_P : 0, PR = CAN_HB ? P::PRIM_RHO : 0;
    const int hw = fv_half_width<W, PERIODIC>(k, nv);
    double p_ref = 0, h2 = 0;  // centre cell: reference pressure, rho g dz / 2
    if constexpr (CAN_HB) {
        if (hb) {
            p_ref = sP[(k * NS + PP) * Nh + n];
            h2 = sP[(k * NS + PR) * Nh + n] * hb_g * sW[k * Nh + n] / 2;
        }
    }
    if (W == 0 || recon == FV_RECON_CONSTANT || hw == 0) {
#pragma unroll
        for (int s = 0; s < NS; ++s) bot[s] = top[s] = sP[(k * NS + s) * Nh + n];
        if constexpr (CAN_HB) {
            if (hb) {
                const double c2 = bot[PP] - p_ref;
                bot[PP] = c2 + (p_ref + h2);
                top[PP] = c2 + (p_ref - h2);
            }
        }
        return;
    }
    const int km = k == 0 ? nv - 1 : k - 1, kp = k == nv - 1 ? 0 : k + 1;
    const double w1 = sW[km * Nh + n], w2 = sW[k * Nh + n], w3 = sW[kp * Nh + n];
    const double wi_top = 1 / (w3 + w2), wi_bot = 1 / (w2 + w1);
    double pm_ref = 0, pp_ref = 0;  // reference pressures of the cells below and above
    if constexpr (CAN_HB) {
        if (hb) {
            const double h1 = sP[(km * NS + PR) * Nh + n] * hb_g * w1 / 2;
            const double h3 = sP[(kp * NS + PR) * Nh + n] * hb_g * w3 / 2;
            pm_ref = p_ref + (h2 + h1);
            pp_ref = p_ref - (h2 + h3);
        }
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        double c1 = sP[(km * NS + s) * Nh + n], c2 = sP[(k * NS + s) * Nh + n], c3 = sP[(kp * NS + s) * Nh + n];
        if constexpr (CAN_HB) {
            if (hb && s == PP) c1 -= pm_ref, c2 -= p_ref, c3 -= pp_ref;
        }
        const double d_top = wi_top * (c3 - c2), d_bot = wi_bot * (c2 - c1);
        const double d = fv_limited_slope(limiter, d_top, d_bot);
        top[s] = c2 + d * w2;
        bot[s] = c2 - d * w2;
    }
    if constexpr (CAN_HB) {
        if (hb) {
            bot[PP] += p_ref + h2;
            top[PP] += p_ref - h2;
        }
    }
}

__host__ __device__ inline int fv_threads(int Nh, int nvert)
{
    const int want = Nh * (nvert + 1);
    return want >= 256 ? 256 : ((want + 63) / 64) * 64;
}
// what a launch may ask for without more ado, and what a work-group may own on gfx950
constexpr size_t FV_LDS_DEFAULT = 64 * 1024, FV_LDS_MAX = 160 * 1024;
inline size_t fv_lds_bytes(int ns, int Nh, int nvert)
{
    return sizeof(double) * (size_t)Nh * ((size_t)ns * nvert + (size_t)ns * (nvert + 1) + nvert);
}

template <class P, int NQ, int W, bool PERIODIC>
__global__ void __launch_bounds__(256) k_fv_tendency(const FvArgs<P> a)
{
    constexpr int Nh = NQ * NQ, NS = P::NS, NAUX = P::NAUX, NGF = P::NGF, NHYP = P::NHYP;
    static_assert(NHYP == 0, "DGFVModel: no hyperdiffusive states (DGFVModel.jl:91)");
    extern __shared__ double fv_lds[];
    const int nv = a.nvert;
    double *sP = fv_lds;                    // primitives [cell][s][node]
    double *sX = sP + NS * nv * Nh;         // face fluxes [face][s][node], face f below cell f
    double *sW = sX + NS * (nv + 1) * Nh;   // cell weights 2 JcV [cell][node]
    const int64_t e0 = a.elems[(int64_t)blockIdx.x * nv] - 1;  // bottom element of this group's stack
    const int nt = (int)blockDim.x, tid = (int)threadIdx.x;
    const int64_t vstride = (int64_t)Nh * a.g.nvgeo;
    constexpr int NFP = Nh;  // stride of the face tables (Nfp_max of an (N_h, 0) grid)
    const bool hb = P::PRIM_P >= 0 && a.hydrostatic;
    const double hb_g = P::prim_gravity(a.prm);
    // ---- phase 1
    for (int w = tid; w < nv * Nh; w += nt) {
        const int k = w / Nh, n = w - k * Nh;
        const int64_t e = e0 + k;
        Vec<NS> q, prim;
        Vec<NAUX> ax;
        load_state<NS, Nh>(q, a.Q, n, e);
        load_state<NAUX, Nh>(ax, a.aux, n, e);
        law_prognostic_to_primitive<P>(a.prm, prim, q, ax);
#pragma unroll
        for (int s = 0; s < NS; ++s) sP[(k * NS + s) * Nh + n] = prim[s];
        sW[k * Nh + n] = 2 * a.g.vgeo[n + Nh * JCV + vstride * e];
    }
    __syncthreads();
    // ---- phase 2: faces 0 .. nv (face nv of a periodic stack is face 0)
    const int nfaces = PERIODIC ? nv : nv + 1;
    for (int w = tid; w < nfaces * Nh; w += nt) {
        const int f = w / Nh, n = w - f * Nh;
        Vec<NS> flux, bot, top, QM, QPn, QcM, QcP;
        Vec<NAUX> auxcM, auxcP, auxM, auxPn;
        Vec<NGF> gfM, gfP;
        Vec<NHYP> hypM, hypP;
        double nrm[3];
        flux.negzero();
#pragma unroll
        for (int s = 0; s < NGF; ++s) gfM[s] = gfP[s] = 0.0;
        const bool bottom_bc = !PERIODIC && f == 0, top_bc = !PERIODIC && f == nv;
        // the cell whose face this is ("minus"): the cell above the face, or the top cell
        const int km = top_bc ? nv - 1 : f;
        const int64_t eM = e0 + km;
        const int face = top_bc ? 5 : 4;
        const double *sg = a.g.sgeo + 5 * (n + (int64_t)NFP * (face + 6 * eM));
        nrm[0] = sg[SN1], nrm[1] = sg[SN2], nrm[2] = sg[SN3];
        load_state<NS, Nh>(QcM, a.Q, n, eM);
        load_state<NAUX, Nh>(auxcM, a.aux, n, eM);
        if (NGF > 0 && needs_gradflux<P>(a.prm)) load_gf<P, Nh>(gfM, a.gf, n, eM);
        fv_reconstruct<P, W, PERIODIC>(sP, sW, Nh, nv, n, km, a.recon, a.limiter, hb, hb_g, bot, top);
        const double wM = sW[km * Nh + n];
        law_face_auxiliary_state<P>(a.prm, auxM, auxcM, top_bc ? wM : -wM);
        law_primitive_to_prognostic<P>(a.prm, QM, top_bc ? top : bot, auxM);
        if (bottom_bc || top_bc) {
            const int bctag = (int)a.g.elemtobndy[face + 6 * eM];
            // the cell's own face state is the ghost and state_bottom1 (:337-394, :645-717)
#pragma unroll
            for (int s = 0; s < NS; ++s) QPn[s] = QM[s];
#pragma unroll
            for (int s = 0; s < NAUX; ++s) auxPn[s] = auxM[s];
            P::boundary_state(a.prm, BS_FIRST, bctag, QPn, auxPn, nrm, QM, auxM, a.t, QM, auxM);
            nf_first_order<P>(a.prm, a.nf_first, flux, nrm, QM, auxM, QPn, auxPn, a.t, DIR_VERTICAL);
#pragma unroll
            for (int s = 0; s < NS; ++s) QcP[s] = QcM[s];
#pragma unroll
            for (int s = 0; s < NAUX; ++s) auxcP[s] = auxcM[s];
#pragma unroll
            for (int s = 0; s < NGF; ++s) gfP[s] = gfM[s];
            Vec<3 * NS> FP;
            FP.negzero();
            P::boundary_flux_second_order(a.prm, bctag, FP, QcP, gfP, hypP, auxcP, nrm, QcM, gfM, hypM, auxcM, a.t,
                                          QcM, gfM, auxcM);
#pragma unroll
            for (int s = 0; s < NS; ++s) flux[s] += FP[3 * s] * nrm[0] + FP[3 * s + 1] * nrm[1] + FP[3 * s + 2] * nrm[2];
        } else {
            // the cell below the face ("plus"): its top reconstruction
            const int kp = f == 0 ? nv - 1 : f - 1;
            const int64_t eP = e0 + kp;
            Vec<NS> botP, topP;
            load_state<NS, Nh>(QcP, a.Q, n, eP);
            load_state<NAUX, Nh>(auxcP, a.aux, n, eP);
            if (NGF > 0 && needs_gradflux<P>(a.prm)) load_gf<P, Nh>(gfP, a.gf, n, eP);
            fv_reconstruct<P, W, PERIODIC>(sP, sW, Nh, nv, n, kp, a.recon, a.limiter, hb, hb_g, botP, topP);
            law_face_auxiliary_state<P>(a.prm, auxPn, auxcP, sW[kp * Nh + n]);
            law_primitive_to_prognostic<P>(a.prm, QPn, topP, auxPn);
            nf_first_order<P>(a.prm, a.nf_first, flux, nrm, QM, auxM, QPn, auxPn, a.t, DIR_VERTICAL);
            // CentralNumericalFluxSecondOrder on the cell states (:558-572)
            Vec<3 * NS> FM, FP;
            FM.negzero();
            P::flux_second_order(a.prm, FM, QcM, gfM, hypM, auxcM, a.t);
            FP.negzero();
            P::flux_second_order(a.prm, FP, QcP, gfP, hypP, auxcP, a.t);
            const double nh0 = nrm[0] / 2, nh1 = nrm[1] / 2, nh2 = nrm[2] / 2;
#pragma unroll
            for (int s = 0; s < NS; ++s)
                flux[s] += (FM[3 * s] + FP[3 * s]) * nh0 + (FM[3 * s + 1] + FP[3 * s + 1]) * nh1 +
                           (FM[3 * s + 2] + FP[3 * s + 2]) * nh2;
        }
#pragma unroll
        for (int s = 0; s < NS; ++s) sX[(f * NS + s) * Nh + n] = flux[s];
    }
    __syncthreads();
    // ---- phase 3
    for (int w = tid; w < nv * Nh; w += nt) {
        const int k = w / Nh, n = w - k * Nh;
        const int64_t e = e0 + k;
        const double vMI = a.g.vgeo[n + Nh * VMI + vstride * e];
        auto sM_of = [&](int face, int64_t el) { return a.g.sgeo[5 * (n + (int64_t)NFP * (face + 6 * el)) + SSM]; };
        Vec<NS> S;
        S.negzero();
        if constexpr (P::HAS_SOURCE) {
            if (a.add_source) {
                Vec<NS> q;
                Vec<NAUX> ax;
                Vec<NGF> lgf;
                Vec<P::NDER> lder;
                load_state<NS, Nh>(q, a.Q, n, e);
                load_state<NAUX, Nh>(ax, a.aux, n, e);
#pragma unroll
                for (int s = 0; s < NGF; ++s) lgf[s] = 0.0;
                if (NGF > 0 && needs_gradflux<P>(a.prm)) load_gf<P, Nh>(lgf, a.gf, n, e);
                load_state<P::NDER, Nh>(lder, a.derived, n, e);
                P::source(a.prm, S, q, lgf, ax, lder, a.t, a.model_dir);
            }
        }
        const bool src = P::HAS_SOURCE && a.add_source;
        const double sMb = sM_of(4, e);  // the face below the cell
        const bool wrap_top = PERIODIC && k == nv - 1;
        // the face above the cell is the bottom face of the cell above (the top boundary face)
        const int fu = wrap_top ? 0 : k + 1;
        const double sMu = (!PERIODIC && k == nv - 1) ? sM_of(5, e) : sM_of(4, wrap_top ? e0 : e + 1);
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int64_t o = n + (int64_t)Nh * (s + (int64_t)NS * e);
            const double fb = sX[(k * NS + s) * Nh + n], ft = sX[(fu * NS + s) * Nh + n];
            auto write = [&](double lt) {
                if (a.increment)
                    a.tendency[o] += lt;
                else
                    a.tendency[o] = a.beta != 0 ? lt + a.beta * a.tendency[o] : lt;
            };
            if (wrap_top) {
                // the top cell of a periodic stack: written with the face above it first (eV_up = 1),
                // its bottom-face term arrives with += (:634-643)
                double lt = -0.0;
                if (src) lt += S[s];
                lt += a.alpha * sMu * vMI * ft;
                write(lt);
                double l2 = -a.alpha * sMb * vMI * fb;
                if (src) l2 += S[s];
                a.tendency[o] += l2;
            } else {
                double lt = -a.alpha * sMb * vMI * fb;
                if (src) lt += S[s];
                if (!PERIODIC && k == nv - 1)
                    lt -= a.alpha * sMu * vMI * ft;
                else
                    lt += a.alpha * sMu * vMI * ft;
                write(lt);
            }
        }
    }
}

// vert_fvm_interface_gradients! (:741-944): thread = (node, element of the list), three-cell
// stencil, G* the mass-weighted interpolation to the face, boundary faces through the central
// gradient boundary flux, the result through compute_gradient_flux!.
template <class P, int NQ, bool PERIODIC>
__global__ void __launch_bounds__(256) k_fv_gradients(const FvArgs<P> a)
{
    constexpr int Nh = NQ * NQ, NS = P::NS, NAUX = P::NAUX, NGRAD = P::NGRAD, NGF = P::NGF;
    constexpr int NFP = Nh;
    const int64_t I = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (I >= a.nelems * Nh) return;
    const int n = (int)(I % Nh);
    const int64_t e = a.elems[I / Nh] - 1;
    const int nv = a.nvert, eV = (int)(e % nv);
    const int64_t vstride = (int64_t)Nh * a.g.nvgeo;
    int64_t els[3] = {e, e, e};
    int bc[2] = {0, 0};
    if (eV > 0)
        els[0] = e - 1;
    else if (PERIODIC)
        els[0] = e + nv - 1;
    else
        bc[0] = (int)a.g.elemtobndy[4 + 6 * e];
    if (eV < nv - 1)
        els[2] = e + 1;
    else if (PERIODIC)
        els[2] = e - nv + 1;
    else
        bc[1] = (int)a.g.elemtobndy[5 + 6 * e];
    Vec<NS> q[3];
    Vec<NAUX> ax[3];
    Vec<NGRAD> G[3];
    double M[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        load_state<NS, Nh>(q[k], a.Q, n, els[k]);
        load_state<NAUX, Nh>(ax[k], a.aux, n, els[k]);
        M[k] = a.g.vgeo[n + Nh * VM + vstride * els[k]];
        G[k].negzero();
        P::gradient_argument(a.prm, G[k], q[k], ax[k], a.t);
    }
    const double vMI = a.g.sgeo[5 * (n + (int64_t)NFP * (4 + 6 * e)) + SVMI];
    Vec<3 * NGRAD> nG;
    nG.negzero();
#pragma unroll
    for (int f = 0; f < 2; ++f) {
        const double *sg = a.g.sgeo + 5 * (n + (int64_t)NFP * (4 + f + 6 * e));
        const double nrm[3] = {sg[SN1], sg[SN2], sg[SN3]}, sM = sg[SSM];
        if (bc[f] == 0) {
#pragma unroll
            for (int s = 0; s < NGRAD; ++s) {
                const double Gs = (M[f] * G[f + 1][s] + M[f + 1] * G[f][s]) / (M[f] + M[f + 1]);
#pragma unroll
                for (int d = 0; d < 3; ++d) nG[d + 3 * s] += vMI * sM * nrm[d] * Gs;
            }
        } else {
            // numerical_boundary_flux_gradient!(CentralNumericalFluxGradient(), ...): the plus side is
            // the cell itself (els[2 f] == e on a boundary)
            Vec<NS> QP, Q1;
            Vec<NAUX> auxP, aux1;
            Vec<NGRAD> GP;
#pragma unroll
            for (int s = 0; s < NS; ++s) QP[s] = q[2 * f][s], Q1[s] = __builtin_nan("");
#pragma unroll
            for (int s = 0; s < NAUX; ++s) auxP[s] = ax[2 * f][s], aux1[s] = __builtin_nan("");
            P::boundary_state(a.prm, BS_GRADIENT, bc[f], QP, auxP, nrm, q[1], ax[1], a.t, Q1, aux1);
            GP.negzero();
            P::gradient_argument(a.prm, GP, QP, auxP, a.t);
#pragma unroll
            for (int s = 0; s < NGRAD; ++s)
#pragma unroll
                for (int d = 0; d < 3; ++d) nG[d + 3 * s] += vMI * sM * (nrm[d] * GP[s]);
        }
    }
    Vec<NGF> lgf;
    lgf.negzero();
    if constexpr (NGF > 0) law_gradient_flux<P>(a.prm, lgf, nG, q[1], ax[1], a.t, G[1]);
#pragma unroll
    for (int s = 0; s < NGF; ++s) {
        const int64_t o = gf_at<P, Nh>(n, s, e);
        if (a.increment)
            a.gf[o] += lgf[s];
        else
            a.gf[o] = lgf[s];
    }
}

}  // namespace cmdg
