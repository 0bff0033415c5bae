// Device functor for DryAtmosAcousticGravityLinearModel, the linear balance law the reference's
// entropy-stable baroclinic wave solves implicitly in the vertical (an ordinary DGModel law next to
// the ESDGModel handle of physics_esdg_dryatmos.h).  Restates, term by term and in the reference's
// summation order:
//   test/Numerics/ESDGMethods/DryAtmos/linear.jl:16-24 (linearized_pressure), :85-95 (wavespeed
//   soundspeed(ref.rho, ref.p)), :97-105 (boundary tags (1, 2), the full model's wall), :133-149
//   (flux_first_order!), :150-167 (source!: vertical and every direction only); no second-order
//   terms, no gradients.
// The reference's compile-time settings are fixed as physics_esdg_dryatmos.h fixes them:
// total_energy = false (pL = (gamma - 1) rho e reads no Phi, the energy gets the work of gravity as a
// source) and fluctuation_gravity = false.
//
// State: rho, rho u[3], rho e.  The auxiliary array is the ESDG model's own, shared with it
// (DGModel(...; state_auxiliary = esdg.state_auxiliary)): Phi, grad Phi[3], ref_state.{T, p, rho,
// rho e}; the law needs the reference state, so the count is always 8.  Faces read ref.p, ref.rho and
// ref.rho e.  Parameter block: the full model's (EsdgDryAtmos::make_params).
#pragma once
#include "physics_esdg_dryatmos.h"

namespace cmdg {

struct EsdgDryAtmosLinearAG : LawDefaults {
    using Full = EsdgDryAtmos;
    using Params = Full::Params;
    static constexpr int OGRAD = 1, OREF = 4;  // grad Phi; ref.T, ref.p, ref.rho, ref.rho e
    static constexpr int NS = 5, NAUX = 8, NGRAD = 0, NGF = 0;
    static constexpr bool HAS_SOURCE = true;
    static constexpr int NFAUX = 3;
    __host__ __device__ static constexpr int face_aux(int i) { return OREF + 1 + i; }
    static constexpr GradFlux GRADFLUX = GradFlux::never;
    static void make_params(Params &p, const int32_t *ip, const double *dp) { Full::make_params(p, ip, dp); }

    // linearized_pressure  linear.jl:16-24 (total_energy = false)
    __device__ __forceinline__ static double linearized_pressure(const Params &m, double, double rhoe, double)
    {
        return (m.gamma - 1) * rhoe;
    }
    // flux_first_order!  :133-149; F[d + 3 s] arrives as -0
    __device__ static void flux_first_order(const Params &m, double *F, const double *Q, const double *aux, double,
                                            int)
    {
#pragma unroll
        for (int d = 0; d < 3; ++d) F[d] = Q[1 + d];  // flux.rho = rho u
        const double pL = linearized_pressure(m, Q[0], Q[4], aux[0]);
#pragma unroll
        for (int d = 0; d < 3; ++d) F[d + 3 * (1 + d)] += pL;  // flux.rho u += pL I
        const double h_ref = (aux[OREF + 3] + aux[OREF + 1]) / aux[OREF + 2];
#pragma unroll
        for (int d = 0; d < 3; ++d) F[d + 12] = h_ref * Q[1 + d];  // flux.rho e
    }
    // source!  :150-167
    __device__ static void source(const Params &, double *S, const double *Q, const double *, const double *aux,
                                  const double *, double, int direction)
    {
        if (direction == DIR_HORIZONTAL) return;
#pragma unroll
        for (int d = 0; d < 3; ++d) S[1 + d] -= Q[0] * aux[OGRAD + d];
        S[4] -= Q[1] * aux[OGRAD] + Q[2] * aux[OGRAD + 1] + Q[3] * aux[OGRAD + 2];
    }
    // wavespeed  :85-95
    __device__ static void wavespeed(const Params &m, double *ws, const double *, const double *, const double *aux,
                                     double, int)
    {
        const double c = Full::soundspeed(m, aux[OREF + 2], aux[OREF + 1]);
#pragma unroll
        for (int s = 0; s < NS; ++s) ws[s] = c;
    }
    // boundary_state!(nf, bc, lm, args...) = boundary_state!(nf, bc, lm.atmos, args...)  :98-105
    __device__ static void boundary_state(const Params &m, int kind, int bctag, double *QP, double *auxP,
                                          const double *n, const double *QM, const double *auxM, double t,
                                          const double *Q1, const double *aux1)
    {
        Full::boundary_state(m, kind, bctag, QP, auxP, n, QM, auxM, t, Q1, aux1);
    }
};

}  // namespace cmdg
