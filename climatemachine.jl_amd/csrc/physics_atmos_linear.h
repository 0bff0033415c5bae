// Device functor for AtmosAcousticGravityLinearModel, the linear balance law the reference's
// IMEX configurations solve implicitly in the vertical, of the dry law (MOIST = false) and of the
// moist LES law with EquilMoist (MOIST = true).  Restates, term by term and in the reference's
// summation order:
//   src/Atmos/Model/linear.jl:17-72 (linearized_air_pressure, DryModel / EquilMoist), :95-345 (state
//       layout shared with the full model, no second-order terms, wavespeed soundspeed(ref.T),
//       AtmosBC boundary), linear_atmos_tendencies.jl (which terms),
//   linear_tendencies.jl (Advect, LinearPressureGradient, LinearEnergyFlux, Gravity source).
// The auxiliary array is the full model's (Phi, grad Phi, reference state ...), shared with it
// (DGModel(...; state_auxiliary = dg.state_auxiliary)): NAUX is the full model's count.  The moist
// law's first 15 columns are the dry layout (MoistAtmosModel.init_state_auxiliary), so Phi and the
// reference state sit in the same columns for both.
//
// Parameter block: the full model's (climatemachine.jl_amd/atmos.py, moist.py); this law reads
// dparam[2..6] R_d cp_d cv_d T_0 grav, and the moist one dparam[16] R_v, [20] LH_v0, [21] LH_s0.
// Moist: the sixth state rho q_tot has no flux and no source (linear_atmos_tendencies.jl:17-23,
// 34) and enters only p_lin.  Boundaries: every tag is AtmosBC() (Impenetrable FreeSlip,
// Insulating; the plus side's rho q_tot is the minus side's), boundary_conditions(
// ::AtmosLinearModel) at linear.jl:215-216.
//
// ORIENT = false: AtmosAcousticLinearModel (linear.jl:214-245, linear_tendencies.jl:55-60) of a dry
// model with NoOrientation(): no Phi columns (the reference state follows the coordinates), e_pot = 0
// in p_lin and in the energy flux ((ref.rho e + ref.p) / ref.rho - e_pot) rho u, no source.
#pragma once
#include "cmdg_common.h"
#include "law_defaults.h"

namespace cmdg {

struct AtmosLinearParams {
    double R_d, cp_d, cv_d, T_0;
    double e_int_v0, e_int_i0;  // EquilMoist only
};

template <int NAUX_FULL, bool MOIST = false, bool ORIENT = true>
struct AtmosLinearAG : LawDefaults {
    static_assert(ORIENT || !MOIST, "the moist acoustic law is not laid out");
    using Params = AtmosLinearParams;
    // auxiliary layout of DryAtmos with orientation and reference state (physics_atmos.h), which
    // MoistAtmos keeps in its first 15 columns (physics_moist.h)
    static constexpr int OPHI = 3, OREF = ORIENT ? 7 : 3;
    static constexpr int NS = MOIST ? 6 : 5, NAUX = NAUX_FULL, NGRAD = 0, NGF = 0;
    static constexpr bool HAS_SOURCE = ORIENT;
    // faces read Phi and the reference rho, p, T, rho e
    static constexpr int NFAUX = ORIENT ? 5 : 4;
    __host__ __device__ static constexpr int face_aux(int i)
    {
        return ORIENT ? (i == 0 ? OPHI : OREF + (i - 1)) : OREF + i;
    }
    static constexpr GradFlux GRADFLUX = GradFlux::never;
    static void make_params(Params &p, const int32_t *, const double *dp)
    {
        p.R_d = dp[2];
        p.cp_d = dp[3];
        p.cv_d = dp[4];
        p.T_0 = dp[5];
        // e_int_v0 = LH_v0 - R_v T_0, e_int_i0 = LH_s0 - LH_v0 (physics_moist.h)
        p.e_int_v0 = MOIST ? dp[20] - dp[16] * dp[5] : 0.0;
        p.e_int_i0 = MOIST ? dp[21] - dp[20] : 0.0;
    }
    // linearized_air_pressure (linear.jl:17-36): DryModel passes no moisture terms; EquilMoist
    // (:57-72) passes rho q_tot, with rho q_liq = rho q_ice = 0 kept in the reference's order
    __device__ static double p_lin(const Params &m, const double *Q, const double *aux)
    {
        if constexpr (!ORIENT) return Q[0] * m.R_d * m.T_0 + m.R_d / m.cv_d * Q[4];
        const double rhoe_pot = Q[0] * aux[OPHI];
        if constexpr (MOIST)
            return Q[0] * m.R_d * m.T_0 +
                   m.R_d / m.cv_d * (Q[4] - rhoe_pot - (Q[5] - 0.0) * m.e_int_v0 + 0.0 * (m.e_int_i0 + m.e_int_v0));
        else
            return Q[0] * m.R_d * m.T_0 + m.R_d / m.cv_d * (Q[4] - rhoe_pot);
    }
    __device__ static double soundspeed(const Params &m, double T)
    {
        const double gamma = m.cp_d / m.cv_d;
        return sqrt(gamma * m.R_d * T);
    }

    __device__ static void flux_first_order(const Params &m, double *F, const double *Q,
                                            const double *aux, double, int)
    {
        const double pL = p_lin(m, Q, aux);
        const double h_ref = (aux[OREF + 3] + aux[OREF + 1]) / aux[OREF];
#pragma unroll
        for (int d = 0; d < 3; ++d) F[d] = Q[1 + d];  // Advect
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int d = 0; d < 3; ++d) F[d + 3 * (1 + c)] = d == c ? pL : 0.0;  // pL I
#pragma unroll
        for (int d = 0; d < 3; ++d) F[d + 12] = h_ref * Q[1 + d];  // LinearEnergyFlux
    }
    // Gravity (linear_tendencies.jl: -rho grad Phi in VerticalDirection / EveryDirection only)
    __device__ static void source(const Params &, double *S, const double *Q, const double *,
                                  const double *aux, const double *, double, int direction)
    {
        S[0] = 0;
        S[4] = 0;
        if constexpr (MOIST) S[5] = 0;
#pragma unroll
        for (int d = 0; d < 3; ++d)
            S[1 + d] = !ORIENT || direction == DIR_HORIZONTAL ? 0.0 : -Q[0] * aux[OPHI + 1 + d];
    }
    // wavespeed(::AtmosLinearModel) = soundspeed_air(ref.T) (linear.jl:200-212)
    __device__ static void wavespeed(const Params &m, double *ws, const double *, const double *,
                                     const double *aux, double, int)
    {
        const double c = soundspeed(m, aux[OREF + 2]);
#pragma unroll
        for (int s = 0; s < NS; ++s) ws[s] = c;
    }
    // atmos_boundary_state! of AtmosBC(): Impenetrable(FreeSlip) reflects the normal momentum,
    // Insulating leaves the energy, rho q_tot passes through; the plus-side auxiliary state is the
    // minus side's
    __device__ static void boundary_state(const Params &, int, int, double *QP, double *,
                                          const double *n, const double *QM, const double *,
                                          double, const double *, const double *)
    {
        const double dn = QM[1] * n[0] + QM[2] * n[1] + QM[3] * n[2];
        const double f = 2 * dn;
#pragma unroll
        for (int d = 0; d < 3; ++d) QP[1 + d] -= f * n[d];
    }
};

}  // namespace cmdg
