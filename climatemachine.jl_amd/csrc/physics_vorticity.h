// Device functor for the reference's VorticityModel (src/Diagnostics/vorticity_balancelaw.jl): a
// mini balance law whose tendency, evaluated with beta = 0, is Omega_bl = curl u in weak form with
// central face fluxes -- the `vort2` of the AtmosGCMDefault diagnostics group.  State: Omega_bl (3);
// auxiliary: u (3), filled by the caller; first-order flux: the antisymmetric matrix of :76-80; no
// gradient, gradient-flux or hyperdiffusive variables, no second-order flux, no source, no nodal
// auxiliary update; every boundary tag is the `nothing` condition (:92-93): boundary_state! does
// nothing, the plus side stays the copy of the minus side, state and auxiliary
// (DGModel_kernels.jl:686-692).  Used with CMDG_CENTRAL_FIRST_ORDER.
#pragma once
#include "cmdg_common.h"
#include "law_defaults.h"

namespace cmdg {

struct VorticityParams {
    int unused;
};

struct VorticityLaw : LawDefaults {
    using Params = VorticityParams;
    static constexpr int NS = 3, NAUX = 3, NGRAD = 0, NGF = 0, NFAUX = 3;
    __host__ __device__ static constexpr int face_aux(int i) { return i; }
    static constexpr GradFlux GRADFLUX = GradFlux::never;
    static void make_params(Params &p, const int32_t *, const double *) { p.unused = 0; }

    // flux.Omega_bl = [0 u3 -u2; -u3 0 u1; u2 -u1 0]: row d, column c -> F[d + 3 c]
    __device__ static void flux_first_order(const Params &, double *F, const double *, const double *aux, double,
                                            int)
    {
        const double u1 = aux[0], u2 = aux[1], u3 = aux[2];
        F[1 + 3 * 0] -= u3;
        F[2 + 3 * 0] += u2;
        F[0 + 3 * 1] += u3;
        F[2 + 3 * 1] -= u1;
        F[0 + 3 * 2] -= u2;
        F[1 + 3 * 2] += u1;
    }
    __device__ static void wavespeed(const Params &, double *ws, const double *, const double *, const double *,
                                     double, int)
    {
        ws[0] = ws[1] = ws[2] = 0.0;
    }
};

}  // namespace cmdg
