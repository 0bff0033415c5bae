// Device functor for the reference's PressureGradientModel (src/Atmos/Model/ref_state.jl:196-233):
// a mini balance law whose tendency is the DG gradient of the auxiliary field p, "computed as
// div(p I) ... to be numerically consistent with the way this gradient is computed in the
// dynamics".  State: grad p (3); auxiliary: p (1); first-order flux F.grad_p -= p I; no
// source, no second-order terms, boundary_state! does nothing (plus side = minus side).
#pragma once
#include "cmdg_common.h"
#include "law_defaults.h"

namespace cmdg {

struct PGradParams {
    int unused;
};

struct PressureGradient : LawDefaults {
    using Params = PGradParams;
    static constexpr int NS = 3, NAUX = 1, NGRAD = 0, NGF = 0, NFAUX = 1;
    static constexpr GradFlux GRADFLUX = GradFlux::never;
    static void make_params(Params &p, const int32_t *, const double *) { p.unused = 0; }

    __device__ static void flux_first_order(const Params &, double *F, const double *,
                                            const double *aux, double, int)
    {
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int d = 0; d < 3; ++d) F[d + 3 * c] -= aux[0] * (d == c ? 1.0 : 0.0);
    }
    __device__ static void wavespeed(const Params &, double *ws, const double *, const double *,
                                     const double *, double, int)
    {
        ws[0] = ws[1] = ws[2] = 0.0;
    }
};

}  // namespace cmdg
