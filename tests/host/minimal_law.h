// The smallest balance law the engine takes: advection of one scalar by a constant velocity, with
// the mandatory members of csrc/law_defaults.h and nothing else.  tests/test_abi_symbols.py builds
// it as an engine plug-in: every kernel an EngineT instantiates compiles on the defaults alone.
#pragma once
#include "law_defaults.h"

struct MinimalLawParams {
    double u[3];
};

struct MinimalLaw : cmdg::LawDefaults {
    using Params = MinimalLawParams;
    static constexpr int NS = 1, NAUX = 0, NGRAD = 0, NGF = 0;
    static void make_params(Params &p, const int32_t *, const double *dp)
    {
        for (int d = 0; d < 3; ++d) p.u[d] = dp[d];
    }
    __host__ __device__ static bool needs_gradflux(const Params &) { return false; }
    __device__ static void flux_first_order(const Params &m, double *F, const double *Q, const double *, double, int)
    {
        for (int d = 0; d < 3; ++d) F[d] += m.u[d] * Q[0];
    }
    __device__ static void wavespeed(const Params &m, double *ws, const double *n, const double *, const double *,
                                     double, int)
    {
        ws[0] = fabs(n[0] * m.u[0] + n[1] * m.u[1] + n[2] * m.u[2]);
    }
};
