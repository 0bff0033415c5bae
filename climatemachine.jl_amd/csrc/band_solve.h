// The substitution kernel of the column solver (columnlu.hip), in a header so that a law's engine
// unit can carry the instantiation of an order only that law is compiled for.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace cmdg {

// band_forward_kernel! then band_back_kernel! on one matrix column per lane.  W = p + 1 = q + 1 =
// NQV * NS: the row loaded ahead (behind) is the same (node, state) of the next (previous)
// element.  The window shifts by one register per row, so its indices are static; it stays in
// registers for every compiled (NQV, NS) (scratch 0).
template <int NQV, int NS>
__global__ void __launch_bounds__(64) k_band_solve(double *X, const double *B, const double *A, int64_t ncol,
                                                   int nvert, int nqh2)
{
    constexpr int W = NQV * NS, p = W - 1, q = W - 1, P = p + q + 1;
    const int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (c >= ncol) return;
    const int Np = nqh2 * NQV;
    const int64_t h = c / nqh2;
    const int ij = (int)(c % nqh2);
    const int64_t n = (int64_t)W * nvert;
    // node (k, s) of vertical element v of this column in the (Np, nstate, nelem) layout
    auto idx = [&](int v, int r) -> int64_t {
        const int k = r / NS, s = r % NS;
        return ((h * nvert + v) * NS + s) * (int64_t)Np + ij + (int64_t)nqh2 * k;
    };
    auto L = [&](int64_t col, int d) -> double { return A[(col * P + d) * ncol + c]; };
    double lb[W];
#pragma unroll
    for (int r = 0; r < W; ++r) lb[r] = B[idx(0, r)];
    for (int v = 0; v < nvert; ++v) {
        // one row per iteration: unrolling the rows of an element hoisted every row's p band
        // loads at once and spilled the window to scratch
#pragma unroll 1
        for (int r = 0; r < W; ++r) {
            const int64_t jj = (int64_t)v * W + r;
#pragma unroll
            for (int ii = 1; ii <= p; ++ii) lb[ii] -= L(jj, ii + q) * lb[0];
            X[idx(v, r)] = lb[0];
#pragma unroll
            for (int ii = 0; ii < p; ++ii) lb[ii] = lb[ii + 1];
            lb[p] = 0.0;
            if (jj + p + 1 < n) lb[p] = B[idx(v + 1, r)];
        }
    }
#pragma unroll
    for (int r = 0; r < W; ++r) lb[r] = X[idx(nvert - 1, r)];
    for (int v = nvert - 1; v >= 0; --v) {
#pragma unroll 1
        for (int r = W - 1; r >= 0; --r) {
            const int64_t jj = (int64_t)v * W + r;
            lb[q] /= L(jj, q);
#pragma unroll
            for (int ii = 0; ii < q; ++ii) lb[ii] -= L(jj, ii) * lb[q];
            X[idx(v, r)] = lb[q];
#pragma unroll
            for (int ii = q - 1; ii >= 0; --ii) lb[ii + 1] = lb[ii];
            lb[0] = 0.0;
            if (jj - q > 0) lb[0] = X[idx(v - 1, r)];
        }
    }
}

// k_band_solve<4, 5>: N = 3 with five states, the order DryAtmosAcousticGravityLinearModel adds; defined
// next to that law (engine_esdg_linear.hip)
void band_solve_nqv4_ns5(dim3 grid, dim3 block, hipStream_t st, double *X, const double *B, const double *A,
                         int64_t ncol, int nvert, int nqh2);

}  // namespace cmdg
