// ManyColumnLU (src/Numerics/SystemSolvers/columnwise_lu_solver.jl): the banded column solver of
// the implicit steppers (steppers.hip, multirate.hip).
//
// The operator is I - alpha L of a vertical-direction DG model on a stacked grid (the dry linear
// law, nstate = 5, or the moist one, nstate = 6): a banded matrix per column, one column = one horizontal node (i, j) of one stack of elements, n = Nq_v nstate
// nvert unknowns ordered (state, vertical node, element) fastest first, bandwidths
// p = q = Nq_v nstate - 1 (eband = 1, an inviscid law: columnwise_lu_solver.jl:56-74, :339-349).
//
// Band layout: band[(col * P + d) * ncol + c], P = p + q + 1, d = row - col + q (the reference's
// A[i, j, d, col, h] with the column index c innermost).  Every kernel runs one matrix column c
// per lane, so the 64 lanes of a wave read 512 contiguous bytes per (matrix column, diagonal).
//
// Assembly by probing (update_banded_matrix!, :404-480): one unit per (state, vertical node,
// element mod 3) in every column, one evaluation of the vertical DG at t = NaN, the result
// scattered into the band as Q + (-alpha) dQ (EulerOperator, BackwardEulerSolvers.jl:21-40).
// Factorisation (band_lu_kernel!, :555-600) and substitution (band_forward_kernel! /
// band_back_kernel!, :615-780) keep the reference's operations and order, without pivoting;
// the substitutions keep the p + 1 wide window of the solution in registers.
#include <math.h>

#include <string>
#include <vector>

#include "band_solve.h"
#include "stepping.h"

namespace cmdg {
namespace {

// work-groups of nt lanes for the band kernels: one matrix column per lane
unsigned blocks(int64_t n, int nt) { return (unsigned)((n + nt - 1) / nt); }

__global__ void k_probe_set(double *Q, int64_t nreal, int Np, int NS, int nqh2, int nvert, int kin,
                            int sin_, int ev0)
{
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= nreal * NS * Np) return;
    const int n = (int)(i % Np);
    const int s = (int)((i / Np) % NS);
    const int64_t e = i / ((int64_t)Np * NS);
    const int v = (int)(e % nvert), k = n / nqh2;
    Q[i] = (k == kin && s == sin_ && (v - ev0) % 3 == 0 && v >= ev0) ? 1.0 : 0.0;
}

// every real node of dQ belongs to the band of the probed column in its own or an adjacent element
__global__ void k_probe_scatter(double *band, const double *Q, const double *dQ, int64_t nreal,
                                int Np, int NS, int nqh2, int nqv, int nvert, int kin, int sin_, int ev0,
                                int p, int q, int64_t ncol, double eps)
{
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= nreal * NS * Np) return;
    const int n = (int)(i % Np);
    const int s = (int)((i / Np) % NS);
    const int64_t e = i / ((int64_t)Np * NS);
    const int v = (int)(e % nvert), k = n / nqh2, ij = n % nqh2;
    const int64_t c = (e / nvert) * nqh2 + ij;
    int evin = -1;
    for (int dv = -1; dv <= 1; ++dv) {
        const int ev = v + dv;
        if (ev >= ev0 && ev < nvert && (ev - ev0) % 3 == 0) evin = ev;
    }
    if (evin < 0) return;
    const int64_t jj = sin_ + (int64_t)NS * kin + (int64_t)NS * nqv * evin;
    const int64_t ii = s + (int64_t)NS * k + (int64_t)NS * nqv * v;
    const int64_t bb = ii - jj;
    if (bb < -q || bb > p) return;
    const int P = p + q + 1;
    band[(jj * P + (bb + q)) * ncol + c] = Q[i] + eps * dQ[i];
}

// band_lu_kernel!: no pivoting, one matrix column per lane
__global__ void k_band_lu(double *A, int64_t ncol, int64_t n, int p, int q)
{
    const int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (c >= ncol) return;
    const int P = p + q + 1;
    auto at = [&](int64_t col, int d) -> double & { return A[(col * P + d) * ncol + c]; };
    for (int64_t kk = 0; kk < n; ++kk) {
        const double Aq = at(kk, q);
        for (int ii = 1; ii <= p; ++ii) at(kk, q + ii) /= Aq;
        for (int jj = 1; jj <= q; ++jj) {
            if (jj + kk < n) {
                const double Ajj = at(kk + jj, q - jj);
                for (int ii = 1; ii <= p; ++ii) at(kk + jj, q + ii - jj) -= at(kk, q + ii) * Ajj;
            }
        }
    }
}

}  // namespace
}  // namespace cmdg

using namespace cmdg;

struct cmdg_columnlu : cmdg::BackwardEuler {
    int dev = 0;  // the linear handle's device (destroy does not need the handle any more)
    int nvert = 0, nqh2 = 0, nqv = 0, ns = 0, p = 0, q = 0, P = 0;
    int64_t ncol = 0, n = 0;
    double alpha_lu = 0;
    int state = 0;  // 0 empty, 1 assembled (I - alpha L), 2 factored
    DevBuf<double> band, probe, dprobe;
    // stepping.h: enqueued on the linear handle's stream, errors also on its engine
    double alpha() const override { return state == 2 ? alpha_lu : NAN; }  // NaN while the band is not factored
    int ready(double a) override;
    int solve(double *X, const double *B, double t) override;
};

namespace {

// the (vertical order, state count) pairs k_band_solve is compiled for
bool compiled(int nqv, int ns) { return ns == 5 ? (nqv >= 4 && nqv <= 6) : ns == 6 && (nqv == 5 || nqv == 7); }
const char *const compiled_pairs =
    "vertical order / state count not compiled in (have N = 3, 4, 5 with five states, N = 4, 6 with six)";

int lu_fail(cmdg_columnlu *lu, int code, const std::string &msg)
{
    if (lu && lu->lin) lu->lin->err = "columnlu: " + msg;
    return code;
}

int hip_ok(cmdg_columnlu *lu, hipError_t r, const char *what)
{
    if (r == hipSuccess) return CMDG_OK;
    return lu_fail(lu, CMDG_ERR_HIP, std::string(what) + ": " + hipGetErrorString(r));
}

int assemble(cmdg_columnlu *lu, double alpha)
{
    EngineBase *e = lu->lin->eng;
    hipStream_t st = e->s_comp;
    const int NS = lu->ns;
    const int64_t len = e->nreal * NS * e->Np;
    const size_t bytes = (size_t)lu->n * lu->P * lu->ncol * sizeof(double);
    if (int r = hip_ok(lu, hipMemsetAsync(lu->band, 0, bytes, st), "hipMemsetAsync")) return r;
    const int nev = lu->nvert < 3 ? lu->nvert : 3;
    for (int ev0 = 0; ev0 < nev; ++ev0)
        for (int s = 0; s < NS; ++s)
            for (int k = 0; k < lu->nqv; ++k) {
                hipLaunchKernelGGL(k_probe_set, dim3(grid_one_per_thread(len)), dim3(256), 0, st, lu->probe, e->nreal,
                                   e->Np, NS, lu->nqh2, lu->nvert, k, s, ev0);
                if (int r = cmdg_rhs_async(lu->lin, lu->dprobe, lu->probe, NAN, 1.0, 0.0)) return r;
                hipLaunchKernelGGL(k_probe_scatter, dim3(grid_one_per_thread(len)), dim3(256), 0, st, lu->band,
                                   lu->probe, lu->dprobe, e->nreal, e->Np, NS, lu->nqh2, lu->nqv, lu->nvert,
                                   k, s, ev0, lu->p, lu->q, lu->ncol, -alpha);
            }
    lu->alpha_lu = alpha;
    lu->state = 1;
    return hip_ok(lu, hipGetLastError(), "assembly kernels");
}

int factor(cmdg_columnlu *lu)
{
    hipLaunchKernelGGL(k_band_lu, dim3(blocks(lu->ncol, 64)), dim3(64), 0, lu->lin->eng->s_comp, lu->band,
                       lu->ncol, lu->n, lu->p, lu->q);
    lu->state = 2;
    return hip_ok(lu, hipGetLastError(), "band_lu");
}

int update(cmdg_columnlu *lu, double alpha)
{
    if (int r = assemble(lu, alpha)) return r;
    return factor(lu);
}

// solve on the linear handle's stream
int solve(cmdg_columnlu *lu, double *X, const double *B)
{
    if (lu->state != 2) return lu_fail(lu, CMDG_ERR_INVALID, "the band is not factored");
    hipStream_t st = lu->lin->eng->s_comp;
    const dim3 g(blocks(lu->ncol, 64)), b(64);
    if (lu->ns == 5 && lu->nqv == 4)  // (the order of the ESDG linear law alone: engine_esdg_linear.hip)
        band_solve_nqv4_ns5(g, b, st, X, B, lu->band, lu->ncol, lu->nvert, lu->nqh2);
    else if (lu->ns == 5 && lu->nqv == 5)
        hipLaunchKernelGGL((k_band_solve<5, 5>), g, b, 0, st, X, B, lu->band, lu->ncol, lu->nvert, lu->nqh2);
    else if (lu->ns == 5 && lu->nqv == 6)
        hipLaunchKernelGGL((k_band_solve<6, 5>), g, b, 0, st, X, B, lu->band, lu->ncol, lu->nvert, lu->nqh2);
    else if (lu->ns == 6 && lu->nqv == 5)
        hipLaunchKernelGGL((k_band_solve<5, 6>), g, b, 0, st, X, B, lu->band, lu->ncol, lu->nvert, lu->nqh2);
    else if (lu->ns == 6 && lu->nqv == 7)
        hipLaunchKernelGGL((k_band_solve<7, 6>), g, b, 0, st, X, B, lu->band, lu->ncol, lu->nvert, lu->nqh2);
    else
        return lu_fail(lu, CMDG_ERR_UNSUPPORTED, compiled_pairs);
    return hip_ok(lu, hipGetLastError(), "band solve");
}

}  // namespace

int cmdg_columnlu::ready(double a)
{
    const int r = update(this, a);
    if (r) lin->eng->err = lin->err;
    return r;
}
int cmdg_columnlu::solve(double *X, const double *B, double)
{
    const int r = ::solve(this, X, B);
    if (r) lin->eng->err = lin->err;
    return r;
}

namespace cmdg {
BackwardEuler *columnlu_solver(cmdg_columnlu_handle lu) { return lu; }
}  // namespace cmdg

extern "C" {

int cmdg_columnlu_create(cmdg_handle linear, int32_t nvertelem, double alpha, cmdg_columnlu_handle *out)
{
    if (!linear || !out || nvertelem < 1) return CMDG_ERR_INVALID;
    *out = nullptr;
    EngineBase *e = linear->eng;
    DevGuard guard_(e);
    cmdg_columnlu tmp;
    tmp.lin = linear;
    if (e->fv)
        return lu_fail(&tmp, CMDG_ERR_UNSUPPORTED, "column LU is not available on a DGFVModel handle (finite-volume vertical)");
    if (e->esdg)
        return lu_fail(&tmp, CMDG_ERR_UNSUPPORTED, "column LU is not available on an ESDGModel handle");
    if (e->direction != DIR_VERTICAL || !e->stacked)
        return lu_fail(&tmp, CMDG_ERR_INVALID, "the operator must be a VerticalDirection DG model on a stacked grid");
    if ((e->ns != 5 && e->ns != 6) || e->ngf != 0)
        return lu_fail(&tmp, CMDG_ERR_UNSUPPORTED,
                       "five or six prognostic states and no second-order terms (eband = 1) only");
    if (!compiled(e->NQV, e->ns)) return lu_fail(&tmp, CMDG_ERR_UNSUPPORTED, compiled_pairs);
    if (e->nreal % nvertelem != 0)
        return lu_fail(&tmp, CMDG_ERR_INVALID, "the real elements are not whole stacks");
    {
        // a vertically periodic stack couples its top and bottom elements, which the band cannot
        // hold: every stack's bottom (face 5) and top (face 6) must be boundary faces
        std::vector<int64_t> etb((size_t)6 * e->nreal);
        if (int r = hip_ok(&tmp, hipMemcpy(etb.data(), e->g.elemtobndy, etb.size() * sizeof(int64_t),
                                           hipMemcpyDefault),
                           "hipMemcpy(elemtobndy)"))
            return r;
        for (int64_t h = 0; h < e->nreal / nvertelem; ++h)
            if (etb[4 + 6 * (h * nvertelem)] == 0 || etb[5 + 6 * (h * nvertelem + nvertelem - 1)] == 0)
                return lu_fail(&tmp, CMDG_ERR_UNSUPPORTED,
                               "vertically periodic stacks are not supported (stack " + std::to_string(h) +
                                   " has no boundary face at its bottom or top; the band cannot hold the "
                                   "coupling of its top and bottom elements)");
    }
    auto *lu = new cmdg_columnlu;
    lu->lin = linear;
    lu->dev = e->dev;
    lu->nvert = nvertelem;
    lu->nqh2 = e->NQ * e->NQ;
    lu->nqv = e->NQV;
    lu->ns = e->ns;
    const int NS = lu->ns;
    lu->p = lu->q = lu->nqv * NS - 1;  // lower_bandwidth(N, nstate, eband = 1)
    lu->P = lu->p + lu->q + 1;
    lu->ncol = (e->nreal / nvertelem) * lu->nqh2;
    lu->n = (int64_t)lu->nqv * NS * nvertelem;
    const size_t band = (size_t)lu->n * lu->P * lu->ncol * sizeof(double);
    const size_t states = 2 * (size_t)e->nelem * NS * e->Np * sizeof(double);
    size_t freeb = 0, total = 0;
    int r = hip_ok(lu, hipMemGetInfo(&freeb, &total), "hipMemGetInfo");
    if (!r && band + states + (64u << 20) > freeb) {
        char msg[256];
        snprintf(msg, sizeof msg,
                 "the band needs %.3f GB (%lld columns x %lld rows (%d states) x %d diagonals x 8 B) plus "
                 "%.3f GB of probe states; %.3f GB of device memory are free",
                 band / 1e9, (long long)lu->ncol, (long long)lu->n, NS, lu->P, states / 1e9, freeb / 1e9);
        r = lu_fail(lu, CMDG_ERR_INVALID, msg);
    }
    if (!r) r = hip_ok(lu, lu->band.alloc(band / sizeof(double)), "hipMalloc(band)");
    if (!r) r = hip_ok(lu, lu->probe.alloc(states / 2 / sizeof(double)), "hipMalloc(probe)");
    if (!r) r = hip_ok(lu, lu->dprobe.alloc(states / 2 / sizeof(double)), "hipMalloc(probe)");
    if (!r) r = hip_ok(lu, hipMemset(lu->probe, 0, states / 2), "hipMemset");
    if (!r) r = hip_ok(lu, hipMemset(lu->dprobe, 0, states / 2), "hipMemset");
    if (!r) r = update(lu, alpha);
    if (!r) r = hip_ok(lu, hipStreamSynchronize(e->s_comp), "hipStreamSynchronize");
    if (r) {
        cmdg_columnlu_destroy(lu);
        return r;
    }
    *out = lu;
    return CMDG_OK;
}

int cmdg_columnlu_assemble(cmdg_columnlu_handle lu, double alpha)
{
    if (!lu) return CMDG_ERR_INVALID;
    DevGuard guard_(lu->lin->eng);
    if (int r = assemble(lu, alpha)) return r;
    return hip_ok(lu, hipStreamSynchronize(lu->lin->eng->s_comp), "hipStreamSynchronize");
}

int cmdg_columnlu_update(cmdg_columnlu_handle lu, double alpha)
{
    if (!lu) return CMDG_ERR_INVALID;
    DevGuard guard_(lu->lin->eng);
    if (int r = update(lu, alpha)) return r;
    return hip_ok(lu, hipStreamSynchronize(lu->lin->eng->s_comp), "hipStreamSynchronize");
}

int cmdg_columnlu_solve(cmdg_columnlu_handle lu, double *Q, const double *Qrhs)
{
    if (!lu || !Q || !Qrhs) return CMDG_ERR_INVALID;
    DevGuard guard_(lu->lin->eng);
    if (int r = solve(lu, Q, Qrhs)) return r;
    return hip_ok(lu, hipStreamSynchronize(lu->lin->eng->s_comp), "hipStreamSynchronize");
}

int cmdg_columnlu_info(cmdg_columnlu_handle lu, int64_t out[8])
{
    if (!lu || !out) return CMDG_ERR_INVALID;
    out[0] = lu->n;
    out[1] = lu->p;
    out[2] = lu->q;
    out[3] = lu->ncol;
    out[4] = lu->n * lu->P * lu->ncol * (int64_t)sizeof(double);
    out[5] = lu->state;
    out[6] = lu->nvert;
    out[7] = lu->nqv;
    return CMDG_OK;
}

int cmdg_columnlu_alpha(cmdg_columnlu_handle lu, double *alpha)
{
    if (!lu || !alpha) return CMDG_ERR_INVALID;
    *alpha = lu->alpha_lu;
    return CMDG_OK;
}

int cmdg_columnlu_export_band(cmdg_columnlu_handle lu, int64_t column, double *out)
{
    if (!lu || !out || column < 0 || column >= lu->ncol) return CMDG_ERR_INVALID;
    DevGuard guard_(lu->lin->eng);
    if (int r = hip_ok(lu, hipStreamSynchronize(lu->lin->eng->s_comp), "hipStreamSynchronize")) return r;
    // element (d, col) of the reference's A[:, :] at out[col * P + d]
    return hip_ok(lu, hipMemcpy2D(out, sizeof(double), lu->band + column, lu->ncol * sizeof(double),
                                  sizeof(double), (size_t)lu->n * lu->P, hipMemcpyDeviceToHost),
                  "hipMemcpy2D");
}

int cmdg_columnlu_destroy(cmdg_columnlu_handle lu)
{
    if (!lu) return CMDG_ERR_INVALID;
    {
        // the linear handle may already be destroyed: bind the device by hand, wait for it
        int prev = -1;
        (void)hipGetDevice(&prev);
        (void)hipSetDevice(lu->dev);
        (void)hipDeviceSynchronize();
        delete lu;  // (frees the band and the probe states on their device)
        if (prev >= 0) (void)hipSetDevice(prev);
    }
    return CMDG_OK;
}

}  // extern "C"
