// Restarted GMRES for (I - alpha L) Q = Qrhs over the real elements of one handle:
// GeneralizedMinimalResidual (src/Numerics/SystemSolvers/generalized_minimal_residual_solver.jl:24-161)
// driven by linearsolve! (SystemSolvers.jl:240-286) on EulerOperator(L, -alpha)
// (BackwardEulerSolvers.jl:125-196).  Dots and norms are plain fp64 sums over the real elements
// (weighted_norm = false, SystemSolvers.jl:21), single rank.
//
// One inner iteration j (0-based; the Krylov vectors v_0 .. v_M are the solver's own arrays):
//   the operator     w = v_{j+1} holds a copy of v_j (left by k_gmres_scale); one evaluation of L
//                    with (alpha, beta) = (-alpha, 1) makes it v_j - alpha L v_j
//   k_gmres_mgs      launch l = 0 .. j+1, modified Gram-Schmidt in sequence: the prologue of launch l
//                    sums the block partials launch l - 1 left (every block the same partials in
//                    the same order) into H[l-1, j]; the pass does w -= H[l-1, j] v_{l-1} and leaves
//                    the block partials of dot(w, v_l), the last launch those of |w|^2
//   k_gmres_small    one wave: H[j+1, j] = |w|, the stored rotations on the new column, the new
//                    rotation, g0; |g0[j+1]| goes to pinned host memory (the one host wait of the
//                    iteration reads it); on the last iteration of a cycle y = R \ g0
//   k_gmres_scale    v_{j+1} = w / H[j+1, j], and the copy the next evaluation starts from
// After a cycle k_gmres_lincomb does Q += sum_i y_i v_i (linearcombination!, increment = true);
// k_gmres_residual forms r = Qrhs - A Q of initialize! with the partials of |r|^2 in the same pass.
// No atomics and no in-launch protocol between blocks: partial sums are combined across a launch
// boundary in a fixed order, so a repeated solve repeats its bits.
#include <math.h>

#include <algorithm>
#include <string>
#include <vector>

#include "stepping.h"

using namespace cmdg;

namespace {

constexpr int MAXM = CMDG_GMRES_MAX_M;
constexpr unsigned MAXBLK = 1024;  // block partials of one pass (four work-groups per compute unit)
enum { SMALL_INIT = 1, SMALL_ITER = 2, SMALL_BACKSUB = 4 };

// the solver's small matrices, in device memory
struct GmresDev {
    double *H;     // (M + 1, M) column-major
    double *cs, *sn;  // the rotations
    double *g0;    // M + 1
    double *y;     // M
    double *scal;  // the divisor k_gmres_scale applies
    int M;
};

__device__ inline double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// sum over a work-group of 256, the same value in every thread
__device__ inline double block_sum(double v, double *lds)
{
    v = wave_sum(v);
    __syncthreads();  // (lds may still be read from the previous sum)
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((lds[0] + lds[1]) + lds[2]) + lds[3];
}

// the partials of the previous launch, summed by every block in the same order
__device__ inline double combine(const double *__restrict__ part, int n, double *lds)
{
    double a = 0.0;
    for (int k = threadIdx.x; k < n; k += 256) a += part[k];
    return block_sum(a, lds);
}

// w -= h v_prev (h = the combined partials of the previous launch, also stored to *hslot), then the
// block partial of dot(w, v_dot), or of |w|^2 (NORM).  vprev == NULL: the first launch of a column.
template <bool NORM>
__global__ void __launch_bounds__(256) k_gmres_mgs(double *__restrict__ w, const double *__restrict__ vprev,
                                                  const double *__restrict__ vdot,
                                                  const double *__restrict__ part_in, int nin,
                                                  double *__restrict__ part_out, double *__restrict__ hslot,
                                                  int64_t n)
{
    __shared__ double lds[4];
    double h = 0.0;
    if (vprev) {
        h = combine(part_in, nin, lds);
        if (blockIdx.x == 0 && threadIdx.x == 0) *hslot = h;
    }
    double acc = 0.0;
    for (int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        double x = w[i];
        if (vprev) {
            x -= h * vprev[i];
            w[i] = x;
        }
        acc += NORM ? x * x : x * vdot[i];
    }
    acc = block_sum(acc, lds);
    if (threadIdx.x == 0) part_out[blockIdx.x] = acc;
}

// r = Qrhs - r (r holds A Q on entry) with the block partials of |r|^2
__global__ void __launch_bounds__(256) k_gmres_residual(double *__restrict__ r, const double *__restrict__ Qrhs,
                                                       double *__restrict__ part_out, int64_t n)
{
    __shared__ double lds[4];
    double acc = 0.0;
    for (int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double x = Qrhs[i] - r[i];
        r[i] = x;
        acc += x * x;
    }
    acc = block_sum(acc, lds);
    if (threadIdx.x == 0) part_out[blockIdx.x] = acc;
}

// v ./= scal; next (when given) takes a copy: the array the next operator evaluation increments
__global__ void __launch_bounds__(256) k_gmres_scale(double *__restrict__ v, double *__restrict__ next,
                                                    const double *__restrict__ scal, int64_t n)
{
    const double s = scal[0];
    for (int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double x = v[i] / s;
        v[i] = x;
        if (next) next[i] = x;
    }
}

// Q += sum_{i < nj} y_i v_i, the terms added in order (linearcombination!, SystemSolvers.jl:288-297)
__global__ void __launch_bounds__(256) k_gmres_lincomb(double *__restrict__ Q, const double *__restrict__ basis,
                                                      int64_t stride, const double *__restrict__ y, int nj,
                                                      int64_t n)
{
    __shared__ double ys[MAXM];
    if (threadIdx.x < nj) ys[threadIdx.x] = y[threadIdx.x];
    __syncthreads();
    for (int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        double q = Q[i];
#pragma unroll 4
        for (int k = 0; k < nj; ++k) q += ys[k] * basis[k * stride + i];
        Q[i] = q;
    }
}

// givens(f, g, ...) of LinearAlgebra (givensAlgorithm) for magnitudes that need no rescaling
__device__ inline void givens(double f, double g, double &c, double &s)
{
    if (g == 0) {
        c = 1;
        s = 0;
    } else if (f == 0) {
        c = 0;
        s = 1;
    } else {
        const double r = sqrt(f * f + g * g);
        c = f / r;
        s = g / r;
        if (fabs(f) > fabs(g) && c < 0) {
            c = -c;
            s = -s;
        }
    }
}

// One wave.  SMALL_INIT: the residual norm of initialize! to host_out, g0 = (norm, 0, ...) and the
// divisor of v_0, unless rtol norm < atol (initialize! then returns before it touches either).
// SMALL_ITER: column j.  SMALL_BACKSUB: y = UpperTriangular(H[0:nj, 0:nj]) \ g0[0:nj], nj = j + 1.
__global__ void __launch_bounds__(64) k_gmres_small(const GmresDev d, int mode, int j,
                                                   const double *__restrict__ part, int nin, double rtol,
                                                   double atol, double *__restrict__ host_out)
{
    double a = 0.0;
    if (mode & (SMALL_INIT | SMALL_ITER)) {
        for (int k = threadIdx.x; k < nin; k += 64) a += part[k];
        a = wave_sum(a);
    }
    if (threadIdx.x != 0) return;
    const int ld = d.M + 1;
    if (mode & SMALL_INIT) {
        const double nrm = sqrt(a);
        host_out[0] = nrm;
        if (rtol * nrm < atol) {
            d.scal[0] = 1.0;
        } else {
            for (int i = 0; i <= d.M; ++i) d.g0[i] = 0.0;
            d.g0[0] = nrm;
            d.scal[0] = nrm;
        }
    }
    if (mode & SMALL_ITER) {
        double *Hc = d.H + (int64_t)ld * j;
        const double hn = sqrt(a);
        d.scal[0] = hn;
        for (int k = 0; k < j; ++k) {  // H[1:j, j] = Omega H[1:j, j]
            const double a1 = Hc[k], a2 = Hc[k + 1];
            Hc[k] = d.cs[k] * a1 + d.sn[k] * a2;
            Hc[k + 1] = -d.sn[k] * a1 + d.cs[k] * a2;
        }
        double c, s;
        const double f = Hc[j];
        givens(f, hn, c, s);
        d.cs[j] = c;
        d.sn[j] = s;
        Hc[j] = c * f + s * hn;
        Hc[j + 1] = -s * f + c * hn;
        const double g1 = d.g0[j], g2 = d.g0[j + 1];
        d.g0[j] = c * g1 + s * g2;
        d.g0[j + 1] = -s * g1 + c * g2;
        host_out[0] = fabs(d.g0[j + 1]);
    }
    if (mode & SMALL_BACKSUB) {
        const int nj = j + 1;
        for (int i = 0; i < nj; ++i) d.y[i] = d.g0[i];
        for (int col = nj - 1; col >= 0; --col) {
            const double x = d.y[col] / d.H[col + (int64_t)ld * col];
            d.y[col] = x;
            for (int i = col - 1; i >= 0; --i) d.y[i] -= d.H[i + (int64_t)ld * col] * x;
        }
    }
}

}  // namespace

struct cmdg_gmres : cmdg::BackwardEuler {
    int dev = 0;
    int M = 0;
    double rtol = 0, atol = 0;
    double alpha_ = NAN;  // the alpha the backward-Euler solver was last made ready for
    int64_t stride = 0;   // doubles between Krylov vectors
    DevBuf<double> basis, small, part;
    GmresDev d{};
    double *host = nullptr;  // pinned: the norm a small kernel leaves for the host
    std::vector<cmdg_gmres_info> log;  // the solves since the last step entry began

    cmdg_gmres() { iterative = true; }
    ~cmdg_gmres() override
    {
        if (host) (void)hipHostFree(host);
    }
    double alpha() const override { return alpha_; }
    int ready(double a) override  // prefactorize(::AbstractIterativeSystemSolver) = nothing
    {
        alpha_ = a;
        return CMDG_OK;
    }
    int solve(double *X, const double *B, double t) override
    {
        cmdg_gmres_info info;
        const int r = run(alpha_, X, B, t, real_len(lin->eng), &info);
        if (!r) log.push_back(info);
        return r;
    }
    int fail(int code, const std::string &msg)
    {
        lin->err = "gmres: " + msg;
        return lin->eng->fail(code, lin->err);
    }
    int hip_ok(hipError_t r, const char *what)
    {
        if (r == hipSuccess) return CMDG_OK;
        return fail(CMDG_ERR_HIP, std::string(what) + ": " + hipGetErrorString(r));
    }
    int run(double alpha, double *X, const double *B, double t, int64_t max_iters, cmdg_gmres_info *info);
};

namespace {

int64_t basis_bytes(const EngineBase *e, int M)
{
    return (int64_t)(M + 1) * e->nelem * e->ns * e->Np * (int64_t)sizeof(double);
}

// would the Krylov basis of M + 1 state arrays fit next to 64 MB of headroom?
int check_fits(cmdg_handle lin, int M, int64_t free_bytes, std::string &msg)
{
    const EngineBase *e = lin->eng;
    const int64_t need = basis_bytes(e, M);
    if (need + (64ll << 20) <= free_bytes) return CMDG_OK;
    char buf[256];
    snprintf(buf, sizeof buf,
             "the Krylov basis needs %.3f GB (M + 1 = %d state arrays of %lld elements x %d states x %d "
             "nodes x 8 B); %.3f GB of device memory are free",
             need / 1e9, M + 1, (long long)e->nelem, e->ns, e->Np, free_bytes / 1e9);
    msg = buf;
    return CMDG_ERR_INVALID;
}

int check_args(cmdg_handle lin, int M, double rtol, double atol, std::string &msg)
{
    if (M < 1 || M > MAXM) {
        msg = "the restart length M must be 1 to " + std::to_string(MAXM) + ", not " + std::to_string(M);
        return CMDG_ERR_INVALID;
    }
    if (!(rtol >= 0) || !(atol >= 0)) {
        char buf[128];
        snprintf(buf, sizeof buf, "rtol and atol must be >= 0 (rtol = %g, atol = %g)", rtol, atol);
        msg = buf;
        return CMDG_ERR_INVALID;
    }
    if (lin->eng->communicate()) {
        msg = "a handle with halo neighbours is not supported: a multi-rank solve needs an all-reduce per "
              "dot product and one convergence decision for every rank (a follow-up)";
        return CMDG_ERR_UNSUPPORTED;
    }
    return CMDG_OK;
}

int refuse(cmdg_handle lin, int code, const std::string &msg)
{
    lin->err = "gmres: " + msg;
    return code;
}

}  // namespace

int cmdg_gmres::run(double alpha, double *X, const double *B, double t, int64_t max_iters, cmdg_gmres_info *info)
{
    EngineBase *e = lin->eng;
    hipStream_t st = e->s_comp;
    const int64_t n = real_len(e);
    const unsigned nb = std::min(nblocks(n), MAXBLK);
    const dim3 g(nb), b(256);
    auto V = [&](int i) { return basis + (int64_t)i * stride; };
    double *part2[2] = {part, part + MAXBLK};
    *info = cmdg_gmres_info{};
    if (!(alpha == alpha)) return fail(CMDG_ERR_INVALID, "alpha is NaN (the solver was not made ready for an alpha)");
    // out = in - alpha L(in); `out` holds a copy of `in` already
    auto apply = [&](double *out, double *in) {
        RhsCtx c;
        c.tendency = out;
        c.Qin = in;
        c.t = t;
        c.alpha = -alpha;
        c.beta = 1.0;
        return e->rhs_async(c);
    };
    auto wait_norm = [&](double &v) {
        if (int r = hip_ok(hipGetLastError(), "kernel launch")) return r;
        if (int r = hip_ok(hipStreamSynchronize(st), "hipStreamSynchronize")) return r;
        v = *(volatile double *)host;
        return (int)CMDG_OK;
    };
    // initialize!: v_0 = Qrhs - A Q, its norm to the host
    auto initialize = [&](double &nrm) {
        if (int r = hip_ok(hipMemcpyAsync(V(0), X, sizeof(double) * n, hipMemcpyDeviceToDevice, st), "hipMemcpyAsync"))
            return r;
        if (int r = apply(V(0), X)) return r;
        hipLaunchKernelGGL(k_gmres_residual, g, b, 0, st, V(0), B, part2[0], n);
        hipLaunchKernelGGL(k_gmres_small, dim3(1), dim3(64), 0, st, d, (int)SMALL_INIT, 0, (const double *)part2[0],
                           (int)nb, rtol, atol, host);
        return wait_norm(nrm);
    };
    auto not_finite = [&](int64_t iters) {
        return fail(CMDG_ERR_INVALID, "norm of residual is not finite after " + std::to_string(iters) +
                                          " iterations of `doiteration!`");
    };
    double nrm = 0;
    if (int r = initialize(nrm)) return r;
    info->residual_norm = nrm;
    double threshold = rtol * nrm;
    info->threshold = threshold;
    if (!std::isfinite(nrm)) return not_finite(0);
    if (threshold < atol) {  // converged before the first iteration: Q is not touched
        info->converged = 1;
        return CMDG_OK;
    }
    threshold = std::max(threshold, atol);
    info->threshold = threshold;
    hipLaunchKernelGGL(k_gmres_scale, g, b, 0, st, V(0), V(1), (const double *)d.scal, n);
    int64_t iters = 0;
    bool converged = false;
    double res = nrm;
    while (!converged && iters < max_iters) {
        const int jmax = (int)std::min<int64_t>(M, max_iters - iters);
        int j = 0;
        for (;;) {
            double *w = V(j + 1);
            if (int r = apply(w, V(j))) return r;
            for (int l = 0; l <= j; ++l)
                hipLaunchKernelGGL(k_gmres_mgs<false>, g, b, 0, st, w, (const double *)(l ? V(l - 1) : nullptr),
                                   (const double *)V(l), (const double *)part2[(l + 1) & 1], (int)nb, part2[l & 1],
                                   d.H + (int64_t)(M + 1) * j + (l ? l - 1 : 0), n);
            hipLaunchKernelGGL(k_gmres_mgs<true>, g, b, 0, st, w, (const double *)V(j), (const double *)nullptr,
                               (const double *)part2[j & 1], (int)nb, part2[(j + 1) & 1],
                               d.H + (int64_t)(M + 1) * j + j, n);
            const bool last = j + 1 == jmax;
            hipLaunchKernelGGL(k_gmres_small, dim3(1), dim3(64), 0, st, d, SMALL_ITER | (last ? SMALL_BACKSUB : 0), j,
                               (const double *)part2[(j + 1) & 1], (int)nb, rtol, atol, host);
            if (int r = wait_norm(res)) return r;  // the iteration's one host wait
            if (!std::isfinite(res)) return not_finite(iters + j + 1);
            if (res < threshold) {
                converged = true;
                if (!last)
                    hipLaunchKernelGGL(k_gmres_small, dim3(1), dim3(64), 0, st, d, (int)SMALL_BACKSUB, j,
                                       (const double *)nullptr, 0, rtol, atol, host);
                break;
            }
            if (last) break;
            hipLaunchKernelGGL(k_gmres_scale, g, b, 0, st, w, V(j + 2), (const double *)d.scal, n);
            ++j;
        }
        const int nj = j + 1;
        iters += nj;
        hipLaunchKernelGGL(k_gmres_lincomb, g, b, 0, st, X, (const double *)basis, stride, (const double *)d.y, nj, n);
        if (!converged && iters < max_iters) {  // restart from the new residual; the threshold stays
            if (int r = initialize(nrm)) return r;
            if (!std::isfinite(nrm)) return not_finite(iters);
            hipLaunchKernelGGL(k_gmres_scale, g, b, 0, st, V(0), V(1), (const double *)d.scal, n);
        }
    }
    info->iterations = iters;
    info->converged = converged ? 1 : 0;
    info->residual_norm = res;
    return hip_ok(hipGetLastError(), "kernel launch");
}

namespace cmdg {
BackwardEuler *gmres_solver(cmdg_gmres_handle g)
{
    g->log.clear();
    return g;
}
}  // namespace cmdg

extern "C" {

int cmdg_gmres_fits(cmdg_handle linear, int32_t M, int64_t free_bytes, int64_t *basis_bytes_out)
{
    if (!linear) return CMDG_ERR_INVALID;
    if (M < 1 || M > MAXM)
        return refuse(linear, CMDG_ERR_INVALID, "the restart length M must be 1 to " + std::to_string(MAXM) +
                                                    ", not " + std::to_string(M));
    if (basis_bytes_out) *basis_bytes_out = basis_bytes(linear->eng, M);
    std::string msg;
    if (int r = check_fits(linear, M, free_bytes, msg)) return refuse(linear, r, msg);
    return CMDG_OK;
}

int cmdg_gmres_create(cmdg_handle linear, int32_t M, double rtol, double atol, cmdg_gmres_handle *out)
{
    if (!linear || !out) return CMDG_ERR_INVALID;
    *out = nullptr;
    EngineBase *e = linear->eng;
    DevGuard guard_(e);
    std::string msg;
    if (int r = check_args(linear, M, rtol, atol, msg)) return refuse(linear, r, msg);
    size_t freeb = 0, total = 0;
    if (hipMemGetInfo(&freeb, &total) != hipSuccess) return refuse(linear, CMDG_ERR_HIP, "hipMemGetInfo failed");
    if (int r = check_fits(linear, M, (int64_t)freeb, msg)) return refuse(linear, r, msg);
    auto *g = new cmdg_gmres;
    g->lin = linear;
    g->dev = e->dev;
    g->M = M;
    g->rtol = rtol;
    g->atol = atol;
    g->stride = e->nelem * (int64_t)e->ns * e->Np;
    // H, cs, sn, g0, y, scal
    const size_t nsmall = (size_t)(M + 1) * M + 2 * (size_t)M + (M + 1) + M + 1;
    int r = g->hip_ok(g->basis.alloc_zeroed((size_t)(M + 1) * g->stride, e->s_comp), "hipMalloc(Krylov basis)");
    if (!r) r = g->hip_ok(g->small.alloc_zeroed(nsmall, e->s_comp), "hipMalloc");
    if (!r) r = g->hip_ok(g->part.alloc_zeroed(2 * MAXBLK, e->s_comp), "hipMalloc");
    if (!r) r = g->hip_ok(hipHostMalloc((void **)&g->host, sizeof(double), hipHostMallocDefault), "hipHostMalloc");
    if (!r) r = g->hip_ok(hipStreamSynchronize(e->s_comp), "hipStreamSynchronize");
    if (r) {
        delete g;
        return r;
    }
    double *p = g->small;
    g->d.M = M;
    g->d.H = p;
    p += (size_t)(M + 1) * M;
    g->d.cs = p;
    p += M;
    g->d.sn = p;
    p += M;
    g->d.g0 = p;
    p += M + 1;
    g->d.y = p;
    p += M;
    g->d.scal = p;
    *out = g;
    return CMDG_OK;
}

int cmdg_gmres_prepare(cmdg_gmres_handle g, double alpha)
{
    if (!g) return CMDG_ERR_INVALID;
    return g->ready(alpha);
}

int cmdg_gmres_solve(cmdg_gmres_handle g, double alpha, double *Q, const double *Qrhs, double t, int64_t max_iters,
                     cmdg_gmres_info *info)
{
    if (!g || !Q || !Qrhs || !info) return CMDG_ERR_INVALID;
    DevGuard guard_(g->lin->eng);
    g->lin->eng->err.clear();
    if (max_iters < 0) max_iters = real_len(g->lin->eng);  // linearsolve!'s default: length(Q)
    return set_err(g->lin, g->run(alpha, Q, Qrhs, t, max_iters, info));
}

int cmdg_gmres_step_info(cmdg_gmres_handle g, int32_t capacity, cmdg_gmres_info *out, int32_t *nsolves)
{
    if (!g || !nsolves || capacity < 0 || (capacity > 0 && !out)) return CMDG_ERR_INVALID;
    *nsolves = (int32_t)g->log.size();
    for (int32_t i = 0; i < capacity && i < *nsolves; ++i) out[i] = g->log[i];
    return CMDG_OK;
}

int cmdg_gmres_destroy(cmdg_gmres_handle g)
{
    if (!g) return CMDG_ERR_INVALID;
    // the linear handle may already be destroyed: bind the device by hand, wait for it
    int prev = -1;
    (void)hipGetDevice(&prev);
    (void)hipSetDevice(g->dev);
    (void)hipDeviceSynchronize();
    delete g;
    if (prev >= 0) (void)hipSetDevice(prev);
    return CMDG_OK;
}

}  // extern "C"
