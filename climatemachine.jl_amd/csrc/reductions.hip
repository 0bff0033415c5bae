// Reductions of state arrays (MPIStateArrays.jl:583-807): weightedsum, dot, p-norms, euclidean
// distance, sum / maximum / minimum, with one value in total or one per state (dims = (1, 3)).
//
// Two stages, no atomics.  Stage 1: one thread per real node (n, e) of an (Np, nstate, nelem)
// array, grid-stride; M = vgeo[n, VM, e] is read once per node and the chosen states are walked
// inside the thread (up to CH per launch), each load contiguous along n across a wave.  Terms are
// formed and accumulated in double-double (hi + lo, the reference's DoubleFloat): TwoProd with an
// explicit fma, TwoSum for the additions; the thread's accumulators are folded across the wave
// (xor butterfly), then across the block's waves in wave order, and the block writes one (hi, lo)
// pair per output slot to a fixed position.  Stage 2: one block folds the partials of every output
// in a fixed order.  The block count depends on the array only, so the same input gives the same
// bits on every call.  This file is compiled with -ffp-contract=off and no fast-math (Makefile):
// the error-free transformations are exact only if the compiler rewrites none of them.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <unordered_map>
#include <vector>

#include "engine_base.h"
#include "rccl.h"
#include "reductions.h"

namespace cmdg {
namespace {

enum { T_SUM, T_DOT, T_DIST, T_ABS, T_SQR, T_POW, T_AMAX, T_MAX, T_MIN };
constexpr int CH = 8;        // chosen states per stage-1 launch
constexpr int NT = 256;      // threads per block, both stages
constexpr int NW = NT / 64;  // waves per block
constexpr int NB_MAX = 2048; // stage-1 blocks: 8 per CU on the 256 CUs of an MI355X

// maximum / minimum that propagate a NaN in either argument (Julia's max / min)
__host__ __device__ inline double nmax(double a, double b) { return (a > b || a != a) ? a : b; }
__host__ __device__ inline double nmin(double a, double b) { return (a < b || a != a) ? a : b; }

template <int T>
__device__ inline DD init()
{
    if constexpr (T == T_MAX) return {-INFINITY, 0.0};
    if constexpr (T == T_MIN) return {INFINITY, 0.0};
    return {0.0, 0.0};
}
template <int T>
__device__ inline void fold(DD &acc, DD t)
{
    if constexpr (T == T_MIN) acc.hi = nmin(acc.hi, t.hi);
    else if constexpr (T == T_MAX || T == T_AMAX) acc.hi = nmax(acc.hi, t.hi);
    else acc = dd_add(acc, t);
}
// the term of one node of one state (the table of include/cmdg.h); M only when weighted
template <int T>
__device__ inline DD term(double a, double b, double M, double p, int weighted)
{
    DD v;
    if constexpr (T == T_SUM) v = {a, 0.0};
    else if constexpr (T == T_DOT) v = two_prod(a, b);
    else if constexpr (T == T_DIST) {
        const DD d = two_sum(a, -b);  // a - b exactly
        v = two_prod(d.hi, d.hi);
        v.lo = fma(2.0 * d.hi, d.lo, v.lo);
        v = fast_two_sum(v.hi, v.lo);
    } else if constexpr (T == T_ABS) v = {fabs(a), 0.0};
    else if constexpr (T == T_SQR) v = two_prod(a, a);
    else if constexpr (T == T_POW) v = {pow(fabs(a), p), 0.0};
    else if constexpr (T == T_AMAX) return {fabs(a), 0.0};
    else return {a, 0.0};
    if (weighted) v = dd_mul_d(v, M);
    return v;
}

template <int T>
__device__ inline DD wave_fold(DD v)
{
    for (int off = 32; off > 0; off >>= 1) {
        const DD o = {__shfl_xor(v.hi, off), __shfl_xor(v.lo, off)};
        fold<T>(v, o);
    }
    return v;
}

// column offsets (Np * s) of the chosen states of one launch
struct Chunk {
    int64_t off[CH];
    int nk;
};

// Stage 1.  PS: one accumulator per chosen state (dims = (1, 3)), else one for the chunk.  part is
// [slot][block] (hi, lo); this launch writes slots slot0 .. slot0 + (PS ? nk : 1) - 1.
template <int T, bool PS>
__global__ __launch_bounds__(NT) void k_reduce_partial(
    const double *__restrict__ A, const double *__restrict__ B, const double *__restrict__ vgeo,
    int64_t vstride, int64_t voff, int64_t estride, uint32_t Np, uint32_t nnodes, Chunk c, double p,
    int weighted, int slot0, double *__restrict__ part)
{
    constexpr int NA = PS ? CH : 1;
    constexpr bool HAS_B = T == T_DOT || T == T_DIST;
    DD acc[NA];
#pragma unroll
    for (int k = 0; k < NA; ++k) acc[k] = init<T>();
    for (uint32_t i = blockIdx.x * NT + threadIdx.x; i < nnodes; i += gridDim.x * NT) {
        const uint32_t e = i / Np, n = i - e * Np;
        const int64_t base = (int64_t)e * estride + n;
        const double M = weighted ? vgeo[(int64_t)e * vstride + voff + n] : 1.0;
        double a[CH], b[CH];
#pragma unroll
        for (int k = 0; k < CH; ++k) {
            a[k] = k < c.nk ? A[base + c.off[k]] : 0.0;
            b[k] = HAS_B && k < c.nk ? B[base + c.off[k]] : 0.0;
        }
#pragma unroll
        for (int k = 0; k < CH; ++k)
            if (k < c.nk) fold<T>(acc[PS ? k : 0], term<T>(a[k], b[k], M, p, weighted));
    }
    __shared__ DD sh[NW][NA];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < NA; ++k) {
        const DD v = wave_fold<T>(acc[k]);
        if (lane == 0) sh[w][k] = v;
    }
    __syncthreads();
    const int k = threadIdx.x;
    if (k < (PS ? c.nk : 1)) {
        DD v = sh[0][k];
        for (int j = 1; j < NW; ++j) fold<T>(v, sh[j][k]);
        double *q = part + 2 * ((int64_t)(slot0 + k) * gridDim.x + blockIdx.x);
        q[0] = v.hi;
        q[1] = v.lo;
    }
}

// Stage 2: output o folds slots [o * spo, (o + 1) * spo) of nb blocks each, in a fixed order.
template <int T>
__global__ __launch_bounds__(NT) void k_reduce_final(const double *__restrict__ part, int nb, int spo,
                                                     int nout, double *__restrict__ out)
{
    __shared__ DD sh[NW];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int nv = spo * nb;
    for (int o = 0; o < nout; ++o) {
        DD v = init<T>();
        for (int j = threadIdx.x; j < nv; j += NT) {
            const double *q = part + 2 * ((int64_t)o * nv + j);
            fold<T>(v, {q[0], q[1]});
        }
        v = wave_fold<T>(v);
        if (lane == 0) sh[w] = v;
        __syncthreads();
        if (threadIdx.x == 0) {
            DD r = sh[0];
            for (int j = 1; j < NW; ++j) fold<T>(r, sh[j]);
            out[2 * o] = r.hi;
            out[2 * o + 1] = r.lo;
        }
        __syncthreads();
    }
}

// ---- per-engine scratch, allocated on first use (EngineBase keeps no member for it) ------------
struct Scratch {
    DevBuf<double> part, out, gather;
    double *host = nullptr;  // pinned
    size_t npart = 0, nout = 0, ngather = 0, nhost = 0;
};
std::mutex g_scratch_m;
std::unordered_map<const EngineBase *, Scratch> g_scratch;

// buffer p of at least n doubles (grown, never shrunk): on the device, or pinned on the host
hipError_t grow(DevBuf<double> &p, size_t &cap, size_t n)
{
    if (n <= cap) return hipSuccess;
    cap = 0;
    const hipError_t r = p.alloc(n);
    if (r == hipSuccess) cap = n;
    return r;
}
hipError_t grow_host(double *&p, size_t &cap, size_t n)
{
    if (n <= cap) return hipSuccess;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
    const hipError_t r = hipHostMalloc((void **)&p, sizeof(double) * n, hipHostMallocDefault);
    if (r == hipSuccess) cap = n;
    return r;
}

Scratch &scratch(const EngineBase *e)
{
    std::lock_guard<std::mutex> lk(g_scratch_m);
    return g_scratch[e];
}

int effective_weighted(const cmdg_reduce_desc *d)
{
    switch (d->op) {
    case CMDG_RED_WEIGHTEDSUM:
    case CMDG_RED_DISTANCE: return 1;
    case CMDG_RED_DOT: return d->weighted != 0;
    case CMDG_RED_NORM: return isfinite(d->p) && d->weighted != 0;  // MPIStateArrays.jl:589
    default: return 0;
    }
}

int term_kind(const cmdg_reduce_desc *d)
{
    switch (d->op) {
    case CMDG_RED_WEIGHTEDSUM:
    case CMDG_RED_SUM: return T_SUM;
    case CMDG_RED_DOT: return T_DOT;
    case CMDG_RED_DISTANCE: return T_DIST;
    case CMDG_RED_MAX: return T_MAX;
    case CMDG_RED_MIN: return T_MIN;
    default: return isinf(d->p) ? T_AMAX : d->p == 1.0 ? T_ABS : d->p == 2.0 ? T_SQR : T_POW;
    }
}

struct Launch {
    const double *A, *B, *vgeo;
    int64_t vstride, voff, estride;
    uint32_t Np, nnodes;
    double p;
    int weighted, nb;
    double *part, *out;
    hipStream_t st;
};

template <int T>
void launch(const Launch &L, const std::vector<int> &sel, bool per_state)
{
    const int nsel = (int)sel.size(), nchunk = (nsel + CH - 1) / CH;
    for (int c = 0; c < nchunk; ++c) {
        Chunk ch{};
        ch.nk = std::min(CH, nsel - c * CH);
        for (int k = 0; k < ch.nk; ++k) ch.off[k] = (int64_t)L.Np * sel[c * CH + k];
        if (per_state)
            hipLaunchKernelGGL((k_reduce_partial<T, true>), dim3(L.nb), dim3(NT), 0, L.st, L.A, L.B, L.vgeo,
                               L.vstride, L.voff, L.estride, L.Np, L.nnodes, ch, L.p, L.weighted, c * CH, L.part);
        else
            hipLaunchKernelGGL((k_reduce_partial<T, false>), dim3(L.nb), dim3(NT), 0, L.st, L.A, L.B, L.vgeo,
                               L.vstride, L.voff, L.estride, L.Np, L.nnodes, ch, L.p, L.weighted, c, L.part);
    }
    const int nout = per_state ? nsel : 1, spo = per_state ? 1 : nchunk;
    hipLaunchKernelGGL((k_reduce_final<T>), dim3(1), dim3(NT), 0, L.st, L.part, L.nb, spo, nout, L.out);
}

// Shewchuk's exact summation with correct rounding (the algorithm of Python's math.fsum)
double exact_sum(const std::vector<double> &v)
{
    std::vector<double> ps;
    double special = 0.0;
    bool nan = false, inf = false;
    for (double x : v) {
        if (x != x) {
            nan = true;
            continue;
        }
        if (isinf(x)) {
            special += x;  // +inf + -inf = NaN
            inf = true;
            continue;
        }
        size_t i = 0;
        for (size_t j = 0; j < ps.size(); ++j) {
            double y = ps[j];
            if (fabs(x) < fabs(y)) std::swap(x, y);
            const double hi = x + y, lo = y - (hi - x);
            if (lo != 0.0) ps[i++] = lo;
            x = hi;
        }
        ps.resize(i);
        ps.push_back(x);
    }
    if (nan) return NAN;
    if (inf) return special;
    size_t n = ps.size();
    double hi = 0.0;
    if (n > 0) {
        hi = ps[--n];
        double lo = 0.0;
        while (n > 0) {
            const double x = hi, y = ps[--n];
            hi = x + y;
            lo = y - (hi - x);
            if (lo != 0.0) break;
        }
        // round half to even across the partials that follow
        if (n > 0 && ((lo < 0.0 && ps[n - 1] < 0.0) || (lo > 0.0 && ps[n - 1] > 0.0))) {
            const double y = lo * 2.0, x = hi + y;
            if (y == x - hi) hi = x;
        }
    }
    return hi;
}

}  // namespace

int reduce_nout(const cmdg_reduce_desc *d)
{
    if (!d->per_state) return 1;
    return d->states ? d->nstates : d->nstate;
}

int reduce_check(const cmdg_reduce_desc *d, std::string &err)
{
    if (!d) {
        err = "reduce: no descriptor";
        return CMDG_ERR_INVALID;
    }
    if (d->op < CMDG_RED_WEIGHTEDSUM || d->op > CMDG_RED_MIN) {
        err = "reduce: unknown op";
        return CMDG_ERR_INVALID;
    }
    if (d->op == CMDG_RED_NORM && !(d->p > 0.0)) {  // (false for NaN too)
        err = "reduce: norm needs p > 0 (1, 2, any finite p or INFINITY), not NaN";
        return CMDG_ERR_INVALID;
    }
    if (d->nstate < 1) {
        err = "reduce: nstate < 1";
        return CMDG_ERR_INVALID;
    }
    if (d->states) {
        if (d->nstates < 1) {
            err = "reduce: an empty state subset";
            return CMDG_ERR_INVALID;
        }
        for (int i = 0; i < d->nstates; ++i)
            if (d->states[i] < 0 || d->states[i] >= d->nstate) {
                err = "reduce: state index " + std::to_string(d->states[i]) + " out of range [0, " +
                      std::to_string(d->nstate) + ")";
                return CMDG_ERR_INVALID;
            }
    }
    return CMDG_OK;
}

int reduce_device(EngineBase *e, const cmdg_reduce_desc *d, const double *A, const double *B,
                  const double **d_result)
{
    std::string err;
    if (reduce_check(d, err)) return e->fail(CMDG_ERR_INVALID, err);
    if (!A) return e->fail(CMDG_ERR_INVALID, "reduce: A is NULL");
    if ((d->op == CMDG_RED_DOT || d->op == CMDG_RED_DISTANCE) && !B)
        return e->fail(CMDG_ERR_INVALID, "reduce: dot / euclidean_distance need B");
    const int weighted = effective_weighted(d);
    if (weighted && (!e->g.vgeo || e->g.nvgeo <= VM))
        return e->fail(CMDG_ERR_INVALID, "reduce: weighted reduction on a handle without vgeo weights");
    const int64_t nn = (int64_t)e->Np * e->nreal;
    if (nn > (int64_t)UINT32_MAX - (int64_t)NB_MAX * NT)
        return e->fail(CMDG_ERR_INVALID, "reduce: more than 2^32 real nodes");
    std::vector<int> sel;
    if (d->states) sel.assign(d->states, d->states + d->nstates);
    else
        for (int s = 0; s < d->nstate; ++s) sel.push_back(s);
    const bool ps = d->per_state != 0;
    const int nsel = (int)sel.size(), nchunk = (nsel + CH - 1) / CH;
    const int nout = ps ? nsel : 1;
    const int nb = (int)std::max<int64_t>(1, std::min<int64_t>(NB_MAX, (nn + NT - 1) / NT));
    Scratch &s = scratch(e);
    const size_t nslots = ps ? (size_t)nsel : (size_t)nchunk;
    hipError_t r = grow(s.part, s.npart, nslots * nb * 2);
    if (r == hipSuccess) r = grow(s.out, s.nout, (size_t)nout * 2);
    if (r != hipSuccess) return e->fail(CMDG_ERR_HIP, std::string("reduce: scratch: ") + hipGetErrorString(r));
    Launch L{A, B, e->g.vgeo, (int64_t)e->Np * e->g.nvgeo, (int64_t)e->Np * VM, (int64_t)e->Np * d->nstate,
             (uint32_t)e->Np, (uint32_t)nn, d->p, weighted, nb, s.part, s.out, e->s_comp};
    switch (term_kind(d)) {
    case T_SUM: launch<T_SUM>(L, sel, ps); break;
    case T_DOT: launch<T_DOT>(L, sel, ps); break;
    case T_DIST: launch<T_DIST>(L, sel, ps); break;
    case T_ABS: launch<T_ABS>(L, sel, ps); break;
    case T_SQR: launch<T_SQR>(L, sel, ps); break;
    case T_POW: launch<T_POW>(L, sel, ps); break;
    case T_AMAX: launch<T_AMAX>(L, sel, ps); break;
    case T_MAX: launch<T_MAX>(L, sel, ps); break;
    default: launch<T_MIN>(L, sel, ps); break;
    }
    r = hipGetLastError();
    if (r != hipSuccess) return e->fail(CMDG_ERR_HIP, std::string("reduce launch: ") + hipGetErrorString(r));
    *d_result = s.out;
    return CMDG_OK;
}

int reduce_gather_buffer(EngineBase *e, size_t n, double **buf)
{
    Scratch &s = scratch(e);
    const hipError_t r = grow(s.gather, s.ngather, n);
    if (r != hipSuccess) return e->fail(CMDG_ERR_HIP, std::string("reduce: gather buffer: ") + hipGetErrorString(r));
    *buf = s.gather;
    return CMDG_OK;
}

int reduce_host_buffer(EngineBase *e, size_t n, double **buf)
{
    Scratch &s = scratch(e);
    const hipError_t r = grow_host(s.host, s.nhost, n);
    if (r != hipSuccess) return e->fail(CMDG_ERR_HIP, std::string("reduce: host buffer: ") + hipGetErrorString(r));
    *buf = s.host;
    return CMDG_OK;
}

int reduce_combine(const cmdg_reduce_desc *d, const double *partials, int nranks, double *out,
                   std::string &err)
{
    if (int r = reduce_check(d, err)) return r;
    if (!partials || !out || nranks < 1) {
        err = "reduce_combine: NULL partials / out or nranks < 1";
        return CMDG_ERR_INVALID;
    }
    const int nout = reduce_nout(d);
    const bool extremum = d->op == CMDG_RED_MAX || d->op == CMDG_RED_MIN ||
                          (d->op == CMDG_RED_NORM && isinf(d->p));
    std::vector<double> v((size_t)nranks * 2);
    for (int o = 0; o < nout; ++o) {
        double x;
        if (extremum) {
            x = partials[2 * o];
            for (int r = 1; r < nranks; ++r) {
                const double y = partials[2 * ((size_t)r * nout + o)];
                x = d->op == CMDG_RED_MIN ? nmin(x, y) : nmax(x, y);
            }
        } else {
            for (int r = 0; r < nranks; ++r) {  // rank order
                v[2 * r] = partials[2 * ((size_t)r * nout + o)];
                v[2 * r + 1] = partials[2 * ((size_t)r * nout + o) + 1];
            }
            x = exact_sum(v);
            if (d->op == CMDG_RED_DISTANCE || (d->op == CMDG_RED_NORM && d->p == 2.0)) x = sqrt(x);
            else if (d->op == CMDG_RED_NORM && d->p != 1.0) x = pow(x, 1.0 / d->p);
        }
        out[o] = x;
    }
    return CMDG_OK;
}

void reduce_release(EngineBase *e)
{
    std::lock_guard<std::mutex> lk(g_scratch_m);
    auto it = g_scratch.find(e);
    if (it == g_scratch.end()) return;
    if (it->second.host) (void)hipHostFree(it->second.host);
    g_scratch.erase(it);  // (frees the device buffers)
}

}  // namespace cmdg

using namespace cmdg;

extern "C" {

// this rank's nout (hi, lo) pairs into host (the engine's device current)
static int reduce_to_host(EngineBase *e, const cmdg_reduce_desc *d, const double *A, const double *B,
                          double *host)
{
    const double *r = nullptr;
    double *stage = nullptr;
    const size_t n = 2 * (size_t)reduce_nout(d);
    if (int rc = reduce_device(e, d, A, B, &r)) return rc;
    if (int rc = reduce_host_buffer(e, n, &stage)) return rc;
    if (hipMemcpyAsync(stage, r, sizeof(double) * n, hipMemcpyDeviceToHost, e->s_comp) != hipSuccess ||
        hipStreamSynchronize(e->s_comp) != hipSuccess)
        return e->fail(CMDG_ERR_HIP, "reduce: copy of the partials failed");
    memcpy(host, stage, sizeof(double) * n);
    return CMDG_OK;
}

int cmdg_reduce_local(cmdg_handle h, const cmdg_reduce_desc *d, const double *A, const double *B,
                      double *partials_host)
{
    if (!h || !partials_host) return CMDG_ERR_INVALID;
    DevGuard guard_(h->eng);
    return set_err(h, reduce_to_host(h->eng, d, A, B, partials_host));
}

int cmdg_reduce_combine(const cmdg_reduce_desc *d, const double *partials, int32_t nranks, double *out)
{
    std::string err;
    const int r = reduce_combine(d, partials, nranks, out, err);
    if (r) set_create_err("cmdg_reduce_combine: " + err);
    return r;
}

int cmdg_reduce(cmdg_handle h, const cmdg_reduce_desc *d, const double *A, const double *B,
                double *out_host)
{
    if (!h || !out_host) return CMDG_ERR_INVALID;
    DevGuard guard_(h->eng);
    EngineBase *e = h->eng;
    if (e->transport == TRANSPORT_LOCAL && e->nranks > 1)
        return set_err(h, e->fail(CMDG_ERR_INVALID, "cmdg_reduce: the handle is one rank of a local-transport "
                                                    "group; reduce the group with cmdg_group_reduce"));
    std::string err;
    if (reduce_check(d, err)) return set_err(h, e->fail(CMDG_ERR_INVALID, err));
    const int nout = reduce_nout(d);
    const int nranks = e->transport == TRANSPORT_RCCL && e->nccl_comm ? e->nranks : 1;
    std::vector<double> parts(2 * (size_t)nout * nranks);
    if (nranks == 1 && e->transport != TRANSPORT_RCCL) {
        if (int r = reduce_to_host(e, d, A, B, parts.data())) return set_err(h, r);
    } else {  // every rank's partials, in rank order, on every rank
        const double *r = nullptr;
        double *gath = nullptr, *stage = nullptr;
        if (int rc = reduce_device(e, d, A, B, &r)) return set_err(h, rc);
        if (int rc = reduce_gather_buffer(e, parts.size(), &gath)) return set_err(h, rc);
        if (int rc = reduce_host_buffer(e, parts.size(), &stage)) return set_err(h, rc);
        if (int rc = rccl::AllGather(r, gath, 2 * (size_t)nout, rccl::kDouble, e->nccl_comm, e->s_comp))
            return set_err(h, e->fail(CMDG_ERR_COMM, std::string("reduce: ncclAllGather: ") + rccl::GetErrorString(rc)));
        if (hipMemcpyAsync(stage, gath, sizeof(double) * parts.size(), hipMemcpyDeviceToHost, e->s_comp) != hipSuccess ||
            hipStreamSynchronize(e->s_comp) != hipSuccess)
            return set_err(h, e->fail(CMDG_ERR_HIP, "reduce: copy of the gathered partials failed"));
        memcpy(parts.data(), stage, sizeof(double) * parts.size());
    }
    if (reduce_combine(d, parts.data(), nranks, out_host, err)) return set_err(h, e->fail(CMDG_ERR_INVALID, err));
    return CMDG_OK;
}

int cmdg_group_reduce(cmdg_handle *handles, int32_t n, const cmdg_reduce_desc *d, const double **A,
                      const double **B, double *out_host)
{
    if (!A || !out_host) return CMDG_ERR_INVALID;
    GroupCall gc(handles, n);
    if (!gc.ok()) return CMDG_ERR_INVALID;
    EngineBase *e0 = handles[0]->eng;
    for (int i = 0; i < n; ++i) {
        EngineBase *e = handles[i]->eng;
        if (n > 1 && (e->transport != TRANSPORT_LOCAL || e->nranks != n || e->rank != i))
            return gc.finish(e->fail(CMDG_ERR_INVALID, "cmdg_group_reduce: handle i must be rank i of "
                                                       "one group of n connected with cmdg_comm_connect_local"));
    }
    std::string err;
    if (reduce_check(d, err)) return gc.finish(e0->fail(CMDG_ERR_INVALID, err));
    const size_t per = 2 * (size_t)reduce_nout(d);
    std::vector<double> parts(per * n);
    for (int i = 0; i < n; ++i)
        if (int r = reduce_to_host(handles[i]->eng, d, A[i], B ? B[i] : nullptr, parts.data() + per * i))
            return gc.finish(r);
    if (reduce_combine(d, parts.data(), n, out_host, err)) return gc.finish(e0->fail(CMDG_ERR_INVALID, err));
    return CMDG_OK;
}

}  // extern "C"
