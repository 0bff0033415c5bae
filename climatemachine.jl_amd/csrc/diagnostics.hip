// AtmosLESDefault diagnostics (src/Diagnostics/atmos_les_default.jl, atmos_common.jl, helpers.jl):
// the level reductions over the nodal diagnostics D of kernels.h k_les_nodal.
//
// Levels: L = Nqk * nvertelem, evk = Nqk * ev + k, element e = ev + eh * nvertelem (0-based).
// k_les_partial: a work-group owns one vertical element index ev and a slice of the horizontal
// elements; thread n keeps node n = (i, j, k) of the element and walks the slice with one
// double-double accumulator per variable in registers.  Every term is the rounded double expression
// the reference writes, evaluated left to right (this unit is compiled with -ffp-contract=off and no
// fast-math, Makefile).  The Nq^2 threads of each k are then folded through LDS in a fixed order:
// first over i by thread (j, k), then over j by thread k.  k_les_fold folds the slices in slice order,
// k_les_finish combines the ranks in rank order and does the finishing arithmetic of :687-773 and
// :815-846, so that the higher-order pass finds the finished averages of its level on the device.
// No floating-point atomics; the slice length depends on the grid only: the same input gives the
// same bits.
//
// AtmosGCMDefault diagnostics (src/Diagnostics/atmos_gcm_default.jl, diagnostic_fields.jl): the entries
// cmdg_vector_gradients, cmdg_vorticity and cmdg_gcm_nodal at the end of this file; their kernels need
// the order (and the nodal pass the law) and live in kernels.h, the finishing pass in interpolation.hip.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <unordered_map>
#include <vector>

#include "diagnostics.h"
#include "engine_base.h"
#include "kernels_nodal.h"
#include "rccl.h"
#include "reductions.h"

namespace cmdg {
namespace {

constexpr int V_MH = 11, V_X3 = 14, V_JCV = 15;  // _MH, _x3, _JcV (Grids.jl:76-92), 0-based
constexpr int NSIMPLE_DRY = 13, NSIMPLE_MOIST = 20, NHO_DRY = 11, NHO_MOIST = 21;
// the moist simple pass carries three sums more: MH q_liq rho rho, MH q_ice rho rho (:666-667) and the
// number of nodes with condensate
constexpr int NEXTRA_MOIST = 3;
enum { PASS_GEOM = 0, PASS_SIMPLE = 1, PASS_HO = 2 };
// positions in a row of finished simple averages
enum { A_U = 0, A_V, A_W, A_AVG_RHO, A_RHO, A_TEMP, A_PRES, A_THD, A_ET, A_EI, A_HT, A_HI, A_W_HT_SGS,
       A_QT, A_QL, A_QI, A_QV, A_THV, A_THL, A_W_QT_SGS, A_LIQ2, A_ICE2, A_COUNT };
// columns of D (physics_atmos.h / physics_moist.h les_diagnostics)
enum { D_TEMP = 0, D_PRES, D_THD, D_EI, D_HT, D_HI, D_DH3, D_QL, D_QI, D_QV, D_THV, D_THL, D_HC, D_DQ3 };

template <bool MOIST, int PASS>
struct NVars {
    static constexpr int value = PASS == PASS_GEOM     ? 1
                                 : PASS == PASS_SIMPLE ? (MOIST ? NSIMPLE_MOIST + NEXTRA_MOIST : NSIMPLE_DRY)
                                                       : (MOIST ? NHO_MOIST : NHO_DRY);
};

struct PartialArgs {
    const double *Q, *D, *vgeo, *avg;  // avg: (L, navg) finished simple averages (PASS_HO)
    double *part;                      // (nslice, L, NV) (hi, lo)
    int64_t nhorz, slice_len;
    int ns, nd, nvgeo, navg, Np, Nij, NQ, NQV, nvert, L;
};

template <bool MOIST, int PASS>
__global__ __launch_bounds__(512) void k_les_partial(PartialArgs a)
{
    constexpr int NV = NVars<MOIST, PASS>::value;
    __shared__ DD sh[512], sh2[64];
    const int tid = threadIdx.x, Np = a.Np;
    const int ev = blockIdx.y;
    const int k = tid / a.Nij;
    const int evk = a.NQV * ev + k;
    DD acc[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) acc[v] = {0.0, 0.0};
    double ha_u = 0, ha_v = 0, ha_w = 0, ha_rho = 0, ha_thd = 0, ha_ei = 0;
    double ha_qt = 0, ha_ql = 0, ha_qi = 0, ha_qv = 0, ha_thv = 0, ha_thl = 0;
    if constexpr (PASS == PASS_HO) {
        const double *ha = a.avg + (int64_t)evk * a.navg;
        ha_u = ha[A_U], ha_v = ha[A_V], ha_w = ha[A_W], ha_rho = ha[A_AVG_RHO], ha_thd = ha[A_THD], ha_ei = ha[A_EI];
        if constexpr (MOIST)
            ha_qt = ha[A_QT], ha_ql = ha[A_QL], ha_qi = ha[A_QI], ha_qv = ha[A_QV], ha_thv = ha[A_THV],
            ha_thl = ha[A_THL];
    }
    const int64_t eh0 = (int64_t)blockIdx.x * a.slice_len;
    const int64_t eh1 = eh0 + a.slice_len < a.nhorz ? eh0 + a.slice_len : a.nhorz;
    for (int64_t eh = eh0; eh < eh1; ++eh) {
        const int64_t e = ev + eh * a.nvert;
        const double MH = a.vgeo[tid + (int64_t)Np * (V_MH + (int64_t)a.nvgeo * e)];
        double t[NV];
        if constexpr (PASS == PASS_GEOM) {
            t[0] = MH;
        } else {
            const double *q = a.Q + tid + (int64_t)Np * a.ns * e;
            const double *d = a.D + tid + (int64_t)Np * a.nd * e;
            const double rho = q[0];
            if constexpr (PASS == PASS_SIMPLE) {
                t[A_U] = MH * q[Np];
                t[A_V] = MH * q[2 * Np];
                t[A_W] = MH * q[3 * Np];
                t[A_AVG_RHO] = MH * rho;
                t[A_RHO] = MH * rho * rho;
                t[A_TEMP] = MH * d[D_TEMP * Np] * rho;
                t[A_PRES] = MH * d[D_PRES * Np] * rho;
                t[A_THD] = MH * d[D_THD * Np] * rho;
                t[A_ET] = MH * q[4 * Np];
                t[A_EI] = MH * d[D_EI * Np] * rho;
                t[A_HT] = MH * d[D_HT * Np] * rho;
                t[A_HI] = MH * d[D_HI * Np] * rho;
                t[A_W_HT_SGS] = MH * d[D_DH3 * Np] * rho;
                if constexpr (MOIST) {
                    const double ql = d[D_QL * Np], qi = d[D_QI * Np];
                    t[A_QT] = MH * q[5 * Np];
                    t[A_QL] = MH * ql * rho;
                    t[A_QI] = MH * qi * rho;
                    t[A_QV] = MH * d[D_QV * Np] * rho;
                    t[A_THV] = MH * d[D_THV * Np] * rho;
                    t[A_THL] = MH * d[D_THL * Np] * rho;
                    t[A_W_QT_SGS] = MH * d[D_DQ3 * Np] * rho;
                    t[A_LIQ2] = MH * ql * rho * rho;
                    t[A_ICE2] = MH * qi * rho * rho;
                    t[A_COUNT] = d[D_HC * Np];
                }
            } else {
                const double up = q[Np] / rho - ha_u;
                const double vp = q[2 * Np] / rho - ha_v;
                const double wp = q[3 * Np] / rho - ha_w;
                const double eip = d[D_EI * Np] - ha_ei;
                const double thdp = d[D_THD * Np] - ha_thd;
                t[0] = MH * (up * up) * rho;
                t[1] = MH * (vp * vp) * rho;
                t[2] = MH * (wp * wp) * rho;
                t[3] = MH * (wp * wp * wp) * rho;
                t[4] = 0.5 * (t[0] + t[1] + t[2]);
                t[5] = MH * (eip * eip) * rho;
                t[6] = MH * wp * up * rho;
                t[7] = MH * wp * vp * rho;
                t[8] = MH * wp * (rho - ha_rho) * rho;
                t[9] = MH * wp * thdp * rho;
                t[10] = MH * wp * eip * rho;
                if constexpr (MOIST) {
                    const double qtp = q[5 * Np] / rho - ha_qt;
                    const double qlp = d[D_QL * Np] - ha_ql;
                    const double qip = d[D_QI * Np] - ha_qi;
                    const double qvp = d[D_QV * Np] - ha_qv;
                    const double thvp = d[D_THV * Np] - ha_thv;
                    const double thlp = d[D_THL * Np] - ha_thl;
                    t[11] = MH * (qtp * qtp) * rho;
                    t[12] = MH * (thlp * thlp) * rho;
                    t[13] = MH * wp * qtp * rho;
                    t[14] = MH * wp * qlp * rho;
                    t[15] = MH * wp * qip * rho;
                    t[16] = MH * wp * qvp * rho;
                    t[17] = MH * wp * thvp * rho;
                    t[18] = MH * wp * thlp * rho;
                    t[19] = MH * qtp * thlp * rho;
                    t[20] = MH * qtp * eip * rho;
                }
            }
        }
#pragma unroll
        for (int v = 0; v < NV; ++v) acc[v] = dd_add_d(acc[v], t[v]);
    }
    // fold the Nq^2 nodes of each k: thread r = (j, k) over i, then thread k over j
    const int nrow = a.NQ * a.NQV;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        sh[tid] = acc[v];
        __syncthreads();
        if (tid < nrow) {
            DD s = sh[tid * a.NQ];
            for (int i = 1; i < a.NQ; ++i) s = dd_add(s, sh[tid * a.NQ + i]);
            sh2[tid] = s;
        }
        __syncthreads();
        if (tid < a.NQV) {
            DD s = sh2[tid * a.NQ];
            for (int j = 1; j < a.NQ; ++j) s = dd_add(s, sh2[tid * a.NQ + j]);
            double *p = a.part + 2 * (((int64_t)blockIdx.x * a.L + a.NQV * ev + tid) * NV + v);
            p[0] = s.hi;
            p[1] = s.lo;
        }
    }
}

// out[idx] = part[0][idx] + part[1][idx] + ... in slice order, idx < n; two (hi, lo) pairs follow:
// the node columns with condensate (cover; NULL: 0) and the node columns of this rank
__global__ __launch_bounds__(256) void k_les_fold(const double *__restrict__ part, int nslice, int64_t n,
                                                  const unsigned long long *__restrict__ cover, double ncol,
                                                  double *__restrict__ out)
{
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * 256) {
        DD s = {part[2 * idx], part[2 * idx + 1]};
        for (int sl = 1; sl < nslice; ++sl) {
            const double *p = part + 2 * ((int64_t)sl * n + idx);
            s = dd_add(s, {p[0], p[1]});
        }
        out[2 * idx] = s.hi;
        out[2 * idx + 1] = s.lo;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        out[2 * n] = cover ? (double)*cover : 0.0;
        out[2 * n + 1] = 0.0;
        out[2 * n + 2] = ncol;
        out[2 * n + 3] = 0.0;
    }
}

// a node column (eh, i, j) has condensate on some level: qc_gt_0_full (:285-288, 736-741)
__global__ __launch_bounds__(256) void k_les_cover(const double *__restrict__ D, int nd, int Np, int Nij, int NQV,
                                                   int nvert, int64_t ncol, unsigned long long *__restrict__ count)
{
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= ncol) return;
    const int64_t eh = c / Nij;
    const int ij = (int)(c - eh * Nij);
    bool any = false;
    for (int ev = 0; ev < nvert; ++ev) {
        const double *d = D + (int64_t)Np * (D_HC + (int64_t)nd * (ev + eh * nvert));
        for (int k = 0; k < NQV; ++k) any = any || d[ij + Nij * k] != 0.0;
    }
    if (any) atomicAdd(count, 1ull);  // (an integer count: exact in any order)
}

// gath: (nranks, L * NV + 2) (hi, lo), combined in rank order; raw (L * NV + 2) the rounded sums.
// PASS_SIMPLE: avg = raw / MH_z, then every variable but avg_rho / avg_rho (:687-773; the count stays
// a count).  PASS_HO: avg = raw / MH_z / avg_rho of simple (:815-846).
__global__ __launch_bounds__(64) void k_les_finish(const double *__restrict__ gath, int nranks, int L, int NV, int pass,
                                                   const double *__restrict__ MH_z, const double *__restrict__ simple,
                                                   int navg, double *__restrict__ raw, double *__restrict__ avg)
{
    const int64_t nb = (int64_t)L * NV + 2;
    const int evk = blockIdx.x * 64 + threadIdx.x;
    if (evk < L) {
        for (int v = 0; v < NV; ++v) {
            const int64_t idx = (int64_t)evk * NV + v;
            DD s = {gath[2 * idx], gath[2 * idx + 1]};
            for (int r = 1; r < nranks; ++r) s = dd_add(s, {gath[2 * (r * nb + idx)], gath[2 * (r * nb + idx) + 1]});
            raw[idx] = s.hi;
        }
        if (pass == PASS_SIMPLE) {
            double *a = avg + (int64_t)evk * NV;
            const double *r = raw + (int64_t)evk * NV;
            for (int v = 0; v < NV; ++v) a[v] = v == A_COUNT ? r[v] : r[v] / MH_z[evk];
            const double avg_rho = a[A_AVG_RHO];
            for (int v = 0; v < NV; ++v)
                if (v != A_AVG_RHO && v != A_COUNT) a[v] /= avg_rho;
        } else if (pass == PASS_HO) {
            const double avg_rho = simple[(int64_t)evk * navg + A_AVG_RHO];
            for (int v = 0; v < NV; ++v) {
                const int64_t idx = (int64_t)evk * NV + v;
                avg[idx] = raw[idx] / MH_z[evk] / avg_rho;
            }
        }
    }
    if (evk == 0) {
        for (int x = 0; x < 2; ++x) {
            const int64_t idx = (int64_t)L * NV + x;
            DD s = {gath[2 * idx], gath[2 * idx + 1]};
            for (int r = 1; r < nranks; ++r) s = dd_add(s, {gath[2 * (r * nb + idx)], gath[2 * (r * nb + idx) + 1]});
            raw[idx] = s.hi;
        }
    }
}

// zvals[evk]: x3 of the last node visited on the level (last horizontal element, i = j = Nq);
// jcv[evk]: JcV of node (1, 1, k) of element ev of the first stack
__global__ __launch_bounds__(64) void k_les_levels(const double *__restrict__ vgeo, int nvgeo, int Np, int Nij, int NQV,
                                                   int nvert, int64_t nhorz, double *__restrict__ zvals,
                                                   double *__restrict__ jcv)
{
    const int evk = blockIdx.x * 64 + threadIdx.x;
    if (evk >= NQV * nvert) return;
    const int ev = evk / NQV, k = evk - ev * NQV;
    const int64_t elast = ev + (nhorz - 1) * nvert;
    zvals[evk] = vgeo[Nij * k + Nij - 1 + (int64_t)Np * (V_X3 + (int64_t)nvgeo * elast)];
    jcv[evk] = vgeo[Nij * k + (int64_t)Np * (V_JCV + (int64_t)nvgeo * ev)];
}

// vorticity_kernel! (diagnostic_fields.jl:382-396): vgrad (nreal, 9, Np) -> vort (nreal, 3, Np); n = nreal Np
__global__ __launch_bounds__(256) void k_vorticity(const double *__restrict__ vgrad, double *__restrict__ vort,
                                                   int Np, int64_t n)
{
    for (int64_t I = (int64_t)blockIdx.x * 256 + threadIdx.x; I < n; I += (int64_t)gridDim.x * 256) {
        const int64_t e = I / Np;
        const int node = (int)(I - e * Np);
        double g[9], om[3];
#pragma unroll
        for (int c = 0; c < 9; ++c) g[c] = vgrad[node + (int64_t)Np * (c + 9 * e)];
        vorticity_node(g, om);
#pragma unroll
        for (int c = 0; c < 3; ++c) vort[node + (int64_t)Np * (c + 3 * e)] = om[c];
    }
}

// ---- per-engine state ---------------------------------------------------------------------------
struct LesState {
    bool inited = false;
    int nvert = 0, L = 0, nd = 0, moist = 0, nvs = 0, nvh = 0, nslice = 0;
    int64_t nhorz = 0, slice_len = 0;
    DevBuf<double> D, part, dd, gath, MH_z, lev, rawS, avgS, rawH, avgH;
    DevBuf<unsigned long long> cover;
    size_t ngath = 0;
    double *host = nullptr;  // pinned staging
    size_t nhost = 0;
    std::vector<double> zvals, Mvert;
    int nsimple() const { return moist ? NSIMPLE_MOIST : NSIMPLE_DRY; }
};
std::mutex g_les_m;
std::unordered_map<const EngineBase *, LesState> g_les;
LesState &state(const EngineBase *e)
{
    std::lock_guard<std::mutex> lk(g_les_m);
    return g_les[e];
}

int hip_fail(EngineBase *e, const char *what, hipError_t r)
{
    return e->fail(CMDG_ERR_HIP, std::string("les diagnostics: ") + what + ": " + hipGetErrorString(r));
}
#define LESCHK(call)                                       \
    do {                                                   \
        const hipError_t r_ = (call);                      \
        if (r_ != hipSuccess) return hip_fail(e, #call, r_); \
    } while (0)

int host_buffer(EngineBase *e, LesState &s, size_t n)
{
    if (n <= s.nhost) return CMDG_OK;
    if (s.host) (void)hipHostFree(s.host);
    s.host = nullptr;
    s.nhost = 0;
    LESCHK(hipHostMalloc((void **)&s.host, sizeof(double) * n, hipHostMallocDefault));
    s.nhost = n;
    return CMDG_OK;
}

// what every entry checks: the law, the grid, the stack height; fills the sizes of s
int setup(EngineBase *e, LesState &s, int nvert)
{
    int nd = 0, moist = 0;
    if (int r = e->launch_les_nodal(nullptr, 0.0, nullptr, &nd, &moist)) return r;
    if (!e->stacked)
        return e->fail(CMDG_ERR_INVALID, "les diagnostics: the grid is not stacked (levels are defined on a "
                                         "stacked topology)");
    if (e->fv || e->NQV < 2)
        return e->fail(CMDG_ERR_INVALID, "les diagnostics: the vertical polynomial order is 0");
    if (nvert < 1 || e->nreal < 1 || e->nreal % nvert != 0)
        return e->fail(CMDG_ERR_INVALID, "les diagnostics: nvertelem < 1 or the real elements are not a whole "
                                         "number of stacks of nvertelem");
    if (!e->g.vgeo || e->g.nvgeo <= V_JCV)
        return e->fail(CMDG_ERR_INVALID, "les diagnostics: vgeo lacks the MH / x3 / JcV columns");
    if (e->Np > 512 || e->NQ * e->NQV > 64)
        return e->fail(CMDG_ERR_UNSUPPORTED, "les diagnostics: more than 512 nodes per element");
    s.nvert = nvert;
    s.L = e->NQV * nvert;
    s.nd = nd;
    s.moist = moist;
    s.nvs = moist ? NSIMPLE_MOIST + NEXTRA_MOIST : NSIMPLE_DRY;
    s.nvh = moist ? NHO_MOIST : NHO_DRY;
    s.nhorz = e->nreal / nvert;
    // slices: about 1024 work-groups, at least two elements each; a function of the grid alone
    const int64_t want = std::max<int64_t>(1, 1024 / nvert);
    s.slice_len = std::max<int64_t>(2, (s.nhorz + want - 1) / want);
    s.nslice = (int)((s.nhorz + s.slice_len - 1) / s.slice_len);
    return CMDG_OK;
}

int alloc_buffers(EngineBase *e, LesState &s)
{
    const size_t nvmax = (size_t)std::max(s.nvs, s.nvh);
    const size_t nb = (size_t)s.L * nvmax + 2;
    LESCHK(s.D.alloc((size_t)e->nelem * s.nd * e->Np));
    LESCHK(s.part.alloc(2 * (size_t)s.nslice * s.L * nvmax));
    LESCHK(s.dd.alloc(2 * nb));
    LESCHK(s.MH_z.alloc((size_t)s.L + 2));
    LESCHK(s.lev.alloc(2 * (size_t)s.L));
    LESCHK(s.rawS.alloc(nb));
    LESCHK(s.avgS.alloc(nb));
    LESCHK(s.rawH.alloc(nb));
    LESCHK(s.avgH.alloc(nb));
    LESCHK(s.cover.alloc(1));
    return host_buffer(e, s, 4 * nb + 2 * (size_t)s.L);
}

template <int PASS>
void launch_partial(EngineBase *e, LesState &s, const double *Q)
{
    PartialArgs a{};
    a.Q = Q;
    a.D = s.D;
    a.vgeo = e->g.vgeo;
    a.avg = s.avgS;
    a.part = s.part;
    a.nhorz = s.nhorz;
    a.slice_len = s.slice_len;
    a.ns = e->ns;
    a.nd = s.nd;
    a.nvgeo = e->g.nvgeo;
    a.navg = s.nvs;
    a.Np = e->Np;
    a.Nij = e->NQ * e->NQ;
    a.NQ = e->NQ;
    a.NQV = e->NQV;
    a.nvert = s.nvert;
    a.L = s.L;
    const dim3 grid((unsigned)s.nslice, (unsigned)s.nvert), block((unsigned)e->Np);
    if (s.moist && PASS != PASS_GEOM)
        hipLaunchKernelGGL((k_les_partial<true, PASS>), grid, block, 0, e->s_comp, a);
    else
        hipLaunchKernelGGL((k_les_partial<false, PASS>), grid, block, 0, e->s_comp, a);
}

int nvars(const LesState &s, int pass) { return pass == PASS_GEOM ? 1 : pass == PASS_SIMPLE ? s.nvs : s.nvh; }

// this rank's (L * NV + 2) double-double sums of one pass into s.dd, enqueued on the compute stream
int stage(EngineBase *e, LesState &s, int pass, const double *Q, double t)
{
    const int NV = nvars(s, pass);
    const int64_t n = (int64_t)s.L * NV;
    const unsigned long long *cover = nullptr;
    if (pass == PASS_SIMPLE) {
        int nd, moist;
        if (int r = e->launch_les_nodal(Q, t, s.D, &nd, &moist)) return r;
        launch_partial<PASS_SIMPLE>(e, s, Q);
        if (s.moist) {
            const int Nij = e->NQ * e->NQ;
            const int64_t ncol = s.nhorz * Nij;
            LESCHK(hipMemsetAsync(s.cover, 0, sizeof(unsigned long long), e->s_comp));
            hipLaunchKernelGGL(k_les_cover, dim3((unsigned)((ncol + 255) / 256)), dim3(256), 0, e->s_comp, s.D.get(),
                               s.nd, e->Np, Nij, e->NQV, s.nvert, ncol, s.cover.get());
            cover = s.cover;
        }
    } else if (pass == PASS_HO) {
        launch_partial<PASS_HO>(e, s, Q);
    } else {
        launch_partial<PASS_GEOM>(e, s, Q);
    }
    hipLaunchKernelGGL(k_les_fold, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 1024)), dim3(256), 0, e->s_comp,
                       s.part.get(), s.nslice, n, cover, (double)(s.nhorz * e->NQ * e->NQ), s.dd.get());
    return e->launch_status("les diagnostics");
}

// combines nranks gathered buffers (device) and finishes the pass on the compute stream
int finish(EngineBase *e, LesState &s, int pass, const double *gath, int nranks)
{
    const int NV = nvars(s, pass);
    // (the geometry pass leaves MH_z itself: L sums and the two counts behind them)
    double *raw = pass == PASS_GEOM ? s.MH_z.get() : pass == PASS_SIMPLE ? s.rawS.get() : s.rawH.get();
    double *avg = pass == PASS_SIMPLE ? s.avgS.get() : s.avgH.get();
    hipLaunchKernelGGL(k_les_finish, dim3((unsigned)((s.L + 63) / 64)), dim3(64), 0, e->s_comp, gath, nranks, s.L, NV,
                       pass, s.MH_z.get(), s.avgS.get(), s.nvs, raw, avg);
    return e->launch_status("les diagnostics");
}

int gather_buffer(EngineBase *e, LesState &s, size_t n)
{
    if (n <= s.ngath) return CMDG_OK;
    s.ngath = 0;
    LESCHK(s.gath.alloc(n));
    s.ngath = n;
    return CMDG_OK;
}

// stage + (all-gather across an RCCL communicator) + finish of one pass of a single handle
int pass_single(EngineBase *e, LesState &s, int pass, const double *Q, double t)
{
    if (int r = stage(e, s, pass, Q, t)) return r;
    const size_t per = 2 * ((size_t)s.L * nvars(s, pass) + 2);
    if (e->transport == TRANSPORT_RCCL && e->nccl_comm) {
        if (int r = gather_buffer(e, s, per * e->nranks)) return r;
        if (int rc = rccl::AllGather(s.dd, s.gath, per, rccl::kDouble, e->nccl_comm, e->s_comp))
            return e->fail(CMDG_ERR_COMM, std::string("les diagnostics: ncclAllGather: ") + rccl::GetErrorString(rc));
        return finish(e, s, pass, s.gath, e->nranks);
    }
    return finish(e, s, pass, s.dd, 1);
}

// the same for the ranks of a local group: the partials travel through the host
int pass_group(cmdg_handle *handles, int n, int pass, const double *const *Q, double t)
{
    LesState &s0 = state(handles[0]->eng);
    const size_t per = 2 * ((size_t)s0.L * nvars(s0, pass) + 2);
    std::vector<double> all(per * n);
    for (int i = 0; i < n; ++i) {
        EngineBase *e = handles[i]->eng;
        LesState &s = state(e);
        if (int r = stage(e, s, pass, Q ? Q[i] : nullptr, t)) return r;
        LESCHK(hipMemcpyAsync(all.data() + per * i, s.dd, sizeof(double) * per, hipMemcpyDeviceToHost, e->s_comp));
    }
    for (int i = 0; i < n; ++i) {
        EngineBase *e = handles[i]->eng;
        LESCHK(hipStreamSynchronize(e->s_comp));
    }
    for (int i = 0; i < n; ++i) {
        EngineBase *e = handles[i]->eng;
        LesState &s = state(e);
        if (int r = gather_buffer(e, s, per * n)) return r;
        LESCHK(hipMemcpyAsync(s.gath, all.data(), sizeof(double) * per * n, hipMemcpyHostToDevice, e->s_comp));
        if (int r = finish(e, s, pass, s.gath, n)) return r;
        LESCHK(hipStreamSynchronize(e->s_comp));  // (`all` is pageable: the copy must have left it)
    }
    return CMDG_OK;
}

// zvals and Mvert = omega_k JcV[1, k, ev, eh = 1] (:781-788) of this rank, to the host
int levels_to_host(EngineBase *e, LesState &s, const double *omega)
{
    hipLaunchKernelGGL(k_les_levels, dim3((unsigned)((s.L + 63) / 64)), dim3(64), 0, e->s_comp, e->g.vgeo, e->g.nvgeo,
                       e->Np, e->NQ * e->NQ, e->NQV, s.nvert, s.nhorz, s.lev.get(), s.lev.get() + s.L);
    LESCHK(hipMemcpyAsync(s.host, s.lev, sizeof(double) * 2 * s.L, hipMemcpyDeviceToHost, e->s_comp));
    LESCHK(hipStreamSynchronize(e->s_comp));
    s.zvals.assign(s.host, s.host + s.L);
    s.Mvert.resize(s.L);
    for (int evk = 0; evk < s.L; ++evk) s.Mvert[evk] = (omega ? omega[evk % e->NQV] : 0.0) * s.host[s.L + evk];
    return CMDG_OK;
}

int init_outputs(EngineBase *e, LesState &s, double *zvals, double *MH_z)
{
    LESCHK(hipMemcpyAsync(s.host, s.MH_z, sizeof(double) * s.L, hipMemcpyDeviceToHost, e->s_comp));
    LESCHK(hipStreamSynchronize(e->s_comp));
    if (MH_z) memcpy(MH_z, s.host, sizeof(double) * s.L);
    if (zvals) memcpy(zvals, s.zvals.data(), sizeof(double) * s.L);
    s.inited = true;
    return CMDG_OK;
}

// the final copy-out of a collection and the scalars that need every level (host arithmetic in
// the reference's order)
int copy_out(EngineBase *e, LesState &s, const cmdg_les_result *out)
{
    const size_t nS = (size_t)s.L * s.nvs, nH = (size_t)s.L * s.nvh;
    double *h = s.host;
    LESCHK(hipMemcpyAsync(h, s.rawS, sizeof(double) * (nS + 2), hipMemcpyDeviceToHost, e->s_comp));
    LESCHK(hipMemcpyAsync(h + nS + 2, s.avgS, sizeof(double) * nS, hipMemcpyDeviceToHost, e->s_comp));
    LESCHK(hipMemcpyAsync(h + 2 * nS + 2, s.rawH, sizeof(double) * nH, hipMemcpyDeviceToHost, e->s_comp));
    LESCHK(hipMemcpyAsync(h + 2 * nS + 2 + nH, s.avgH, sizeof(double) * nH, hipMemcpyDeviceToHost, e->s_comp));
    LESCHK(hipStreamSynchronize(e->s_comp));
    const double *rawS = h, *avgS = h + nS + 2, *rawH = h + 2 * nS + 2, *avgH = rawH + nH;
    const int ns = s.nsimple();
    for (int evk = 0; evk < s.L; ++evk) {
        if (out->simple_sums) memcpy(out->simple_sums + (size_t)evk * ns, rawS + (size_t)evk * s.nvs, sizeof(double) * ns);
        if (out->simple_avgs) memcpy(out->simple_avgs + (size_t)evk * ns, avgS + (size_t)evk * s.nvs, sizeof(double) * ns);
    }
    if (out->ho_sums) memcpy(out->ho_sums, rawH, sizeof(double) * nH);
    if (out->ho_avgs) memcpy(out->ho_avgs, avgH, sizeof(double) * nH);
    if (!s.moist) return CMDG_OK;
    const double ncover = rawS[nS], ncol = rawS[nS + 1];
    double top = -100000.0, base = 100000.0, lwp = 0.0, iwp = 0.0;  // ("In honor of PyCLES!", :626-628)
    for (int evk = 0; evk < s.L; ++evk) {
        const double *r = rawS + (size_t)evk * s.nvs, *a = avgS + (size_t)evk * s.nvs;
        if (r[A_COUNT] > 0.0) {
            top = std::max(top, s.zvals[evk]);
            base = std::min(base, s.zvals[evk]);
        }
        lwp += a[A_LIQ2] * s.Mvert[evk];
        iwp += a[A_ICE2] * s.Mvert[evk];
        if (out->cloud_levels) {
            double *c = out->cloud_levels + 6 * (size_t)evk;
            c[0] = r[A_COUNT];
            c[1] = ncol;
            c[2] = r[A_LIQ2];
            c[3] = r[A_ICE2];
            c[4] = a[A_LIQ2];
            c[5] = a[A_ICE2];
        }
    }
    if (out->cloud_scalars) {
        double *c = out->cloud_scalars;
        c[0] = top == -100000.0 ? NAN : top;
        c[1] = base == 100000.0 ? NAN : base;
        c[2] = ncover / ncol;
        c[3] = lwp;
        c[4] = iwp;
        c[5] = ncover;
        c[6] = ncol;
        c[7] = 0.0;
    }
    return CMDG_OK;
}

int check_group(cmdg_handle *handles, int n, const char *who)
{
    for (int i = 0; i < n; ++i) {
        EngineBase *e = handles[i]->eng;
        if (n > 1 && (e->transport != TRANSPORT_LOCAL || e->nranks != n || e->rank != i))
            return e->fail(CMDG_ERR_INVALID, std::string(who) + ": handle i must be rank i of one group of n "
                                                                "connected with cmdg_comm_connect_local");
    }
    return CMDG_OK;
}

int refuse_group_member(EngineBase *e, const char *who)
{
    if (e->transport == TRANSPORT_LOCAL && e->nranks > 1)
        return e->fail(CMDG_ERR_INVALID, std::string(who) + ": the handle is one rank of a local-transport group; "
                                                            "use the cmdg_group_les_* form");
    return CMDG_OK;
}

// what the three GCM entries refuse before they ask the engine
int gcm_refusals(EngineBase *e, const char *who)
{
    if (e->fv || e->NQV < 2)
        return e->fail(CMDG_ERR_UNSUPPORTED, std::string(who) + ": a DGFVModel handle (vertical polynomial order "
                                                                "0) has no vertical derivative matrix");
    if (e->esdg) return e->fail(CMDG_ERR_UNSUPPORTED, std::string(who) + ": not served for an ESDGModel handle");
    return CMDG_OK;
}

// the launch status, then the wait: the entries return when their output is ready
int gcm_done(cmdg_handle h, const char *who)
{
    EngineBase *e = h->eng;
    if (int r = e->launch_status(who)) return set_err(h, r);
    if (hipStreamSynchronize(e->s_comp) != hipSuccess)
        return set_err(h, e->fail(CMDG_ERR_HIP, std::string(who) + ": the kernel failed"));
    return CMDG_OK;
}

}  // namespace

void les_release(EngineBase *e)
{
    std::lock_guard<std::mutex> lk(g_les_m);
    auto it = g_les.find(e);
    if (it == g_les.end()) return;
    if (it->second.host) (void)hipHostFree(it->second.host);
    g_les.erase(it);  // (frees the device buffers)
}

}  // namespace cmdg

using namespace cmdg;

extern "C" {

int cmdg_les_query(cmdg_handle h, int32_t nvertelem, int32_t *out)
{
    if (!h || !out) return CMDG_ERR_INVALID;
    DevGuard guard_(h->eng);
    LesState tmp;
    if (int r = setup(h->eng, tmp, nvertelem)) return set_err(h, r);
    out[0] = tmp.nd;
    out[1] = tmp.nsimple();
    out[2] = tmp.nvh;
    out[3] = tmp.L;
    return CMDG_OK;
}

int cmdg_les_nodal(cmdg_handle h, const double *Q, double t, double *D)
{
    if (!h) return CMDG_ERR_INVALID;
    DevGuard guard_(h->eng);
    EngineBase *e = h->eng;
    if (!Q || !D) return set_err(h, e->fail(CMDG_ERR_INVALID, "cmdg_les_nodal: Q or D is NULL"));
    int nd, moist;
    if (int r = e->launch_les_nodal(Q, t, D, &nd, &moist)) return set_err(h, r);
    if (int r = e->launch_status("cmdg_les_nodal")) return set_err(h, r);
    if (hipStreamSynchronize(e->s_comp) != hipSuccess)
        return set_err(h, e->fail(CMDG_ERR_HIP, "cmdg_les_nodal: the nodal pass failed"));
    return CMDG_OK;
}

int cmdg_les_init(cmdg_handle h, int32_t nvertelem, const double *omega, double *zvals, double *MH_z)
{
    if (!h) return CMDG_ERR_INVALID;
    DevGuard guard_(h->eng);
    EngineBase *e = h->eng;
    if (int r = refuse_group_member(e, "cmdg_les_init")) return set_err(h, r);
    LesState &s = state(e);
    s.inited = false;
    if (int r = setup(e, s, nvertelem)) return set_err(h, r);
    if (int r = alloc_buffers(e, s)) return set_err(h, r);
    if (int r = pass_single(e, s, PASS_GEOM, nullptr, 0.0)) return set_err(h, r);
    if (int r = levels_to_host(e, s, omega)) return set_err(h, r);
    return set_err(h, init_outputs(e, s, zvals, MH_z));
}

int cmdg_les_collect(cmdg_handle h, const double *Q, double t, const cmdg_les_result *out)
{
    if (!h) return CMDG_ERR_INVALID;
    DevGuard guard_(h->eng);
    EngineBase *e = h->eng;
    if (int r = refuse_group_member(e, "cmdg_les_collect")) return set_err(h, r);
    LesState &s = state(e);
    if (!s.inited)
        return set_err(h, e->fail(CMDG_ERR_INVALID, "cmdg_les_collect: cmdg_les_init has not run on this handle"));
    if (!Q || !out) return set_err(h, e->fail(CMDG_ERR_INVALID, "cmdg_les_collect: Q or out is NULL"));
    if (int r = pass_single(e, s, PASS_SIMPLE, Q, t)) return set_err(h, r);
    if (int r = pass_single(e, s, PASS_HO, Q, t)) return set_err(h, r);
    return set_err(h, copy_out(e, s, out));
}

int cmdg_group_les_init(cmdg_handle *handles, int32_t n, int32_t nvertelem, const double *omega, double *zvals,
                        double *MH_z)
{
    GroupCall gc(handles, n);
    if (!gc.ok()) return CMDG_ERR_INVALID;
    if (int r = check_group(handles, n, "cmdg_group_les_init")) return gc.finish(r);
    for (int i = 0; i < n; ++i) {
        EngineBase *e = handles[i]->eng;
        LesState &s = state(e);
        s.inited = false;
        if (int r = setup(e, s, nvertelem)) return gc.finish(r);
        if (s.nd != state(handles[0]->eng).nd || s.L != state(handles[0]->eng).L)
            return gc.finish(e->fail(CMDG_ERR_INVALID, "cmdg_group_les_init: the ranks differ in law or levels"));
        if (int r = alloc_buffers(e, s)) return gc.finish(r);
    }
    if (int r = pass_group(handles, n, PASS_GEOM, nullptr, 0.0)) return gc.finish(r);
    for (int i = n - 1; i >= 0; --i) {  // (rank 0 last: its zvals and MH_z are the ones returned)
        EngineBase *e = handles[i]->eng;
        LesState &s = state(e);
        if (int r = levels_to_host(e, s, omega)) return gc.finish(r);
        if (int r = init_outputs(e, s, zvals, MH_z)) return gc.finish(r);
    }
    return CMDG_OK;
}

int cmdg_group_les_collect(cmdg_handle *handles, int32_t n, const double *const *Q, double t,
                           const cmdg_les_result *out)
{
    if (!Q || !out) return CMDG_ERR_INVALID;
    GroupCall gc(handles, n);
    if (!gc.ok()) return CMDG_ERR_INVALID;
    if (int r = check_group(handles, n, "cmdg_group_les_collect")) return gc.finish(r);
    for (int i = 0; i < n; ++i) {
        EngineBase *e = handles[i]->eng;
        if (!state(e).inited)
            return gc.finish(e->fail(CMDG_ERR_INVALID, "cmdg_group_les_collect: cmdg_group_les_init has not run on "
                                                       "these handles"));
        if (!Q[i]) return gc.finish(e->fail(CMDG_ERR_INVALID, "cmdg_group_les_collect: a NULL state array"));
    }
    if (int r = pass_group(handles, n, PASS_SIMPLE, Q, t)) return gc.finish(r);
    if (int r = pass_group(handles, n, PASS_HO, Q, t)) return gc.finish(r);
    return gc.finish(copy_out(handles[0]->eng, state(handles[0]->eng), out));
}

// ---- AtmosGCMDefault diagnostics: VectorGradients, Vorticity, the nodal pass -----------------------
// (the kernels need the order, and the nodal pass the law: kernels.h, launched by EngineT)
int cmdg_vector_gradients(cmdg_handle h, const double *Q, double *vgrad)
{
    if (!h) return CMDG_ERR_INVALID;
    DevGuard guard_(h->eng);
    EngineBase *e = h->eng;
    if (!Q || !vgrad) return set_err(h, e->fail(CMDG_ERR_INVALID, "cmdg_vector_gradients: Q or vgrad is NULL"));
    if (int r = gcm_refusals(e, "cmdg_vector_gradients")) return set_err(h, r);
    if (int r = e->launch_vector_gradients(Q, vgrad)) return set_err(h, r);
    return gcm_done(h, "cmdg_vector_gradients");
}

int cmdg_vorticity(cmdg_handle h, const double *vgrad, double *vort)
{
    if (!h) return CMDG_ERR_INVALID;
    DevGuard guard_(h->eng);
    EngineBase *e = h->eng;
    if (!vgrad || !vort) return set_err(h, e->fail(CMDG_ERR_INVALID, "cmdg_vorticity: vgrad or vort is NULL"));
    if (int r = gcm_refusals(e, "cmdg_vorticity")) return set_err(h, r);
    const int64_t n = e->nreal * e->Np;
    if (n > 0)
        hipLaunchKernelGGL(k_vorticity, dim3(nblocks(n)), dim3(256), 0, e->s_comp, vgrad, vort, e->Np, n);
    return gcm_done(h, "cmdg_vorticity");
}

int cmdg_gcm_nodal(cmdg_handle h, const double *Q, double t, double *G, double *u)
{
    if (!h) return CMDG_ERR_INVALID;
    DevGuard guard_(h->eng);
    EngineBase *e = h->eng;
    if (!Q || !G || !u) return set_err(h, e->fail(CMDG_ERR_INVALID, "cmdg_gcm_nodal: Q, G or u is NULL"));
    if (int r = gcm_refusals(e, "cmdg_gcm_nodal")) return set_err(h, r);
    if (int r = e->launch_gcm_nodal(Q, t, G, u)) return set_err(h, r);
    return gcm_done(h, "cmdg_gcm_nodal");
}

}  // extern "C"
