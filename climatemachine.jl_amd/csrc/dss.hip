// Direct stiffness summation, dss!(Q, grid) of src/Numerics/Mesh/DSS.jl.
//
// The reference's device kernel gives one thread a whole vertex, edge or face and loops over the
// states inside it: neighbouring threads then run different loops over different tables and touch
// unrelated addresses.  Here the host flattens every shared node into a group of (element base, node)
// members (dss_tables.h) and one lane owns one group: it gathers the members in the reference's
// order, adds them starting from -0.0 and scatters the sum to every member.  Groups are disjoint
// (checked at create), so the in-place update needs no atomics, and additions in a fixed order are
// all there is: the result equals the reference's host loops bit for bit, in every run.
//
// A wave holds groups of one member count (uniform trip count) and, for faces -- seven in ten of
// the groups at N = 4 -- the interior nodes of one face on consecutive lanes, so its loads and stores
// fall into runs of one (state, element) row.  The member indices are loaded once, [member][lane] so
// that the load is coalesced, and stay in registers over the loop over states; groups of more than
// REG members (vertices of high valence) walk their list per state instead.  (Taking several states
// at a time, to have their loads in flight together, was measured: 0.312 against 0.317 ms on the
// benchmark sphere at half the occupancy, so the loop stays plain.)
#include <string.h>

#include <optional>
#include <vector>

#include "dss_tables.h"
#include "engine_base.h"

namespace cmdg {

namespace {
constexpr int NT = 256;  // four waves per work-group
constexpr int REG = 8;   // members whose offsets are kept in registers
static_assert(NT % DSS_WAVE == 0, "whole waves per work-group");

template <int N>
__device__ __forceinline__ void dss_fixed(const DssMember *__restrict__ m, double *__restrict__ Q, int nstate, int Np)
{
    int64_t at[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const DssMember mj = m[j * DSS_WAVE];
        at[j] = (int64_t)mj.elbase * nstate + mj.node;
    }
    for (int s = 0; s < nstate; ++s) {
        double *Qs = Q + (int64_t)s * Np;
        double v[N];
#pragma unroll
        for (int j = 0; j < N; ++j) v[j] = Qs[at[j]];
        double sum = -0.0;
#pragma unroll
        for (int j = 0; j < N; ++j) sum += v[j];
#pragma unroll
        for (int j = 0; j < N; ++j) Qs[at[j]] = sum;
    }
}

__global__ __launch_bounds__(NT) void k_dss(const DssWave *__restrict__ waves, const DssMember *__restrict__ members,
                                            double *__restrict__ Q, int nstate, int Np, int64_t nwaves)
{
    const int64_t w = (int64_t)blockIdx.x * (NT / DSS_WAVE) + threadIdx.x / DSS_WAVE;
    const int lane = threadIdx.x % DSS_WAVE;
    if (w >= nwaves) return;
    const DssWave wd = waves[w];  // the same for the whole wave
    if (lane >= wd.lanes) return;
    const DssMember *m = members + wd.moff + lane;
    switch (wd.n) {
    case 1: dss_fixed<1>(m, Q, nstate, Np); return;
    case 2: dss_fixed<2>(m, Q, nstate, Np); return;
    case 3: dss_fixed<3>(m, Q, nstate, Np); return;
    case 4: dss_fixed<4>(m, Q, nstate, Np); return;
    case 5: dss_fixed<5>(m, Q, nstate, Np); return;
    case 6: dss_fixed<6>(m, Q, nstate, Np); return;
    case 7: dss_fixed<7>(m, Q, nstate, Np); return;
    case 8: dss_fixed<REG>(m, Q, nstate, Np); return;
    default: break;
    }
    for (int s = 0; s < nstate; ++s) {
        double *Qs = Q + (int64_t)s * Np;
        double sum = -0.0;
        for (int j = 0; j < wd.n; ++j) {
            const DssMember mj = m[(int64_t)j * DSS_WAVE];
            sum += Qs[(int64_t)mj.elbase * nstate + mj.node];
        }
        for (int j = 0; j < wd.n; ++j) {
            const DssMember mj = m[(int64_t)j * DSS_WAVE];
            Qs[(int64_t)mj.elbase * nstate + mj.node] = sum;
        }
    }
}
}  // namespace

struct DssObj {
    int dev = 0;
    int Np = 0;
    int64_t nelem = 0, nwaves = 0;
    int64_t info[4] = {0, 0, 0, 0};
    DevBuf<DssWave> waves;
    DevBuf<DssMember> members;
};

namespace {
int dss_create(const cmdg_dss_desc *d, DssObj **out, std::string &err)
{
    *out = nullptr;
    DssTables t;
    if (int r = dss_flatten(d, t, err)) return r;
    DssObj *o = new DssObj;
    (void)hipGetDevice(&o->dev);
    o->Np = t.Np;
    o->nelem = t.nelem;
    o->nwaves = (int64_t)t.waves.size();
    memcpy(o->info, t.info, sizeof(o->info));
    bool ok = true;
    if (o->nwaves > 0) {
        ok = o->waves.alloc(t.waves.size()) == hipSuccess && o->members.alloc(t.members.size()) == hipSuccess &&
             hipMemcpy(o->waves, t.waves.data(), t.waves.size() * sizeof(DssWave), hipMemcpyHostToDevice) == hipSuccess &&
             hipMemcpy(o->members, t.members.data(), t.members.size() * sizeof(DssMember), hipMemcpyHostToDevice) ==
                 hipSuccess;
    }
    if (!ok) {
        (void)hipGetLastError();
        delete o;
        err = "cmdg_dss_create: device allocation or copy failed";
        return CMDG_ERR_HIP;
    }
    *out = o;
    return CMDG_OK;
}

// enqueue the summation on st; wait for it if asked
int dss_apply(const DssObj *o, double *Q, int nstate, hipStream_t st, bool wait, std::string &err)
{
    if (o->nwaves > 0) {
        const int64_t nblocks = (o->nwaves + NT / DSS_WAVE - 1) / (NT / DSS_WAVE);
        hipLaunchKernelGGL(k_dss, dim3((unsigned)nblocks), dim3(NT), 0, st, o->waves, o->members, Q, nstate, o->Np,
                           o->nwaves);
    }
    hipError_t r = hipGetLastError();
    if (r == hipSuccess && wait) r = hipStreamSynchronize(st);
    if (r != hipSuccess) {
        err = std::string("cmdg_dss_apply: ") + hipGetErrorString(r);
        return CMDG_ERR_HIP;
    }
    return CMDG_OK;
}

// the object must be of the handle's grid and device before the handle's exchange maps serve its array
int dss_fits(EngineBase *e, const DssObj *o)
{
    if (e->dev != o->dev) return e->fail(CMDG_ERR_INVALID, "cmdg_dss: the object lives on another device than the handle");
    if (e->Np != o->Np || e->nelem != o->nelem)
        return e->fail(
            CMDG_ERR_INVALID, "cmdg_dss: the object is of a grid with Np = " + std::to_string(o->Np) + ", " +
                                  std::to_string(o->nelem) + " elements; the handle has Np = " + std::to_string(e->Np) +
                                  ", " + std::to_string(e->nelem));
    return CMDG_OK;
}
}  // namespace

}  // namespace cmdg

// ---- the C entries ------------------------------------------------------------------------------
using namespace cmdg;

extern "C" {

int cmdg_dss_create(cmdg_handle h, const cmdg_dss_desc *d, cmdg_dss_t *out)
{
    if (!d || !out) return CMDG_ERR_INVALID;
    std::optional<DevGuard> guard_;
    if (h) guard_.emplace(h->eng);
    DssObj *o = nullptr;
    std::string err;
    const int r = dss_create(d, &o, err);
    *out = reinterpret_cast<cmdg_dss_t>(o);
    return object_call_done(h, r, err);
}

int cmdg_dss_destroy(cmdg_handle h, cmdg_dss_t dss)
{
    if (!dss) return CMDG_ERR_INVALID;
    DssObj *o = reinterpret_cast<DssObj *>(dss);
    std::optional<DevGuard> guard_;
    if (h) {
        guard_.emplace(h->eng);
        h->eng->synchronize();
    }
    ObjectDevice dev_(o->dev);
    (void)hipStreamSynchronize(nullptr);  // (calls without a handle have returned; see include/cmdg.h)
    delete o;
    return CMDG_OK;
}

int cmdg_dss_info(cmdg_dss_t dss, int64_t out[4])
{
    if (!dss || !out) return CMDG_ERR_INVALID;
    memcpy(out, reinterpret_cast<const DssObj *>(dss)->info, 4 * sizeof(int64_t));
    return CMDG_OK;
}

int cmdg_dss_apply(cmdg_handle h, cmdg_dss_t dss, double *Q, int32_t nstate)
{
    if (!dss || !Q || nstate < 1) return CMDG_ERR_INVALID;
    const DssObj *o = reinterpret_cast<const DssObj *>(dss);
    std::optional<DevGuard> guard_;
    if (h) guard_.emplace(h->eng);
    std::string err;
    if (h && h->eng->dev != o->dev)
        return object_call_done(h, CMDG_ERR_INVALID, "cmdg_dss_apply: the object lives on another device than the handle");
    ObjectDevice dev_(o->dev);
    return object_call_done(h, dss_apply(o, Q, nstate, h ? h->eng->s_comp : nullptr, !h, err), err);
}

int cmdg_dss(cmdg_handle h, cmdg_dss_t dss, double *Q, int32_t nstate)
{
    if (!dss || !Q || nstate < 1) return CMDG_ERR_INVALID;
    if (!h) {
        set_create_err("cmdg_dss: the ghost exchange needs a handle (cmdg_dss_apply sums without one)");
        return CMDG_ERR_INVALID;
    }
    const DssObj *o = reinterpret_cast<const DssObj *>(dss);
    DevGuard guard_(h->eng);
    EngineBase *e = h->eng;
    if (int r = dss_fits(e, o)) return set_err(h, r);
    e->invalidate_sends();  // the caller's array: always packed
    if (int r = e->halo_begin(SLOT_Q, Q, nstate)) return set_err(h, r);
    if (int r = e->halo_end(SLOT_Q, Q, nstate)) return set_err(h, r);  // (the compute stream waits for the ghosts)
    std::string err;
    if (int r = dss_apply(o, Q, nstate, e->s_comp, false, err)) return set_err(h, e->fail(r, err));
    return set_err(h, e->synchronize());
}

int cmdg_group_dss(cmdg_handle *handles, int32_t n, const cmdg_dss_t *dss, double **Q, int32_t nstate)
{
    if (!dss || !Q || nstate < 1) return CMDG_ERR_INVALID;
    for (int i = 0; i < n; ++i)
        if (!dss[i] || !Q[i]) return CMDG_ERR_INVALID;
    GroupCall gc(handles, n);
    if (!gc.ok()) return CMDG_ERR_INVALID;
    const DssObj *const *o = reinterpret_cast<const DssObj *const *>(dss);
    for (int i = 0; i < n; ++i)
        if (int r = dss_fits(handles[i]->eng, o[i])) return gc.finish(r);
    for (int i = 0; i < n; ++i) handles[i]->eng->invalidate_sends();
    for (int i = 0; i < n; ++i)
        if (int r = handles[i]->eng->halo_begin(SLOT_Q, Q[i], nstate)) return gc.finish(r);
    for (int i = 0; i < n; ++i)
        if (int r = handles[i]->eng->halo_end(SLOT_Q, Q[i], nstate)) return gc.finish(r);
    std::string err;
    for (int i = 0; i < n; ++i)
        if (int r = dss_apply(o[i], Q[i], nstate, handles[i]->eng->s_comp, false, err))
            return gc.finish(handles[i]->eng->fail(r, err));
    for (int i = 0; i < n; ++i)
        if (int r = handles[i]->eng->synchronize()) return gc.finish(r);
    return CMDG_OK;
}

}  // extern "C"
