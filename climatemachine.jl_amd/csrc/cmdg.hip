// libcmdg: engine orchestration + the C ABI declared in include/cmdg.h.
#include <dlfcn.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <new>
#include <tuple>

#include "stepping.h"
#include "reductions.h"
#include "interpolation.h"

namespace cmdg {

// ---- RCCL, resolved lazily so that single-GPU use has no link-time dependency -------
namespace rccl {
typedef struct { char internal[128]; } uid_t;
typedef int (*GetUniqueId_t)(uid_t *);
typedef int (*CommInitRank_t)(void **, int, uid_t, int);
typedef int (*CommDestroy_t)(void *);
typedef int (*GroupStart_t)();
typedef int (*GroupEnd_t)();
typedef int (*Send_t)(const void *, size_t, int, int, void *, hipStream_t);
typedef int (*Recv_t)(void *, size_t, int, int, void *, hipStream_t);
typedef const char *(*GetErrorString_t)(int);
typedef int (*AllGather_t)(const void *, void *, size_t, int, void *, hipStream_t);
static void *lib = nullptr;
static GetUniqueId_t GetUniqueId;
static CommInitRank_t CommInitRank;
static CommDestroy_t CommDestroy;
static GroupStart_t GroupStart;
static GroupEnd_t GroupEnd;
static Send_t Send;
static Recv_t Recv;
static GetErrorString_t GetErrorString;
static AllGather_t AllGather;
constexpr int kDouble = 8;  // ncclFloat64 / ncclDouble
static bool load(std::string &err)
{
    if (lib) return true;
    // one RCCL instance per process: the path the caller names (CMDG_RCCL_LIB, e.g. the copy
    // torch ships and has loaded already), else whatever is loaded, else the system library
    const char *names[] = {"librccl.so.1", "librccl.so", nullptr};
    if (const char *p = getenv("CMDG_RCCL_LIB"))
        if (*p) lib = dlopen(p, RTLD_NOW | RTLD_GLOBAL);
    for (int i = 0; names[i] && !lib; ++i) lib = dlopen(names[i], RTLD_NOW | RTLD_GLOBAL | RTLD_NOLOAD);
    for (int i = 0; names[i] && !lib; ++i) lib = dlopen(names[i], RTLD_NOW | RTLD_GLOBAL);
    if (!lib) {
        err = std::string("cannot load librccl: ") + dlerror();
        return false;
    }
#define SYM(n)                                                \
    n = (n##_t)dlsym(lib, "nccl" #n);                         \
    if (!n) {                                                 \
        err = "librccl lacks nccl" #n;                        \
        return false;                                         \
    }
    SYM(GetUniqueId) SYM(CommInitRank) SYM(CommDestroy) SYM(GroupStart) SYM(GroupEnd) SYM(Send)
        SYM(Recv) SYM(GetErrorString) SYM(AllGather)
#undef SYM
    return true;
}
}  // namespace rccl

// ---- roctx, resolved lazily: ranges cost nothing when nobody listens ----------------------
namespace {
typedef int (*roctx_push_t)(const char *);
typedef int (*roctx_pop_t)();
roctx_push_t g_roctx_push = nullptr;
roctx_pop_t g_roctx_pop = nullptr;
int g_roctx_state = 0;  // 0 not tried, 1 available, -1 absent
void roctx_resolve()
{
    g_roctx_state = -1;
    const char *names[] = {"librocprofiler-sdk-roctx.so.1", "librocprofiler-sdk-roctx.so", "libroctx64.so.4",
                           "libroctx64.so", nullptr};
    const char *want = getenv("CMDG_ROCTX");
    void *lib = nullptr;
    for (int i = 0; names[i] && !lib; ++i) lib = dlopen(names[i], RTLD_NOW | RTLD_NOLOAD);
    if (!lib && want && *want && *want != '0')
        for (int i = 0; names[i] && !lib; ++i) lib = dlopen(names[i], RTLD_NOW | RTLD_GLOBAL);
    if (!lib) return;
    g_roctx_push = (roctx_push_t)dlsym(lib, "roctxRangePushA");
    g_roctx_pop = (roctx_pop_t)dlsym(lib, "roctxRangePop");
    if (g_roctx_push && g_roctx_pop) g_roctx_state = 1;
}
}  // namespace
void roctx_push(const char *name)
{
    if (g_roctx_state == 0) roctx_resolve();
    if (g_roctx_state == 1) g_roctx_push(name);
}
void roctx_pop()
{
    if (g_roctx_state == 1) g_roctx_pop();
}

int dbg_sync()
{
    static const int v = [] {
        const char *p = getenv("CMDG_DBG_SYNC");
        return p ? atoi(p) : 0;
    }();
    return v;
}

hipError_t ev_record(hipEvent_t e, hipStream_t s) { return hipEventRecord(e, s); }

int EngineBase::launch_status(const char *what)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(CMDG_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
    return CMDG_OK;
}

int EngineBase::order(hipStream_t earlier, hipStream_t later)
{
    if (earlier == later) return CMDG_OK;
    if (dbg_sync() & 1) (void)hipStreamSynchronize(earlier);
    if (ev_record(ev_comp, earlier) != hipSuccess || hipStreamWaitEvent(later, ev_comp, 0) != hipSuccess)
        return fail(CMDG_ERR_HIP, "stream ordering failed");
    return CMDG_OK;
}

int EngineBase::ensure_Imat(const double *host)
{
    if (d_Imat) return CMDG_OK;
    if (!host) return fail(CMDG_ERR_INVALID, "Imat is NULL");
    if (d_Imat.alloc(NQ * NQ) != hipSuccess ||
        hipMemcpy(d_Imat, host, sizeof(double) * NQ * NQ, hipMemcpyHostToDevice) != hipSuccess)
        return fail(CMDG_ERR_HIP, "Imat upload failed");
    return CMDG_OK;
}

int set_err(cmdg_handle h, int code)
{
    if (h && h->eng && code != CMDG_OK) h->err = h->eng->err;
    return code;
}

GroupCall::GroupCall(cmdg_handle *h, cmdg_handle *h2, int n, bool pairs)
{
    if (!h || (pairs && !h2) || n < 1) return;
    for (int i = 0; i < n; ++i)
        if (!h[i] || (pairs && !h2[i])) return;
    for (int i = 0; i < n; ++i) {  // (members in order, each with the prefix of its message)
        const std::string r = std::to_string(i);
        members.push_back({h[i], pairs ? "pair " + r + " (slow): " : "rank " + r + ": "});
        if (pairs) members.push_back({h2[i], "pair " + r + " (fast): "});
    }
    for (auto &m : members) {
        if (m.first->eng->worker) m.first->eng->worker->wait_idle();
        m.first->eng->err.clear();
    }
    dev.emplace(h[0]->eng);
}

GroupCall::GroupCall(const std::vector<std::pair<cmdg_handle, std::string>> &named)
{
    if (named.empty()) return;
    for (auto &m : named)
        if (!m.first) return;
    for (auto &m : named) {
        bool merged = false;
        for (auto &have : members)
            if (have.first == m.first) {
                have.second = have.second.substr(0, have.second.size() - 2) + " / " + m.second + ": ";
                merged = true;
            }
        if (!merged) members.push_back({m.first, m.second + ": "});
    }
    for (auto &m : members) {
        if (m.first->eng->worker) m.first->eng->worker->wait_idle();
        m.first->eng->err.clear();
    }
    dev.emplace(named[0].first->eng);
}

int GroupCall::finish(int rc)
{
    if (rc == CMDG_OK) return rc;
    std::string msg = cmdg_status_string(rc);
    for (auto &m : members)
        if (!m.first->eng->err.empty()) {
            msg = m.second + m.first->eng->err;
            break;
        }
    for (auto &m : members) m.first->err = msg;
    return rc;
}

// ---------------------------------------------------------------------------------
// What has an order; the members' destructors free everything else, the two streams last.
EngineBase::~EngineBase()
{
    delete worker;  // (drains its queue first)
    worker = nullptr;
    if (s_comp) hipStreamSynchronize(s_comp);
    if (s_comm) hipStreamSynchronize(s_comm);
    prof_collect();
    if (graph_exec) hipGraphExecDestroy(graph_exec);
    if (nccl_comm && rccl::CommDestroy) rccl::CommDestroy(nccl_comm);
}

int EngineBase::init(const cmdg_desc *d)
{
    Np = NQ * NQ * NQV;
    Nfp = NQ * (NQ > NQV ? NQ : NQV);  // Nfp_max, the stride of the face tables
    if (d->N[0] != d->N[1] || d->N[0] != NQ - 1 || d->N[2] != NQV - 1)
        return fail(CMDG_ERR_INVALID, "cmdg_create: polynomial orders do not match the engine");
    if (NQV != NQ && !d->Dv)
        return fail(CMDG_ERR_INVALID, "cmdg_create: Dv is required when the vertical order differs");
    nreal = d->nreal;
    nghost = d->nghost;
    nelem = nreal + nghost;
    nf_first = d->nf_first;
    direction = d->direction;
    diffusion_direction = d->diffusion_direction;
    stacked = d->stacked;
    if (!d->vgeo || !d->sgeo || !d->vmapM || !d->vmapP || !d->elemtobndy || !d->D ||
        !d->state_auxiliary)
        return fail(CMDG_ERR_INVALID, "cmdg_create: a required grid/state pointer is NULL");
    if (d->nvgeo < 11) return fail(CMDG_ERR_INVALID, "cmdg_create: vgeo needs >= 11 columns");
    if (d->ninterior + d->nexterior != nreal)
        return fail(CMDG_ERR_INVALID, "cmdg_create: interior + exterior != nreal");
    if ((d->ninterior > 0 && !d->interiorelems) || (d->nexterior > 0 && !d->exteriorelems))
        return fail(CMDG_ERR_INVALID, "cmdg_create: element list pointer is NULL");
    if (direction < 0 || direction > 2 || diffusion_direction < 0 || diffusion_direction > 2)
        return fail(CMDG_ERR_INVALID, "cmdg_create: bad direction");
    g.vgeo = d->vgeo;
    g.sgeo = d->sgeo;
    g.vmapM = d->vmapM;
    g.vmapP = d->vmapP;
    g.elemtobndy = d->elemtobndy;
    g.nvgeo = d->nvgeo;
    d_interior = d_interior_user = d->interiorelems;
    ninterior = d->ninterior;
    d_exterior = d_exterior_user = d->exteriorelems;
    nexterior = d->nexterior;
    d_activedofs = d->activedofs;
    d_vmapsend = d->vmapsend;
    nvmapsend = d->nvmapsend;
    d_vmaprecv = d->vmaprecv;
    nvmaprecv = d->nvmaprecv;
    if (d->nnabr > 0) {
        if (!d->nabrtorank || !d->nabrtovmapsend || !d->nabrtovmaprecv || !d->vmapsend ||
            !d->vmaprecv)
            return fail(CMDG_ERR_INVALID, "cmdg_create: halo tables missing");
        nabrtorank.assign(d->nabrtorank, d->nabrtorank + d->nnabr);
        nabrsend.assign(d->nabrtovmapsend, d->nabrtovmapsend + 2 * d->nnabr);
        nabrrecv.assign(d->nabrtovmaprecv, d->nabrtovmaprecv + 2 * d->nnabr);
    }
    HIPCHK(hipGetDevice(&dev));
    HIPCHK(s_comp.create(hipStreamNonBlocking));
    {
        // CMDG_HALO_PRIORITY=1: the halo stream (the latency chain of a partitioned run: exchange ->
        // exterior launch -> exchange ...) as a high-priority stream, so that its small kernels go
        // ahead of the interior launches' blocks.  Off by default: it gains nothing measurable at
        // 5 400 elements per rank (profiles/r03_halo_exposure_*).  The two-rank local-transport
        // failure once seen with both models of the split-explicit ocean on priority streams was a
        // hipMemset of the work states not ordered before the first stage, not the priorities
        // (scripts/probe/memset_null_stream_order.py); every fill now goes on s_comp.
        int lo = 0, hi = 0;
        const char *pv = getenv("CMDG_HALO_PRIORITY");
        if (communicate() && pv && *pv == '1' && hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess && hi < lo)
            HIPCHK(s_comm.create(hipStreamNonBlocking, hi));
        else
            HIPCHK(s_comm.create(hipStreamNonBlocking));
    }
    for (int i = 0; i < 2; ++i) {
        HIPCHK(ev_int[i].create(hipEventDisableTiming));
        HIPCHK(ev_ext[i].create(hipEventDisableTiming));
    }
    HIPCHK(gev_fork.create(hipEventDisableTiming));
    if (const char *v = getenv("CMDG_STEP_GRAPH")) step_graph = *v && *v != '0';
    HIPCHK(ev_comp.create(hipEventDisableTiming));
    HIPCHK(d_D.alloc(NQ * NQ));
    HIPCHK(hipMemcpy(d_D, d->D, sizeof(double) * NQ * NQ, hipMemcpyHostToDevice));
    g.D = d_D;
    g.Dv = d_D;
    if (NQV != NQ) {
        HIPCHK(d_Dv.alloc(NQV * NQV));
        HIPCHK(hipMemcpy(d_Dv, d->Dv, sizeof(double) * NQV * NQV, hipMemcpyHostToDevice));
        g.Dv = d_Dv;
    }
    {
        // digest of the face tables: one pass over the reference's arrays, checked as it goes
        const int NFT = 4 * NQ * NQV + 2 * NQ * NQ;
        const int64_t nt = std::max<int64_t>(nreal, 1) * NFT;
        DevBuf<int> d_bad;
        int bad = 0;
        HIPCHK(d_faceP.alloc(nt));
        HIPCHK(d_faceG.alloc(4 * nt));
        HIPCHK(d_bad.alloc_zeroed(1, s_comp));  // (stream-ordered before the digest, see below)
        if (nreal > 0)
            hipLaunchKernelGGL(k_face_digest, dim3((unsigned)((nreal * NFT + 255) / 256)), dim3(256), 0,
                               s_comp, g.vgeo, g.nvgeo, g.sgeo, g.vmapM, g.vmapP, g.elemtobndy, NQ,
                               NQV, nreal, d_faceP.get(), d_faceG.get(), d_bad.get());
        hipError_t le = hipGetLastError();
        hipError_t ce = hipMemcpyAsync(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, s_comp);
        hipError_t se = hipStreamSynchronize(s_comp);
        d_bad.reset();
        if (le != hipSuccess || ce != hipSuccess || se != hipSuccess)
            return fail(CMDG_ERR_HIP, "cmdg_create: digest of the face tables failed");
        if (bad & 1)
            return fail(CMDG_ERR_INVALID, "cmdg_create: vmapM is not the face numbering of Grids.jl:586-594");
        if (bad & 2)
            return fail(CMDG_ERR_INVALID, "cmdg_create: sgeo's vMI differs from vgeo's MI at the face nodes (Grids.jl:1097-1101)");
        if (bad & 4)
            return fail(CMDG_ERR_INVALID, "cmdg_create: too many elements for 32-bit face indices");
        g.faceP = d_faceP;
        g.faceG = d_faceG;
    }
    aux = d->state_auxiliary;
    const size_t nd = (size_t)Np * nelem;
    // hipMemset of device memory returns before the fill has run, and on the null stream it is not
    // ordered against this engine's non-blocking streams (scripts/probe/memset_null_stream_order.py):
    // every fill is enqueued on the compute stream, which init() drains before it returns
    gf = gf_node_major() ? nullptr : d->state_gradient_flux;
    gf_user = gf_node_major() ? d->state_gradient_flux : nullptr;
    if (!gf) {
        HIPCHK(gf_own.alloc_zeroed(std::max<size_t>(nd * ngf, 1), s_comp));
        gf = gf_own;
    }
    // Qhypervisc_grad is node-major inside the library (cmdg_common.h); a caller's array receives
    // the reference layout only from cmdg_export_hypervisc_grad (export_hypgrad)
    hypgrad_user = ngl > 0 ? d->Qhypervisc_grad : nullptr;
    HIPCHK(hypgrad.alloc_zeroed(std::max<size_t>(nd * 3 * ngl, 1), s_comp));
    hypdiv = d->Qhypervisc_div;
    if (!hypdiv) {
        HIPCHK(hd_own.alloc_zeroed(std::max<size_t>(nd * nhyp, 1), s_comp));
        hypdiv = hd_own;
    }
    slot_nvar_max = std::max(std::max(ns, ngf), std::max(3 * ngl, nhyp));
    if (communicate()) {
        for (auto &s : slot) {
            HIPCHK(s.sendbuf.alloc(slot_nvar_max * std::max<int64_t>(nvmapsend, 1)));
            HIPCHK(s.recvbuf.alloc(slot_nvar_max * std::max<int64_t>(nvmaprecv, 1)));
            HIPCHK(s.ev_packed.create(hipEventDisableTiming));
            HIPCHK(s.ev_done.create(hipEventDisableTiming));
            HIPCHK(s.ev_pulled.create(hipEventDisableTiming));
        }
    }
    HIPCHK(d_partial.alloc(1024));
    if (communicate())
        if (int r = init_halo_tables()) return r;
    // debugging overrides of the two exchange options (cmdg_set_option still has the last word)
    if (const char *v = getenv("CMDG_REFERENCE_HALO")) reference_halo = *v && *v != '0';
    if (const char *v = getenv("CMDG_HALO_PIPELINE")) no_pipeline = *v == '0';
    if (const char *v = getenv("CMDG_FUSED_COLUMNS")) fused_columns = atoi(v);
    if (int r = init_derived()) return r;
    HIPCHK(hipStreamSynchronize(s_comp));  // the fills have run
    return CMDG_OK;
}

// Tables of the exchange without pack / unpack launches (HaloDev).  Whatever cannot be built
// leaves the corresponding half on the reference's pack / unpack kernels; nothing here fails
// a create that the reference's tables allow.
int EngineBase::init_halo_tables()
{
    const int64_t NFT = 4 * NQ * NQV + 2 * NQ * NQ;
    std::vector<int64_t> vs((size_t)nvmapsend), vr((size_t)nvmaprecv), ext((size_t)nexterior);
    if (nvmapsend) HIPCHK(hipMemcpy(vs.data(), d_vmapsend, sizeof(int64_t) * nvmapsend, hipMemcpyDeviceToHost));
    if (nvmaprecv) HIPCHK(hipMemcpy(vr.data(), d_vmaprecv, sizeof(int64_t) * nvmaprecv, hipMemcpyDeviceToHost));
    if (nexterior) HIPCHK(hipMemcpy(ext.data(), d_exterior_user, sizeof(int64_t) * nexterior, hipMemcpyDeviceToHost));
    // ---- sender: per-element lists of (node, position in vmapsend)
    bool oks = nvmapsend < 2147483647LL;
    std::vector<uint8_t> is_ext((size_t)std::max<int64_t>(nreal, 1), 0);
    for (int64_t e1 : ext)
        if (e1 >= 1 && e1 <= nreal) is_ext[e1 - 1] = 1;
    std::vector<int32_t> off((size_t)nreal + 1, 0);
    for (int64_t i = 0; i < nvmapsend && oks; ++i) {
        const int64_t id = vs[i] - 1, e = id / Np;
        if (id < 0 || e >= nreal || !is_ext[e]) oks = false;
        else off[e + 1] += 1;
    }
    if (oks) {
        for (int64_t e = 0; e < nreal; ++e) off[e + 1] += off[e];
        std::vector<SendEnt> ent((size_t)std::max<int64_t>(nvmapsend, 1));
        std::vector<int32_t> fill(off.begin(), off.end() - 1);
        for (int64_t i = 0; i < nvmapsend; ++i) {
            const int64_t id = vs[i] - 1, e = id / Np;
            ent[fill[e]++] = SendEnt{(int32_t)(id - e * Np), (int32_t)i};
        }
        HIPCHK(d_sendoff.alloc(off.size()));
        HIPCHK(d_sendent.alloc(ent.size()));
        HIPCHK(hipMemcpy(d_sendoff, off.data(), sizeof(int32_t) * off.size(), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_sendent, ent.data(), sizeof(SendEnt) * ent.size(), hipMemcpyHostToDevice));
    }
    direct_send_ok = oks;
    // ---- receiver: position in vmaprecv of every ghost node
    const int64_t ng = nghost * Np, g0 = nreal * Np;
    bool okr = nvmaprecv < 2147483647LL;
    std::vector<int32_t> gs((size_t)std::max<int64_t>(ng, 1), -1);
    for (int64_t i = 0; i < nvmaprecv && okr; ++i) {
        const int64_t id = vr[i] - 1 - g0;
        if (id < 0 || id >= ng || gs[id] >= 0) okr = false;
        else gs[id] = (int32_t)i;
    }
    if (okr && nreal > 0) {  // every ghost node a face of a real element reads is received
        std::vector<int32_t> fP((size_t)(nreal * NFT));
        HIPCHK(hipMemcpy(fP.data(), d_faceP, sizeof(int32_t) * fP.size(), hipMemcpyDeviceToHost));
        for (size_t q = 0; q < fP.size() && okr; ++q)
            if (fP[q] >= g0 && (fP[q] - g0 >= ng || gs[fP[q] - g0] < 0)) okr = false;
    }
    if (okr) {
        HIPCHK(d_ghostslot.alloc(gs.size()));
        HIPCHK(hipMemcpy(d_ghostslot, gs.data(), sizeof(int32_t) * gs.size(), hipMemcpyHostToDevice));
    }
    direct_recv_ok = okr;
    return CMDG_OK;
}

int EngineBase::before_direct_send(int s, hipStream_t st)
{
    if (transport == TRANSPORT_LOCAL && communicate() && direct_send())
        for (int r : nabrtorank) {
            if (dbg_sync() & 32) HIPCHK(hipStreamSynchronize(group[r]->s_comm));
            HIPCHK(hipStreamWaitEvent(st, group[r]->slot[s].ev_pulled, 0));
        }
    return CMDG_OK;
}

int EngineBase::ensure_work()
{
    for (int i = 0; i < 2; ++i)
        if (!W[i]) {
            const size_t n = (size_t)Np * ns * nelem;
            // Allocated inside the first step, while the step's launches are being enqueued: the
            // fill must be ordered before them.  Until round 4 this was a hipMemset -- asynchronous
            // for device memory and, on the null stream, unordered against the non-blocking
            // streams below, so it could land AFTER the first stages had stored into W and zero
            // them (the "priority stream ordering failure" of round 3: high-priority halo streams
            // merely let the stage kernels overtake the fill; scripts/probe/memset_null_stream_order.py).
            HIPCHK(W[i].alloc_zeroed(n, s_comp));
            HIPCHK(hipStreamSynchronize(s_comp));
        }
    return CMDG_OK;
}

// the records of CMDG_OPT_GRADARG_HANDOFF, allocated by the first run that uses them: the fill is
// stream-ordered before the run's launches like that of the work states
int EngineBase::ensure_garg()
{
    if (!garg) {
        const size_t n = std::max<size_t>((size_t)Np * ngl * nelem, 1);
        HIPCHK(garg.alloc_zeroed(n, s_comp));
        HIPCHK(hipStreamSynchronize(s_comp));
    }
    return CMDG_OK;
}

int EngineBase::synchronize()
{
    HIPCHK(hipStreamSynchronize(s_comp));
    HIPCHK(hipStreamSynchronize(s_comm));
    return CMDG_OK;
}

// ---- profiling ---------------------------------------------------------------------
ProfRec &EngineBase::prof_pair(int kernel, bool clamp, Event e1)
{
    ProfRec r{kernel, Event(), std::move(e1), clamp};
    r.e0.create();
    if (!r.e1) r.e1.create();
    prof.push_back(std::move(r));
    return prof.back();
}
void EngineBase::prof_begin(int kernel, hipStream_t st)
{
    if (!profiling) return;
    hipEventRecord(prof_pair(kernel, false).e0, st);
}
void EngineBase::prof_end(hipStream_t st)
{
    if (!profiling) return;
    hipEventRecord(prof.back().e1, st);
}
// the library's Qhypervisc_grad / state_gradient_flux in the reference layout (Np, ncol, nelem), on demand
int EngineBase::export_hypgrad(double *dst)
{
    if (!dst) dst = hypgrad_user;
    if (ngl == 0) return CMDG_OK;
    if (!dst) return fail(CMDG_ERR_INVALID, "cmdg_export_hypervisc_grad: no destination (cmdg_desc.Qhypervisc_grad was NULL)");
    const int64_t n = (int64_t)Np * 3 * ngl * nelem;
    hipLaunchKernelGGL(k_export_node_major, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s_comp, dst, hypgrad, Np,
                       3 * ngl, nelem);
    HIPCHK(hipStreamSynchronize(s_comp));
    return CMDG_OK;
}
int EngineBase::export_gradflux(double *dst)
{
    if (!dst) dst = gf_node_major() ? gf_user : gf;
    if (ngf == 0) return CMDG_OK;
    if (!dst) return fail(CMDG_ERR_INVALID, "cmdg_export_gradient_flux: no destination (cmdg_desc.state_gradient_flux was NULL)");
    const int64_t n = (int64_t)Np * ngf * nelem;
    if (gf_node_major()) {
        hipLaunchKernelGGL(k_export_node_major, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s_comp, dst, gf, Np,
                           ngf, nelem);
    } else if (dst != gf) {
        HIPCHK(hipMemcpyAsync(dst, gf, sizeof(double) * n, hipMemcpyDeviceToDevice, s_comp));
    }
    HIPCHK(hipStreamSynchronize(s_comp));
    return CMDG_OK;
}
void EngineBase::prof_collect()
{
    for (auto &r : prof) {
        hipEventSynchronize(r.e1);
        float ms = 0;
        if (hipEventElapsedTime(&ms, r.e0, r.e1) == hipSuccess) {
            prof_ms[r.kernel] += r.clamp && ms < 0 ? 0.0f : ms;
            prof_n[r.kernel] += 1;
        }
    }
    prof.clear();  // (destroys the events)
}

// ---- halo: begin_ghost_exchange! / end_ghost_exchange!  MPIStateArrays.jl:411-483 ----
int EngineBase::halo_begin(int s, double *array, int nvar, int ncol, bool on_halo_stream)
{
    if (int r = halo_pack(s, array, nvar, ncol, on_halo_stream)) return r;
    return halo_post(&s, 1);
}

int EngineBase::halo_pack(int s, double *array, int nvar, int ncol, bool on_halo_stream)
{
    if (!communicate()) return CMDG_OK;
    if (transport == TRANSPORT_NONE)
        return fail(CMDG_ERR_COMM, "halo exchange needs cmdg_comm_init_rccl or cmdg_comm_connect_local");
    Range range_("cmdg:halo:pack");
    HaloSlot &h = slot[s];
    if (h.active) return fail(CMDG_ERR_INVALID, "The current ghost exchange must end before another begins.");
    if (nvar > slot_nvar_max) return fail(CMDG_ERR_INVALID, "halo: nstate too large for the buffers");
    if (ncol == 0) ncol = nvar;
    if (ncol < nvar) return fail(CMDG_ERR_INVALID, "halo: more packed columns than the array has");
    h.nvar = nvar;
    h.ncol = ncol;
    h.array = array;
    // an exterior launch of this evaluation wrote the nodes of vmapsend already
    const bool fresh = h.fresh_for == array && h.fresh_nvar == nvar && direct_send();
    h.fresh_for = nullptr;
    // the data to send is produced on the compute stream -- unless an exterior launch of the
    // halo stream's own pipeline wrote it (pipelined())
    if (capturing && !(fresh && on_halo_stream))
        return fail(CMDG_ERR_UNSUPPORTED, "step graph: an exchange of this step would have to be packed");
    if (!(fresh && on_halo_stream)) {
        if (dbg_sync() & 2) HIPCHK(hipStreamSynchronize(s_comp));
        HIPCHK(ev_record(ev_comp, s_comp));
        HIPCHK(hipStreamWaitEvent(s_comm, ev_comp, 0));
    }
    if (transport == TRANSPORT_LOCAL) {
        // neighbours must have pulled the previous payload of this slot
        for (int r : nabrtorank) {
            if (dbg_sync() & 4) HIPCHK(hipStreamSynchronize(group[r]->s_comm));
            HIPCHK(hipStreamWaitEvent(s_comm, group[r]->slot[s].ev_pulled, 0));
        }
    }
    if (nvmapsend > 0 && !fresh) {
        const int64_t n = nvmapsend * nvar;
        prof_begin(CMDG_K_PACK, s_comm);
        hipLaunchKernelGGL(k_fillsendbuf, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s_comm,
                           h.sendbuf, array, d_vmapsend, nvmapsend, Np, nvar, ncol,
                           (int)node_major(array));
        prof_end(s_comm);
    }
    if (!capturing) HIPCHK(ev_record(h.ev_packed, s_comm));  // (read by the local transport only)
    return CMDG_OK;
}

int EngineBase::halo_post(const int *slots, int nslots)
{
    if (!communicate()) return CMDG_OK;
    Range range_("cmdg:halo:transport");
    const auto host_t0 = std::chrono::steady_clock::now();
    struct HostTimer {  // host time spent posting exchanges (cmdg_query CMDG_Q_HOST_POST_NS)
        EngineBase *e;
        std::chrono::steady_clock::time_point t0;
        ~HostTimer()
        {
            e->host_post_ns += std::chrono::duration_cast<std::chrono::nanoseconds>(
                                   std::chrono::steady_clock::now() - t0).count();
            e->host_post_n += 1;
        }
    } host_timer_{this, host_t0};
    if (transport == TRANSPORT_RCCL) {
        // one group for everything that begins here: every neighbour pair has its own xGMI
        // link, and one group costs one RCCL launch however many arrays travel
        prof_begin(CMDG_K_TRANSPORT, s_comm);
        if (rccl::GroupStart()) return fail(CMDG_ERR_COMM, "ncclGroupStart failed");
        for (int q = 0; q < nslots; ++q) {
            HaloSlot &h = slot[slots[q]];
            const int nvar = h.nvar;
            for (size_t n = 0; n < nabrtorank.size(); ++n) {
                const int64_t r0 = nabrrecv[2 * n] - 1, rn = nabrrecv[2 * n + 1] - r0;
                const int64_t s0 = nabrsend[2 * n] - 1, sn = nabrsend[2 * n + 1] - s0;
                int rc = rccl::Recv(h.recvbuf + r0 * nvar, (size_t)(rn * nvar), rccl::kDouble,
                                    nabrtorank[n], nccl_comm, s_comm);
                if (!rc)
                    rc = rccl::Send(h.sendbuf + s0 * nvar, (size_t)(sn * nvar), rccl::kDouble,
                                    nabrtorank[n], nccl_comm, s_comm);
                if (rc) {
                    rccl::GroupEnd();
                    return fail(CMDG_ERR_COMM, std::string("ncclSend/Recv: ") + rccl::GetErrorString(rc));
                }
            }
        }
        if (int rc = rccl::GroupEnd())
            return fail(CMDG_ERR_COMM, std::string("ncclGroupEnd: ") + rccl::GetErrorString(rc));
        prof_end(s_comm);
    }
    // only now: a failure above leaves the slots free for the next call
    for (int q = 0; q < nslots; ++q) slot[slots[q]].active = true;
    return CMDG_OK;
}

// Launch order of the element lists (results do not depend on it).  Column by column, a tall
// stack fills an XCD's work-group slots by itself and the expensive horizontal face gathers find
// nothing of their neighbours in its L2; tiles of TILE_C columns x TILE_L levels put horizontal
// neighbours (consecutive columns of the Hilbert order) in flight together:
// profiles/r02_ab_launch_tiles.txt (BOMEX, 32 levels: -8 % on k_tendency; rising bubble, 20: -3 %;
// ocean box, 16, and Held-Suarez, 8: nothing to gain).
int EngineBase::set_stack_height(int nv)
{
    constexpr int TILE_C = 32, TILE_L = 4, MIN_HEIGHT = 17;
    if (nv < 0 || (nv > 0 && (!stacked || nreal % nv != 0)))
        return fail(CMDG_ERR_INVALID, "stack height: not a stacked topology or nreal is not a multiple of it");
    if (fv) return CMDG_OK;  // the finite-volume pass walks the caller's lists stack by stack
    HIPCHK(hipStreamSynchronize(s_comp));
    d_interior = d_interior_user;
    d_exterior = d_exterior_user;
    if (nv < MIN_HEIGHT) return CMDG_OK;
    for (int which = 0; which < 2; ++which) {
        const int64_t n = which ? nexterior : ninterior;
        if (n == 0) continue;
        std::vector<int64_t> h((size_t)n);
        HIPCHK(hipMemcpy(h.data(), which ? d_exterior_user : d_interior_user, sizeof(int64_t) * n,
                         hipMemcpyDeviceToHost));
        auto key = [&](int64_t e1) {
            const int64_t e = e1 - 1, col = e / nv, lev = e % nv;
            return std::make_tuple(col / TILE_C, lev / TILE_L, col % TILE_C, lev % TILE_L);
        };
        std::stable_sort(h.begin(), h.end(), [&](int64_t x, int64_t y) { return key(x) < key(y); });
        DevBuf<int64_t> &own = which ? d_exterior_tiled : d_interior_tiled;
        if (!own) HIPCHK(own.alloc(n));
        HIPCHK(hipMemcpy(own, h.data(), sizeof(int64_t) * n, hipMemcpyHostToDevice));
        (which ? d_exterior : d_interior) = own;
    }
    return CMDG_OK;
}

// CMDG_OPT_STREAM_PRIORITY: both streams of the handle at the highest (1), the default (0) or the
// lowest (-1) priority.  Two handles whose launches run side by side -- the two models of the
// split-explicit ocean -- can say who yields: measured there, the barotropic model's small
// launches are best run at the lowest priority (they hide behind the slow model's evaluation
// anyway, and every slot they take slows the kernels on the critical path).
int EngineBase::set_stream_priority(int level)
{
    int lo = 0, hi = 0;
    HIPCHK(hipDeviceGetStreamPriorityRange(&lo, &hi));
    if (level < -1 || level > 1) return fail(CMDG_ERR_INVALID, "stream priority: 0 (default), 1 (highest) or -1 (lowest)");
    if (int r = synchronize()) return r;
    drop_graph();
    Stream nc, nm;
    const int prio = level > 0 ? hi : (level < 0 ? lo : 0);
    HIPCHK(nc.create(hipStreamNonBlocking, prio));
    HIPCHK(nm.create(hipStreamNonBlocking, prio));
    s_comp = std::move(nc);  // (the old streams are drained: synchronize() above)
    s_comm = std::move(nm);
    stream_priority = level;
    return CMDG_OK;
}

void EngineBase::abort_exchanges()
{
    for (auto &h : slot) {
        h.active = false;
        h.fresh_for = nullptr;
    }
}

int EngineBase::halo_end(int s, double *array, int nvar, bool unpack, bool on_halo_stream)
{
    if (!communicate()) return CMDG_OK;
    Range range_(unpack ? "cmdg:halo:end+unpack" : "cmdg:halo:end");
    HaloSlot &h = slot[s];
    if (!h.active) return fail(CMDG_ERR_INVALID, "A ghost exchange must begin before it ends.");
    if (h.array != array || h.nvar != nvar)
        return fail(CMDG_ERR_INVALID, "halo_end does not match the pending halo_begin");
    h.active = false;
    if (transport == TRANSPORT_LOCAL) {
        for (size_t n = 0; n < nabrtorank.size(); ++n) {
            EngineBase *peer = group[nabrtorank[n]];
            int m = -1;
            for (size_t q = 0; q < peer->nabrtorank.size(); ++q)
                if (peer->nabrtorank[q] == rank) m = (int)q;
            if (m < 0) return fail(CMDG_ERR_COMM, "local transport: neighbour lists are not symmetric");
            const int64_t r0 = nabrrecv[2 * n] - 1, rn = nabrrecv[2 * n + 1] - r0;
            const int64_t s0 = peer->nabrsend[2 * m] - 1, sn = peer->nabrsend[2 * m + 1] - s0;
            if (rn != sn) return fail(CMDG_ERR_COMM, "local transport: send/recv sizes differ");
            if (dbg_sync() & 8) HIPCHK(hipStreamSynchronize(peer->s_comm));
            HIPCHK(hipStreamWaitEvent(s_comm, peer->slot[s].ev_packed, 0));
            if (n == 0) prof_begin(CMDG_K_TRANSPORT, s_comm);
            HIPCHK(hipMemcpyAsync(h.recvbuf + r0 * nvar, peer->slot[s].sendbuf + s0 * nvar,
                                  sizeof(double) * rn * nvar, hipMemcpyDeviceToDevice, s_comm));
        }
        if (!nabrtorank.empty()) prof_end(s_comm);
        HIPCHK(ev_record(h.ev_pulled, s_comm));
    }
    if (nvmaprecv > 0 && unpack) {
        const int64_t n = nvmaprecv * nvar;
        prof_begin(CMDG_K_UNPACK, s_comm);
        hipLaunchKernelGGL(k_transferrecvbuf, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                           s_comm, array, h.recvbuf, d_vmaprecv, nvmaprecv, Np, nvar, h.ncol,
                           (int)node_major(array));
        prof_end(s_comm);
    }
    if (on_halo_stream) return CMDG_OK;  // the consumer is the next launch of the halo stream
    HIPCHK(ev_record(h.ev_done, s_comm));
    if (profiling) {
        // exposed time of this exchange: from the moment the compute stream has nothing left to
        // do but wait (its interior launches are done) to the moment the ghosts are in place
        ProfRec &r = prof_pair(CMDG_K_HALO_EXPOSED, true);
        hipEventRecord(r.e0, s_comp);
        hipEventRecord(r.e1, s_comm);
    }
    if (dbg_sync() & 16) HIPCHK(hipStreamSynchronize(s_comm));
    HIPCHK(hipStreamWaitEvent(s_comp, h.ev_done, 0));
    return CMDG_OK;
}

// ---- (dg::DGModel)(tendency, Q, _, t, alpha, beta)   DGModel.jl:85-427 -----------------
// The evaluation is cut into segments at the points where the reference ends a ghost
// exchange, so that a single host thread can drive several ranks in lock step (local
// transport).  With fused volume+interface kernels an element list is processed whole:
// interior elements while the halo is in flight, exterior elements after it arrived.
int EngineBase::rhs_segment(int seg, const RhsCtx &c)
{
    const bool comm = exchanges();
    const bool gfl = gf_live();  // is state_gradient_flux read by anybody?
    const bool grad = gfl || nhyp > 0;
    const bool hyper = nhyp > 0;
    // exterior launches write the send buffers / consumers read the receive buffers (HaloDev)
    const bool dsend = comm && direct_send(), unpack = !(comm && direct_recv());
    // exterior launches and exchanges on the halo stream, interior launches on the compute stream
    const bool pipe = pipelined() && !has_hooks;
    hipStream_t s_ext = pipe ? s_comm : s_comp;
    // of Qhypervisc_div's nhyp columns the Laplacian pass writes, and the next pass reads, ngl
    const int nhd = ngl;
    int r;
#define TRY(x) \
    if ((r = (x)) != CMDG_OK) return r
    // interior launch I_p of a pass (enqueued before its exterior launch): waits for E_(p-1)
    // a capture has events of its own (the eager ones keep their last eager record), and its first
    // launches wait for nothing of the step before: graphs launched on one stream run in order
    const Event *const EI = capturing ? gev_int : ev_int, *const EE = capturing ? gev_ext : ev_ext;
    // index of pass q's event: alternating parity when eager, one event per pass in a capture
    auto evi = [&](int64_t q) { return capturing ? (int)((cap_pass + (q - pass_seq)) % NGEV) : (int)(q & 1); };
    auto interior_begin = [&]() -> int {
        ++pass_seq;
        if (capturing) ++cap_pass;
        if (!pipe) return CMDG_OK;
        if (capturing && cap_interior++ == 0) return CMDG_OK;
        if (profiling && prof_ext_done) {
            // exposed: the compute stream idle until the previous exterior launch is done
            hipEventRecord(prof_pair(CMDG_K_HALO_EXPOSED, true, std::move(prof_ext_done)).e0, s_comp);
        }
        if (dbg_sync() & 64) HIPCHK(hipStreamSynchronize(s_comm));
        HIPCHK(hipStreamWaitEvent(s_comp, EE[evi(pass_seq - 1)], 0));
        return CMDG_OK;
    };
    auto interior_end = [&]() -> int {
        if (pipe) HIPCHK(ev_record(EI[evi(pass_seq)], s_comp));
        return CMDG_OK;
    };
    // exterior launch E_p: waits for I_(p-1)
    auto exterior_begin = [&]() -> int {
        if (pipe && !(capturing && cap_exterior++ == 0)) {
            if (dbg_sync() & 64) HIPCHK(hipStreamSynchronize(s_comp));
            HIPCHK(hipStreamWaitEvent(s_comm, EI[evi(pass_seq - 1)], 0));
        }
        return CMDG_OK;
    };
    auto exterior_end = [&]() -> int {
        if (pipe) HIPCHK(ev_record(EE[evi(pass_seq)], s_comm));
        if (pipe && profiling) {
            prof_ext_done.create();  // (one that no interior launch took is destroyed)
            hipEventRecord(prof_ext_done, s_comm);
        }
        return CMDG_OK;
    };
    switch (seg) {
    case 0:
        if (has_hooks) {
            if (!c.pre_done) TRY(run_pre_hooks(c));  // update_auxiliary_state!(realelems) of the law
            slot[SLOT_Q].fresh_for = nullptr;  // (its filters rewrite Q)
        }
        if (!(grad && fused_update_aux())) launch_update_aux(c, 0, nreal);
        if (comm) TRY(halo_begin(SLOT_Q, c.Qin, ns, 0, pipe));
        if (grad) {
            TRY(interior_begin());
            launch_gradients(c, d_interior, ninterior, false, s_comp);
            TRY(interior_end());
        }
        break;
    case 1:
        if (!grad) break;
        if (comm) {
            TRY(halo_end(SLOT_Q, c.Qin, ns, unpack, pipe));
            if (unpack) launch_update_aux(c, nreal, nelem);
            // update_auxiliary_state!(ghostelems): the flow deviation of the ghost stacks
            if (has_hooks && hooks.has_flow_deviation)
                TRY(flow_deviation(c.Qin, nreal / hooks.nvertelem, nghost / hooks.nvertelem));
            // ... and, for a law that integrates in update_auxiliary_state! itself (SplitExplicit01's
            // OceanModel), the column operators over the received face pencils of the ghost stacks:
            // the kinematic pressure the rank-boundary faces read on their plus side
            if (has_hooks && hooks.ops_before_gradients) TRY(run_column_ops(c, nreal, nelem));
        }
        if (dsend && gfl) TRY(before_direct_send(SLOT_GF, s_ext));
        if (dsend && hyper) TRY(before_direct_send(SLOT_HG, s_ext));
        TRY(exterior_begin());
        launch_gradients(c, d_exterior, nexterior, comm, s_ext);
        TRY(exterior_end());
        if (dsend && gfl && !gradient_filter) mark_fresh(SLOT_GF, gf, ngf);
        if (dsend && hyper) mark_fresh(SLOT_HG, hypgrad, 3 * ngl);
        if (gradient_filter && gfl) {  // (:185-193)
            if (gf_node_major()) {  // the filter kernels work on the reference layout
                const int64_t n = (int64_t)Np * ngf * nelem;
                const unsigned nb = (unsigned)((n + 255) / 256);
                if (!gf_scratch) HIPCHK(gf_scratch.alloc(n));
                hipLaunchKernelGGL(k_export_node_major, dim3(nb), dim3(256), 0, s_comp, gf_scratch, gf, Np, ngf, nelem);
                TRY(filter_apply(gradient_filter, gf_scratch, ngf));
                hipLaunchKernelGGL(k_import_node_major, dim3(nb), dim3(256), 0, s_comp, gf, gf_scratch, Np, ngf, nelem);
            } else {
                TRY(filter_apply(gradient_filter, gf, ngf));
            }
        }
        if (comm) {  // both begin here: packed back to back, posted in one group
            int slots[2], ns_ = 0;
            if (gfl) {
                TRY(halo_pack(SLOT_GF, gf, ngf, 0, pipe));
                slots[ns_++] = SLOT_GF;
            }
            if (hyper) {
                TRY(halo_pack(SLOT_HG, hypgrad, 3 * ngl, 0, pipe));
                slots[ns_++] = SLOT_HG;
            }
            if (ns_) TRY(halo_post(slots, ns_));
        }
        // update_auxiliary_state_gradient!(realelems)  (DGModel.jl:210-222)
        if (has_hooks && gfl) TRY(run_gradient_hooks(c, 0, nreal));
        if (hyper) {
            TRY(interior_begin());
            launch_divgrad(c, d_interior, ninterior, false, s_comp);
            TRY(interior_end());
        }
        break;
    case 2:
        if (!hyper) break;
        if (comm) TRY(halo_end(SLOT_HG, hypgrad, 3 * ngl, unpack, pipe));
        if (dsend) TRY(before_direct_send(SLOT_HD, s_ext));
        TRY(exterior_begin());
        launch_divgrad(c, d_exterior, nexterior, comm, s_ext);
        TRY(exterior_end());
        if (dsend) mark_fresh(SLOT_HD, hypdiv, nhd);
        if (comm) TRY(halo_begin(SLOT_HD, hypdiv, nhd, nhyp, pipe));
        TRY(interior_begin());
        launch_gradlap(c, d_interior, ninterior, false, s_comp);
        TRY(interior_end());
        break;
    case 3:
        if (hyper) {
            if (comm) TRY(halo_end(SLOT_HD, hypdiv, nhd, unpack, pipe));
            if (dsend) TRY(before_direct_send(SLOT_HG, s_ext));
            TRY(exterior_begin());
            launch_gradlap(c, d_exterior, nexterior, comm, s_ext);
            TRY(exterior_end());
            if (dsend) mark_fresh(SLOT_HG, hypgrad, 3 * ngl);
            if (comm) TRY(halo_begin(SLOT_HG, hypgrad, 3 * ngl, 0, pipe));
        }
        TRY(interior_begin());
        launch_tendency(c, d_interior, ninterior, false, s_comp);
        TRY(interior_end());
        break;
    case 4:  // the exchanges the tendency pass waits for end here, on every rank of a local group,
             // before any rank's exterior launch overwrites a send buffer (case 5)
        if (comm) {
            if (grad) {
                if (gfl) {
                    TRY(halo_end(SLOT_GF, gf, ngf, unpack, pipe));
                    // update_auxiliary_state_gradient!(ghostelems)  (DGModel.jl:355-361)
                    if (has_hooks) TRY(run_gradient_hooks(c, nreal, nelem));
                }
                if (hyper) TRY(halo_end(SLOT_HG, hypgrad, 3 * ngl, unpack, pipe));
            } else {
                TRY(halo_end(SLOT_Q, c.Qin, ns, unpack, pipe));
                if (unpack) launch_update_aux(c, nreal, nelem);
            }
        }
        break;
    case 5:
        if (dsend && c.lsrk) TRY(before_direct_send(SLOT_Q, s_ext));
        TRY(exterior_begin());
        launch_tendency(c, d_exterior, nexterior, comm, s_ext);
        TRY(exterior_end());
        if (dsend && c.lsrk) mark_fresh(SLOT_Q, c.Qout, ns);
        // whatever follows on the compute stream (a filter, the caller's next call, the next
        // evaluation's first interior launch) finds this evaluation complete
        if (pipe && (dbg_sync() & 128)) HIPCHK(hipStreamSynchronize(s_comm));
        if (pipe) HIPCHK(hipStreamWaitEvent(s_comp, EE[evi(pass_seq)], 0));
        if (tendency_filter) TRY(filter_apply(tendency_filter, c.tendency, ns));  // (:417-425)
        if (c.update_after) {
            const int64_t n = (int64_t)Np * ns * nreal;
            hipLaunchKernelGGL(k_lsrk_update, dim3(nblocks(n)), dim3(256), 0, s_comp, c.tendency, c.Qin,
                               c.rka_next, c.rkb_dt, n);
        }
        break;
    default: break;
    }
#undef TRY
    if (dbg_sync() & 512) HIPCHK(hipDeviceSynchronize());
    return launch_status("kernel launch");
}

int EngineBase::rhs_async(const RhsCtx &c)
{
    if (transport == TRANSPORT_LOCAL && communicate())
        return fail(CMDG_ERR_INVALID, "handles connected locally must be driven by the cmdg_group_* calls");
    invalidate_sends();  // the caller's Q: nothing is known about its send buffer
    for (int s = 0; s < NSEG; ++s)
        if (int r = rhs_segment(s, c)) {
            abort_exchanges();
            return r;
        }
    return CMDG_OK;
}

// keep_fresh: the state read is what the previous stage's fused update wrote (its exterior launch
// filled the send buffer of Q already); otherwise nothing is known about the send buffers
int group_rhs(std::vector<EngineBase *> &g, std::vector<RhsCtx> &c, bool keep_fresh)
{
    if (!keep_fresh)
        for (auto *e : g) e->invalidate_sends();
    for (auto &x : c) x.pre_done = false;
    if (dbg_sync() & 256) (void)hipDeviceSynchronize();
    // handles whose update_auxiliary_state! evaluates a nested operator: the nested operators of
    // the group exchange among themselves, so they run in lock step too, between the two halves
    // of the composition (a single handle does the same inside segment 0, run_pre_hooks)
    bool nested = false;
    for (auto *e : g) nested = nested || (e->has_hooks && e->hooks.pre_rhs_handle);
    if (nested && g.size() > 1) {
        std::vector<EngineBase *> ch;
        std::vector<RhsCtx> cc(g.size());
        for (size_t i = 0; i < g.size(); ++i) {
            if (!(g[i]->has_hooks && g[i]->hooks.pre_rhs_handle))
                return g[i]->fail(CMDG_ERR_INVALID, "local group: every rank needs the nested operator");
            if (int r = g[i]->run_pre_hooks_a(c[i], cc[i])) return r;
            ch.push_back(g[i]->hooks.pre_rhs_handle->eng);
        }
        for (auto *e : ch) e->err.clear();
        if (int r = group_rhs(ch, cc)) {
            for (size_t i = 0; i < ch.size(); ++i)
                if (!ch[i]->err.empty()) return g[i]->fail(r, "nested operator: " + ch[i]->err);
            return r;
        }
        for (size_t i = 0; i < g.size(); ++i) {
            if (int r = g[i]->run_pre_hooks_b(c[i])) return r;
            c[i].pre_done = true;
        }
    }
    for (int s = 0; s < EngineBase::NSEG; ++s)
        for (size_t i = 0; i < g.size(); ++i)
            if (int r = g[i]->rhs_segment(s, c[i])) {
                for (auto *e : g) e->abort_exchanges();
                return r;
            }
    return CMDG_OK;
}

// ---- courant / min_node_distance: rank-local extremum, the caller Allreduces ------------
int EngineBase::courant(int mode, int kind, const double *Q, double dt, double t, int dir,
                        double *out)
{
    if (dir < 0 || dir > 2 || kind < 0 || kind > 3) return fail(CMDG_ERR_INVALID, "courant: bad argument");
    if (g.nvgeo < 15) return fail(CMDG_ERR_INVALID, "courant: vgeo lacks the coordinate columns");
    if (nreal == 0) {  // typemin / typemax (SpaceDiscretization.jl:359-361, Grids.jl:481-483)
        *out = mode == 0 ? INFINITY : -INFINITY;
        return CMDG_OK;
    }
    if (!d_elemred) HIPCHK(d_elemred.alloc(nreal + 1));
    if (int r = launch_courant(mode, kind, Q, dt, t, dir, d_elemred)) return r;
    hipLaunchKernelGGL(k_extremum, dim3(1), dim3(1024), 0, s_comp, d_elemred, nreal, mode == 0,
                       d_elemred + nreal);
    HIPCHK(hipMemcpyAsync(out, d_elemred + nreal, sizeof(double), hipMemcpyDeviceToHost, s_comp));
    HIPCHK(hipStreamSynchronize(s_comp));
    return CMDG_OK;
}

int EngineBase::wsum2(const double *A, const double *B, int nvar, int weighted, double *out)
{
    const int nb = 512;
    hipLaunchKernelGGL(k_wsum2, dim3(nb), dim3(256), 0, s_comp, A, B, g.vgeo, g.nvgeo, Np, nvar,
                       nreal, weighted, d_partial);
    double h[nb];
    HIPCHK(hipMemcpyAsync(h, d_partial, sizeof(double) * nb, hipMemcpyDeviceToHost, s_comp));
    HIPCHK(hipStreamSynchronize(s_comp));
    double acc = 0;
    for (int i = 0; i < nb; ++i) acc += h[i];
    *out = acc;
    return CMDG_OK;
}

}  // namespace cmdg

// =====================================================================================
// C ABI
// =====================================================================================
using namespace cmdg;

static thread_local std::string g_create_err;

// ---- engine plug-ins: balance-law functors / template combinations outside the compiled set ----
// A plug-in is a shared object built from this library's own headers (csrc/engine.h + a
// physics_*.h, one translation unit instantiating make_engine<Law, Nq>) that exports
//   cmdg::EngineBase *cmdg_plugin_make_engine(const cmdg_desc *, char *err, int errlen)
// returning NULL for a descriptor it does not serve.  climatemachine.jl_amd/plugins.py writes and
// builds them with hipcc (the reference compiles a law's pointwise functions into its kernels when
// the model is first run; this is the ahead-of-time equivalent for a C ABI).
namespace {
typedef EngineBase *(*plugin_make_t)(const cmdg_desc *, char *, int);
std::vector<plugin_make_t> g_plugin_make;
std::vector<std::string> g_plugin_path;
bool g_plugins_env_read = false;
int load_plugin(const char *path, std::string &err)
{
    for (const auto &p : g_plugin_path)
        if (p == path) return CMDG_OK;
    void *lib = dlopen(path, RTLD_NOW | RTLD_LOCAL);
    if (!lib) {
        err = std::string("cannot load plug-in: ") + dlerror();
        return CMDG_ERR_INVALID;
    }
    plugin_make_t f = (plugin_make_t)dlsym(lib, "cmdg_plugin_make_engine");
    if (!f) {
        err = std::string(path) + " does not export cmdg_plugin_make_engine";
        dlclose(lib);
        return CMDG_ERR_INVALID;
    }
    // a plug-in shares the C++ layout of EngineBase with the library: one built against other
    // headers is refused here instead of corrupting a handle later
    typedef unsigned long (*plugin_abi_t)();
    plugin_abi_t abi = (plugin_abi_t)dlsym(lib, "cmdg_plugin_abi");
    if (!abi || abi() != engine_abi_stamp()) {
        err = std::string(path) + (abi ? " was built against another libcmdg (engine layout differs): rebuild it"
                                       : " does not export cmdg_plugin_abi");
        dlclose(lib);
        return CMDG_ERR_INVALID;
    }
    g_plugin_make.push_back(f);
    g_plugin_path.push_back(path);
    return CMDG_OK;
}
EngineBase *plugin_engine(const cmdg_desc *d, std::string &err)
{
    if (!g_plugins_env_read) {
        g_plugins_env_read = true;
        if (const char *env = getenv("CMDG_PLUGINS")) {
            std::string all(env), e2;
            size_t a = 0;
            while (a <= all.size()) {
                const size_t b = all.find(':', a);
                const std::string one = all.substr(a, b == std::string::npos ? std::string::npos : b - a);
                if (!one.empty() && load_plugin(one.c_str(), e2) != CMDG_OK) err += e2 + "; ";
                if (b == std::string::npos) break;
                a = b + 1;
            }
        }
    }
    for (plugin_make_t f : g_plugin_make) {
        char buf[512] = {0};
        if (EngineBase *e = f(d, buf, (int)sizeof(buf))) return e;
        if (buf[0]) err += std::string(buf) + "; ";
    }
    if (g_plugin_make.empty() && err.empty()) err = "none loaded";
    return nullptr;
}
}  // namespace


extern "C" {

const char *cmdg_version(void) { return "cmdg 0.1 (gfx950)"; }

int cmdg_load_plugin(const char *path)
{
    if (!path) return CMDG_ERR_INVALID;
    std::string err;
    const int r = load_plugin(path, err);
    if (r) g_create_err = err;
    return r;
}

const char *cmdg_status_string(int status)
{
    switch (status) {
    case CMDG_OK: return "ok";
    case CMDG_ERR_INVALID: return "invalid argument";
    case CMDG_ERR_HIP: return "HIP runtime error";
    case CMDG_ERR_NO_DEVICE: return "no gfx950 device";
    case CMDG_ERR_COMM: return "communication error";
    case CMDG_ERR_UNSUPPORTED: return "unsupported physics / polynomial order";
    default: return "unknown status";
    }
}

int cmdg_physics_counts(int32_t physics_id, const int32_t *iparam, int32_t out[6])
{
    if (!iparam || !out) return CMDG_ERR_INVALID;
    switch (physics_id) {
    case CMDG_PHYSICS_ADVECTION_DIFFUSION: return counts_advdiff(iparam, out);
    case CMDG_PHYSICS_DRY_ATMOS: return counts_atmos(iparam, out);
    case CMDG_PHYSICS_HYDROSTATIC_BOUSSINESQ: return counts_ocean(iparam, out);
    case CMDG_PHYSICS_PRESSURE_GRADIENT: return counts_pgrad(iparam, out);
    case CMDG_PHYSICS_SHALLOW_WATER: return counts_sw(iparam, out);
    case CMDG_PHYSICS_MOIST_ATMOS: return counts_moist(iparam, out);
    case CMDG_PHYSICS_ATMOS_LINEAR_AG: return counts_atmos_linear(iparam, out);
    case CMDG_PHYSICS_MOIST_LINEAR_AG: return counts_moist_linear(iparam, out);
    case CMDG_PHYSICS_ATMOS_LINEAR_ACOUSTIC: return counts_atmos_acoustic(iparam, out);
    case CMDG_PHYSICS_OCEAN_SE01:
    case CMDG_PHYSICS_CONTINUITY3D_SE01:
    case CMDG_PHYSICS_BAROTROPIC_SE01: return counts_se01(physics_id, out);
    case CMDG_PHYSICS_ESDG_DRY_ATMOS: return counts_esdg_dryatmos(iparam, out);
    default: return CMDG_ERR_UNSUPPORTED;
    }
}

int cmdg_atmos_host_constants(const int32_t *iparam, const double *dparam, double out[7])
{
    if (!iparam || !dparam || !out) return CMDG_ERR_INVALID;
    return host_constants_atmos(iparam, dparam, out);
}

static int create_handle(const cmdg_desc *d, const cmdg_fv_desc *fv, cmdg_handle *out, const cmdg_esdg_desc *esdg = nullptr)
{
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        g_create_err = "no HIP device visible";
        return CMDG_ERR_NO_DEVICE;
    }
    if (d->dim != 3 || d->N[0] != d->N[1]) {
        g_create_err = "only dim == 3 with one horizontal polynomial order is compiled in";
        return CMDG_ERR_UNSUPPORTED;
    }
    if (d->nf_first < CMDG_RUSANOV || d->nf_first > CMDG_ROE_MOIST_LVPP) {
        g_create_err = "unknown first-order numerical flux";
        return CMDG_ERR_INVALID;
    }
    if (d->nf_first >= CMDG_ROE && d->nf_first <= CMDG_LMARS && d->physics_id != CMDG_PHYSICS_DRY_ATMOS) {
        g_create_err = "Roe / HLLC / LMARS numerical fluxes are methods of the dry atmosphere law only";
        return CMDG_ERR_UNSUPPORTED;
    }
    if (d->nf_first >= CMDG_ROE_MOIST && d->physics_id != CMDG_PHYSICS_MOIST_ATMOS) {
        g_create_err = "RoeNumericalFluxMoist is a method of the moist atmosphere law (EquilMoist) only";
        return CMDG_ERR_UNSUPPORTED;
    }
    std::string err;
    EngineBase *e = nullptr;
    if (esdg) {
        e = make_engine_esdg(d, esdg, err);
        if (!e) {
            g_create_err = err;
            return CMDG_ERR_UNSUPPORTED;
        }
    } else if (fv) {
        if (d->physics_id == CMDG_PHYSICS_ADVECTION_DIFFUSION)
            e = make_engine_advdiff_fv(d, fv, err);
        else
            err = "cmdg_create_dgfv: the finite-volume passes are compiled for the AdvectionDiffusion law only";
        if (!e) {
            g_create_err = err;
            return CMDG_ERR_UNSUPPORTED;
        }
    } else
    switch (d->physics_id) {
    case CMDG_PHYSICS_ADVECTION_DIFFUSION: e = make_engine_advdiff(d, err); break;
    case CMDG_PHYSICS_DRY_ATMOS: e = make_engine_atmos(d, err); break;
    case CMDG_PHYSICS_HYDROSTATIC_BOUSSINESQ: e = make_engine_ocean(d, err); break;
    case CMDG_PHYSICS_PRESSURE_GRADIENT: e = make_engine_pgrad(d, err); break;
    case CMDG_PHYSICS_SHALLOW_WATER: e = make_engine_sw(d, err); break;
    case CMDG_PHYSICS_MOIST_ATMOS: e = make_engine_moist(d, err); break;
    case CMDG_PHYSICS_ATMOS_LINEAR_AG: e = make_engine_atmos_linear(d, err); break;
    case CMDG_PHYSICS_MOIST_LINEAR_AG: e = make_engine_moist_linear(d, err); break;
    case CMDG_PHYSICS_ATMOS_LINEAR_ACOUSTIC: e = make_engine_atmos_acoustic(d, err); break;
    case CMDG_PHYSICS_OCEAN_SE01:
    case CMDG_PHYSICS_CONTINUITY3D_SE01:
    case CMDG_PHYSICS_BAROTROPIC_SE01: e = make_engine_se01(d, err); break;
    default: err = "unknown physics_id"; break;
    }
    if (!e) {  // not compiled in: ask the plug-ins (cmdg_load_plugin / CMDG_PLUGINS)
        std::string perr;
        e = plugin_engine(d, perr);
        if (!e) {
            g_create_err = perr.empty() ? err : err + "; plug-ins: " + perr;
            return CMDG_ERR_UNSUPPORTED;
        }
    }
    int r = e->init(d);
    if (r == CMDG_OK && fv) r = e->init_fv();
    if (esdg) e->reference_halo = true;  // the face phase reads ghost neighbours from the ghost elements
    if (r != CMDG_OK) {
        g_create_err = e->err;
        delete e;
        return r;
    }
    cmdg_context *c = new (std::nothrow) cmdg_context();
    if (!c) {
        delete e;
        return CMDG_ERR_INVALID;
    }
    c->eng = e;
    *out = c;
    return CMDG_OK;
}

int cmdg_create(const cmdg_desc *d, cmdg_handle *out)
{
    if (!d || !out) return CMDG_ERR_INVALID;
    if (d->dim == 3 && d->N[2] == 0) {
        *out = nullptr;
        g_create_err = "cmdg_create: N[2] == 0 is a finite-volume vertical: use cmdg_create_dgfv";
        return CMDG_ERR_INVALID;
    }
    if (d->physics_id == CMDG_PHYSICS_ESDG_DRY_ATMOS) {
        *out = nullptr;
        g_create_err = "cmdg_create: the DryAtmosModel of the entropy-stable discretisation has no DGModel passes: "
                       "use cmdg_create_esdg";
        return CMDG_ERR_INVALID;
    }
    return create_handle(d, nullptr, out);
}

// DGFVModel(balance_law, grid, fv_reconstruction, nf1, nf2, nfgrad; direction)  DGFVModel.jl:22-69
int cmdg_create_dgfv(const cmdg_desc *d, const cmdg_fv_desc *fv, cmdg_handle *out)
{
    if (!d || !fv || !out) return CMDG_ERR_INVALID;
    *out = nullptr;
    auto refuse = [&](int code, const char *msg) {
        g_create_err = msg;
        return code;
    };
    if (d->dim != 3 || d->N[2] != 0)
        return refuse(CMDG_ERR_INVALID, "cmdg_create_dgfv: the vertical polynomial order N[2] must be 0 (use cmdg_create otherwise)");
    if (!d->stacked)
        return refuse(CMDG_ERR_INVALID, "cmdg_create_dgfv: the finite-volume vertical needs a stacked grid");
    if (fv->nvertelem < 2)
        return refuse(CMDG_ERR_INVALID, "cmdg_create_dgfv: nvertelem < 2");
    if (fv->reconstruction != CMDG_FV_CONSTANT && fv->reconstruction != CMDG_FV_LINEAR)
        return refuse(CMDG_ERR_INVALID, "cmdg_create_dgfv: unknown reconstruction");
    if (fv->width < 0 || fv->width > 3)
        return refuse(CMDG_ERR_INVALID, "cmdg_create_dgfv: reconstruction width outside 0..3");
    if (fv->reconstruction == CMDG_FV_LINEAR && fv->width == 0)
        return refuse(CMDG_ERR_INVALID, "cmdg_create_dgfv: a linear reconstruction needs width >= 1");
    if (fv->reconstruction == CMDG_FV_CONSTANT && fv->width != 0)
        return refuse(CMDG_ERR_INVALID, "cmdg_create_dgfv: the constant reconstruction has width 0");
    if (fv->limiter != CMDG_FV_VANLEER && fv->limiter != CMDG_FV_NOLIMITER)
        return refuse(CMDG_ERR_INVALID, "cmdg_create_dgfv: unknown slope limiter");
    if (d->nreal % fv->nvertelem != 0 || d->nghost % fv->nvertelem != 0)
        return refuse(CMDG_ERR_INVALID, "cmdg_create_dgfv: element counts are not multiples of nvertelem");
    return create_handle(d, fv, out);
}

// ESDGModel(balance_law, grid; volume_numerical_flux_first_order, surface_numerical_flux_first_order)
// ESDGModel.jl:75-94
int cmdg_create_esdg(const cmdg_desc *d, const cmdg_esdg_desc *ed, cmdg_handle *out)
{
    if (!d || !ed || !out) return CMDG_ERR_INVALID;
    *out = nullptr;
    auto refuse = [&](int code, const char *msg) {
        g_create_err = msg;
        return code;
    };
    if (d->physics_id != CMDG_PHYSICS_ESDG_DRY_ATMOS)
        return refuse(CMDG_ERR_UNSUPPORTED, "cmdg_create_esdg: the two-point fluxes are defined for CMDG_PHYSICS_ESDG_DRY_ATMOS only");
    if (d->dim != 3)
        return refuse(CMDG_ERR_UNSUPPORTED, "cmdg_create_esdg: only dim == 3 is compiled in");
    if (d->N[0] != d->N[1] || d->N[0] != d->N[2])
        return refuse(CMDG_ERR_UNSUPPORTED, "cmdg_create_esdg: mixed polynomial orders are not compiled in (one order in every direction)");
    if (d->N[0] != 3 && d->N[0] != 4)
        return refuse(CMDG_ERR_UNSUPPORTED, "cmdg_create_esdg: the flux-differencing kernel is compiled for polynomial orders 3 and 4");
    const int vf = ed->volume_flux, sf = ed->surface_flux;
    if (vf != CMDG_ESDG_FLUX_NONE && vf != CMDG_ESDG_FLUX_ENTROPY_CONSERVATIVE && vf != CMDG_ESDG_FLUX_CENTRAL &&
        vf != CMDG_ESDG_FLUX_KG)
        return refuse(CMDG_ERR_INVALID, "cmdg_create_esdg: unknown volume flux");
    if (sf != CMDG_ESDG_FLUX_NONE && sf != CMDG_ESDG_FLUX_ENTROPY_CONSERVATIVE && sf != CMDG_ESDG_FLUX_RUSANOV &&
        sf != CMDG_ESDG_FLUX_ENTROPY_CONSERVATIVE_PENALTY && sf != CMDG_ESDG_FLUX_MATRIX)
        return refuse(CMDG_ERR_INVALID, "cmdg_create_esdg: unknown surface flux");
    cmdg_desc dd = *d;  // (nf_first, direction: not read by an ESDG handle)
    dd.nf_first = CMDG_RUSANOV;
    dd.direction = dd.diffusion_direction = CMDG_EVERY_DIRECTION;
    return create_handle(&dd, nullptr, out, ed);
}

int cmdg_esdg_entropy(cmdg_handle h, const double *Q, double *beta, double *eta)
{
    if (!h || !Q) return CMDG_ERR_INVALID;
    DevGuard guard_(h->eng);
    return set_err(h, h->eng->launch_entropy(Q, beta, eta));
}

// what a DGFVModel handle adds to init(): exchanges packed / unpacked as the reference does, and
// element lists that are whole stacks, bottom element first
int EngineBase::init_fv()
{
    reference_halo = true;
    const int nv = fv_nvert;
    // (fv.h fv_lds_bytes: primitives, face fluxes and cell weights of one stack)
    if (sizeof(double) * NQ * NQ * ((size_t)ns * nv + (size_t)ns * (nv + 1) + nv) > 64 * 1024)
        return fail(CMDG_ERR_UNSUPPORTED, "cmdg_create_dgfv: a stack of this height does not fit the 64 KiB of LDS "
                                          "the finite-volume pass stages it in");
    for (int which = 0; which < 2; ++which) {
        const int64_t n = which ? nexterior : ninterior;
        if (n == 0) continue;
        std::vector<int64_t> h((size_t)n);
        HIPCHK(hipMemcpy(h.data(), which ? d_exterior_user : d_interior_user, sizeof(int64_t) * n, hipMemcpyDeviceToHost));
        bool ok = n % nv == 0;
        for (int64_t i = 0; ok && i < n; ++i)
            ok = h[i] >= 1 && h[i] <= nreal && (h[i] - 1) % nv == i % nv && (i % nv == 0 || h[i] == h[i - 1] + 1);
        if (!ok)
            return fail(CMDG_ERR_INVALID, "cmdg_create_dgfv: interiorelems / exteriorelems must list whole stacks, "
                                          "bottom element first");
    }
    return CMDG_OK;
}

int cmdg_destroy(cmdg_handle h)
{
    if (!h) return CMDG_ERR_INVALID;
    {
        DevGuard guard_(h->eng);
        // handles whose hooks evaluate this one as their nested operator cannot evaluate any more
        // (they would compute something else than the law they were given): their next evaluation
        // fails until cmdg_set_rhs_hooks gives them new hooks; the nested operator of this handle
        // forgets its parent
        for (EngineBase *parent : h->eng->nested_in) {
            parent->synchronize();
            parent->hooks.pre_rhs_handle = nullptr;
            parent->hooks_orphaned = true;
        }
        if (h->eng->has_hooks && h->eng->hooks.pre_rhs_handle && h->eng->hooks.pre_rhs_handle->eng) {
            auto &v = h->eng->hooks.pre_rhs_handle->eng->nested_in;
            v.erase(std::remove(v.begin(), v.end(), h->eng), v.end());
        }
        // members of a local group keep pointers to each other: detach the survivors
        for (EngineBase *peer : h->eng->group)
            if (peer && peer != h->eng) {
                peer->group.clear();
                peer->transport = TRANSPORT_NONE;
            }
        reduce_release(h->eng);
        delete h->eng;
    }
    delete h;
    return CMDG_OK;
}

const char *cmdg_last_error(cmdg_handle h)
{
    if (!h) return g_create_err.c_str();
    return h->err.c_str();
}

int cmdg_rhs_async(cmdg_handle h, double *tendency, double *Q, double t, double alpha, double beta)
{
    if (!h || !tendency || !Q) return CMDG_ERR_INVALID;
    DevGuard guard_(h->eng);
    RhsCtx c;
    c.tendency = tendency;
    c.Qin = Q;
    c.t = t;
    c.alpha = alpha;
    c.beta = beta;
    return set_err(h, h->eng->rhs_async(c));
}

int cmdg_rhs(cmdg_handle h, double *tendency, double *Q, double t, double alpha, double beta)
{
    int r = cmdg_rhs_async(h, tendency, Q, t, alpha, beta);
    if (r) return r;
    DevGuard guard_(h->eng);
    return set_err(h, h->eng->synchronize());
}

int cmdg_synchronize(cmdg_handle h)
{
    if (!h) return CMDG_ERR_INVALID;
    DevGuard guard_(h->eng);  // (waits for deferred runs)
    if (h->eng->worker) {     // a deferred run that failed reports here
        std::lock_guard<std::mutex> lk(h->eng->worker->m);
        if (const int r = h->eng->worker->deferred_rc) {
            h->eng->err = h->eng->worker->deferred_err;
            h->eng->worker->deferred_rc = 0;
            h->eng->worker->deferred_err.clear();
            return set_err(h, r);
        }
    }
    return set_err(h, h->eng->synchronize());
}

int cmdg_set_option(cmdg_handle h, int32_t option, int32_t value)
{
    if (!h) return CMDG_ERR_INVALID;
    DevGuard guard_(h->eng);
    EngineBase *e = h->eng;
    switch (option) {
    case CMDG_OPT_KEEP_GRADFLUX:
        e->drop_graph();
        e->keep_gradflux = value != 0;
        return CMDG_OK;
    case CMDG_OPT_STACK_HEIGHT:
        e->drop_graph();
        return set_err(h, e->set_stack_height(value));
    case CMDG_OPT_REFERENCE_HALO:
        if (int r = e->synchronize()) return set_err(h, r);
        e->drop_graph();
        e->reference_halo = value != 0 || e->fv || e->esdg;
        e->invalidate_sends();
        return CMDG_OK;
    case CMDG_OPT_STEP_GRAPH:
        if (int r = e->synchronize()) return set_err(h, r);
        e->drop_graph();
        e->step_graph = value != 0;
        e->graph_failed = false;
        return CMDG_OK;
    case CMDG_OPT_STREAM_PRIORITY: return set_err(h, e->set_stream_priority(value));
    case CMDG_OPT_ASYNC_RUN:
        if (value && !e->worker) {
            e->worker = new (std::nothrow) RunWorker();
            if (!e->worker) return set_err(h, e->fail(CMDG_ERR_INVALID, "async run: out of memory"));
            e->worker->start();
        } else if (!value && e->worker) {
            delete e->worker;  // (idle: DevGuard waited)
            e->worker = nullptr;
        }
        return CMDG_OK;
    case CMDG_OPT_TENDENCY_PAIRS:
    case CMDG_OPT_TENDENCY_FOUR_WAVES: return CMDG_OK;  // retired: no effect
    case CMDG_OPT_GRADARG_HANDOFF: e->gradarg_handoff = value != 0; return CMDG_OK;
    case CMDG_OPT_HALO_PIPELINE:
        if (int r = e->synchronize()) return set_err(h, r);
        e->drop_graph();
        e->no_pipeline = value == 0;
        e->invalidate_sends();
        return CMDG_OK;
    default: return set_err(h, e->fail(CMDG_ERR_INVALID, "cmdg_set_option: unknown option"));
    }
}

int cmdg_query(cmdg_handle h, int32_t what, int64_t *out)
{
    if (!h || !out) return CMDG_ERR_INVALID;
    const EngineBase *e = h->eng;
    switch (what) {
    case CMDG_Q_GRADFLUX_LIVE: *out = e->gf_live(); return CMDG_OK;
    case CMDG_Q_LAW_NEEDS_GRADFLUX: *out = e->law_needs_gradflux(); return CMDG_OK;
    case CMDG_Q_NDERIVED: *out = e->law_nder(); return CMDG_OK;
    case CMDG_Q_NUPDATED_AUX: *out = e->has_update_aux() ? e->law_nupd() : 0; return CMDG_OK;
    case CMDG_Q_FUSED_UPDATE_AUX: *out = e->has_update_aux() && e->fused_update_aux(); return CMDG_OK;
    case CMDG_Q_DIRECT_SEND: *out = e->communicate() && e->direct_send(); return CMDG_OK;
    case CMDG_Q_DIRECT_RECV: *out = e->communicate() && e->direct_recv(); return CMDG_OK;
    case CMDG_Q_TENDENCY_ELEMS_PER_GROUP: *out = e->tendency_epb(); return CMDG_OK;
    case CMDG_Q_GRAPH_STEPS: *out = e->graph_steps; return CMDG_OK;
    case CMDG_Q_TENDENCY_PAIRS: *out = -1; return CMDG_OK;  // retired option: always off
    case CMDG_Q_GRADARG_HANDOFF: *out = e->handoff_used; return CMDG_OK;
    case CMDG_Q_GRADARG_REFRESHES: *out = e->handoff_refreshes; return CMDG_OK;
    case CMDG_Q_HOST_POST_NS: *out = e->host_post_ns; return CMDG_OK;
    case CMDG_Q_HOST_POST_COUNT: *out = e->host_post_n; return CMDG_OK;
    case CMDG_Q_HALO_PIPELINE: *out = e->pipelined() && !e->has_hooks; return CMDG_OK;
    default:
        if (what >= CMDG_Q_STATE_READ && what < CMDG_Q_STATE_READ + 4) {
            *out = e->law_state_read(what - CMDG_Q_STATE_READ);
            return CMDG_OK;
        }
        if (what >= CMDG_Q_AUX_READ && what < CMDG_Q_AUX_READ + 4) {
            *out = e->law_aux_read(what - CMDG_Q_AUX_READ);
            return CMDG_OK;
        }
        return set_err(h, h->eng->fail(CMDG_ERR_INVALID, "cmdg_query: unknown item"));
    }
}

int cmdg_export_hypervisc_grad(cmdg_handle h, double *dst)
{
    if (!h) return CMDG_ERR_INVALID;
    DevGuard guard_(h->eng);
    return set_err(h, h->eng->export_hypgrad(dst));
}

int cmdg_export_gradient_flux(cmdg_handle h, double *dst)
{
    if (!h) return CMDG_ERR_INVALID;
    DevGuard guard_(h->eng);
    return set_err(h, h->eng->export_gradflux(dst));
}

int cmdg_halo_begin(cmdg_handle h, double *array, int32_t nstate)
{
    if (!h || !array) return CMDG_ERR_INVALID;
    DevGuard guard_(h->eng);
    h->eng->invalidate_sends();  // the caller's array: always packed
    return set_err(h, h->eng->halo_begin(SLOT_Q, array, nstate));
}
int cmdg_halo_end(cmdg_handle h, double *array, int32_t nstate)
{
    if (!h || !array) return CMDG_ERR_INVALID;
    DevGuard guard_(h->eng);
    return set_err(h, h->eng->halo_end(SLOT_Q, array, nstate));
}

int cmdg_fillsendbuf(double *sendbuf, const double *buf, const int64_t *vmapsend, int64_t nvmap,
                     int32_t Np, int32_t nstate)
{
    if (!sendbuf || !buf || !vmapsend || nvmap < 0 || Np < 1 || nstate < 1) return CMDG_ERR_INVALID;
    if (nvmap == 0) return CMDG_OK;
    const int64_t n = nvmap * nstate;
    hipLaunchKernelGGL(k_fillsendbuf, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, sendbuf, buf,
                       vmapsend, nvmap, Np, nstate, nstate);
    return hipGetLastError() == hipSuccess && hipStreamSynchronize(0) == hipSuccess ? CMDG_OK : CMDG_ERR_HIP;
}

int cmdg_transferrecvbuf(double *buf, const double *recvbuf, const int64_t *vmaprecv,
                         int64_t nvmap, int32_t Np, int32_t nstate)
{
    if (!buf || !recvbuf || !vmaprecv || nvmap < 0 || Np < 1 || nstate < 1) return CMDG_ERR_INVALID;
    if (nvmap == 0) return CMDG_OK;
    const int64_t n = nvmap * nstate;
    hipLaunchKernelGGL(k_transferrecvbuf, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, buf,
                       recvbuf, vmaprecv, nvmap, Np, nstate, nstate);
    return hipGetLastError() == hipSuccess && hipStreamSynchronize(0) == hipSuccess ? CMDG_OK : CMDG_ERR_HIP;
}

int cmdg_comm_unique_id(void *out128)
{
    std::string err;
    if (!out128) return CMDG_ERR_INVALID;
    if (!rccl::load(err)) {
        g_create_err = err;
        return CMDG_ERR_COMM;
    }
    rccl::uid_t id;
    if (rccl::GetUniqueId(&id)) return CMDG_ERR_COMM;
    memcpy(out128, &id, sizeof(id));
    return CMDG_OK;
}

int cmdg_comm_init_rccl(cmdg_handle h, const void *unique_id128, int32_t rank, int32_t nranks)
{
    if (!h || !unique_id128 || rank < 0 || rank >= nranks) return CMDG_ERR_INVALID;
    DevGuard guard_(h->eng);
    EngineBase *e = h->eng;
    if (!rccl::load(e->err)) return set_err(h, CMDG_ERR_COMM);
    rccl::uid_t id;
    memcpy(&id, unique_id128, sizeof(id));
    if (int rc = rccl::CommInitRank(&e->nccl_comm, nranks, id, rank))
        return set_err(h, e->fail(CMDG_ERR_COMM, std::string("ncclCommInitRank: ") +
                                                   rccl::GetErrorString(rc)));
    e->transport = TRANSPORT_RCCL;
    e->rank = rank;
    e->nranks = nranks;
    return CMDG_OK;
}

int cmdg_comm_selftest(cmdg_handle h, int64_t count)
{
    if (!h || count < 1) return CMDG_ERR_INVALID;
    DevGuard guard_(h->eng);
    EngineBase *e = h->eng;
    if (e->transport != TRANSPORT_RCCL || !e->nccl_comm)
        return set_err(h, e->fail(CMDG_ERR_COMM, "selftest: RCCL transport not initialised"));
    DevBuf<double> src, dst;
    std::vector<double> host((size_t)count), back((size_t)count, -1.0);
    for (int64_t i = 0; i < count; ++i) host[i] = 0.5 * (double)i + 1e-3 * e->rank;
    int rc = CMDG_OK;
    if (src.alloc(count) != hipSuccess || dst.alloc(count) != hipSuccess)
        rc = e->fail(CMDG_ERR_HIP, "selftest: hipMalloc failed");
    if (!rc && hipMemcpy(src, host.data(), sizeof(double) * count, hipMemcpyHostToDevice) != hipSuccess)
        rc = e->fail(CMDG_ERR_HIP, "selftest: upload failed");
    if (!rc) {
        int n = rccl::GroupStart();
        if (!n) n = rccl::Recv(dst, (size_t)count, rccl::kDouble, e->rank, e->nccl_comm, e->s_comm);
        if (!n) n = rccl::Send(src, (size_t)count, rccl::kDouble, e->rank, e->nccl_comm, e->s_comm);
        int g = rccl::GroupEnd();
        if (n || g) rc = e->fail(CMDG_ERR_COMM, std::string("selftest: ") + rccl::GetErrorString(n ? n : g));
    }
    if (!rc && hipStreamSynchronize(e->s_comm) != hipSuccess) rc = e->fail(CMDG_ERR_HIP, "selftest: sync failed");
    if (!rc && hipMemcpy(back.data(), dst, sizeof(double) * count, hipMemcpyDeviceToHost) != hipSuccess)
        rc = e->fail(CMDG_ERR_HIP, "selftest: download failed");
    if (!rc && memcmp(back.data(), host.data(), sizeof(double) * count) != 0)
        rc = e->fail(CMDG_ERR_COMM, "selftest: payload mismatch");
    return set_err(h, rc);
}

int cmdg_comm_connect_local(cmdg_handle *handles, int32_t n)
{
    GroupCall gc(handles, n);
    if (!gc.ok()) return CMDG_ERR_INVALID;
    std::vector<EngineBase *> g;
    for (int i = 0; i < n; ++i) {
        g.push_back(handles[i]->eng);
        if (g[i]->dev != g[0]->dev)
            return gc.finish(g[i]->fail(CMDG_ERR_INVALID, "local transport: the handles of a group live on one device"));
    }
    for (int i = 0; i < n; ++i) {
        g[i]->group = g;
        g[i]->rank = i;
        g[i]->nranks = n;
        g[i]->transport = TRANSPORT_LOCAL;
        for (int r : g[i]->nabrtorank)
            if (r < 0 || r >= n) return gc.finish(g[i]->fail(CMDG_ERR_COMM, "neighbour rank outside the local group"));
    }
    return CMDG_OK;
}

int cmdg_group_rhs(cmdg_handle *handles, int32_t n, double **tendency, double **Q, double t,
                   double alpha, double beta)
{
    if (!tendency || !Q) return CMDG_ERR_INVALID;
    for (int i = 0; i < n; ++i)
        if (!tendency[i] || !Q[i]) return CMDG_ERR_INVALID;
    GroupCall gc(handles, n);
    if (!gc.ok()) return CMDG_ERR_INVALID;
    std::vector<EngineBase *> g;
    std::vector<RhsCtx> c(n);
    for (int i = 0; i < n; ++i) {
        g.push_back(handles[i]->eng);
        c[i].tendency = tendency[i];
        c[i].Qin = Q[i];
        c[i].t = t;
        c[i].alpha = alpha;
        c[i].beta = beta;
    }
    return gc.finish(group_rhs(g, c));
}

int cmdg_group_halo(cmdg_handle *handles, int32_t n, double **arrays, int32_t nstate)
{
    if (!arrays) return CMDG_ERR_INVALID;
    for (int i = 0; i < n; ++i)
        if (!arrays[i]) return CMDG_ERR_INVALID;
    GroupCall gc(handles, n);
    if (!gc.ok()) return CMDG_ERR_INVALID;
    for (int i = 0; i < n; ++i) handles[i]->eng->invalidate_sends();
    for (int i = 0; i < n; ++i)
        if (int r = handles[i]->eng->halo_begin(SLOT_Q, arrays[i], nstate)) return gc.finish(r);
    for (int i = 0; i < n; ++i)
        if (int r = handles[i]->eng->halo_end(SLOT_Q, arrays[i], nstate)) return gc.finish(r);
    for (int i = 0; i < n; ++i)
        if (int r = handles[i]->eng->synchronize()) return gc.finish(r);
    return CMDG_OK;
}

int cmdg_norm2_local(cmdg_handle h, const double *A, int32_t nstate, int32_t weighted,
                     double *out_host)
{
    if (!h || !A || !out_host) return CMDG_ERR_INVALID;
    DevGuard guard_(h->eng);
    return set_err(h, h->eng->wsum2(A, nullptr, nstate, weighted, out_host));
}
int cmdg_distance2_local(cmdg_handle h, const double *A, const double *B, int32_t nstate,
                         double *out_host)
{
    if (!h || !A || !B || !out_host) return CMDG_ERR_INVALID;
    DevGuard guard_(h->eng);
    return set_err(h, h->eng->wsum2(A, B, nstate, 1, out_host));
}

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
    if (r) g_create_err = "cmdg_reduce_combine: " + err;
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

int cmdg_courant(cmdg_handle h, int32_t kind, const double *Q, double dt, double simtime,
                 int32_t direction, double *out_host)
{
    if (!h || !Q || !out_host) return CMDG_ERR_INVALID;
    DevGuard guard_(h->eng);
    if (h->eng->fv)
        return set_err(h, h->eng->fail(CMDG_ERR_UNSUPPORTED, "courant: the device Courant number is not defined "
                                                             "for a finite-volume vertical (DGFVModel handle)"));
    return set_err(h, h->eng->courant(1, kind, Q, dt, simtime, direction, out_host));
}

int cmdg_min_node_distance(cmdg_handle h, int32_t direction, double *out_host)
{
    if (!h || !out_host) return CMDG_ERR_INVALID;
    DevGuard guard_(h->eng);
    if (h->eng->fv)
        return set_err(h, h->eng->fail(CMDG_ERR_UNSUPPORTED, "min_node_distance: on a DGFVModel handle the vertical "
                                                             "distance is the cell height 2 JcV; use the host grid's"));
    return set_err(h, h->eng->courant(0, 0, nullptr, 0.0, 0.0, direction, out_host));
}

int cmdg_indefinite_stack_integral(cmdg_handle h, const double *Q, int32_t nstate, double *aux,
                                   int32_t naux, int32_t nvertelem, const double *Imat,
                                   const cmdg_stack_integral_desc *d)
{
    if (!h || !aux || !d || naux < 1) return CMDG_ERR_INVALID;
    DevGuard guard_(h->eng);
    return set_err(h, h->eng->stack_integral(false, Q, nstate, aux, naux, nvertelem, Imat, d));
}

int cmdg_reverse_indefinite_stack_integral(cmdg_handle h, double *aux, int32_t naux,
                                           int32_t nvertelem, const cmdg_stack_integral_desc *d)
{
    if (!h || !aux || !d || naux < 1) return CMDG_ERR_INVALID;
    DevGuard guard_(h->eng);
    return set_err(h, h->eng->stack_integral(true, nullptr, 0, aux, naux, nvertelem, nullptr, d));
}

int cmdg_filter_create(cmdg_handle h, const cmdg_filter_desc *d, cmdg_filter *out)
{
    if (!h || !d || !out) return CMDG_ERR_INVALID;
    DevGuard guard_(h->eng);
    FilterObj *f = nullptr;
    int r = h->eng->filter_create(d, &f);
    *out = reinterpret_cast<cmdg_filter>(f);
    return set_err(h, r);
}

int cmdg_filter_destroy(cmdg_handle h, cmdg_filter f)
{
    if (!h || !f) return CMDG_ERR_INVALID;
    DevGuard guard_(h->eng);
    EngineBase *e = h->eng;
    FilterObj *o = reinterpret_cast<FilterObj *>(f);
    e->synchronize();
    if (e->gradient_filter == o) e->gradient_filter = nullptr;
    if (e->tendency_filter == o) e->tendency_filter = nullptr;
    if (e->step_filter == o) e->step_filter = nullptr;
    // a recorded update_auxiliary_state! composition may name this filter: drop it from there
    {
        int k = 0;
        for (int i = 0; i < e->hooks.npre; ++i)
            if (e->hooks.pre_filter[i] != f) e->hooks.pre_filter[k++] = e->hooks.pre_filter[i];
        e->hooks.npre = k;
    }
    delete o;
    return CMDG_OK;
}

int cmdg_filter_apply(cmdg_handle h, cmdg_filter f, double *Q, int32_t nstate)
{
    if (!h || !f || !Q || nstate < 1) return CMDG_ERR_INVALID;
    DevGuard guard_(h->eng);
    return set_err(h, h->eng->filter_apply(reinterpret_cast<FilterObj *>(f), Q, nstate));
}

// ---- interpolation (interpolation.hip) ------------------------------------------------------
namespace {
// the device of an interpolation object made current for a call without a handle
struct InterpDevice {
    int prev = -1;
    bool changed = false;
    explicit InterpDevice(int dev)
    {
        if (hipGetDevice(&prev) == hipSuccess && prev != dev) changed = hipSetDevice(dev) == hipSuccess;
    }
    ~InterpDevice()
    {
        if (changed) (void)hipSetDevice(prev);
    }
};
// one epilogue: the message goes to the handle, or to cmdg_last_error(NULL) without one
int interp_done(cmdg_handle h, int r, const std::string &err)
{
    if (r == CMDG_OK) return r;
    if (h) return set_err(h, h->eng->fail(r, err));
    g_create_err = err;
    return r;
}
}  // namespace

int cmdg_interp_create(cmdg_handle h, const cmdg_interp_desc *d, cmdg_interp *out)
{
    if (!d || !out) return CMDG_ERR_INVALID;
    std::optional<DevGuard> guard_;
    if (h) guard_.emplace(h->eng);
    InterpObj *o = nullptr;
    std::string err;
    const int r = interp_create(d, &o, err);
    *out = reinterpret_cast<cmdg_interp>(o);
    return interp_done(h, r, err);
}

int cmdg_interp_destroy(cmdg_handle h, cmdg_interp it)
{
    if (!it) return CMDG_ERR_INVALID;
    InterpObj *o = reinterpret_cast<InterpObj *>(it);
    std::optional<DevGuard> guard_;
    if (h) {
        guard_.emplace(h->eng);
        h->eng->synchronize();
    }
    InterpDevice dev_(interp_device(o));
    (void)hipStreamSynchronize(nullptr);  // (calls without a handle have returned; see include/cmdg.h)
    interp_destroy(o);
    return CMDG_OK;
}

int cmdg_interp_apply(cmdg_handle h, cmdg_interp it, const double *Q, int32_t nstate, int64_t nelemQ, double *v)
{
    if (!it || !Q || !v || nstate < 1) return CMDG_ERR_INVALID;
    const InterpObj *o = reinterpret_cast<const InterpObj *>(it);
    std::optional<DevGuard> guard_;
    if (h) guard_.emplace(h->eng);
    std::string err;
    if (h && h->eng->dev != interp_device(o))
        return interp_done(h, CMDG_ERR_INVALID, "cmdg_interp_apply: the object lives on another device than the handle");
    InterpDevice dev_(interp_device(o));
    return interp_done(h, interp_apply(o, Q, nstate, nelemQ, v, h ? h->eng->s_comp : nullptr, !h, err), err);
}

int cmdg_interp_project(cmdg_handle h, cmdg_interp it, double *v, int32_t nstate, const int32_t uvwi[3])
{
    if (!it || !v || !uvwi || nstate < 1) return CMDG_ERR_INVALID;
    const InterpObj *o = reinterpret_cast<const InterpObj *>(it);
    std::optional<DevGuard> guard_;
    if (h) guard_.emplace(h->eng);
    std::string err;
    if (h && h->eng->dev != interp_device(o))
        return interp_done(h, CMDG_ERR_INVALID, "cmdg_interp_project: the object lives on another device than the handle");
    InterpDevice dev_(interp_device(o));
    return interp_done(h, interp_project(o, v, nstate, uvwi, h ? h->eng->s_comp : nullptr, !h, err), err);
}

int cmdg_interp_scatter(cmdg_handle h, const cmdg_interp *its, int32_t n, const double *const *v, int32_t nstate,
                        double *fiv)
{
    if (!its || !v || !fiv || n < 1 || nstate < 1) return CMDG_ERR_INVALID;
    for (int i = 0; i < n; ++i)
        if (!its[i]) return CMDG_ERR_INVALID;
    const InterpObj *const *o = reinterpret_cast<const InterpObj *const *>(its);
    std::optional<DevGuard> guard_;
    if (h) guard_.emplace(h->eng);
    std::string err;
    if (h && h->eng->dev != interp_device(o[0]))
        return interp_done(h, CMDG_ERR_INVALID, "cmdg_interp_scatter: the objects live on another device than the handle");
    InterpDevice dev_(interp_device(o[0]));
    return interp_done(h, interp_scatter(o, n, v, nstate, fiv, h ? h->eng->s_comp : nullptr, !h, err), err);
}

int cmdg_set_filters(cmdg_handle h, cmdg_filter gradient_filter, cmdg_filter tendency_filter,
                     cmdg_filter step_filter)
{
    if (!h) return CMDG_ERR_INVALID;
    DevGuard guard_(h->eng);
    EngineBase *e = h->eng;
    auto *gfl = reinterpret_cast<FilterObj *>(gradient_filter);
    auto *tfl = reinterpret_cast<FilterObj *>(tendency_filter);
    for (FilterObj *o : {gfl, tfl})
        if (o && o->target != CMDG_TARGET_INDICES)
            return set_err(h, e->fail(CMDG_ERR_INVALID, "gradient/tendency filters take FilterIndices targets"));
    // filters decide which streams the next evaluation's launches go to: start it from a clean slate
    if (int r = e->synchronize()) return set_err(h, r);
    e->invalidate_sends();
    e->drop_graph();
    e->gradient_filter = gfl;
    e->tendency_filter = tfl;
    e->step_filter = reinterpret_cast<FilterObj *>(step_filter);
    return CMDG_OK;
}

int cmdg_set_rhs_hooks(cmdg_handle h, const cmdg_rhs_hooks *hooks)
{
    if (!h) return CMDG_ERR_INVALID;
    DevGuard guard_(h->eng);
    if (int r = h->eng->synchronize()) return set_err(h, r);  // (hooks change the stream layout too)
    h->eng->invalidate_sends();
    h->eng->drop_graph();
    return set_err(h, h->eng->set_hooks(hooks));
}

int cmdg_profile_enable(cmdg_handle h, int32_t on)
{
    if (!h) return CMDG_ERR_INVALID;
    DevGuard guard_(h->eng);
    h->eng->drop_graph();
    h->eng->profiling = on != 0;
    return CMDG_OK;
}
int cmdg_profile_get(cmdg_handle h, int32_t kernel, double *total_ms, int64_t *launches)
{
    if (!h || kernel < 0 || kernel >= CMDG_K_COUNT) return CMDG_ERR_INVALID;
    DevGuard guard_(h->eng);
    h->eng->synchronize();
    h->eng->prof_collect();
    if (total_ms) *total_ms = h->eng->prof_ms[kernel];
    if (launches) *launches = h->eng->prof_n[kernel];
    return CMDG_OK;
}
int cmdg_profile_reset(cmdg_handle h)
{
    if (!h) return CMDG_ERR_INVALID;
    DevGuard guard_(h->eng);
    h->eng->synchronize();
    h->eng->prof_collect();
    for (int i = 0; i < CMDG_K_COUNT; ++i) {
        h->eng->prof_ms[i] = 0;
        h->eng->prof_n[i] = 0;
    }
    return CMDG_OK;
}

}  // extern "C"
