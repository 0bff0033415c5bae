// libcmdg: the engine's construction and its evaluation (rhs_segment), and the C entries of
// include/cmdg.h for them; the exchange is in halo.hip, the create path in create.hip.
#include <dlfcn.h>

#include <algorithm>
#include <new>
#include <tuple>

#include "lapfused_tables.h"
#include "rccl.h"
#include "stepping.h"

namespace cmdg {

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

// One-time digest of the reference face tables (see GridDev); bad[0] collects what does not
// hold: bit 0 vmap- is not the canonical face numbering, bit 1 sgeo's vMI is not vgeo's MI at
// the face node, bit 2 a plus-side id does not fit 32 bits.
static __global__ void k_face_digest(const double *__restrict__ vgeo, int nvgeo,
                                     const double *__restrict__ sgeo,
                                     const int64_t *__restrict__ vmapM,
                                     const int64_t *__restrict__ vmapP,
                                     const int64_t *__restrict__ elemtobndy, int NQ, int NQV,
                                     int64_t nreal, int32_t *__restrict__ faceP,
                                     double *__restrict__ faceG, double *__restrict__ faceW,
                                     int32_t *__restrict__ facePr, int *__restrict__ bad)
{
    const int Np = NQ * NQ * NQV, Nfph = NQ * NQV, Nfpv = NQ * NQ;
    const int Nfp = Nfph > Nfpv ? Nfph : Nfpv, NFT = 4 * Nfph + 2 * Nfpv;
    const int64_t I = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (I >= nreal * NFT) return;
    const int64_t e = I / NFT;
    const int t = (int)(I % NFT);
    int f, n;
    if (t < 4 * Nfph) {
        f = t / Nfph;
        n = t % Nfph;
    } else {
        f = 4 + (t - 4 * Nfph) / Nfpv;
        n = (t - 4 * Nfph) % Nfpv;
    }
    const int64_t o = n + (int64_t)Nfp * (f + 6 * e);
    const int a = n % NQ, b = n / NQ;
    int vid;
    switch (f) {
    case 0: vid = NQ * (a + NQ * b); break;
    case 1: vid = (NQ - 1) + NQ * (a + NQ * b); break;
    case 2: vid = a + NQ * NQ * b; break;
    case 3: vid = a + NQ * ((NQ - 1) + NQ * b); break;
    case 4: vid = n; break;
    default: vid = n + NQ * NQ * (NQV - 1); break;
    }
    int flags = 0;
    const int64_t idM = vmapM[o] - 1;
    if (idM != e * Np + vid) flags |= 1;
    int64_t idP = vmapP[o] - 1;
    if (elemtobndy[f + 6 * e] != 0) idP = e * Np + vid;  // DGModel_kernels.jl:686-692
    if (idP < 0 || idP > 2147483647LL) flags |= 4;
    faceP[I] = (int32_t)idP;
    const int64_t eP = idP >= 0 ? idP / Np : 0;
    facePr[I] = (int32_t)(eP * Np + ring_slot_of(NQ, NQV, (int)(idP - eP * Np)));
    const double *sg = sgeo + 5 * o;
#pragma unroll
    for (int c = 0; c < 4; ++c) faceG[((int64_t)4 * e + c) * NFT + t] = sg[c];
    const double mi = vgeo[vid + (int64_t)Np * (VMI + (int64_t)nvgeo * e)];
    if (!(sg[SVMI] == mi)) flags |= 2;
    faceW[I] = mi * sg[SSM];  // fp.vMI * fp.sM as the passes formed it
    if (flags) atomicOr(bad, flags);
}

// The doubles of the fused Laplacian pass's table (lapT of k_lapfused) once the host has found tP
// and tE (lapfused_tables.h): the neighbour's horizontal metric rows at the plus node, its normal and
// lift weight at its own face task of the shared node; and, behind these rows, the edge block: its
// normal and lift weight at tE, for the two tasks of a row that have one.
static __global__ void k_lapfused_fill(const double *__restrict__ vgeo, int nvgeo, const int32_t *__restrict__ faceP,
                                       const double *__restrict__ faceG, const double *__restrict__ faceW,
                                       const int32_t *__restrict__ lapI, const int32_t *__restrict__ tE_of, int NQ,
                                       int NQV, int64_t nreal, double *__restrict__ lapT)
{
    const int Np = NQ * NQ * NQV, Nfph = NQ * NQV, NL = 4 * Nfph, NFT = NL + 2 * NQ * NQ, NE = 8 * NQV;
    const int64_t I = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (I >= nreal * NL) return;
    const int64_t e = I / NL;
    const int t = (int)(I % NL);
    const int64_t idP = faceP[NFT * e + t], N = idP / Np;
    const int vidP = (int)(idP - N * Np), tP = lapI[(2 * e + 0) * NL + t], tE = tE_of[I];
    const double *vg = vgeo + (int64_t)Np * nvgeo * N + vidP;
    const int rows[6] = {XI1X1, XI1X2, XI1X3, XI2X1, XI2X2, XI2X3};
    double *dst = lapT + (int64_t)(10 * NL + 4 * NE) * e + t;
#pragma unroll
    for (int c = 0; c < 6; ++c) dst[(int64_t)c * NL] = vg[(int64_t)rows[c] * Np];
#pragma unroll
    for (int c = 0; c < 3; ++c) dst[(int64_t)(6 + c) * NL] = faceG[((int64_t)4 * N + c) * NFT + tP];
    dst[(int64_t)9 * NL] = faceW[NFT * N + tP];
    if (tE < 0) return;
    const bool last = lapfused_index_in_face(NQ, tP / Nfph, vidP) == NQ - 1;
    double *edge = lapT + (int64_t)(10 * NL + 4 * NE) * e + 10 * NL + lapfused_edge_slot(NQV, t / Nfph, (t % Nfph) / NQ, last);
#pragma unroll
    for (int c = 0; c < 3; ++c) edge[c * NE] = faceG[((int64_t)4 * N + c) * NFT + tE];
    edge[3 * NE] = faceW[NFT * N + tE];
}

// CMDG_OPT_FUSED_LAPLACIAN: is this a handle whose hand-off evaluations can take k_lapfused?  What
// can be known at create is decided here, once: the law and order hand gradient arguments on, one
// rank without ghosts, horizontal diffusion, a Laplacian pass that overwrites all of
// Qhypervisc_grad (what the gradient pass would have left there is then seen by nobody), and a grid
// that lapfused_build accepts.  Everything else keeps the two kernels (lapfused_ok stays false).
int EngineBase::init_lapfused()
{
    if (!garg_capable() || ngl <= 0 || nhyp != 3 * ngl || diffusion_direction != DIR_HORIZONTAL || nghost != 0 ||
        communicate() || fv || esdg || nreal < 1)
        return CMDG_OK;
    const int NFT = 4 * NQ * NQV + 2 * NQ * NQ, NL = 4 * NQ * NQV;
    std::vector<int32_t> h_faceP((size_t)(nreal * NFT));
    std::vector<int64_t> h_bndy((size_t)(6 * nreal));
    HIPCHK(hipMemcpy(h_faceP.data(), d_faceP, sizeof(int32_t) * h_faceP.size(), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(h_bndy.data(), g.elemtobndy, sizeof(int64_t) * h_bndy.size(), hipMemcpyDeviceToHost));
    LapFusedTables tab;
    lapfused_build(NQ, NQV, nreal, h_faceP.data(), h_bndy.data(), tab);
    if (!tab.eligible) return CMDG_OK;
    // lapI[e][c][t]: tP and idE; tE goes to the kernel that fills lapT and no further
    std::vector<int32_t> h_lapI((size_t)(2 * NL * nreal));
    for (int64_t e = 0; e < nreal; ++e)
        for (int t = 0; t < NL; ++t) {
            h_lapI[(size_t)((2 * e + 0) * NL + t)] = tab.tP[(size_t)(NL * e + t)];
            h_lapI[(size_t)((2 * e + 1) * NL + t)] = tab.idE[(size_t)(NL * e + t)];
        }
    DevBuf<int32_t> d_tE;
    HIPCHK(d_lapI.alloc(h_lapI.size()));
    HIPCHK(d_tE.alloc(tab.tE.size()));
    HIPCHK(d_lapT.alloc((size_t)((10 * NL + 4 * 8 * NQV) * nreal)));
    HIPCHK(hipMemcpy(d_lapI, h_lapI.data(), sizeof(int32_t) * h_lapI.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_tE, tab.tE.data(), sizeof(int32_t) * tab.tE.size(), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_lapfused_fill, dim3((unsigned)((nreal * NL + 255) / 256)), dim3(256), 0, s_comp, g.vgeo,
                       g.nvgeo, d_faceP.get(), d_faceG.get(), d_faceW.get(), d_lapI.get(), d_tE.get(), NQ, NQV, nreal,
                       d_lapT.get());
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(s_comp) != hipSuccess)
        return fail(CMDG_ERR_HIP, "cmdg_create: the tables of the fused Laplacian pass failed");
    lapfused_ok = true;
    return CMDG_OK;
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
        HIPCHK(d_faceW.alloc(nt));
        HIPCHK(d_facePr.alloc(nt));
        HIPCHK(d_bad.alloc_zeroed(1, s_comp));  // (stream-ordered before the digest, see below)
        if (nreal > 0)
            hipLaunchKernelGGL(k_face_digest, dim3((unsigned)((nreal * NFT + 255) / 256)), dim3(256), 0,
                               s_comp, g.vgeo, g.nvgeo, g.sgeo, g.vmapM, g.vmapP, g.elemtobndy, NQ,
                               NQV, nreal, d_faceP.get(), d_faceG.get(), d_faceW.get(), d_facePr.get(),
                               d_bad.get());
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
        g.faceW = d_faceW;
        g.facePr = d_facePr;
    }
    if (int r = init_lapfused()) return r;
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

// the records of CMDG_OPT_GRADARG_HANDOFF (gradient arguments, and the Laplacians of the run's
// ring-ordered evaluations), allocated by the first run that uses them: the fill is stream-ordered
// before the run's launches like that of the work states
int EngineBase::ensure_garg()
{
    if (!garg) {
        const size_t n = std::max<size_t>((size_t)Np * ngl * nelem, 1);
        HIPCHK(garg.alloc_zeroed(n, s_comp));
        HIPCHK(lapr.alloc_zeroed(n, s_comp));
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
// ---------------------------------------------------------------------------------
// A node-major array of the library (ncol, Np, nelem) into the reference layout (Np, ncol, nelem) of
// a caller that asked for it (create_states.jl:17-26), and back.
static __global__ void k_export_node_major(double *__restrict__ dst, const double *__restrict__ src, int Np,
                                           int ncol, int64_t nelem)
{
    const int64_t I = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (I >= (int64_t)Np * ncol * nelem) return;
    const int64_t e = I / ((int64_t)Np * ncol);
    const int r = (int)(I - e * Np * ncol), s = r / Np, n = r - s * Np;
    dst[I] = src[s + (int64_t)ncol * (n + (int64_t)Np * e)];
}
static __global__ void k_import_node_major(double *__restrict__ dst, const double *__restrict__ src, int Np,
                                           int ncol, int64_t nelem)
{
    const int64_t I = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (I >= (int64_t)Np * ncol * nelem) return;
    const int64_t e = I / ((int64_t)Np * ncol);
    const int r = (int)(I - e * Np * ncol), n = r / ncol, s = r - n * ncol;
    dst[I] = src[n + (int64_t)Np * (s + (int64_t)ncol * e)];
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
    // a pass launch between a begin and its end: the bracket is closed whether the launch failed (the
    // engine class has no kernel for what it was asked) or not, and the launch's failure comes first
    auto closed = [&](int launched, auto &end) -> int {
        const int ended = end();
        return launched != CMDG_OK ? launched : ended;
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
            TRY(closed(launch_gradients(c, d_interior, ninterior, false, s_comp), interior_end));
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
        TRY(closed(launch_gradients(c, d_exterior, nexterior, comm, s_ext), exterior_end));
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
            TRY(closed(launch_divgrad(c, d_interior, ninterior, false, s_comp), interior_end));
        }
        break;
    case 2:
        if (!hyper) break;
        if (comm) TRY(halo_end(SLOT_HG, hypgrad, 3 * ngl, unpack, pipe));
        if (dsend) TRY(before_direct_send(SLOT_HD, s_ext));
        TRY(exterior_begin());
        TRY(closed(launch_divgrad(c, d_exterior, nexterior, comm, s_ext), exterior_end));
        if (dsend) mark_fresh(SLOT_HD, hypdiv, nhd);
        if (comm) TRY(halo_begin(SLOT_HD, hypdiv, nhd, nhyp, pipe));
        TRY(interior_begin());
        TRY(closed(launch_gradlap(c, d_interior, ninterior, false, s_comp), interior_end));
        break;
    case 3:
        if (hyper) {
            if (comm) TRY(halo_end(SLOT_HD, hypdiv, nhd, unpack, pipe));
            if (dsend) TRY(before_direct_send(SLOT_HG, s_ext));
            TRY(exterior_begin());
            TRY(closed(launch_gradlap(c, d_exterior, nexterior, comm, s_ext), exterior_end));
            if (dsend) mark_fresh(SLOT_HG, hypgrad, 3 * ngl);
            if (comm) TRY(halo_begin(SLOT_HG, hypgrad, 3 * ngl, 0, pipe));
        }
        TRY(interior_begin());
        TRY(closed(launch_tendency(c, d_interior, ninterior, false, s_comp), interior_end));
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
        TRY(closed(launch_tendency(c, d_exterior, nexterior, comm, s_ext), exterior_end));
        if (dsend && c.lsrk) mark_fresh(SLOT_Q, c.Qout, ns);
        // whatever follows on the compute stream (a filter, the caller's next call, the next
        // evaluation's first interior launch) finds this evaluation complete
        if (pipe && (dbg_sync() & 128)) HIPCHK(hipStreamSynchronize(s_comm));
        if (pipe) HIPCHK(hipStreamWaitEvent(s_comp, EE[evi(pass_seq)], 0));
        if (tendency_filter) TRY(filter_apply(tendency_filter, c.tendency, ns));  // (:417-425)
        if (c.update_after) {
            const int64_t n = (int64_t)Np * ns * nreal;
            lsrk_update(s_comp, c.tendency, c.Qin, c.rka_next, c.rkb_dt, n);
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

// extremum of n values into out[0] (one block)
static __global__ void k_extremum(const double *__restrict__ v, int64_t n, int is_min,
                                  double *__restrict__ out)
{
    __shared__ double s[1024];
    double a = is_min ? INFINITY : -INFINITY;
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x) a = is_min ? fmin(a, v[i]) : fmax(a, v[i]);
    s[threadIdx.x] = a;
    __syncthreads();
    for (int h = blockDim.x / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h)
            s[threadIdx.x] = is_min ? fmin(s[threadIdx.x], s[threadIdx.x + h])
                                    : fmax(s[threadIdx.x], s[threadIdx.x + h]);
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = s[0];
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

// ---------------------------------------------------------------------------------
// local part of norm / euclidean_distance (MPIStateArrays.jl:583-644): per-block
// partial sums in a fixed order (deterministic), finished on the host.
static __global__ void k_wsum2(const double *__restrict__ A, const double *__restrict__ B,
                        const double *__restrict__ vgeo, int nvgeo, int Np, int nvar,
                        int64_t nreal, int weighted, double *__restrict__ partial)
{
    __shared__ double sh[256];
    const int64_t total = (int64_t)Np * nvar * nreal;
    double acc = 0.0;
    for (int64_t I = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; I < total;
         I += (int64_t)gridDim.x * blockDim.x) {
        const int64_t e = I / ((int64_t)Np * nvar);
        const int n = (int)(I % Np);
        double d = A[I];
        if (B) d -= B[I];
        const double w = weighted ? vgeo[n + (int64_t)Np * (VM + (int64_t)nvgeo * e)] : 1.0;
        acc += w * d * d;
    }
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = sh[0];
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

extern "C" {

const char *cmdg_version(void) { return "cmdg 0.1 (gfx950)"; }

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

int cmdg_esdg_entropy(cmdg_handle h, const double *Q, double *beta, double *eta)
{
    if (!h || !Q) return CMDG_ERR_INVALID;
    DevGuard guard_(h->eng);
    return set_err(h, h->eng->launch_entropy(Q, beta, eta));
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
    case CMDG_OPT_FUSED_LAPLACIAN: e->fused_laplacian = value != 0; return CMDG_OK;
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
    case CMDG_Q_FUSED_LAPLACIAN: *out = e->fused_launches; return CMDG_OK;
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
