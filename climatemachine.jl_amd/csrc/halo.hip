// libcmdg: the ghost exchange -- the RCCL loader, the tables of the exchange without pack / unpack
// launches, begin_ghost_exchange! / end_ghost_exchange! and the transports' C entries.
#include <dlfcn.h>

#include <chrono>
#include <cstring>

#include "engine_base.h"
#include "rccl.h"

namespace cmdg {

// ---- RCCL, resolved lazily so that single-GPU use has no link-time dependency -------
namespace rccl {
static void *lib = nullptr;
GetUniqueId_t GetUniqueId;
CommInitRank_t CommInitRank;
CommDestroy_t CommDestroy;
GroupStart_t GroupStart;
GroupEnd_t GroupEnd;
Send_t Send;
Recv_t Recv;
GetErrorString_t GetErrorString;
AllGather_t AllGather;
bool load(std::string &err)
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

// ---------------------------------------------------------------------------------
// kernel_fillsendbuf! / kernel_transferrecvbuf!  MPIStateArrays.jl:837-871
// (nvar = columns per position of the packed buffer = the leading columns of the ncol-column array;
// the reference packs whole arrays, nvar == ncol)
static __global__ void k_fillsendbuf(double *__restrict__ sendbuf, const double *__restrict__ buf,
                              const int64_t *__restrict__ vmapsend, int64_t nvmap, int Np,
                              int nvar, int ncol, int node_major = 0)
{
    const int64_t I = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (I >= nvmap * nvar) return;
    const int64_t i = I / nvar;
    const int s = (int)(I % nvar);
    const int64_t id = vmapsend[i] - 1;
    const int64_t e = id / Np, n = id % Np;
    sendbuf[s + (int64_t)nvar * i] = node_major ? buf[s + (int64_t)ncol * (n + (int64_t)Np * e)]
                                                : buf[n + (int64_t)Np * (s + (int64_t)ncol * e)];
}
static __global__ void k_transferrecvbuf(double *__restrict__ buf, const double *__restrict__ recvbuf,
                                  const int64_t *__restrict__ vmaprecv, int64_t nvmap, int Np,
                                  int nvar, int ncol, int node_major = 0)
{
    const int64_t I = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (I >= nvmap * nvar) return;
    const int64_t i = I / nvar;
    const int s = (int)(I % nvar);
    const int64_t id = vmaprecv[i] - 1;
    const int64_t e = id / Np, n = id % Np;
    buf[node_major ? s + (int64_t)ncol * (n + (int64_t)Np * e) : n + (int64_t)Np * (s + (int64_t)ncol * e)] =
        recvbuf[s + (int64_t)nvar * i];
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

}  // namespace cmdg

using namespace cmdg;

extern "C" {

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
        set_create_err(err);
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

}  // extern "C"
