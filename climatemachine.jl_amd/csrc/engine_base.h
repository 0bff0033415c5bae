// Host-side engine: owns streams, events, halo buffers and work buffers of one handle
// and enqueues the passes of one right-hand-side evaluation in the order of the
// reference's `(dg::DGModel)(tendency, Q, _, t, alpha, beta)`
// (src/Numerics/DGMethods/DGModel.jl:85-427).  The physics/polynomial-order specific
// kernel launches live in EngineLaw<P, NQ> (engine_law.h) and EngineT<P, NQ> (engine.h); nothing here
// needs the pass kernels, so the steppers, the solvers and the C entries compile against this header
// alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <condition_variable>
#include <deque>
#include <functional>
#include <mutex>
#include <optional>
#include <string>
#include <thread>
#include <vector>

#include "../../include/cmdg.h"
#include "cmdg_common.h"
#include "owned.h"

namespace cmdg {

enum { SLOT_Q = 0, SLOT_GF = 1, SLOT_HG = 2, SLOT_HD = 3, NSLOT = 4 };
enum { TRANSPORT_NONE = 0, TRANSPORT_LOCAL = 1, TRANSPORT_RCCL = 2 };

struct HaloSlot {
    DevBuf<double> sendbuf, recvbuf;
    Event ev_packed, ev_done, ev_pulled;
    bool active = false;  // begin issued, end pending
    int nvar = 0;         // columns per position of the packed buffers
    int ncol = 0;         // columns of the array (>= nvar: the leading nvar travel)
    double *array = nullptr;
    // the array whose nodes of vmapsend an exterior launch has already written to sendbuf
    // (halo_pack then launches nothing); NULL: sendbuf is stale
    const double *fresh_for = nullptr;
    int fresh_nvar = 0;
};

// where a step of cmdg_lsrk_run stands in the run, for the steps that hand gradient arguments from
// stage to stage (CMDG_OPT_GRADARG_HANDOFF); a step that is given none does not hand anything on
struct StepInRun {
    bool first_step, last_step;
};

// what the fused update of a stage leaves for the next stage's gradient pass: nothing (the ordinary
// kernel), the gradient-argument records alone, or the records and the nodal auxiliary refresh
enum class GargOut { none, records, records_refresh };

struct RhsCtx {
    double *tendency = nullptr;
    double *Qin = nullptr;   // state read by this evaluation (ghosts refreshed in place)
    double *Qout = nullptr;  // LSRK: updated state
    double t = 0, alpha = 1, beta = 0;
    const double *tptr = nullptr;  // time in device memory instead (captured steps)
    bool lsrk = false;         // fused update inside k_tendency
    bool update_after = false; // separate update!() after the (filtered) tendency
    // CMDG_OPT_GRADARG_HANDOFF, set by cmdg_lsrk_run alone (handoff_stage, lsrk_run.hip): the gradient
    // pass reads the records the previous stage's update left / what the fused update leaves
    // An evaluation that reads the records hands its Laplacians on as ring-ordered records
    // (cmdg_common.h ring_slot); hypdiv_out: its Laplacian pass also writes the caller's
    // Qhypervisc_div (the run's last evaluation: the array ends a run as the ordinary kernels leave it).
    bool garg_in = false;
    bool hypdiv_out = true;
    // CMDG_OPT_FUSED_LAPLACIAN: the gradient and Laplacian passes of this evaluation are one launch
    // (kernels.h k_lapfused); only where garg_in holds on an eligible handle
    bool lap_fused = false;
    GargOut garg_out = GargOut::none;
    double rkb_dt = 0, rka_next = 0;
    // the law's update_auxiliary_state!(realelems) composition has run already (group_rhs runs the
    // nested operators of a local group in lock step before segment 0)
    bool pre_done = false;
};

// one `Filters.apply!` call site: filter + target + direction (include/cmdg.h)
struct FilterObj {
    int kind = 0, target = 0, direction = 0;
    int nindices = 0;
    int indices[CMDG_MAX_FILTER_STATES] = {0};
    int aux_ref_rho = 0, aux_ref_rhoe = 0;
    DevBuf<double> d_Fh, d_Fv;
};

// roctx range around the host-side enqueue of a phase (the reference instruments the same five
// halo phases with NVTX, MPIStateArrays.jl:419-439,465-480): a no-op unless the roctx library is
// in the process (rocprofv3 --marker-trace) or CMDG_ROCTX=1 asks for it to be loaded
void roctx_push(const char *name);
void roctx_pop();
// CMDG_DBG_SYNC=<bitmask>: localise a missing stream dependency by turning one class of
// event edges at a time into a host-side hipStreamSynchronize (scripts/probe/priority_order_sweep.sh)
//   1 order() of the split-explicit steppers   2 halo_pack: compute -> halo stream
//   4 halo_pack: neighbours' ev_pulled         8 halo_end: neighbours' ev_packed
//   16 halo_end: ev_done -> compute stream     32 before_direct_send
//   64 interior_begin / exterior_begin         128 the join at the end of segment 5
//   256 device synchronize before every group_rhs   512 device synchronize after every segment
int dbg_sync();
hipError_t ev_record(hipEvent_t e, hipStream_t s);
// work-groups of 256 for a grid-stride launch over n items
inline unsigned nblocks(int64_t n) { return (unsigned)std::min<int64_t>((n + 255) / 256, 65535); }
struct Range {
    explicit Range(const char *name) { roctx_push(name); }
    ~Range() { roctx_pop(); }
    Range(const Range &) = delete;
    Range &operator=(const Range &) = delete;
};

struct ProfRec {
    int kernel;
    Event e0, e1;
    bool clamp;  // record max(0, elapsed): e1 may precede e0 (exposed halo time)
};

// CMDG_OPT_ASYNC_RUN: cmdg_lsrk_run hands the run to a thread of the handle's own and returns; the
// caller's thread is not the one that spends a millisecond per step inside hipGraphLaunch (or
// posting RCCL groups).  One job at a time, in order; every other ABI entry of the handle first
// waits until the worker is idle (DevGuard), so the handle is still driven by one thread at a time.
// A failure of a deferred run is reported by the next cmdg_synchronize.
struct RunWorker {
    std::thread th;
    std::mutex m;
    std::condition_variable cv;
    std::deque<std::function<int()>> jobs;
    bool stop = false, busy = false;
    int deferred_rc = 0;
    std::string deferred_err;
    std::thread::id tid;
    void start()
    {
        th = std::thread([this] {
            std::unique_lock<std::mutex> lk(m);
            for (;;) {
                cv.wait(lk, [this] { return stop || !jobs.empty(); });
                if (jobs.empty()) return;  // (stop, drained)
                auto job = std::move(jobs.front());
                jobs.pop_front();
                busy = true;
                lk.unlock();
                const int r = job();
                lk.lock();
                busy = false;
                if (r && !deferred_rc) deferred_rc = r;
                cv.notify_all();
            }
        });
        tid = th.get_id();
    }
    void submit(std::function<int()> f)
    {
        {
            std::lock_guard<std::mutex> lk(m);
            jobs.push_back(std::move(f));
        }
        cv.notify_all();
    }
    void wait_idle()
    {
        if (std::this_thread::get_id() == tid) return;  // (the worker's own calls)
        std::unique_lock<std::mutex> lk(m);
        cv.wait(lk, [this] { return jobs.empty() && !busy; });
    }
    ~RunWorker()
    {
        if (th.joinable()) {
            {
                std::lock_guard<std::mutex> lk(m);
                stop = true;
            }
            cv.notify_all();
            th.join();
        }
    }
};

// inside a member of EngineBase: a failed HIP call ends the function with the engine's message set
#define HIPCHK(call)                                                                     \
    do {                                                                                 \
        hipError_t e_ = (call);                                                          \
        if (e_ != hipSuccess)                                                            \
            return fail(CMDG_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)

struct EngineBase {
    // declared first, so destroyed last: after every member that was used on them
    Stream s_comp, s_comm;
    RunWorker *worker = nullptr;  // CMDG_OPT_ASYNC_RUN
    // ---- configuration (copied from cmdg_desc) ---------------------------------------
    int NQ = 0, NQV = 0, Np = 0, Nfp = 0;  // horizontal / vertical points per direction
    int64_t nreal = 0, nghost = 0, nelem = 0;
    int ns = 0, naux = 0, ngrad = 0, ngf = 0, ngl = 0, nhyp = 0;
    int nf_first = 0, direction = 0, diffusion_direction = 0, stacked = 0;
    GridDev g{};
    const int64_t *d_interior = nullptr, *d_exterior = nullptr;
    // CMDG_OPT_STACK_HEIGHT: the caller's lists and the engine's own tiled copies of them
    const int64_t *d_interior_user = nullptr, *d_exterior_user = nullptr;
    DevBuf<int64_t> d_interior_tiled, d_exterior_tiled;
    int set_stack_height(int nv);
    int set_stream_priority(int level);  // CMDG_OPT_STREAM_PRIORITY
    int stream_priority = 0;
    int64_t ninterior = 0, nexterior = 0;
    const uint8_t *d_activedofs = nullptr;
    DevBuf<double> d_D;
    DevBuf<int32_t> d_faceP;  // digested face tables (GridDev::faceP / faceG / faceW)
    DevBuf<double> d_faceG;
    DevBuf<double> d_faceW;
    DevBuf<int32_t> d_facePr;
    const int64_t *d_vmapsend = nullptr, *d_vmaprecv = nullptr;
    int64_t nvmapsend = 0, nvmaprecv = 0;
    std::vector<int> nabrtorank;
    std::vector<int64_t> nabrsend, nabrrecv;  // 2*nnabr (first,last) 1-based
    // gf and hypdiv may be the caller's arrays: views, with gf_own / hd_own holding the library's own
    double *aux = nullptr, *gf = nullptr, *hypdiv = nullptr;
    DevBuf<double> hypgrad;  // (always the library's own)
    DevBuf<double> derived;  // (Np, NDER, nelem), library-owned
    DevBuf<double> gf_own, hd_own;
    // the caller's Qhypervisc_grad / state_gradient_flux (reference layout) when the working copy is
    // node-major: written by cmdg_export_* only; gf_scratch: reference-layout copy for a gradient filter
    double *hypgrad_user = nullptr, *gf_user = nullptr;
    DevBuf<double> gf_scratch;
    bool node_major(const double *array) const
    {
        return array == hypgrad || (array == gf && gf_node_major());
    }
    // ---- runtime -----------------------------------------------------------------------
    int dev = 0;  // the device this engine was created on (every ABI entry binds to it)
    Event ev_comp;
    HaloSlot slot[NSLOT];
    int slot_nvar_max = 0;
    DevBuf<double> W[2];  // LSRK work states
    // ---- CMDG_OPT_GRADARG_HANDOFF (kernels.h GradArgHandoff) --------------------------------
    // (ngl, Np, nelem) gradient arguments of the next stage's input, written by the fused update
    // and read by the next gradient pass of the same cmdg_lsrk_run; never trusted across calls
    DevBuf<double> garg;
    // (ngl, Np, nelem) Laplacians of the run's ring-ordered evaluations (the ones whose gradient pass
    // reads garg): k_divgrad<RING> writes them, k_gradlap<RING> reads and gathers them
    DevBuf<double> lapr;
    bool gradarg_handoff = true;   // the option
    bool handoff_used = false;     // did the last cmdg_lsrk_run use it (cmdg_query)
    int64_t handoff_refreshes = 0; // hand-off updates of the last run that carried the auxiliary refresh
    virtual bool garg_capable() const = 0;  // the law and order have the two instantiations
    // the law's refreshed columns are read by no pass: only the run's last hand-off update refreshes
    virtual bool refresh_elidable() const = 0;
    bool handoff_eligible() const
    {
        return gradarg_handoff && garg_capable() && !gf_live() && ngl > 0 && has_update_aux() &&
               fused_update_aux() && !has_hooks && !step_filter && !tendency_filter && !gradient_filter &&
               !step_graph && nghost == 0 && !communicate();
    }
    int ensure_garg();
    // ---- CMDG_OPT_FUSED_LAPLACIAN (kernels.h k_lapfused, lapfused_tables.h) ------------------
    DevBuf<int32_t> d_lapI;  // lapI / lapT of k_lapfused: allocated at create on an eligible grid only
    DevBuf<double> d_lapT;
    bool fused_laplacian = true;   // the option
    bool lapfused_ok = false;      // the tables exist
    int64_t fused_launches = 0;    // fused launches of the last cmdg_lsrk_run (cmdg_query)
    int init_lapfused();           // decides eligibility of the grid, once, at create
    // the hand-off evaluations of a run take the fused pass (the grid is eligible: lapfused_ok)
    bool lapfused_eligible() const { return fused_laplacian && lapfused_ok; }
    DevBuf<double> d_partial;           // reduction scratch
    int transport = TRANSPORT_NONE;
    int rank = 0, nranks = 1;
    std::vector<EngineBase *> group;    // local transport: engine of every rank
    void *nccl_comm = nullptr;
    const FilterObj *gradient_filter = nullptr, *tendency_filter = nullptr,
                    *step_filter = nullptr;
    bool profiling = false;
    std::vector<ProfRec> prof;
    double prof_ms[CMDG_K_COUNT] = {0};
    int64_t prof_n[CMDG_K_COUNT] = {0};
    std::string err;

    virtual ~EngineBase();
    int init(const cmdg_desc *d);
    int fail(int code, const std::string &msg)
    {
        err = msg;
        return code;
    }
    // hipGetLastError after the launches of a call (per thread: one check covers a whole group)
    int launch_status(const char *what);
    // make stream `later` wait for everything enqueued so far on `earlier` (through ev_comp)
    int order(hipStream_t earlier, hipStream_t later);
    bool communicate() const { return !nabrtorank.empty(); }
    // a DGFVModel handle (cmdg_create_dgfv, engine_fv.h): NQV == 1, finite volume in the vertical.
    // Its exchanges are packed and unpacked as the reference does (the vertical pass increments what
    // an exterior launch would already have sent), and the LSRK update is the separate kernel after
    // the finite-volume pass.
    bool fv = false;
    int fv_nvert = 0;
    // an ESDGModel handle (cmdg_create_esdg, engine_esdg.hip): one flux-differencing launch per element
    // list; like a DGFVModel handle it unpacks its exchange, uses the separate LSRK update and stays
    // eager
    bool esdg = false;
    bool fused_lsrk() const { return tendency_filter == nullptr && !fv && !esdg; }
    int init_fv();
    virtual int fv_prepare() { return CMDG_OK; }  // (engine_fv.h: HB flag against the law, LDS limit of a tall stack)
    // the orders the column operators and the filters are compiled for (one order in every direction)
    bool column_orders() const { return NQ >= 2 && NQ <= 8 && NQV == NQ; }
    // does an evaluation of this handle exchange ghosts (DGModel.jl:104-108: not the vertical
    // operator of a stacked mesh)
    bool exchanges() const { return communicate() && !(stacked && direction == DIR_VERTICAL); }

    // physics / order specific launches; `exterior`: the launch of the exterior element list of a
    // handle with neighbours (writes the send buffers of what it produces, see HaloDev).  A pass launch
    // fails, with the message set, when the engine class has no kernel for what it is asked.
    virtual int launch_gradients(const RhsCtx &c, const int64_t *elems, int64_t n, bool exterior, hipStream_t st) = 0;
    virtual int launch_divgrad(const RhsCtx &c, const int64_t *elems, int64_t n, bool exterior, hipStream_t st) = 0;
    virtual int launch_gradlap(const RhsCtx &c, const int64_t *elems, int64_t n, bool exterior, hipStream_t st) = 0;
    virtual int launch_tendency(const RhsCtx &c, const int64_t *elems, int64_t n, bool exterior, hipStream_t st) = 0;
    virtual void launch_update_aux(const RhsCtx &c, int64_t e0, int64_t e1) = 0;
    virtual bool has_update_aux() const = 0;
    virtual bool law_needs_gradflux() const = 0;
    virtual bool gf_node_major() const = 0;  // state_gradient_flux kept (ngf, Np, nelem) inside the library
    bool keep_gradflux = false;  // CMDG_OPT_KEEP_GRADFLUX
    // is state_gradient_flux formed (and exchanged) by an evaluation?
    bool gf_live() const
    {
        return ngf > 0 && (keep_gradflux || law_needs_gradflux() || has_hooks || gradient_filter);
    }
    virtual bool fused_update_aux() const = 0;
    // introspection (cmdg_query): per-node columns of the law's time-invariant derived fields,
    // auxiliary columns its nodal refresh rewrites, elements per work-group of the tendency pass
    virtual int law_nder() const = 0;
    virtual int law_nupd() const = 0;
    virtual int tendency_epb() const = 0;
    virtual int law_state_read(int pass) const = 0;
    virtual int law_aux_read(int pass) const = 0;
    virtual int init_derived() = 0;
    // mode 0: per-element minimum node distance, mode 1: per-element maximum Courant number
    virtual int launch_courant(int mode, int kind, const double *Q, double dt, double t, int dir,
                               double *out_elem) = 0;
    // cmdg_esdg_entropy: entropy variables and entropy of the real elements (ESDG handles)
    virtual int launch_entropy(const double *, double *, double *)
    {
        return fail(CMDG_ERR_UNSUPPORTED, "cmdg_esdg_entropy: not an ESDGModel handle (cmdg_create_esdg)");
    }

    // cmdg_les_nodal: the law's nodal AtmosLESDefault diagnostics of the real elements into D
    // (ndiag, Np, nreal), from (Q, aux, gradient flux) as the last evaluation left them; *ndiag and
    // *moist describe the law (D may be NULL to ask for them alone)
    virtual int launch_les_nodal(const double *Q, double t, double *D, int *ndiag, int *moist) = 0;
    // cmdg_vector_gradients: d u_c / d x_m of u = rho u / rho on the real elements, vgrad (nreal, 9, Np)
    virtual int launch_vector_gradients(const double *Q, double *vgrad) = 0;
    // cmdg_gcm_nodal: the nodal pass of the AtmosGCMDefault group (kernels.h k_gcm_nodal) on the real
    // elements: G (nelem, 14, Np) and the velocity u (nelem, 3, Np)
    virtual int launch_gcm_nodal(const double *Q, double t, double *G, double *u) = 0;

    // ---- ghost exchange without pack / unpack launches (HaloDev, cmdg_common.h) -------------
    // tables built at create from vmapsend / vmaprecv / the digested face table; *_ok = they
    // could be built (every node of vmapsend in an exterior element, every ghost node received
    // once, every ghost node a face reads received)
    DevBuf<int32_t> d_sendoff, d_ghostslot;
    DevBuf<SendEnt> d_sendent;
    bool direct_send_ok = false, direct_recv_ok = false;
    bool reference_halo = false;  // CMDG_OPT_REFERENCE_HALO: pack and unpack as the reference does
    int init_halo_tables();
    bool direct_send() const { return direct_send_ok && !reference_halo; }
    // consumers may read the receive buffers unless somebody reads the ghost ELEMENTS of Q: a
    // nodal update_auxiliary_state! of the ghosts that is not fused away, or the hooks
    bool direct_recv() const
    {
        return direct_recv_ok && !reference_halo && !has_hooks && !(has_update_aux() && !fused_update_aux());
    }
    // what a launch is handed: receive side for every launch, send side for exterior ones
    HaloDev halo_dev(bool exterior, double *send0, double *send1) const
    {
        HaloDev h{};
        h.nreal = nreal;
        if (!communicate()) return h;
        if (exterior && direct_send()) {
            h.sendoff = d_sendoff;
            h.sendent = d_sendent;
            h.send[0] = send0;
            h.send[1] = send1;
        }
        if (direct_recv()) {
            h.ghostslot = d_ghostslot;
            h.recvQ = slot[SLOT_Q].recvbuf;
            h.recvGF = slot[SLOT_GF].recvbuf;
            h.recvHG = slot[SLOT_HG].recvbuf;
            h.recvHD = slot[SLOT_HD].recvbuf;
        }
        return h;
    }
    // an exterior launch (on stream st) is about to overwrite sendbuf of slot s: with the local
    // transport the neighbours must have pulled its previous payload
    int before_direct_send(int s, hipStream_t st);
    // ---- two pipelines (handles with neighbours whose exchanges run direct both ways) ---------
    // The exterior launches E_p of the passes and the exchanges X_p they feed form a serial chain
    // X_p -> E_p -> X_(p+1) -> E_(p+1) ...; it runs on the halo stream with no event hop inside,
    // while the interior launches I_p run on the compute stream.  A pass reads what the previous
    // pass wrote for the element and its face neighbours, so I_p waits for E_(p-1) and E_p waits
    // for I_(p-1) (events of alternating parity): the interior work of a pass hides the exchanges
    // of two, and a step costs max(chain, compute) instead of the sum over passes of
    // max(I_p, X_p) + E_p.
    Event ev_int[2], ev_ext[2];
    int64_t pass_seq = 0;  // passes started on this handle
    int64_t host_post_ns = 0, host_post_n = 0;  // host time inside halo_post (RCCL group calls)
    Event prof_ext_done;  // profiling: end of the last exterior launch
    bool no_pipeline = false;  // CMDG_OPT_HALO_PIPELINE = 0
    bool pipelined() const
    {
        return exchanges() && !no_pipeline && direct_send() && direct_recv() && !gradient_filter &&
               !tendency_filter && (!has_update_aux() || fused_update_aux());
    }
    void invalidate_sends()
    {
        for (auto &h : slot) h.fresh_for = nullptr;
    }
    void mark_fresh(int s, const double *array, int nvar)
    {
        slot[s].fresh_for = array;
        slot[s].fresh_nvar = nvar;
    }

    // ---- a whole LSRK step as a HIP graph (CMDG_OPT_STEP_GRAPH) ---------------------------
    // cmdg_lsrk_run can record one step into a HIP graph and replay it: the evaluation times come
    // from device memory, advanced by a one-thread kernel at the head of the graph exactly as
    // updatetime! accumulates them; the first step of every run is issued eagerly, the capture uses
    // events of its own.  Built for the partitioned case -- at 5 400 elements per rank a step is
    // bound by the HOST: posting an RCCL group costs 55 us of host time, 20 of them per step, next
    // to 40 kernel launches and 100 event operations (1.43 ms of enqueueing for a 1.56 ms step) --
    // but RCCL operations inside a capture crash hipStreamEndCapture on this stack, so handles that
    // exchange stay eager (graph_eligible) and the option serves single-rank handles only, where
    // the device is the bound anyway.  Anything else a capture cannot hold (profiling, filters,
    // hooks, an unfused nodal refresh) keeps a run eager too.
    bool step_graph = false;        // the option
    bool capturing = false;         // rhs_segment is being recorded
    int cap_interior = 0, cap_exterior = 0;  // launches begun in this capture
    // (every record of a capture gets an event of its own: 4 passes x 16 stages at most)
    static constexpr int NGEV = 64;
    Event gev_int[NGEV], gev_ext[NGEV], gev_fork;
    int cap_pass = 0;  // passes begun in this capture
    hipGraphExec_t graph_exec = nullptr;
    struct GraphKey {
        const double *Q = nullptr, *dQ = nullptr;
        double dt = 0;
        int nstages = 0;
        double coef[48] = {0};
        bool pipe = false, comm = false;
        bool operator==(const GraphKey &o) const
        {
            if (Q != o.Q || dQ != o.dQ || dt != o.dt || nstages != o.nstages || pipe != o.pipe || comm != o.comm)
                return false;
            for (int i = 0; i < 48; ++i)
                if (coef[i] != o.coef[i]) return false;
            return true;
        }
    } graph_key;
    DevBuf<double> d_gtime;         // [t_next, dt, times[16], rkc[16]]
    int64_t graph_steps = 0;        // steps replayed from the graph (cmdg_query)
    bool graph_failed = false;      // a capture failed: this handle stays eager
    bool graph_eligible() const;
    // whatever changes the launches of an evaluation (options, filters, hooks, profiling) makes a
    // recorded step stale: the next run records again
    void drop_graph()
    {
        if (graph_exec) {
            hipStreamSynchronize(s_comp);
            hipGraphExecDestroy(graph_exec);
            graph_exec = nullptr;
        }
    }
    int capture_step(double *Q, double *dQ, double dt, int nstages, const double *rka,
                     const double *rkb, const double *rkc);
    int run_steps(double *Q, double *dQ, double t, double dt, int64_t nsteps, int nstages,
                  const double *rka, const double *rkb, const double *rkc);

    // orchestration
    static constexpr int NSEG = 6;
    int rhs_segment(int seg, const RhsCtx &c);
    int rhs_async(const RhsCtx &c);
    int lsrk_step(double *Q, double *dQ, double t, double dt, int nstages, const double *rka,
                  const double *rkb, const double *rkc, bool continued = false,
                  const StepInRun *handoff = nullptr);
    // (nvar columns per packed position = the leading columns of the ncol-column array; ncol = 0:
    // the whole array, nvar == ncol, as the reference packs)
    // on_halo_stream (pipelined()): producer and consumer are launches of the halo stream itself
    int export_hypgrad(double *dst);
    int export_gradflux(double *dst);
    int halo_begin(int s, double *array, int nvar, int ncol = 0, bool on_halo_stream = false);
    // begin_ghost_exchange! in two halves, so that exchanges that begin at the same point of an
    // evaluation are packed one after the other and posted in ONE RCCL group
    int halo_pack(int s, double *array, int nvar, int ncol = 0, bool on_halo_stream = false);
    int halo_post(const int *slots, int nslots);
    // unpack = false: the consumers read the receive buffer (direct_recv())
    int halo_end(int s, double *array, int nvar, bool unpack = true, bool on_halo_stream = false);
    void abort_exchanges();  // after a failed call: no exchange is left "begun"
    int ensure_work();
    int synchronize();
    int wsum2(const double *A, const double *B, int nvar, int weighted, double *out);
    int courant(int mode, int kind, const double *Q, double dt, double t, int dir, double *out);
    DevBuf<double> d_elemred;  // (nreal) per-element extrema
    int stack_integral(bool reverse, const double *Q, int nstate, double *aux_arr, int naux_arr,
                       int nvert, const double *Imat_host, const cmdg_stack_integral_desc *d,
                       int64_t h0 = 0, int64_t nh = -1);
    bool has_hooks = false;
    // the nested operator of the hooks was destroyed: evaluations fail until new hooks are set
    bool hooks_orphaned = false;
    cmdg_rhs_hooks hooks{};
    // handles whose hooks evaluate this one as their nested operator (hooks.pre_rhs_handle):
    // cmdg_destroy of this handle detaches it from them
    std::vector<EngineBase *> nested_in;
    int set_hooks(const cmdg_rhs_hooks *hk);
    int run_pre_hooks(const RhsCtx &c);
    // ... in two halves around the evaluation of the nested operator (hooks.pre_rhs_handle)
    int run_pre_hooks_a(const RhsCtx &c, RhsCtx &nested);
    int run_pre_hooks_b(const RhsCtx &c);
    int integrate_velocity(const double *X, int nstate, int col, int nvert, int64_t h0 = 0,
                           int64_t nh = -1);
    int flow_deviation(double *Q, int64_t h0, int64_t nh);
    DevBuf<double> d_flowint;  // (Np, 2, nelem) column integral of the horizontal velocity
    DevBuf<double> d_preT;     // tendency of the nested operator of the hooks (pre_rhs_handle)
    int run_column_ops(const RhsCtx &c, int64_t e0, int64_t e1);
    // the column operators of a recorded composition in one launch (columns.h k_column_chain,
    // k_flow_deviation); CMDG_FUSED_COLUMNS=0 issues them one by one as recorded (A/B, tests)
    // (levels, for A/B: 1 the hooks' column operators, 2 + the pair of pre filters; fusing the
    // stepper's coupling kernels as well was measured slower, profiles/r04_ab_ocean_fused_columns.txt)
    int fused_columns = 2;
    bool column_chain(const RhsCtx &c, int64_t e0, int64_t e1, bool with_copies);
    bool filter_pair(double *Q);
    int run_gradient_hooks(const RhsCtx &c, int64_t e0, int64_t e1);
    DevBuf<double> d_Imat;
    int ensure_Imat(const double *host);  // the steppers' Imat (NQ x NQ): uploaded if absent
    DevBuf<double> d_Dv;  // vertical derivative matrix when the vertical order differs
    int filter_create(const cmdg_filter_desc *d, FilterObj **out);
    int filter_apply(const FilterObj *f, double *Q, int nstate);

    // profiling brackets
    // a new record with both events created (e1 may be given instead: an event recorded already)
    ProfRec &prof_pair(int kernel, bool clamp, Event e1 = Event());
    void prof_begin(int kernel, hipStream_t st);
    void prof_end(hipStream_t st);
    void prof_collect();
};

}  // namespace cmdg

struct cmdg_context {
    cmdg::EngineBase *eng = nullptr;
    std::string err;
};

namespace cmdg {
// Every ABI entry runs with the engine's device current: lazily allocated work buffers and the
// kernels of a handle land on the GPU the handle was created on, whatever device the calling
// thread switched to in between; the caller's current device is restored on return.
struct DevGuard {
    int prev = -1;
    bool changed = false;
    explicit DevGuard(const EngineBase *e)
    {
        if (e->worker) e->worker->wait_idle();  // deferred runs of this handle come first
        if (hipGetDevice(&prev) == hipSuccess && prev != e->dev)
            changed = hipSetDevice(e->dev) == hipSuccess;
    }
    ~DevGuard()
    {
        if (changed) (void)hipSetDevice(prev);
    }
    DevGuard(const DevGuard &) = delete;
    DevGuard &operator=(const DevGuard &) = delete;
};

// The prologue and the one error path of the entries that take several handles (include/cmdg.h,
// at cmdg_comm_connect_local): ok() false means a NULL list, n < 1 or a NULL member, and nothing
// was done.  Otherwise every engine's deferred run is idle, the first engine's device is current
// until the call returns, and every engine's err was cleared, so that a set err marks a member
// that failed in this call.  finish(rc) returns rc, on failure with that member's message on
// every handle.
struct GroupCall {
    GroupCall(cmdg_handle *handles, int n) : GroupCall(handles, nullptr, n, false) {}
    GroupCall(cmdg_handle *slow, cmdg_handle *fast, int n) : GroupCall(slow, fast, n, true) {}
    // members with a role each ("slow", "fast", ...); a handle named twice is one member whose
    // message prefix carries both roles
    explicit GroupCall(const std::vector<std::pair<cmdg_handle, std::string>> &named);
    bool ok() const { return !members.empty(); }
    int finish(int rc);

  private:
    GroupCall(cmdg_handle *h, cmdg_handle *h2, int n, bool pairs);
    std::vector<std::pair<cmdg_handle, std::string>> members;
    std::optional<DevGuard> dev;
};

// the handle's cmdg_last_error takes the engine's message when code is a failure
int set_err(cmdg_handle h, int code);
// the message of cmdg_last_error(NULL), one per thread (create.hip): calls that fail without a handle
void set_create_err(const std::string &msg);

// Objects that are not bound to a handle (interpolation, direct stiffness summation) live on the
// device they were created on: it is made current for a call and the caller's restored on return.
struct ObjectDevice {
    int prev = -1;
    bool changed = false;
    explicit ObjectDevice(int dev)
    {
        if (hipGetDevice(&prev) == hipSuccess && prev != dev) changed = hipSetDevice(dev) == hipSuccess;
    }
    ~ObjectDevice()
    {
        if (changed) (void)hipSetDevice(prev);
    }
    ObjectDevice(const ObjectDevice &) = delete;
    ObjectDevice &operator=(const ObjectDevice &) = delete;
};
// the one epilogue of their entries, which take a handle or NULL: the message goes to the handle, or
// to cmdg_last_error(NULL) without one
inline int object_call_done(cmdg_handle h, int r, const std::string &err)
{
    if (r == CMDG_OK) return r;
    if (h) return set_err(h, h->eng->fail(r, err));
    set_create_err(err);
    return r;
}

// what a plug-in and the library must agree on (cmdg_load_plugin): the layout of the engine base
// class and of the descriptor, folded into one number (plus the revision of its virtual interface,
// which no size shows: 1 = launch_les_nodal, 2 = launch_vector_gradients and launch_gcm_nodal, 3 = the
// pass launchers return a status)
inline unsigned long engine_abi_stamp()
{
    return (unsigned long)sizeof(EngineBase) * 1000003ul + (unsigned long)sizeof(cmdg_desc) * 10007ul +
           (unsigned long)sizeof(RhsCtx) * 101ul + (unsigned long)sizeof(cmdg_rhs_hooks) + 3ul * 100000007ul;
}

}  // namespace cmdg
