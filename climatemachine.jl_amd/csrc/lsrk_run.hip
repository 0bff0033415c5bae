// The fused low-storage Runge-Kutta stepper: one step over a handle or a local group with the 2N
// update inside the tendency pass (dostep!, LowStorageRungeKuttaMethod.jl:102-144), and
// cmdg_lsrk_run on top of it -- eager steps that may hand gradient arguments from stage to stage
// (CMDG_OPT_GRADARG_HANDOFF), or one captured step replayed (CMDG_OPT_STEP_GRAPH).
#include "stepping.h"

namespace cmdg {

// update!  LowStorageRungeKuttaMethod.jl:146-158 (used when a tendency filter sits between
// the right-hand side and the update, so the update cannot be fused into k_tendency)
static __global__ void k_lsrk_update(double *__restrict__ dQ, double *__restrict__ Q, double rka,
                                     double rkb_dt, int64_t n)
{
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        Q[i] += rkb_dt * dQ[i];
        dQ[i] *= rka;
    }
}
void lsrk_update(hipStream_t st, double *dQ, double *Q, double rka_next, double rkb_dt, int64_t n)
{
    hipLaunchKernelGGL(k_lsrk_update, dim3(nblocks(n)), dim3(256), 0, st, dQ, Q, rka_next, rkb_dt, n);
}
void lsrk_update(EngineBase *e, double *dQ, double *Q, double rka_next, double rkb_dt)
{
    lsrk_update(e->s_comp, dQ, Q, rka_next, rkb_dt, real_len(e));
}

// The state rotates Q -> W0 -> W1 -> ... -> Q so that the fused update never writes the array its
// neighbours still read; a one-stage tableau ends in W0 and is copied back.
static void lsrk_stage_buffers(EngineBase *e, double *Q, int s, int nstages, double **in, double **out)
{
    *in = s == 0 ? Q : e->W[(s - 1) % 2];
    *out = s == nstages - 1 && nstages > 1 ? Q : e->W[s % 2];
}

// CMDG_OPT_GRADARG_HANDOFF: what stage s of a step reads, and what its fused update leaves.
struct StageHandoff {
    bool garg_in;  // the gradient pass reads the records the update before it left
    GargOut out;
    bool last_eval;  // the run's last evaluation: the caller's Qhypervisc_div is written
};
// The hand-off lives inside one run, so that nothing is carried over from or into another call:
//  - every evaluation but the run's first reads the records; that one reads Q;
//  - every update but the run's last leaves them; that one is the ordinary kernel;
//  - the auxiliary refresh of an update is seen only after the run's last hand-off update, stage
//    nstages - 2 of the last step: where the law lets the unread ones go (refresh_elidable) the
//    others leave the records alone.  (A one-stage tableau has that update in the step before the
//    last; it refreshes in every update.)
//  - an evaluation that reads the records hands its Laplacians from k_divgrad to k_gradlap as
//    ring-ordered records (RhsCtx::garg_in); only the run's last one writes the caller's
//    Qhypervisc_div as well.
// run == NULL: a step outside cmdg_lsrk_run, or a run that does not hand off.
static StageHandoff handoff_stage(const StepInRun *run, int s, int nstages, bool refresh_elidable)
{
    if (!run) return {false, GargOut::none, true};
    const bool in = !(run->first_step && s == 0);
    if (run->last_step && s == nstages - 1) return {in, GargOut::none, true};
    const bool refresh = !refresh_elidable || nstages == 1 || (run->last_step && s == nstages - 2);
    return {in, refresh ? GargOut::records_refresh : GargOut::records, false};
}

int EngineBase::lsrk_step(double *Q, double *dQ, double t, double dt, int nstages, const double *rka,
                          const double *rkb, const double *rkc, bool continued, const StepInRun *handoff)
{
    std::vector<EngineBase *> one{this};
    double *Qs[1] = {Q}, *dQs[1] = {dQ};
    if (transport == TRANSPORT_LOCAL && communicate())
        return fail(CMDG_ERR_INVALID, "handles connected locally must be driven by the cmdg_group_* calls");
    return group_lsrk_step(one, Qs, dQs, t, dt, nstages, rka, rkb, rkc, continued, nullptr, handoff);
}

int group_lsrk_step(std::vector<EngineBase *> &g, double **Q, double **dQ, double t, double dt,
                    int nstages, const double *rka, const double *rkb, const double *rkc,
                    bool continued, const double *stage_times_dev, const StepInRun *handoff)
{
    if (nstages < 1) return g[0]->fail(CMDG_ERR_INVALID, "lsrk: nstages < 1");
    for (auto *e : g)
        if (int r = e->ensure_work()) return r;
    std::vector<RhsCtx> c(g.size());
    for (int s = 0; s < nstages; ++s) {
        for (size_t i = 0; i < g.size(); ++i) {
            RhsCtx &x = c[i];
            // a tendency filter acts on dQ between rhs! and update!: no fused update then
            const bool fused = g[i]->fused_lsrk();
            if (fused) {
                lsrk_stage_buffers(g[i], Q[i], s, nstages, &x.Qin, &x.Qout);
            } else {
                x.Qin = Q[i];
                x.Qout = nullptr;
            }
            x.tendency = dQ[i];
            x.t = t + rkc[s] * dt;
            x.tptr = stage_times_dev ? stage_times_dev + s : nullptr;
            x.alpha = 1.0;  // rhs!(dQ, Q, p, time + RKC[s] * dt, increment = true)
            x.beta = 1.0;
            x.lsrk = fused;
            x.update_after = !fused;
            x.rkb_dt = rkb[s] * dt;
            x.rka_next = rka[(s + 1) % nstages];
            const StageHandoff h = handoff_stage(handoff, s, nstages, g[i]->refresh_elidable());
            x.garg_in = h.garg_in;
            x.garg_out = h.out;
            x.hypdiv_out = !h.garg_in || h.last_eval;
            if (h.out == GargOut::records_refresh) g[i]->handoff_refreshes += 1;
            x.lap_fused = h.garg_in && g[i]->lapfused_eligible();
            if (x.lap_fused) g[i]->fused_launches += 1;
        }
        if (int r = group_rhs(g, c, s > 0 || continued)) return r;
    }
    for (size_t i = 0; i < g.size(); ++i) {
        EngineBase *e = g[i];
        if (nstages == 1 && e->fused_lsrk())
            if (hipMemcpyAsync(Q[i], e->W[0], sizeof(double) * e->Np * e->ns * e->nreal,
                               hipMemcpyDeviceToDevice, e->s_comp) != hipSuccess)
                return e->fail(CMDG_ERR_HIP, "lsrk: copy back failed");
        // user callback EveryXSimulationSteps(1) of heldsuarez.jl:261-272
        if (e->step_filter) {
            if (int r = e->filter_apply(e->step_filter, Q[i], e->ns)) return r;
            e->invalidate_sends();
        }
    }
    return CMDG_OK;
}

// ---- cmdg_lsrk_run: eager steps, or one captured step replayed (EngineBase::step_graph) -----
namespace {
struct StepTimesInit {
    double t_next, dt;
    int nstages;
    double rkc[16];
};
// [t_next, dt, times[16], rkc[16]] <- the values of a run
__global__ void k_step_times_init(double *g, StepTimesInit v)
{
    g[0] = v.t_next;
    g[1] = v.dt;
    for (int s = 0; s < v.nstages; ++s) g[18 + s] = v.rkc[s];
}
// head of the captured step: the stage times of this step, then t += dt (updatetime!)
__global__ void k_step_times(double *g, int nstages)
{
    const double t = g[0], dt = g[1];
    for (int s = 0; s < nstages; ++s) g[2 + s] = t + g[18 + s] * dt;
    g[0] = t + dt;
}
}  // namespace

bool EngineBase::graph_eligible() const
{
    // A handle that exchanges can be recorded when its exchanges need neither a pack nor an unpack
    // launch from the compute stream (pipelined()) and travel through RCCL.  The groups must then sit
    // on the capture's ORIGIN stream: on HIP 7.0.2 / RCCL 2.26.6 (the stack torch brings) a group
    // recorded on a stream that joined the capture through an event crashes hipStreamEndCapture,
    // whatever the capture mode; on ROCm 7.2 / RCCL 2.27.7 both forms work
    // (scripts/probe/rccl_capture_probe.py, profiles/r04_rccl_capture_probes.txt).  The halo stream
    // is therefore the origin of such a capture and the compute stream the forked one.
    const bool comm_ok = !exchanges() || (transport == TRANSPORT_RCCL && pipelined());
    // (a DGFVModel handle stays eager: its step has never been recorded and replayed on a device, and
    // nothing asks for it yet)
    return step_graph && !fv && !esdg && !graph_failed && !profiling && !step_filter && !tendency_filter &&
           !gradient_filter && !has_hooks && (!has_update_aux() || fused_update_aux()) && comm_ok;
}

int EngineBase::capture_step(double *Q, double *dQ, double dt, int nstages, const double *rka,
                             const double *rkb, const double *rkc)
{
    const bool comm = exchanges();
    if (graph_exec) {
        hipGraphExecDestroy(graph_exec);
        graph_exec = nullptr;
    }
    if (!d_gtime) HIPCHK(d_gtime.alloc(34));
    std::vector<EngineBase *> one{this};
    double *Qs[1] = {Q}, *dQs[1] = {dQ};
    if (4 * nstages + 1 > NGEV) return fail(CMDG_ERR_UNSUPPORTED, "step graph: too many stages");
    for (int i = 0; i < NGEV; ++i) {  // (created on first use: most handles never capture)
        if (!gev_int[i]) HIPCHK(gev_int[i].create(hipEventDisableTiming));
        if (!gev_ext[i]) HIPCHK(gev_ext[i].create(hipEventDisableTiming));
    }
    capturing = true;
    cap_interior = cap_exterior = cap_pass = 0;
    hipGraph_t graph = nullptr;
    int r = CMDG_OK;
    // origin of the capture: the stream the RCCL groups are recorded on (graph_eligible)
    const hipStream_t so = comm ? s_comm : s_comp;
    if (hipStreamBeginCapture(so, hipStreamCaptureModeRelaxed) != hipSuccess) {
        capturing = false;
        return fail(CMDG_ERR_HIP, "step graph: hipStreamBeginCapture failed");
    }
    hipLaunchKernelGGL(k_step_times, dim3(1), dim3(1), 0, so, d_gtime, nstages);
    if (comm) {  // the compute stream joins the capture
        if (hipEventRecord(gev_fork, s_comm) != hipSuccess ||
            hipStreamWaitEvent(s_comp, gev_fork, 0) != hipSuccess)
            r = fail(CMDG_ERR_HIP, "step graph: fork of the compute stream failed");
    }
    if (!r) r = group_lsrk_step(one, Qs, dQs, 0.0, dt, nstages, rka, rkb, rkc, true, d_gtime + 2);
    if (comm && !r) {  // ... and ends in the origin stream
        if (hipEventRecord(gev_fork, s_comp) != hipSuccess ||
            hipStreamWaitEvent(s_comm, gev_fork, 0) != hipSuccess)
            r = fail(CMDG_ERR_HIP, "step graph: join of the compute stream failed");
    }
    const hipError_t ee = hipStreamEndCapture(so, &graph);
    capturing = false;
    if (r || ee != hipSuccess || !graph) {
        if (graph) hipGraphDestroy(graph);
        abort_exchanges();
        (void)hipGetLastError();
        graph_failed = true;
        if (!r) r = fail(CMDG_ERR_HIP, std::string("step graph: hipStreamEndCapture: ") + hipGetErrorString(ee));
        return r;
    }
    const hipError_t ie = hipGraphInstantiate(&graph_exec, graph, nullptr, nullptr, 0);
    hipGraphDestroy(graph);
    if (ie != hipSuccess) {
        graph_exec = nullptr;
        graph_failed = true;
        return fail(CMDG_ERR_HIP, std::string("step graph: hipGraphInstantiate: ") + hipGetErrorString(ie));
    }
    return CMDG_OK;
}

int EngineBase::run_steps(double *Q, double *dQ, double t, double dt, int64_t nsteps, int nstages,
                          const double *rka, const double *rkb, const double *rkc)
{
    // (the step times accumulate as the reference's updatetime! does: t += dt, ODESolvers.jl:96-98)
    int64_t i = 0;
    handoff_used = false;
    handoff_refreshes = 0;
    fused_launches = 0;
    if (nsteps >= 2 && nstages <= 16 && graph_eligible()) {
        if (int r = lsrk_step(Q, dQ, t, dt, nstages, rka, rkb, rkc, false)) return r;  // eager: packs Q
        t += dt;
        i = 1;
        GraphKey key;
        key.Q = Q, key.dQ = dQ, key.dt = dt, key.nstages = nstages;
        key.comm = exchanges();
        key.pipe = pipelined();
        for (int s = 0; s < nstages; ++s) key.coef[s] = rka[s], key.coef[16 + s] = rkb[s], key.coef[32 + s] = rkc[s];
        if (!graph_exec || !(key == graph_key)) {
            if (capture_step(Q, dQ, dt, nstages, rka, rkb, rkc) == CMDG_OK) graph_key = key;
            else graph_failed = true;  // err says why; this run and the later ones go on eagerly
        }
        if (graph_exec && !graph_failed) {
            StepTimesInit v{};
            v.t_next = t, v.dt = dt, v.nstages = nstages;
            for (int s = 0; s < nstages; ++s) v.rkc[s] = rkc[s];
            const hipStream_t so = key.comm ? s_comm : s_comp;
            if (key.comm) {  // the eager step's work on the compute stream comes first
                HIPCHK(hipEventRecord(ev_comp, s_comp));
                HIPCHK(hipStreamWaitEvent(s_comm, ev_comp, 0));
            }
            hipLaunchKernelGGL(k_step_times_init, dim3(1), dim3(1), 0, so, d_gtime, v);
            for (; i < nsteps; ++i, t += dt) {
                HIPCHK(hipGraphLaunch(graph_exec, so));
                graph_steps += 1;
            }
            if (key.comm) {  // whatever the caller enqueues next on the compute stream follows the run
                HIPCHK(hipEventRecord(ev_comp, s_comm));
                HIPCHK(hipStreamWaitEvent(s_comp, ev_comp, 0));
            }
            return CMDG_OK;
        }
        // the capture left the exchange state of a continued step behind: start over from Q
        invalidate_sends();
        for (; i < nsteps; ++i, t += dt)
            if (int r = lsrk_step(Q, dQ, t, dt, nstages, rka, rkb, rkc, false)) return r;
        return CMDG_OK;
    }
    // CMDG_OPT_GRADARG_HANDOFF (handoff_stage): a run of one evaluation has nothing to hand on
    handoff_used = handoff_eligible() && nsteps * nstages >= 2;
    if (handoff_used)
        if (int r = ensure_garg()) return r;
    for (; i < nsteps; ++i, t += dt) {
        const StepInRun pos{i == 0, i == nsteps - 1};
        if (int r = lsrk_step(Q, dQ, t, dt, nstages, rka, rkb, rkc, i > 0, handoff_used ? &pos : nullptr)) return r;
    }
    return CMDG_OK;
}

}  // namespace cmdg

using namespace cmdg;

extern "C" {

int cmdg_lsrk_step(cmdg_handle h, double *Q, double *dQ, double t, double dt, int32_t nstages,
                   const double *rka, const double *rkb, const double *rkc)
{
    if (!h || !Q || !dQ || !rka || !rkb || !rkc) return CMDG_ERR_INVALID;
    DevGuard guard_(h->eng);
    return set_err(h, h->eng->lsrk_step(Q, dQ, t, dt, nstages, rka, rkb, rkc));
}

int cmdg_lsrk_run(cmdg_handle h, double *Q, double *dQ, double t, double dt, int64_t nsteps,
                  int32_t nstages, const double *rka, const double *rkb, const double *rkc)
{
    if (!h || !Q || !dQ || !rka || !rkb || !rkc) return CMDG_ERR_INVALID;
    EngineBase *e = h->eng;
    if (e->worker && nstages >= 1 && nstages <= 16) {  // CMDG_OPT_ASYNC_RUN: the handle's own thread enqueues
        std::vector<double> a(rka, rka + nstages), b(rkb, rkb + nstages), c(rkc, rkc + nstages);
        e->worker->submit([=]() {
            DevGuard guard_(e);
            const int r = e->run_steps(Q, dQ, t, dt, nsteps, nstages, a.data(), b.data(), c.data());
            if (r) {
                std::lock_guard<std::mutex> lk(e->worker->m);
                if (e->worker->deferred_err.empty()) e->worker->deferred_err = e->err;
            }
            return r;
        });
        return CMDG_OK;
    }
    DevGuard guard_(e);
    return set_err(h, e->run_steps(Q, dQ, t, dt, nsteps, nstages, rka, rkb, rkc));
}

int cmdg_group_lsrk_run(cmdg_handle *handles, int32_t n, double **Q, double **dQ, double t,
                        double dt, int64_t nsteps, int32_t nstages, const double *rka,
                        const double *rkb, const double *rkc)
{
    if (!Q || !dQ || !rka || !rkb || !rkc) return CMDG_ERR_INVALID;
    for (int i = 0; i < n; ++i)
        if (!Q[i] || !dQ[i]) return CMDG_ERR_INVALID;
    GroupCall gc(handles, n);
    if (!gc.ok()) return CMDG_ERR_INVALID;
    std::vector<EngineBase *> g;
    for (int i = 0; i < n; ++i) g.push_back(handles[i]->eng);
    for (int64_t s = 0; s < nsteps; ++s, t += dt)
        if (int r = group_lsrk_step(g, Q, dQ, t, dt, nstages, rka, rkb, rkc, s > 0)) return gc.finish(r);
    return CMDG_OK;
}

}  // extern "C"
