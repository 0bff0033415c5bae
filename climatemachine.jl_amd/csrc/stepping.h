// The parts the time steppers are built from (lsrk_run.hip, steppers.hip, multirate.hip,
// split_explicit*.hip): an evaluation and a fused LSRK step over a local group, stream ordering,
// "an operator, or one minus another", the grid checks and the column solver's internal
// interface.  Internal: not installed under include/.
#pragma once
#include <string>

#include "engine_base.h"

namespace cmdg {

// cmdg.hip (next to rhs_segment): one evaluation over the handles of a local group, in lock step
int group_rhs(std::vector<EngineBase *> &g, std::vector<RhsCtx> &c, bool keep_fresh = false);
// lsrk_run.hip: one fused LSRK step over them.  continued: this step follows the previous step of
// the same run with nothing in between; handoff: see EngineBase::lsrk_step
int group_lsrk_step(std::vector<EngineBase *> &g, double **Q, double **dQ, double t, double dt,
                    int nstages, const double *rka, const double *rkb, const double *rkc,
                    bool continued = false, const double *stage_times_dev = nullptr,
                    const StepInRun *handoff = nullptr);

// What a step drives as "a backward-Euler solver" (LinBESolver, BackwardEulerSolvers.jl:112-196) for
// Q = Qhat + alpha L(Q): the linear handle, "make ready for alpha" and "solve into X from B at time
// t", all on the linear handle's stream; errors land on that handle's engine (where
// GroupCall::finish looks).  The column LU (columnlu.hip) and GMRES (gmres.hip) implement it.
struct BackwardEuler {
    cmdg_handle lin = nullptr;
    // X on entry is the solver's initial guess: a step has to fill it (the direct solver ignores it)
    bool iterative = false;
    virtual ~BackwardEuler() = default;
    virtual double alpha() const = 0;     // the alpha it is ready for; NaN: none yet
    virtual int ready(double alpha) = 0;  // update_backward_Euler_solver!
    virtual int solve(double *X, const double *B, double t) = 0;
};
BackwardEuler *columnlu_solver(cmdg_columnlu_handle lu);
// (a step entry's call: also starts the record of the step's solves, cmdg_gmres_step_info)
BackwardEuler *gmres_solver(cmdg_gmres_handle g);

// Work-groups of 256 for a kernel that handles one item per thread and returns past n: every
// item needs its own thread, so the count is not capped (nblocks, engine_base.h, is for grid-stride
// kernels only).
inline unsigned grid_one_per_thread(int64_t n) { return (unsigned)((n + 255) / 256); }

inline int64_t real_len(const EngineBase *e) { return e->nreal * (int64_t)e->ns * e->Np; }

// lsrk_run.hip: update! of the 2N scheme over the first n values of dQ and Q on stream st, and over the
// real elements on the engine's compute stream
void lsrk_update(hipStream_t st, double *dQ, double *Q, double rka_next, double rkb_dt, int64_t n);
void lsrk_update(EngineBase *e, double *dQ, double *Q, double rka_next, double rkb_dt);

// Consecutive operations of one step on different streams: the later stream waits for
// everything enqueued so far on the earlier one.  A step that stays on one stream needs no create().
struct Chain {
    EngineBase *owner;  // takes the messages of ordering failures
    std::string who;    // their prefix: the stepper's name
    Event ev;
    hipStream_t cur = nullptr;
    Chain(EngineBase *e, const char *stepper) : owner(e), who(stepper) {}
    int create()
    {
        if (ev.create(hipEventDisableTiming) != hipSuccess)
            return owner->fail(CMDG_ERR_HIP, who + ": hipEventCreate failed");
        return CMDG_OK;
    }
    int to(hipStream_t s)
    {
        if (cur && cur != s) {
            if (hipEventRecord(ev, cur) != hipSuccess || hipStreamWaitEvent(s, ev, 0) != hipSuccess)
                return owner->fail(CMDG_ERR_HIP, who + ": stream ordering failed");
        }
        cur = s;
        return CMDG_OK;
    }
};

// one operator: `h`, or `h` minus `minus` evaluated as h (alpha, beta) then minus (-alpha, 1)
struct Op {
    cmdg_handle h = nullptr, minus = nullptr;
    int eval(Chain &ch, double *tendency, double *Q, double t, double beta) const
    {
        RhsCtx c;
        c.tendency = tendency;
        c.Qin = Q;
        c.t = t;
        c.alpha = 1.0;
        c.beta = beta;
        if (int r = ch.to(h->eng->s_comp)) return r;
        if (int r = h->eng->rhs_async(c)) return r;
        if (!minus) return CMDG_OK;
        c.alpha = -1.0;
        c.beta = 1.0;
        if (int r = ch.to(minus->eng->s_comp)) return r;
        return minus->eng->rhs_async(c);
    }
};

inline int check_same_grid(const char *stepper, EngineBase *ref, EngineBase *e, const char *what)
{
    const std::string the = std::string(stepper) + ": the " + what + " operator ";
    if (e->nreal != ref->nreal || e->Np != ref->Np || e->NQ != ref->NQ || e->NQV != ref->NQV || e->dev != ref->dev)
        return e->fail(CMDG_ERR_INVALID, the + "lives on another grid than the slow operator");
    if (e->ns != ref->ns)
        return e->fail(CMDG_ERR_INVALID, the + "has " + std::to_string(e->ns) + " states, the slow operator " +
                                             std::to_string(ref->ns) + "; they must be the same (a linear model without the full model's "
                                             "tracers is served by the additive Runge-Kutta step with the column solver only)");
    return CMDG_OK;
}

}  // namespace cmdg
