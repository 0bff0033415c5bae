// The time steppers other than the fused LSRK run (lsrk_run.hip) and the multirate ones
// (multirate.hip, split_explicit*.hip): the 2N update on its own, the strong-stability-preserving
// and 3N low-storage Runge-Kutta steps over one operator, and the low-storage additive
// Runge-Kutta step (AdditiveRungeKuttaMethod.jl, LowStorageVariant) over a full operator and the
// column solver's linear one.
#include "stepping.h"

using namespace cmdg;

namespace {

const char *const LAUNCH = "stepper launch";

// update! of StrongStabilityPreservingRungeKuttaMethod.jl:167-190
__global__ void k_ssprk_update(const double *__restrict__ R, const double *__restrict__ Q,
                               double *__restrict__ Qstage, double rka1, double rka2, double rkb,
                               double dt, int64_t n)
{
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x)
        Qstage[i] = rka1 * Q[i] + rka2 * Qstage[i] + dt * rkb * R[i];
}

// update! of LowStorageRungeKutta3NMethod.jl:201-226
__global__ void k_ls3n_update(double *__restrict__ dQ, double *__restrict__ dR, double *__restrict__ Q,
                              double rka1, double rka2, double rkb1, double rkb2, double dt,
                              int64_t n)
{
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        Q[i] += rkb1 * dt * dQ[i] + rkb2 * dt * dR[i];
        dR[i] += rka2 * dQ[i];
        dQ[i] *= rka1;
    }
}
__global__ void k_fill(double *__restrict__ a, double v, int64_t n)
{
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x)
        a[i] = v;
}

// The additive step's pointers and the coefficients of one launch, by value as the kernel
// argument: Qs[0] is Q; rkcoeff and dtA are the stage's row, bdt is rkb dt.
struct ArkArgs {
    double *Qs[4];
    const double *R[4];
    double rkcoeff[4], dtA[4], bdt[4];
    int64_t len;
};

// stage_update! (LowStorageVariant, AdditiveRungeKuttaMethod.jl:565-605) over the real elements; Qtt
// (when given) is initialised for an iterative solver, which starts from it (:603)
__global__ void __launch_bounds__(256) k_ark_stage(const ArkArgs a, double *Qhat, double *Qtt, int is)
{
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= a.len) return;
    double Qhat_i = a.Qs[0][i];
    double Qst = -0.0;
#pragma unroll
    for (int js = 0; js < 3; ++js) {
        if (js >= is) break;
        const double common = a.rkcoeff[js] * a.Qs[js][i];
        Qhat_i += common + a.dtA[js] * a.R[js][i];
        Qst -= common;
    }
    a.Qs[is][i] = Qst;
    Qhat[i] = Qhat_i;
    if (Qtt) Qtt[i] = Qhat_i;
}

__global__ void k_add(double *a, const double *b, int64_t len)
{
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i < len) a[i] += b[i];
}

// A linear model that ends before the full model's trailing states (AtmosLinearModel carries no
// tracers, AtmosModel.jl:399-406): its arrays are narrow, (Np, nsl, nelem), and the step moves the
// leading nsl columns of the wide (Np, nsf, nelem) arrays in and out.  One thread per narrow entry.
struct Lead {
    int64_t len;  // nreal * nsl * Np
    int nsl, nsf, Np;
    __device__ int64_t wide(int64_t i) const
    {
        const int64_t col = i / Np, e = col / nsl;
        return i + e * (int64_t)(nsf - nsl) * Np;
    }
};
// narrow = the leading columns of wide
__global__ void __launch_bounds__(256) k_lead_get(const Lead l, double *__restrict__ narrow, const double *__restrict__ wide)
{
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i < l.len) narrow[i] = wide[l.wide(i)];
}
// the leading columns of wide = narrow (the linear tendency leaves the trailing columns alone,
// DGModel.jl:98-102)
__global__ void __launch_bounds__(256) k_lead_put(const Lead l, double *__restrict__ wide, const double *__restrict__ narrow)
{
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i < l.len) wide[l.wide(i)] = narrow[i];
}
// Qs += Qtt, where Qtt is Qhat with its leading columns replaced by the solve's result: the column
// solver does Q .= Qrhs and substitutes over the linear model's states only
// (columnwise_lu_solver.jl:119,132).  One thread per wide entry.
__global__ void __launch_bounds__(256) k_add_solved(double *__restrict__ Qs, const double *__restrict__ Qhat,
                                                    const double *__restrict__ Qtt_narrow, int nsl, int nsf, int Np,
                                                    int64_t len)
{
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= len) return;
    const int64_t col = i / Np, e = col / nsf;
    const int s = (int)(col - e * nsf);
    Qs[i] += s < nsl ? Qtt_narrow[i - e * (int64_t)(nsf - nsl) * Np] : Qhat[i];
}

// solution_update! (LowStorageVariant, :670-690)
__global__ void __launch_bounds__(256) k_ark_solution(const ArkArgs a, int nstages)
{
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= a.len) return;
    double q = a.Qs[0][i];
#pragma unroll
    for (int is = 0; is < 4; ++is) {
        if (is >= nstages) break;
        q += a.bdt[is] * a.R[is][i];
    }
    a.Qs[0][i] = q;
}

// The full operator runs on its handle's stream, as do the stage and solution kernels; the linear
// operator, the backward-Euler solve and k_add run on the linear handle's.
int ark_step(cmdg_handle full, BackwardEuler *be, double *Q, double *const *work, double t, double dt,
             int32_t nstages, const double *rka_explicit, const double *rka_implicit, const double *rkb,
             const double *rkc, int32_t split_explicit_implicit)
{
    if (!full || !be || !Q || !work || !rka_explicit || !rka_implicit || !rkb || !rkc) return CMDG_ERR_INVALID;
    const cmdg_handle lin = be->lin;
    GroupCall gc({{full, "full"}, {lin, "linear"}});
    if (!gc.ok()) return CMDG_ERR_INVALID;
    EngineBase *ef = full->eng, *el = lin->eng;
    if (nstages < 2 || nstages > 4) return gc.finish(ef->fail(CMDG_ERR_INVALID, "ark: 2 to 4 stages"));
    // narrow: the linear model's states are the leading ones of a wider full model (tracers)
    const bool narrow = el->ns < ef->ns;
    if (ef->ns < el->ns || (narrow && (be->iterative || ef->esdg)))
        return gc.finish(ef->fail(CMDG_ERR_INVALID,
                                  "ark: the full model has " + std::to_string(ef->ns) + " states, the linear model " +
                                      std::to_string(el->ns) + "; served are equal counts, and with the column solver a "
                                      "linear model that ends before the full model's trailing states (tracers): not "
                                      "with GMRES, not with an ESDGModel"));
    if (ef->nreal != el->nreal || ef->Np != el->Np || ef->dev != el->dev)
        return gc.finish(ef->fail(CMDG_ERR_INVALID, "ark: the full and the linear model live on different grids"));
    // an ESDGModel handle as the full operator: eager evaluations through Op::eval like any other, on
    // one rank (its exchanges have not been driven from inside a step)
    if (ef->esdg && (ef->nghost > 0 || el->nghost > 0))
        return gc.finish(ef->fail(CMDG_ERR_UNSUPPORTED, "ark: an ESDGModel as the full operator on a partitioned grid "
                                                        "is not supported (one rank only)"));
    const int ns = nstages;
    for (int i = 0; i < 2 * ns + 1 + (narrow ? 4 : 0); ++i)
        if (!work[i]) return gc.finish(ef->fail(CMDG_ERR_INVALID, "ark: work array " + std::to_string(i) + " is NULL"));
    auto A = [&](const double *m, int i, int j) { return m[i * ns + j]; };  // row-major (stage, stage)
    // work: Qstages[1..ns-1], Rstages[0..ns-1], Qhat, Qtt; narrow: then four arrays shaped like the
    // linear model's state -- the leading columns of a stage and of its tendency, Qhat and Qtt of the solve
    ArkArgs a{};
    a.Qs[0] = Q;
    for (int i = 1; i < ns; ++i) a.Qs[i] = work[i - 1];
    for (int i = 0; i < ns; ++i) a.R[i] = work[ns - 1 + i];
    double *const *Qs = a.Qs, *const *R = work + ns - 1;
    double *Qhat = work[2 * ns - 1], *Qtt = work[2 * ns];
    a.len = real_len(ef);
    for (int is = 0; is < ns; ++is) a.bdt[is] = rkb[is] * dt;
    const dim3 g(grid_one_per_thread(a.len)), b(256);
    double *nQ = nullptr, *nT = nullptr, *nQhat = nullptr, *nQtt = nullptr;
    Lead lead{};
    if (narrow) {
        nQ = work[2 * ns + 1], nT = work[2 * ns + 2], nQhat = work[2 * ns + 3], nQtt = work[2 * ns + 4];
        lead.len = real_len(el);
        lead.nsl = el->ns, lead.nsf = ef->ns, lead.Np = ef->Np;
    }
    const dim3 gl(grid_one_per_thread(narrow ? lead.len : 1));
    Chain ch(ef, "ark");
    if (int r = ch.create()) return gc.finish(r);
    // the explicit tendency: the full operator, or "full minus linear" as two evaluations (not the
    // reference's fused RemBL kernel)
    const Op expl{full, split_explicit_implicit && !narrow ? lin : nullptr}, impl{lin};
    hipStream_t sf = ef->s_comp, sl = el->s_comp;
    // narrow: R[lead] += sign L(Q[lead]) on the linear handle's stream.  The leading columns of R
    // go through a narrow array, so that the linear operator increments them with (alpha, beta) =
    // (sign, 1) exactly as it increments the whole array of a pair of equal counts: the same bits.
    auto add_linear = [&](double *Rw, double *Qw, double tt, double sign) -> int {
        if (int r = ch.to(sl)) return r;
        hipLaunchKernelGGL(k_lead_get, gl, b, 0, sl, lead, nQ, Qw);
        hipLaunchKernelGGL(k_lead_get, gl, b, 0, sl, lead, nT, Rw);
        RhsCtx c;
        c.tendency = nT;
        c.Qin = nQ;
        c.t = tt;
        c.alpha = sign;
        c.beta = 1.0;
        if (int r = el->rhs_async(c)) return r;
        hipLaunchKernelGGL(k_lead_put, gl, b, 0, sl, lead, Rw, nT);
        return CMDG_OK;
    };
    auto explicit_eval = [&](double *Rw, double *Qw, double tt) -> int {
        if (int r = expl.eval(ch, Rw, Qw, tt, 0.0)) return r;
        return narrow && split_explicit_implicit ? add_linear(Rw, Qw, tt, -1.0) : CMDG_OK;
    };
    if (int r = explicit_eval(R[0], Qs[0], t + rkc[0] * dt)) return gc.finish(r);
    for (int is = 1; is < ns; ++is) {
        for (int js = 0; js < is; ++js) {
            a.rkcoeff[js] = split_explicit_implicit
                                ? A(rka_implicit, is, js) / A(rka_implicit, is, is)
                                : (A(rka_implicit, is, js) - A(rka_explicit, is, js)) / A(rka_implicit, is, is);
            a.dtA[js] = dt * A(rka_explicit, is, js);
        }
        if (int r = ch.to(sf)) return gc.finish(r);
        hipLaunchKernelGGL(k_ark_stage, g, b, 0, sf, a, Qhat, be->iterative ? Qtt : (double *)nullptr, is);
        // Q_tt = Qhat + alpha L(Q_tt), alpha = dt a_ii; the solver is made ready again when alpha changes
        if (int r = ch.to(sl)) return gc.finish(r);
        const double alpha = dt * A(rka_implicit, is, is);
        if (alpha != be->alpha())
            if (int r = be->ready(alpha)) return gc.finish(r);
        if (narrow) {
            hipLaunchKernelGGL(k_lead_get, gl, b, 0, sl, lead, nQhat, Qhat);
            if (int r = be->solve(nQtt, nQhat, t + rkc[is] * dt)) return gc.finish(r);
            hipLaunchKernelGGL(k_add_solved, g, b, 0, sl, Qs[is], Qhat, nQtt, lead.nsl, lead.nsf, lead.Np, a.len);
        } else {
            if (int r = be->solve(Qtt, Qhat, t + rkc[is] * dt)) return gc.finish(r);
            hipLaunchKernelGGL(k_add, g, b, 0, sl, Qs[is], Qtt, a.len);
        }
        if (int r = explicit_eval(R[is], Qs[is], t + rkc[is] * dt)) return gc.finish(r);
    }
    if (split_explicit_implicit)
        // rhs_implicit!(Rstages[is], Qstages[is], p, stagetime, increment = true)
        for (int is = 0; is < ns; ++is)
            if (int r = narrow ? add_linear(R[is], Qs[is], t + rkc[is] * dt, 1.0)
                               : impl.eval(ch, R[is], Qs[is], t + rkc[is] * dt, 1.0))
                return gc.finish(r);
    if (int r = ch.to(sf)) return gc.finish(r);
    hipLaunchKernelGGL(k_ark_solution, g, b, 0, sf, a, ns);
    if (int r = ef->launch_status("ark kernels")) return gc.finish(r);
    if (hipStreamSynchronize(sf) != hipSuccess) return gc.finish(ef->fail(CMDG_ERR_HIP, "ark: hipStreamSynchronize"));
    return CMDG_OK;
}

}  // namespace

extern "C" {

int cmdg_lsrk_update(cmdg_handle h, double *dQ, double *Q, double rka_next, double rkb_dt)
{
    if (!h || !dQ || !Q) return CMDG_ERR_INVALID;
    DevGuard guard_(h->eng);
    lsrk_update(h->eng, dQ, Q, rka_next, rkb_dt);
    return set_err(h, h->eng->launch_status(LAUNCH));
}

int cmdg_ls3n_step(cmdg_handle h, double *Q, double *dQ, double *dR, double t, double dt,
                   int32_t nstages, const double *rka, const double *rkb, const double *rkc)
{
    if (!h || !Q || !dQ || !dR || !rka || !rkb || !rkc || nstages < 1) return CMDG_ERR_INVALID;
    DevGuard guard_(h->eng);
    EngineBase *e = h->eng;
    const int64_t n = real_len(e);
    Chain ch(e, "ls3n");
    hipLaunchKernelGGL(k_fill, dim3(nblocks(n)), dim3(256), 0, e->s_comp, dR, 0.0, n);  // `rv_dR .= -0`: integer -0, i.e. +0.0
    for (int s = 0; s < nstages; ++s) {
        if (int r = Op{h}.eval(ch, dQ, Q, t + rkc[s] * dt, 1.0)) return set_err(h, r);  // increment = true
        const int sn = (s + 1) % nstages;
        hipLaunchKernelGGL(k_ls3n_update, dim3(nblocks(n)), dim3(256), 0, e->s_comp, dQ, dR, Q,
                           rka[2 * sn], rka[2 * sn + 1], rkb[2 * s], rkb[2 * s + 1], dt, n);
    }
    return set_err(h, e->launch_status(LAUNCH));
}

int cmdg_ssprk_step(cmdg_handle h, double *Q, double *Rstage, double *Qstage, double t, double dt,
                    int32_t nstages, const double *rka, const double *rkb, const double *rkc)
{
    if (!h || !Q || !Rstage || !Qstage || !rka || !rkb || !rkc || nstages < 1) return CMDG_ERR_INVALID;
    DevGuard guard_(h->eng);
    EngineBase *e = h->eng;
    const int64_t n = real_len(e);
    Chain ch(e, "ssprk");
    if (hipMemcpyAsync(Qstage, Q, sizeof(double) * n, hipMemcpyDeviceToDevice, e->s_comp) != hipSuccess)
        return set_err(h, e->fail(CMDG_ERR_HIP, "ssprk: copy failed"));
    for (int s = 0; s < nstages; ++s) {
        if (int r = Op{h}.eval(ch, Rstage, Qstage, t + rkc[s] * dt, 0.0)) return set_err(h, r);
        hipLaunchKernelGGL(k_ssprk_update, dim3(nblocks(n)), dim3(256), 0, e->s_comp,
                           (const double *)Rstage, (const double *)Q, Qstage, rka[2 * s],
                           rka[2 * s + 1], rkb[s], dt, n);
    }
    if (hipMemcpyAsync(Q, Qstage, sizeof(double) * n, hipMemcpyDeviceToDevice, e->s_comp) != hipSuccess)
        return set_err(h, e->fail(CMDG_ERR_HIP, "ssprk: copy failed"));
    return set_err(h, e->launch_status(LAUNCH));
}

int cmdg_ark_step(cmdg_handle full, cmdg_columnlu_handle lu, double *Q, double *const *work, double t,
                  double dt, int32_t nstages, const double *rka_explicit, const double *rka_implicit,
                  const double *rkb, const double *rkc, int32_t split_explicit_implicit)
{
    if (!lu) return CMDG_ERR_INVALID;
    return ark_step(full, columnlu_solver(lu), Q, work, t, dt, nstages, rka_explicit, rka_implicit, rkb, rkc,
                    split_explicit_implicit);
}

int cmdg_ark_step_gmres(cmdg_handle full, cmdg_gmres_handle gmres, double *Q, double *const *work, double t,
                        double dt, int32_t nstages, const double *rka_explicit, const double *rka_implicit,
                        const double *rkb, const double *rkc, int32_t split_explicit_implicit)
{
    if (!gmres) return CMDG_ERR_INVALID;
    return ark_step(full, gmres_solver(gmres), Q, work, t, dt, nstages, rka_explicit, rka_implicit, rkb, rkc,
                    split_explicit_implicit);
}

}  // extern "C"
