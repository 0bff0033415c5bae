// Split-explicit barotropic / baroclinic ocean stepper: the exchange functions of
// src/Ocean/SplitExplicit/Communication.jl and dostep! of
// src/Numerics/ODESolvers/SplitExplicitMethod.jl:70-177 over two engines (slow 3-D
// HydrostaticBoussinesqModel, fast ShallowWaterModel on the one-layer extrusion of the 2-D grid).
// Everything is enqueued on the slow engine's compute stream except the fast model's own
// sub-steps; the two streams are ordered with events, the host never waits.
#include <cmath>
#include <vector>

#include "columns.h"
#include "stepping.h"

using namespace cmdg;

namespace {

const char *const LAUNCH = "split explicit launch";

int check(EngineBase *s, EngineBase *f, const cmdg_ocean_coupling_desc *d)
{
    if (!s->stacked || d->nvertelem < 1 || s->nreal % d->nvertelem)
        return s->fail(CMDG_ERR_INVALID, "ocean coupling: slow grid is not stacked by nvertelem");
    if (f->nreal != s->nreal / d->nvertelem)
        return s->fail(CMDG_ERR_INVALID, "ocean coupling: fast grid must hold one element per stack");
    if (f->Np % (s->NQ * s->NQ) || s->Np != s->NQ * s->NQ * s->NQ)
        return s->fail(CMDG_ERR_INVALID, "ocean coupling: horizontal polynomial orders differ");
    if (!(d->H > 0)) return s->fail(CMDG_ERR_INVALID, "ocean coupling: H");
    if (d->slow_u_col < 0 || d->slow_u_col + 2 > s->ns || d->slow_eta_col < 0 ||
        d->slow_eta_col >= s->ns || d->slow_dGu_col < 0 || d->slow_dGu_col + 2 > s->naux ||
        d->fast_eta_col < 0 || d->fast_eta_col >= f->ns || d->fast_U_col < 0 ||
        d->fast_U_col + 2 > f->ns || d->fast_GU_col < 0 || d->fast_GU_col + 2 > f->naux ||
        d->fast_du_col < 0 || d->fast_du_col + 2 > f->naux)
        return s->fail(CMDG_ERR_INVALID, "ocean coupling: column out of range");
    return s->ensure_Imat(d->Imat);
}

int initialize_states(EngineBase *s, const cmdg_ocean_coupling_desc *d)
{
    const int64_t n = (int64_t)s->nreal * 2 * s->Np;
    hipLaunchKernelGGL(k_fill_columns, dim3(nblocks(n)), dim3(256), 0, s->s_comp, s->aux, s->naux,
                       d->slow_dGu_col, 2, -0.0, s->Np, (int64_t)s->nreal);
    return CMDG_OK;
}

int slow_to_fast(EngineBase *s, EngineBase *f, const cmdg_ocean_coupling_desc *d, const double *dQ)
{
    const int Nij = s->NQ * s->NQ, nv = d->nvertelem, Nqk2 = f->Np / Nij;
    const int64_t nh = s->nreal / nv;
    if (int r = s->integrate_velocity(dQ, s->ns, d->slow_u_col, d->nvertelem)) return r;
    if (int r = s->order(f->s_comp, s->s_comp)) return r;
    hipLaunchKernelGGL(k_top_to_layer, dim3(nblocks(nh * f->Np)), dim3(256), 0, s->s_comp, f->aux,
                       f->naux, d->fast_GU_col, (const double *)s->d_flowint, Nij, s->NQ, nv, Nqk2, nh);
    hipLaunchKernelGGL(k_column_minus_top_over_H, dim3(nblocks((int64_t)s->nreal * s->Np)), dim3(256),
                       0, s->s_comp, s->aux, s->naux, d->slow_dGu_col, (const double *)s->aux, s->naux,
                       d->slow_dGu_col, (const double *)s->d_flowint, d->H, Nij, s->NQ, nv,
                       (int64_t)0, nh);
    return s->order(s->s_comp, f->s_comp);
}

int fast_to_slow(EngineBase *s, EngineBase *f, const cmdg_ocean_coupling_desc *d, double *Q3,
                 const double *Q2)
{
    if (int r = s->integrate_velocity(Q3, s->ns, d->slow_u_col, d->nvertelem)) return r;
    const int Nij = s->NQ * s->NQ, nv = d->nvertelem, Nqk2 = f->Np / Nij;
    const int64_t nh = s->nreal / nv;
    if (int r = s->order(f->s_comp, s->s_comp)) return r;
    hipLaunchKernelGGL(k_reconcile_layer, dim3(nblocks(nh * f->Np)), dim3(256), 0, s->s_comp, f->aux,
                       f->naux, d->fast_du_col, Q2, f->ns, d->fast_U_col,
                       (const double *)s->d_flowint, d->H, Nij, s->NQ, nv, Nqk2, nh);
    hipLaunchKernelGGL(k_reconcile_column, dim3(nblocks((int64_t)s->nreal * s->Np)), dim3(256), 0,
                       s->s_comp, Q3, s->ns, d->slow_u_col, d->slow_eta_col, Q2, f->ns, d->fast_U_col,
                       d->fast_eta_col, (const double *)s->d_flowint, d->H, Nij, s->NQ, nv, Nqk2, nh);
    return s->order(s->s_comp, f->s_comp);
}

}  // namespace

extern "C" {

int cmdg_ocean_initialize_states(cmdg_handle slow, cmdg_handle fast, const cmdg_ocean_coupling_desc *d)
{
    if (!d) return CMDG_ERR_INVALID;
    GroupCall gc(&slow, &fast, 1);
    if (!gc.ok()) return CMDG_ERR_INVALID;
    if (int r = check(slow->eng, fast->eng, d)) return gc.finish(r);
    initialize_states(slow->eng, d);
    return gc.finish(slow->eng->launch_status(LAUNCH));
}

int cmdg_ocean_tendency_from_slow_to_fast(cmdg_handle slow, cmdg_handle fast,
                                          const cmdg_ocean_coupling_desc *d, const double *dQ_slow)
{
    if (!d || !dQ_slow) return CMDG_ERR_INVALID;
    GroupCall gc(&slow, &fast, 1);
    if (!gc.ok()) return CMDG_ERR_INVALID;
    if (int r = check(slow->eng, fast->eng, d)) return gc.finish(r);
    if (int r = slow_to_fast(slow->eng, fast->eng, d, dQ_slow)) return gc.finish(r);
    return gc.finish(slow->eng->launch_status(LAUNCH));
}

int cmdg_ocean_reconcile_from_fast_to_slow(cmdg_handle slow, cmdg_handle fast,
                                           const cmdg_ocean_coupling_desc *d, double *Q_slow,
                                           const double *Q_fast)
{
    if (!d || !Q_slow || !Q_fast) return CMDG_ERR_INVALID;
    GroupCall gc(&slow, &fast, 1);
    if (!gc.ok()) return CMDG_ERR_INVALID;
    if (int r = check(slow->eng, fast->eng, d)) return gc.finish(r);
    if (int r = fast_to_slow(slow->eng, fast->eng, d, Q_slow, Q_fast)) return gc.finish(r);
    return gc.finish(slow->eng->launch_status(LAUNCH));
}

// dostep!(Qslow, split::SplitExplicitSolver, param, time) for n (slow, fast) pairs in lock step:
// one pair per rank.  With the RCCL transport a process drives its own pair (n = 1); handles
// connected by cmdg_comm_connect_local are driven together by one host thread (GroupCall: the caller).
static int group_split_explicit_step(int n, cmdg_handle *slow, cmdg_handle *fast,
                                     const cmdg_ocean_coupling_desc *d, int coupled, double **Q3,
                                     double **dQ3, double **dQ2fast, double **Q2, double **dQ2,
                                     double t, double dt, double dt_fast, int nstages,
                                     const double *rka, const double *rkb, const double *rkc)
{
    std::vector<EngineBase *> S(n), F(n);
    for (int i = 0; i < n; ++i) {
        S[i] = slow[i]->eng;
        F[i] = fast[i]->eng;
        if (int r = check(S[i], F[i], d)) return r;
    }
    std::vector<RhsCtx> c(n);
    for (int st = 0; st < nstages; ++st) {
        const double ts = t + rkc[st] * dt;
        for (int i = 0; i < n; ++i) {
            if (coupled) initialize_states(S[i], d);
            c[i] = RhsCtx();
            c[i].Qin = Q3[i];
            c[i].t = ts;
            c[i].alpha = 1.0;
            c[i].tendency = dQ2fast[i];  // slow.rhs!(dQ2fast, Qslow, ...; increment = false)
            c[i].beta = 0.0;
        }
        if (int r = group_rhs(S, c)) return r;
        for (int i = 0; i < n; ++i) {
            if (coupled)
                if (int r = slow_to_fast(S[i], F[i], d, dQ2fast[i])) return r;
            c[i].tendency = dQ3[i];  // slow.rhs!(dQslow, Qslow, ...; increment = true)
            c[i].beta = 1.0;
        }
        if (int r = group_rhs(S, c)) return r;
        // fractional time for the fast sub-steps of this stage
        const double gamma = st == nstages - 1 ? 1 - rkc[st] : rkc[st + 1] - rkc[st];
        const int nsub = dt_fast > 0 ? (int)std::ceil(gamma * dt / dt_fast) : 1;
        const double fdt = gamma * dt / nsub;
        for (int sub = 0; sub < nsub; ++sub)
            if (int r = group_lsrk_step(F, Q2, dQ2, ts + sub * fdt, fdt, nstages, rka, rkb, rkc))
                return r;
        for (int i = 0; i < n; ++i) {
            lsrk_update(S[i], dQ3[i], Q3[i], rka[(st + 1) % nstages], rkb[st] * dt);
            if (coupled)
                if (int r = fast_to_slow(S[i], F[i], d, Q3[i], Q2[i])) return r;
        }
    }
    return S[0]->launch_status(LAUNCH);
}

int cmdg_split_explicit_step(cmdg_handle slow, cmdg_handle fast, const cmdg_ocean_coupling_desc *d,
                             int32_t coupled, double *Q3, double *dQ3, double *dQ2fast, double *Q2,
                             double *dQ2, double t, double dt, double dt_fast, int32_t nstages,
                             const double *rka, const double *rkb, const double *rkc)
{
    if (!slow || !fast || !d || !Q3 || !dQ3 || !dQ2fast || !Q2 || !dQ2 || !rka || !rkb || !rkc ||
        nstages < 1)
        return CMDG_ERR_INVALID;
    if (slow->eng->transport == TRANSPORT_LOCAL && slow->eng->communicate())
        return set_err(slow, slow->eng->fail(CMDG_ERR_INVALID,
                                             "handles connected locally must be driven by "
                                             "cmdg_group_split_explicit_step"));
    GroupCall gc(&slow, &fast, 1);
    return gc.finish(group_split_explicit_step(1, &slow, &fast, d, coupled, &Q3, &dQ3, &dQ2fast, &Q2, &dQ2,
                                               t, dt, dt_fast, nstages, rka, rkb, rkc));
}

int cmdg_group_split_explicit_step(cmdg_handle *slow, cmdg_handle *fast, int32_t n,
                                   const cmdg_ocean_coupling_desc *d, int32_t coupled, double **Q3,
                                   double **dQ3, double **dQ2fast, double **Q2, double **dQ2,
                                   double t, double dt, double dt_fast, int32_t nstages,
                                   const double *rka, const double *rkb, const double *rkc)
{
    if (!d || !Q3 || !dQ3 || !dQ2fast || !Q2 || !dQ2 || !rka || !rkb || !rkc || nstages < 1)
        return CMDG_ERR_INVALID;
    for (int i = 0; i < n; ++i)
        if (!Q3[i] || !dQ3[i] || !dQ2fast[i] || !Q2[i] || !dQ2[i]) return CMDG_ERR_INVALID;
    GroupCall gc(slow, fast, n);
    if (!gc.ok()) return CMDG_ERR_INVALID;
    return gc.finish(group_split_explicit_step(n, slow, fast, d, coupled, Q3, dQ3, dQ2fast, Q2, dQ2, t, dt,
                                               dt_fast, nstages, rka, rkb, rkc));
}

}  // extern "C"
