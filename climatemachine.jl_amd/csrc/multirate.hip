// Multirate infinitesimal GARK stepping (Sandu 2019): the explicit scheme
// (src/Numerics/ODESolvers/MultirateInfinitesimalGARKExplicit.jl) and the decoupled-implicit one
// (MultirateInfinitesimalGARKDecoupledImplicit.jl), with a low-storage 2N Runge-Kutta method as
// the fast solver (LowStorageRungeKuttaMethod.jl, dostep! with an MRIParam).
//
// Two element-wise kernels over the handle's real elements:
//   k_lsrk_mri_update<NR>  lsrk_mri_update!: dq = dQ + sum_j sc_j R_j; Q += rkb dt dq; dQ = rka dq
//   k_mri_qhat<NR>         mri_create_Qhat!: Qhat = Q + sum_j sc_j R_j
// The scalars sc_j do not vary across nodes: the host computes them in the reference kernels'
// operation order (Horner in tau for the update, the sum over k for Qhat) and passes them, with
// the R_j pointers, by value in one argument struct.  A fast stage therefore enqueues one
// evaluation and one launch, with no copy to the device and no host wait.
//
// cmdg_mrigark_step runs one slow step.  Evaluations run on their handle's compute stream, the
// update kernels on the fast handle's and the Qhat kernel and band solve on the column solver's;
// consecutive operations on different streams are ordered by one event.
#include <math.h>

#include <utility>
#include <vector>

#include "stepping.h"
#include "with_constant.h"

using namespace cmdg;

namespace {

constexpr int MAXR = CMDG_MRI_MAXR;
constexpr int MAX_FAST_STAGES = 14;

struct MriArgs {
    double *out;  // dQ (update) or Qhat
    double *Q;
    const double *R[MAXR];
    double sc[MAXR];
    double rka_next, rkb_dt;
    int64_t n;
};

// lsrk_mri_update! (LowStorageRungeKuttaMethod.jl:206-225)
template <int NR>
__global__ void __launch_bounds__(256) k_lsrk_mri_update(const MriArgs a)
{
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    double dq = a.out[i];
#pragma unroll
    for (int j = 0; j < NR; ++j) dq += a.sc[j] * a.R[j][i];
    a.Q[i] += a.rkb_dt * dq;
    a.out[i] = a.rka_next * dq;
}

// mri_create_Qhat! (MultirateInfinitesimalGARKDecoupledImplicit.jl:220-237)
template <int NR>
__global__ void __launch_bounds__(256) k_mri_qhat(const MriArgs a)
{
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    double qh = a.Q[i];
#pragma unroll
    for (int j = 0; j < NR; ++j) qh += a.sc[j] * a.R[j][i];
    a.out[i] = qh;
}

// the kernels are compiled for 1..MAXR forcing arrays; every caller has checked nR against that
int launch_update(EngineBase *e, const MriArgs &a, int nR)
{
    const dim3 g(grid_one_per_thread(a.n)), b(256);
    if (!with_constant<1, MAXR>(nR, [&](auto n) { hipLaunchKernelGGL(k_lsrk_mri_update<n()>, g, b, 0, e->s_comp, a); }))
        return e->fail(CMDG_ERR_UNSUPPORTED, "mri: update not compiled for " + std::to_string(nR) + " forcing arrays");
    return CMDG_OK;
}

int launch_qhat(EngineBase *e, const MriArgs &a, int nR)
{
    const dim3 g(grid_one_per_thread(a.n)), b(256);
    if (!with_constant<1, MAXR>(nR, [&](auto n) { hipLaunchKernelGGL(k_mri_qhat<n()>, g, b, 0, e->s_comp, a); }))
        return e->fail(CMDG_ERR_UNSUPPORTED, "mri: qhat not compiled for " + std::to_string(nR) + " forcing arrays");
    return CMDG_OK;
}

// the low-level entries' common checks and argument struct
int low_level_args(cmdg_handle h, double *out, const double *Q, int nR, const double *const *R,
                   const double *sc, MriArgs *a)
{
    if (nR < 1 || nR > MAXR)
        return h->eng->fail(CMDG_ERR_INVALID, "mri: 1 to " + std::to_string(MAXR) + " forcing arrays, not " +
                                                  std::to_string(nR));
    *a = MriArgs{};
    a->out = out;
    a->Q = const_cast<double *>(Q);
    for (int j = 0; j < nR; ++j) {
        if (!R[j]) return h->eng->fail(CMDG_ERR_INVALID, "mri: forcing array " + std::to_string(j) + " is NULL");
        a->R[j] = R[j];
        a->sc[j] = sc[j];
    }
    a->n = real_len(h->eng);
    return CMDG_OK;
}

int step(const Op &slow, const Op &fast, BackwardEuler *be, const cmdg_mrigark_desc *d, double *Q,
         double *const *work, double t, double dt)
{
    EngineBase *es = slow.h->eng, *ef = fast.h->eng;
    const int ns = d->nstages, NG = d->ngamma, nf = d->fast_nstages;
    const bool implicit = d->kind == CMDG_MRIGARK_DECOUPLED_IMPLICIT;
    // Γ_k[row, col]: explicit (ns, ns), decoupled implicit (2 ns, ns + 1)
    const int ncols = implicit ? ns + 1 : ns, nrows = implicit ? 2 * ns : ns;
    auto G = [&](int k, int row, int col) { return d->gamma[((int64_t)k * nrows + row) * ncols + col]; };
    double *const *R = work;
    double *dQ = work[ns], *Qhat = work[ns + 1];
    Chain ch(es, "mrigark");
    if (int r = ch.create()) return r;
    EngineBase *elu = implicit ? be->lin->eng : nullptr;
    MriArgs a{};
    a.out = dQ;
    a.Q = Q;
    a.n = real_len(ef);
    for (int j = 0; j < MAXR; ++j) a.R[j] = j < ns ? R[j] : nullptr;
    double ts = t;
    for (int s = 0; s < ns; ++s) {
        const double dts = d->dc[s] * dt;
        const double stage_end = ts + dts;
        // slowrhs!(Rs[s], Q, p, ts, increment = false)
        if (int r = slow.eval(ch, R[s], Q, ts, 0.0)) return r;
        // the fast method's coupling coefficients for R_1..R_s
        double gam[CMDG_MRI_MAXGAMMA][MAXR];
        for (int k = 0; k < NG; ++k)
            for (int j = 0; j <= s; ++j) gam[k][j] = implicit ? G(k, 2 * s, j) / d->dc[s] : G(k, s, j);
        // updatetime!(fast, ts); solve!(Q, fast, mriparam; timeend = ts + dts), adjustfinalstep
        double time = ts;
        while (time < stage_end) {
            double dtf = d->fast_dt;
            bool final_step = false;
            if (time + dtf > stage_end) {
                dtf = stage_end - time;
                final_step = true;
            }
            if (!(dtf > 0) || time + dtf == time)
                return ef->fail(CMDG_ERR_INVALID, "mrigark: the fast step does not advance the fast time");
            for (int st = 0; st < nf; ++st) {
                const double stage_time = time + d->fast_rkc[st] * dtf;
                if (int r = fast.eval(ch, dQ, Q, stage_time, 1.0)) return r;
                const double tau = (stage_time - ts) / dts;
                for (int j = 0; j <= s; ++j) {
                    double sc = gam[NG - 1][j];
                    for (int k = NG - 2; k >= 0; --k) sc = sc * tau + gam[k][j];
                    a.sc[j] = sc;
                }
                a.rka_next = d->fast_rka[(st + 1) % nf];
                a.rkb_dt = d->fast_rkb[st] * dtf;
                if (int r = ch.to(ef->s_comp)) return r;
                if (int r = launch_update(ef, a, s + 1)) return r;
            }
            time = final_step ? stage_end : time + dtf;
        }
        if (implicit) {
            // Qhat = Q + sum_j sum_k dt Γ_k[2s, j] / k R_j; Q = (I - alpha L)^-1 Qhat
            MriArgs qa{};
            qa.out = Qhat;
            qa.Q = Q;
            qa.n = a.n;
            for (int j = 0; j <= s; ++j) {
                double sc = dt * G(0, 2 * s + 1, j);  // (/ 1)
                for (int k = 1; k < NG; ++k) sc += dt * G(k, 2 * s + 1, j) / (k + 1);
                qa.R[j] = R[j];
                qa.sc[j] = sc;
            }
            if (int r = ch.to(elu->s_comp)) return r;
            if (int r = launch_qhat(elu, qa, s + 1)) return r;
            const double alpha = dt * G(0, 2 * s + 1, s + 1);
            if (alpha != be->alpha()) {
                if (!d->lu_adjustable) {
                    char msg[224];
                    snprintf(msg, sizeof msg,
                             "mrigark: the column solver is not adjustable (isadjustable = false) and was "
                             "factored for alpha = %.17g; stage %d needs alpha = dt Gamma = %.17g",
                             be->alpha(), s + 1, alpha);
                    return elu->fail(CMDG_ERR_INVALID, msg);
                }
                if (int r = be->ready(alpha)) return r;
            }
            // besolver!(Q, Qhat, alpha, param, stage_end_time): Q is an iterative solver's initial guess
            if (int r = be->solve(Q, Qhat, stage_end)) return r;
        }
        if (int r = ef->launch_status("mrigark kernels")) return r;
        ts += dts;
    }
    if (hipStreamSynchronize(ch.cur) != hipSuccess) return es->fail(CMDG_ERR_HIP, "mrigark: hipStreamSynchronize");
    return CMDG_OK;
}

int check_desc(cmdg_handle slow, cmdg_handle fast, BackwardEuler *lu, const cmdg_mrigark_desc *d,
               double *const *work, double dt)
{
    EngineBase *es = slow->eng, *ef = fast->eng;
    if (d->kind != CMDG_MRIGARK_EXPLICIT && d->kind != CMDG_MRIGARK_DECOUPLED_IMPLICIT)
        return es->fail(CMDG_ERR_INVALID, "mrigark: unknown kind " + std::to_string(d->kind));
    const bool implicit = d->kind == CMDG_MRIGARK_DECOUPLED_IMPLICIT;
    if (d->nstages < 1 || d->nstages > MAXR)
        return es->fail(CMDG_ERR_INVALID, "mrigark: 1 to " + std::to_string(MAXR) + " slow stages, not " +
                                              std::to_string(d->nstages));
    if (d->ngamma < 1 || d->ngamma > CMDG_MRI_MAXGAMMA)
        return es->fail(CMDG_ERR_INVALID, "mrigark: 1 to " + std::to_string(CMDG_MRI_MAXGAMMA) +
                                              " coupling matrices, not " + std::to_string(d->ngamma));
    if (!d->gamma || !d->dc) return es->fail(CMDG_ERR_INVALID, "mrigark: gamma or dc is NULL");
    if (d->fast_nstages < 1 || d->fast_nstages > MAX_FAST_STAGES)
        return ef->fail(CMDG_ERR_INVALID, "mrigark: the fast 2N tableau has " + std::to_string(d->fast_nstages) +
                                              " stages; 1 to " + std::to_string(MAX_FAST_STAGES) + " are supported");
    if (!d->fast_rka || !d->fast_rkb || !d->fast_rkc)
        return ef->fail(CMDG_ERR_INVALID, "mrigark: the fast tableau is NULL");
    if (!(d->fast_dt > 0)) return ef->fail(CMDG_ERR_INVALID, "mrigark: the fast dt must be > 0");
    if (!(dt > 0)) return es->fail(CMDG_ERR_INVALID, "mrigark: dt must be > 0");
    if (!work) return es->fail(CMDG_ERR_INVALID, "mrigark: the work array list is NULL");
    for (int j = 0; j < d->nstages + 1; ++j)
        if (!work[j])
            return es->fail(CMDG_ERR_INVALID, "mrigark: work array " + std::to_string(j) + " (" +
                                                  (j < d->nstages ? "a stage tendency" : "the fast dQ") +
                                                  ") is NULL");
    if (implicit) {
        if (!lu) return es->fail(CMDG_ERR_INVALID, "mrigark: the decoupled-implicit kind needs the column solver");
        if (!work[d->nstages + 1]) return es->fail(CMDG_ERR_INVALID, "mrigark: work array Qhat is NULL");
        if (lu->lin != slow)
            return es->fail(CMDG_ERR_INVALID,
                            "mrigark: the decoupled-implicit slow operator must be the column solver's linear model");
    } else if (lu) {
        return es->fail(CMDG_ERR_INVALID, "mrigark: the explicit kind takes no column solver");
    }
    return CMDG_OK;
}

// the step behind cmdg_mrigark_step and cmdg_mrigark_step_gmres
int mrigark_step(cmdg_handle slow, cmdg_handle slow_minus, cmdg_handle fast, cmdg_handle fast_minus,
                 BackwardEuler *be, const cmdg_mrigark_desc *d, double *Q, double *const *work, double t, double dt)
{
    if (!slow || !fast || !d || !Q) return CMDG_ERR_INVALID;
    std::vector<std::pair<cmdg_handle, std::string>> named{{slow, "slow"}};
    if (slow_minus) named.push_back({slow_minus, "slow minus"});
    named.push_back({fast, "fast"});
    if (fast_minus) named.push_back({fast_minus, "fast minus"});
    GroupCall gc(named);
    if (!gc.ok()) return CMDG_ERR_INVALID;
    EngineBase *es = slow->eng;
    if (slow_minus)
        if (int r = check_same_grid("mrigark", es, slow_minus->eng, "subtracted slow")) return gc.finish(r);
    if (int r = check_same_grid("mrigark", es, fast->eng, "fast")) return gc.finish(r);
    if (fast_minus)
        if (int r = check_same_grid("mrigark", es, fast_minus->eng, "subtracted fast")) return gc.finish(r);
    if (int r = check_desc(slow, fast, be, d, work, dt)) return gc.finish(r);
    if (be && slow_minus)
        return gc.finish(es->fail(CMDG_ERR_INVALID,
                                  "mrigark: the decoupled-implicit slow operator cannot be a remainder"));
    return gc.finish(step(Op{slow, slow_minus}, Op{fast, fast_minus}, be, d, Q, work, t, dt));
}

}  // namespace

extern "C" {

int cmdg_mri_lsrk_update(cmdg_handle h, double *dQ, double *Q, double rka_next, double rkb_dt, int32_t nR,
                         const double *const *R, const double *sc)
{
    if (!h || !dQ || !Q || !R || !sc) return CMDG_ERR_INVALID;
    DevGuard guard_(h->eng);
    MriArgs a;
    if (int r = low_level_args(h, dQ, Q, nR, R, sc, &a)) return set_err(h, r);
    a.rka_next = rka_next;
    a.rkb_dt = rkb_dt;
    if (int r = launch_update(h->eng, a, nR)) return set_err(h, r);
    return set_err(h, h->eng->launch_status("k_lsrk_mri_update"));
}

int cmdg_mri_qhat(cmdg_handle h, double *Qhat, const double *Q, int32_t nR, const double *const *R,
                  const double *sc)
{
    if (!h || !Qhat || !Q || !R || !sc) return CMDG_ERR_INVALID;
    DevGuard guard_(h->eng);
    MriArgs a;
    if (int r = low_level_args(h, Qhat, Q, nR, R, sc, &a)) return set_err(h, r);
    if (int r = launch_qhat(h->eng, a, nR)) return set_err(h, r);
    return set_err(h, h->eng->launch_status("k_mri_qhat"));
}

int cmdg_mrigark_step(cmdg_handle slow, cmdg_handle slow_minus, cmdg_handle fast, cmdg_handle fast_minus,
                      cmdg_columnlu_handle lu, const cmdg_mrigark_desc *d, double *Q, double *const *work,
                      double t, double dt)
{
    return mrigark_step(slow, slow_minus, fast, fast_minus, lu ? columnlu_solver(lu) : nullptr, d, Q, work, t, dt);
}

int cmdg_mrigark_step_gmres(cmdg_handle slow, cmdg_handle slow_minus, cmdg_handle fast, cmdg_handle fast_minus,
                            cmdg_gmres_handle gmres, const cmdg_mrigark_desc *d, double *Q, double *const *work,
                            double t, double dt)
{
    if (!gmres) return CMDG_ERR_INVALID;
    return mrigark_step(slow, slow_minus, fast, fast_minus, gmres_solver(gmres), d, Q, work, t, dt);
}

}  // extern "C"
