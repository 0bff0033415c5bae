/* ORACLE -- TEST INFRASTRUCTURE ONLY (see dg_oracle.h).
 *
 * Pointwise physics of AtmosAcousticGravityLinearModel (dry), physics id 10, restated from
 *   src/Atmos/Model/linear.jl:17-36 (linearized_air_pressure; the moisture terms are zero for
 *       DryModel), :47-56 (linearized_pressure, rho e_pot = rho Phi), :104-117 (the state is the
 *       first five states of the full model), :128-139 (no second-order flux), :158-168
 *       (wavespeed = soundspeed_air(ref.T)), :170-196 (AtmosBC boundary, nothing for second-order
 *       numerical fluxes), :224-245 (first-order flux = sum of the tendencies below),
 *       :257-280 (source: momentum only)
 *   src/Atmos/Model/linear_tendencies.jl (Mass Advect: rho u; Momentum LinearPressureGradient:
 *       pad + p_lin I; Energy LinearEnergyFlux of the AcousticGravity model:
 *       ((ref.rho e + ref.p) / ref.rho) rho u; Gravity source -rho grad Phi in VerticalDirection
 *       and EveryDirection, zero in HorizontalDirection)
 *   src/Atmos/Model/bc_momentum.jl:25-34 (Impenetrable(FreeSlip) for a first-order flux:
 *       rho u+ -= 2 (rho u- . n) n), bc_energy.jl (Insulating: nothing for the first-order flux).
 *
 * The parameter block and the auxiliary array are the full DryAtmosModel's (physics_atmos.c):
 * iparam[0] orientation (needed), [1] reference state (needed), [4] DryBiharmonic, [14]
 * turbulence closure; dparam[2..5] R_d cp_d cv_d T_0.  The law reads Phi, grad Phi and the
 * reference rho, p, T, rho e; the offsets follow the full model's layout.
 */
#include <math.h>
#include <stdlib.h>

#include "dg_oracle.h"

typedef struct {
    double R_d, cp_d, cv_d, T_0;
    int oPhi, oRef;
} atmos_linear_t;

/* linearized_air_pressure(rho, rho e, rho e_pot) (linear.jl:31-35) */
static inline double p_lin(const atmos_linear_t *m, const double *Q, const double *aux)
{
    const double rhoe_pot = Q[0] * aux[m->oPhi];
    return Q[0] * m->R_d * m->T_0 + m->R_d / m->cv_d * (Q[4] - rhoe_pot);
}

static void al_flux1(const void *p_, double *F, const double *Q, const double *aux, double t, int dir)
{
    const atmos_linear_t *m = (const atmos_linear_t *)p_;
    (void)t; (void)dir;
    const double pL = p_lin(m, Q, aux);
    const double *ref = aux + m->oRef; /* rho, p, T, rho e */
    const double h_ref = (ref[3] + ref[1]) / ref[0];
    for (int d = 0; d < 3; ++d) F[d] = Q[1 + d];
    for (int c = 0; c < 3; ++c)
        for (int d = 0; d < 3; ++d) F[d + 3 * (1 + c)] = 0.0 + (d == c ? pL : 0.0);
    for (int d = 0; d < 3; ++d) F[d + 12] = h_ref * Q[1 + d];
}

static void al_flux2(const void *p_, double *F, const double *Q, const double *gf, const double *hyp,
                     const double *aux, double t)
{
    (void)p_; (void)F; (void)Q; (void)gf; (void)hyp; (void)aux; (void)t;
}

/* source!(::AtmosLinearModel) sets source.rho u only; rho and rho e keep the kernel's -0 */
static void al_source(const void *p_, double *S, const double *Q, const double *gf, const double *aux,
                      double t, int dir)
{
    const atmos_linear_t *m = (const atmos_linear_t *)p_;
    (void)gf; (void)t;
    for (int d = 0; d < 3; ++d) S[1 + d] = dir == ORC_HORIZONTAL ? 0.0 : -Q[0] * aux[m->oPhi + 1 + d];
}

static void al_wavespeed(const void *p_, double *ws, const double *n, const double *Q,
                         const double *aux, double t, int facedir)
{
    const atmos_linear_t *m = (const atmos_linear_t *)p_;
    (void)n; (void)Q; (void)t; (void)facedir;
    const double gamma = m->cp_d / m->cv_d;
    const double c = sqrt(gamma * m->R_d * aux[m->oRef + 2]);
    for (int s = 0; s < 5; ++s) ws[s] = c;
}

/* AtmosBC() on every tag; the plus-side auxiliary state is the minus side's (no aux update:
 * boundary_state!(::AtmosLinearModel) calls atmos_boundary_state! only) */
static void al_bstate(const void *p_, int kind, int bctag, double *QP, double *auxP, const double *n,
                      const double *QM, const double *auxM, double t, const double *Q1,
                      const double *aux1)
{
    (void)p_; (void)bctag; (void)auxP; (void)auxM; (void)t; (void)Q1; (void)aux1;
    if (kind != ORC_BS_FIRST) return;
    const double dn = QM[1] * n[0] + QM[2] * n[1] + QM[3] * n[2];
    const double f = 2 * dn;
    for (int d = 0; d < 3; ++d) QP[1 + d] -= f * n[d];
}

static void al_bflux2(const void *p_, int bctag, double *F, double *QP, double *gfP, double *hypP,
                      double *auxP, const double *n, const double *QM, const double *gfM,
                      const double *hypM, const double *auxM, double t, const double *Q1,
                      const double *gf1, const double *aux1)
{
    (void)p_; (void)bctag; (void)F; (void)QP; (void)gfP; (void)hypP; (void)auxP; (void)n;
    (void)QM; (void)gfM; (void)hypM; (void)auxM; (void)t; (void)Q1; (void)gf1; (void)aux1;
}

orc_physics *orc_atmos_linear_new(const int *ip, const double *dp, int nf_first)
{
    if (ip[0] == 0 || ip[1] == 0) return NULL; /* needs an orientation and a reference state */
    if (nf_first != ORC_NF_RUSANOV && nf_first != ORC_NF_CENTRAL) return NULL;
    orc_physics *ph = (orc_physics *)calloc(1, sizeof(orc_physics));
    atmos_linear_t *m = (atmos_linear_t *)calloc(1, sizeof(atmos_linear_t));
    m->R_d = dp[2]; m->cp_d = dp[3]; m->cv_d = dp[4]; m->T_0 = dp[5];
    /* the full model's auxiliary layout (orc_atmos_new) */
    int o = 3;
    m->oPhi = o; o += 4;
    m->oRef = o; o += 7;
    o += ip[14] == 1 ? 1 : 0; /* SmagorinskyLilly Delta */
    o += ip[4] ? 1 : 0;       /* DryBiharmonic Delta */
    o += 2;                   /* DryModel theta_v, T */
    ph->ns = 5;
    ph->naux = o;
    ph->ngrad = ph->ngf = ph->ngl = ph->nhyp = 0;
    ph->nf_first = nf_first;
    ph->p = m;
    ph->flux_first_order = al_flux1;
    ph->flux_second_order = al_flux2;
    ph->source = al_source;
    ph->wavespeed = al_wavespeed;
    ph->boundary_state = al_bstate;
    ph->boundary_flux_second_order = al_bflux2;
    return ph;
}
