// Device functor for the DryAtmosModel of the reference's entropy-stable DG tests
// (test/Numerics/ESDGMethods/DryAtmos/DryAtmos.jl), the law an ESDGModel handle
// (cmdg_create_esdg, esdg.h) evaluates.  Restated term by term:
//   DryAtmos.jl:79-94 (impenetrable wall), :198-280 (flux, wave speed, pressure, total energy,
//   sound speed), :339-409 (entropy variables and entropy), :411-456 (EntropyConservative),
//   :485-503 (CentralVolumeFlux), :505-539 (KGVolumeFlux), :542-561, :801-810 (sources),
//   :564-615 (EntropyConservativeWithPenalty), :617-745 (MatrixFlux);
//   src/Numerics/DGMethods/NumericalFluxes.jl:540-581 (n . H), :589-612 (ave, logave).
// The reference's compile-time settings are fixed as they stand there: total_energy = false
// (the pressure and the energy carry no rho Phi) and fluctuation_gravity = false (the fluctuation
// part of every two-point flux is empty, gravity is a source).  With both off no flux reads Phi:
// the kernels read grad Phi alone (Gravity), and the wall copies Phi to a plus side nobody reads.
//
// State: rho, rho u[3], rho e.  Auxiliary: Phi, grad Phi[3], then ref_state.{T, p, rho, rho e} when
// a DryReferenceState is chosen (filled on the host, read by no kernel).
// Parameter block: iparam[0] orientation (0 flat, 1 spherical; host only), [1] reference state,
// [2] number of sources, [3..4] the sources in the order of m.sources (1 Coriolis, 2 Gravity);
// dparam as the dry atmosphere's (physics_atmos.h): [2..10] R_d cp_d cv_d T_0 grav Omega MSLP day
// planet_radius.
#pragma once
#include "cmdg_common.h"

namespace cmdg {

enum { ESDG_SRC_CORIOLIS = 1, ESDG_SRC_GRAVITY = 2 };
// two-point fluxes (include/cmdg.h CMDG_ESDG_FLUX_*)
enum {
    ESDG_NONE = 0, ESDG_EC = 1, ESDG_CENTRAL = 2, ESDG_KG = 3, ESDG_RUSANOV = 4, ESDG_EC_PENALTY = 5,
    ESDG_MATRIX = 6
};

struct EsdgDryAtmosParams {
    int nsrc, src[2];
    double gamma, grav, Omega, planet_radius;
    // MatrixFlux(Mcut, low_mach, kinetic_energy_preserving)
    double Mcut;
    int low_mach, kep;
};

// ave / logave  NumericalFluxes.jl:589-612
__host__ __device__ __forceinline__ double esdg_ave(double a, double b) { return (a + b) / 2; }
__host__ __device__ __forceinline__ double esdg_logave(double a, double b)
{
    const double zeta = a / b;
    const double f = (zeta - 1) / (zeta + 1);
    const double u = f * f;
    double F;
    if (u < 2.220446049250313e-16) {  // eps(Float64): @evalpoly(u, 1, 1/3, 1/5, 1/7, 1/9)
        F = 1.0 / 9;
        F = F * u + 1.0 / 7;
        F = F * u + 1.0 / 5;
        F = F * u + 1.0 / 3;
        F = F * u + 1.0;
    } else {
        F = log(zeta) / (2 * f);
    }
    return (a + b) / (2 * F);
}

// What the two-point fluxes need of a node, formed once per node by the expressions the reference
// evaluates per pair.  UINV: the velocity as flux_first_order! forms it (rhoinv * rho u, the central
// flux), else rho u / rho.
struct EsdgNode {
    double rho, u[3], rhoe, p, b, usq, e;
};

struct EsdgDryAtmos : LawDefaults {
    using Params = EsdgDryAtmosParams;
    // NAUX: the columns a kernel may read (Phi, grad Phi); the array has four more with a reference
    // state, so its column count travels in the kernel arguments (EsdgArgs::naux)
    static constexpr int NS = 5, NAUX = 4, NGRAD = 0, NGF = 0, NFAUX = 1;
    static constexpr int NENT = 6;  // entropy variables: rho, rho u[3], rho e, Phi
    static constexpr bool HAS_SOURCE = true;
    static constexpr GradFlux GRADFLUX = GradFlux::never;
    static void make_params(Params &p, const int32_t *ip, const double *dp)
    {
        p.nsrc = ip[2] < 0 ? 0 : (ip[2] > 2 ? 2 : ip[2]);
        p.src[0] = ip[3];
        p.src[1] = ip[4];
        p.gamma = dp[3] / dp[4];  // cp_d / cv_d
        p.grav = dp[6];
        p.Omega = dp[7];
        p.planet_radius = dp[10];
        p.Mcut = 0;
        p.low_mach = p.kep = 0;
    }

    // ---- pointwise thermodynamics  DryAtmos.jl:245-280 ------------------------------------
    __device__ __forceinline__ static double pressure(const Params &m, double rho, const double *rhou, double rhoe)
    {
        return (m.gamma - 1) * (rhoe - (rhou[0] * rhou[0] + rhou[1] * rhou[1] + rhou[2] * rhou[2]) / (2 * rho));
    }
    __device__ __forceinline__ static double totalenergy(const Params &m, double rho, const double *rhou, double p)
    {
        return p / (m.gamma - 1) + (rhou[0] * rhou[0] + rhou[1] * rhou[1] + rhou[2] * rhou[2]) / (2 * rho);
    }
    __device__ __forceinline__ static double soundspeed(const Params &m, double rho, double p)
    {
        return sqrt(m.gamma * p / rho);
    }
    template <bool UINV = false>
    __device__ __forceinline__ static void node(const Params &m, EsdgNode &n, const double *Q)
    {
        n.rho = Q[0];
        if constexpr (UINV) {
            const double rhoinv = 1 / Q[0];
#pragma unroll
            for (int d = 0; d < 3; ++d) n.u[d] = rhoinv * Q[1 + d];
        } else {
#pragma unroll
            for (int d = 0; d < 3; ++d) n.u[d] = Q[1 + d] / Q[0];
        }
        n.rhoe = Q[4];
        n.p = pressure(m, Q[0], Q + 1, Q[4]);
        n.b = n.rho / (2 * n.p);
        n.usq = n.u[0] * n.u[0] + n.u[1] * n.u[1] + n.u[2] * n.u[2];
        n.e = Q[4] / Q[0];
    }

    // flux_first_order!  :198-218; F[3 * s + d]
    __device__ static void flux_first_order(const Params &m, double *F, const double *Q, const double *, double, int)
    {
        const double rho = Q[0], rhoinv = 1 / rho, rhoe = Q[4];
        const double u[3] = {rhoinv * Q[1], rhoinv * Q[2], rhoinv * Q[3]};
        const double p = pressure(m, rho, Q + 1, rhoe);
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const double ru = rho * u[d];
            F[d] += ru;
#pragma unroll
            for (int c = 0; c < 3; ++c) F[3 * (1 + c) + d] += (d == c ? p + ru * u[c] : ru * u[c]);
            F[3 * 4 + d] += u[d] * (rhoe + p);
        }
    }
    // wavespeed  :220-237 (one speed for every state)
    __device__ static void wavespeed(const Params &m, double *ws, const double *n, const double *Q, const double *,
                                     double, int)
    {
        const double rho = Q[0];
        const double p = pressure(m, rho, Q + 1, Q[4]);
        const double u[3] = {Q[1] / rho, Q[2] / rho, Q[3] / rho};
        const double uN = fabs(n[0] * u[0] + n[1] * u[1] + n[2] * u[2]);
        const double w = uN + soundspeed(m, rho, p);
#pragma unroll
        for (int s = 0; s < NS; ++s) ws[s] = w;
    }
    // source!  :542-561 (Coriolis), :801-810 (Gravity), in the order of m.sources
    __device__ static void source(const Params &m, double *S, const double *Q, const double *, const double *aux,
                                  const double *, double, int)
    {
        for (int i = 0; i < m.nsrc; ++i) {
            if (m.src[i] == ESDG_SRC_CORIOLIS) {  // source.rho u -= (0, 0, 2 Omega) x rho u
                const double w = 2 * m.Omega;
                S[1] -= 0 * Q[3] - w * Q[2];
                S[2] -= w * Q[1] - 0 * Q[3];
                S[3] -= 0 * Q[2] - 0 * Q[1];
            } else if (m.src[i] == ESDG_SRC_GRAVITY) {
#pragma unroll
                for (int d = 0; d < 3; ++d) S[1 + d] -= Q[0] * aux[1 + d];
                S[4] -= Q[1] * aux[1] + Q[2] * aux[2] + Q[3] * aux[3];
            }
        }
    }
    // boundary_state!  :79-94: tags 1 and 2, the impenetrable wall (QP, auxP enter as copies of the
    // minus side)
    __device__ static void boundary_state(const Params &, int, int, double *QP, double *auxP, const double *n,
                                          const double *QM, const double *auxM, double, const double *,
                                          const double *)
    {
        const double dn = 2 * (QM[1] * n[0] + QM[2] * n[1] + QM[3] * n[2]);
        QP[0] = QM[0];
#pragma unroll
        for (int d = 0; d < 3; ++d) QP[1 + d] -= dn * n[d];
        QP[4] = QM[4];
        auxP[0] = auxM[0];
    }

    // ---- local Courant numbers  :747-793 (kind 0 advective, 1 nondiffusive; the law has no diffusive
    // one): k_hat = grad Phi / grav, norm_u by direction
    static constexpr bool HAS_COURANT = true;
    __device__ static double courant(const Params &m, int kind, const double *Q, const double *aux, const double *,
                                     double dx, double dt, double, int direction)
    {
        const double k[3] = {aux[1] / m.grav, aux[2] / m.grav, aux[3] / m.grav};
        const double dotk = Q[1] * k[0] + Q[2] * k[1] + Q[3] * k[2];
        double normu;
        if (direction == DIR_VERTICAL) {
            normu = fabs(dotk) / Q[0];
        } else {
            double v[3];
#pragma unroll
            for (int d = 0; d < 3; ++d)
                v[d] = direction == DIR_HORIZONTAL ? (Q[1 + d] - dotk * k[d]) / Q[0] : Q[1 + d] / Q[0];
            normu = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        }
        if (kind == 0) return dt * normu / dx;
        const double ss = soundspeed(m, Q[0], pressure(m, Q[0], Q + 1, Q[4]));
        return dt * (normu + ss) / dx;
    }

    // ---- entropy  :339-409 -----------------------------------------------------------------
    __device__ static void state_to_entropy_variables(const Params &m, double *ent, const double *Q, const double *)
    {
        const double rho = Q[0], g = m.gamma;
        const double p = pressure(m, rho, Q + 1, Q[4]);
        const double s = log(p / pow(rho, g));
        const double b = rho / (2 * p);
        const double u[3] = {Q[1] / rho, Q[2] / rho, Q[3] / rho};
        ent[0] = (g - s) / (g - 1) - (u[0] * u[0] + u[1] * u[1] + u[2] * u[2]) * b;
#pragma unroll
        for (int d = 0; d < 3; ++d) ent[1 + d] = 2 * b * u[d];
        ent[4] = -2 * b;
        ent[5] = 2 * rho * b;
    }
    __device__ static void entropy_variables_to_state(const Params &m, double *Q, double *aux, const double *ent)
    {
        const double g = m.gamma;
        const double b = -ent[4] / 2;
        const double rho = ent[5] / (2 * b);
        const double rhou[3] = {rho * ent[1] / (2 * b), rho * ent[2] / (2 * b), rho * ent[3] / (2 * b)};
        const double p = rho / (2 * b);
        const double s = log(p / pow(rho, g));
        const double uu = rhou[0] * rhou[0] + rhou[1] * rhou[1] + rhou[2] * rhou[2];
        const double Phi = uu / (2 * (rho * rho)) - ((g - s) / (g - 1) - ent[0]) / (2 * b);
        Q[0] = rho;
#pragma unroll
        for (int d = 0; d < 3; ++d) Q[1 + d] = rhou[d];
        Q[4] = p / (g - 1) + uu / (2 * rho) + rho * Phi;
        aux[0] = Phi;
    }
    __device__ static double state_to_entropy(const Params &m, const double *Q, const double *)
    {
        const double rho = Q[0], g = m.gamma;
        const double p = pressure(m, rho, Q + 1, Q[4]);
        const double s = log(p / pow(rho, g));
        return -rho * s / (g - 1);
    }

    // ---- two-point volume fluxes, H[d][s] (conservative part; the fluctuation part is empty) ----
    template <int VF>
    __device__ __forceinline__ static void volume_flux(const Params &m, double (&H)[3][NS], const EsdgNode &n1,
                                                       const EsdgNode &n2)
    {
        static_assert(VF == ESDG_EC || VF == ESDG_CENTRAL || VF == ESDG_KG, "a two-point volume flux");
        if constexpr (VF == ESDG_EC) {  // :411-456
            const double rho_avg = esdg_ave(n1.rho, n2.rho);
            const double u_avg[3] = {esdg_ave(n1.u[0], n2.u[0]), esdg_ave(n1.u[1], n2.u[1]), esdg_ave(n1.u[2], n2.u[2])};
            const double b_avg = esdg_ave(n1.b, n2.b);
            const double usq_avg = esdg_ave(n1.usq, n2.usq);
            const double rho_log = esdg_logave(n1.rho, n2.rho);
            const double b_log = esdg_logave(n1.b, n2.b);
            const double Frho[3] = {u_avg[0] * rho_log, u_avg[1] * rho_log, u_avg[2] * rho_log};
            const double pd = rho_avg / (2 * b_avg);
            const double ce = 1 / (2 * (m.gamma - 1) * b_log) - usq_avg / 2;
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                double Fru[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) Fru[c] = d == c ? u_avg[d] * Frho[c] + pd : u_avg[d] * Frho[c];
                H[d][0] = Frho[d];
#pragma unroll
                for (int c = 0; c < 3; ++c) H[d][1 + c] = Fru[c];
                H[d][4] = ce * Frho[d] + (Fru[0] * u_avg[0] + Fru[1] * u_avg[1] + Fru[2] * u_avg[2]);
            }
        } else if constexpr (VF == ESDG_CENTRAL) {  // :485-503, the nodes' u formed as rhoinv * rho u
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const double r1 = n1.rho * n1.u[d], r2 = n2.rho * n2.u[d];
                H[d][0] = (r1 + r2) / 2;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const double f1 = d == c ? n1.p + r1 * n1.u[c] : r1 * n1.u[c];
                    const double f2 = d == c ? n2.p + r2 * n2.u[c] : r2 * n2.u[c];
                    H[d][1 + c] = (f1 + f2) / 2;
                }
                H[d][4] = (n1.u[d] * (n1.rhoe + n1.p) + n2.u[d] * (n2.rhoe + n2.p)) / 2;
            }
        } else {  // KGVolumeFlux  :505-539
            const double rho_avg = esdg_ave(n1.rho, n2.rho);
            const double u_avg[3] = {esdg_ave(n1.u[0], n2.u[0]), esdg_ave(n1.u[1], n2.u[1]), esdg_ave(n1.u[2], n2.u[2])};
            const double e_avg = esdg_ave(n1.e, n2.e);
            const double p_avg = esdg_ave(n1.p, n2.p);
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const double ru = rho_avg * u_avg[d];
                H[d][0] = ru;
#pragma unroll
                for (int c = 0; c < 3; ++c) H[d][1 + c] = d == c ? p_avg + ru * u_avg[c] : ru * u_avg[c];
                H[d][4] = ru * e_avg + p_avg * u_avg[d];
            }
        }
    }

    // ---- surface fluxes: flux += ... for the minus node (QM) against the plus node (QP) ----------
    // EntropyConservative  NumericalFluxes.jl:540-581: n . H of the entropy-conservative two-point flux
    __device__ static void surface_ec(const Params &m, double *flux, const double *n, const double *QM, const double *QP)
    {
        EsdgNode a, b;
        node(m, a, QM);
        node(m, b, QP);
        double H[3][NS];
        volume_flux<ESDG_EC>(m, H, a, b);
#pragma unroll
        for (int s = 0; s < NS; ++s) flux[s] += n[0] * H[0][s] + n[1] * H[1][s] + n[2] * H[2][s];
    }
    // EntropyConservativeWithPenalty  DryAtmos.jl:564-615
    __device__ static void surface_ec_penalty(const Params &m, double *flux, const double *n, const double *QM,
                                              const double *QP)
    {
        surface_ec(m, flux, n, QM, QP);
        double wM[NS], wP[NS];
        wavespeed(m, wM, n, QM, nullptr, 0, 0);
        wavespeed(m, wP, n, QP, nullptr, 0, 0);
        const double mw = wM[0] > wP[0] ? wM[0] : wP[0];
#pragma unroll
        for (int s = 0; s < NS; ++s) flux[s] += mw * (QM[s] - QP[s]) / 2;
    }
    // MatrixFlux  DryAtmos.jl:617-745
    __device__ static void surface_matrix(const Params &m, double *flux, const double *n, const double *QM,
                                          const double *QP)
    {
        surface_ec(m, flux, n, QM, QP);
        const double g = m.gamma;
        const double pi = 3.141592653589793;
        const double om = pi / 3, de = pi / 5;
        const double r[3] = {sin(om) * cos(de), cos(om) * cos(de), sin(de)};
        const double t1[3] = {r[1] * n[2] - r[2] * n[1], r[2] * n[0] - r[0] * n[2], r[0] * n[1] - r[1] * n[0]};
        const double t2[3] = {t1[1] * n[2] - t1[2] * n[1], t1[2] * n[0] - t1[0] * n[2], t1[0] * n[1] - t1[1] * n[0]};
        EsdgNode a, b;
        node(m, a, QM);
        node(m, b, QP);
        const double rho_log = esdg_logave(a.rho, b.rho);
        const double b_log = esdg_logave(a.b, b.b);
        const double u_avg[3] = {esdg_ave(a.u[0], b.u[0]), esdg_ave(a.u[1], b.u[1]), esdg_ave(a.u[2], b.u[2])};
        const double p_avg = esdg_ave(a.rho, b.rho) / (2 * esdg_ave(a.b, b.b));
        const double u2bar = 2 * (u_avg[0] * u_avg[0] + u_avg[1] * u_avg[1] + u_avg[2] * u_avg[2]) -
                             (esdg_ave(a.u[0] * a.u[0], b.u[0] * b.u[0]) + esdg_ave(a.u[1] * a.u[1], b.u[1] * b.u[1]) +
                              esdg_ave(a.u[2] * a.u[2], b.u[2] * b.u[2]));
        const double h_bar = g / (2 * b_log * (g - 1)) + u2bar / 2 + 0;
        double c_bar = sqrt(g * p_avg / rho_log);
        const double uN = u_avg[0] * n[0] + u_avg[1] * n[1] + u_avg[2] * n[2];
        double R[5][5];  // R[i][j]: row i of column j
        for (int i = 0; i < 3; ++i) {
            R[1 + i][0] = u_avg[i] - c_bar * n[i];
            R[1 + i][1] = u_avg[i];
            R[1 + i][2] = t1[i];
            R[1 + i][3] = t2[i];
            R[1 + i][4] = u_avg[i] + c_bar * n[i];
        }
        R[0][0] = 1, R[0][1] = 1, R[0][2] = 0, R[0][3] = 0, R[0][4] = 1;
        R[4][0] = h_bar - c_bar * uN;
        R[4][1] = u2bar / 2 + 0;
        R[4][2] = t1[0] * u_avg[0] + t1[1] * u_avg[1] + t1[2] * u_avg[2];
        R[4][3] = t2[0] * u_avg[0] + t2[1] * u_avg[1] + t2[2] * u_avg[2];
        R[4][4] = h_bar + c_bar * uN;
        if (m.low_mach) {
            const double M = fabs(uN) / c_bar;
            const double lim = M < 1.0 ? M : 1.0;
            c_bar *= lim > m.Mcut ? lim : m.Mcut;
        }
        double ll, lr;
        if (m.kep) {
            ll = fabs(uN) + c_bar;
            lr = ll;
        } else {
            ll = fabs(uN - c_bar);
            lr = fabs(uN + c_bar);
        }
        const double lam[5] = {ll, fabs(uN), fabs(uN), fabs(uN), lr};
        const double T[5] = {rho_log / (2 * g), rho_log * (g - 1) / g, p_avg, p_avg, rho_log / (2 * g)};
        double eM[NENT], eP[NENT], dE[5];
        state_to_entropy_variables(m, eM, QM, nullptr);
        state_to_entropy_variables(m, eP, QP, nullptr);
#pragma unroll
        for (int k = 0; k < 5; ++k) dE[k] = eP[k] - eM[k];
        // flux -= ((((R Lambda) T) R') dE) / 2, products and sums in that order
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            double B[5];
#pragma unroll
            for (int j = 0; j < 5; ++j) B[j] = R[i][j] * lam[j] * T[j];
            double acc = 0;
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                const double A = B[0] * R[k][0] + B[1] * R[k][1] + B[2] * R[k][2] + B[3] * R[k][3] + B[4] * R[k][4];
                acc = k == 0 ? A * dE[0] : acc + A * dE[k];
            }
            flux[i] -= acc / 2;
        }
    }
};

// The law on the auxiliary array of a model with a reference state: the column count a pointwise
// kernel strides by (the Courant kernel loads NAUX columns per node; the flux-differencing passes
// carry the count in their arguments).
struct EsdgDryAtmosRef : EsdgDryAtmos {
    static constexpr int NAUX = 8;
};

}  // namespace cmdg
