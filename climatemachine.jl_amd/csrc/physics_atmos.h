// Device functor for the dry AtmosModel configurations in scope (Held-Suarez GCM,
// isentropic vortex, dry LES-type boxes).  Restates, term by term and in the reference's
// summation order:
//   src/Atmos/Model/AtmosModel.jl:625-690 (gradient argument), :808-828 (wavespeed)
//   src/Atmos/Model/tendencies_mass.jl:5-7, tendencies_momentum.jl:13-29,52-55,62-84,
//       tendencies_energy.jl:7-21,37-56, atmos_tendencies.jl (which terms, which order)
//   src/Atmos/Model/energy.jl:17-28,48-57; moisture.jl:47-62 (DryModel aux refresh)
//   src/Atmos/Model/bc_momentum.jl:25-52, bc_energy.jl:10-20, boundaryconditions.jl:60-131
//   src/Common/TurbulenceClosures/TurbulenceClosures.jl:354-420 (constant viscosity),
//       :411-497 (SmagorinskyLilly), :877-912 (DryBiharmonic)
//   experiments/AtmosGCM/heldsuarez.jl:106-172 (HeldSuarezForcing)
// Dry thermodynamics: closed forms of Thermodynamics.jl 0.3.2 (PhaseDry).
//
// Parameter block: see the host side (climatemachine.jl_amd/atmos.py) -- iparam[0]
// orientation, [1] hydrostatic reference state, [2] subtract_off, [3] viscosity kind,
// [4] DryBiharmonic, [5] source bits, [6] nbc, [7..13] bc kinds; dparam[0] viscosity,
// [1] tau, [2..12] R_d cp_d cv_d T_0 grav Omega MSLP day planet_radius inv_Pr_turb kappa_d,
// [13] C_smag; iparam[14] turbulence closure (0 constant viscosity, 1 SmagorinskyLilly);
// iparam[15] bit 0 WithDivergence stress, bit 1 total_specific_enthalpy == 0 (the override of
// test/Numerics/DGMethods/compressible_Navier_Stokes/mms_bc_atmos.jl:50-51).  Source bit 8 =
// MMSSource{3}, boundary kind 2 = InitStateBC with the manufactured solution (same test).
// NTracers (src/Atmos/Model/tracers.jl, tendencies_tracers.jl, bc_tracer.jl): iparam[15] bits 8..15
// the number of tracers NT (at most ATMOS_MAX_TRACERS), dparam[16 + k] the diffusivity ratio
// delta_chi[k].  The tracers follow every other component: prognostic rho chi[NT] after rho e,
// gradient chi[NT] last, gradient flux grad chi (3 x NT, tracer k owns entries 3 k .. 3 k + 2) last,
// auxiliary delta_chi[NT] after moisture.theta_v / air_T.
#pragma once
#include <type_traits>

#include "cmdg_common.h"
#include "exact_quotient.h"
#include "law_defaults.h"

namespace cmdg {

struct AtmosParams {
    int orient, subtract, kinematic, src, nbc;
    int bc[8];
    double visc, tau, R_d, cp_d, cv_d, T_0, grav, Omega, MSLP, day, invPr, C_smag;
    int withdiv, zero_h;  // WithDivergence stress; total_specific_enthalpy overridden to zero
    // Quotients and products of the members above that the pointwise functions used to form per
    // thread -- an fp64 division is ten VALU instructions, spent on a value all lanes share.
    // make_params evaluates the very expressions the device code had (an IEEE double division or
    // product gives the same bits on the host); cmdg_atmos_host_constants returns them in this order.
    double k_a, k_f, k_s;   // Held-Suarez rates 1 / (40 day), 1 / day, 1 / (4 day)
    double kappa;           // R_d / cp_d (the Exner exponent)
    double gamma, gamma_R;  // cp_d / cv_d; gamma * R_d (soundspeed)
    double R_ratio;         // R_m / R_d of a dry phase: R_d / R_d (virtual_pottemp)
};
// The block of a law with shared reciprocals (DryAtmos<..., XQ = true>): the uniform divisors of per-lane
// values, each with its reciprocal (one IEEE division on the host) -- quot(x, m.r_grav) has the bits of
// x / m.grav in four instructions (exact_quotient.h).  A type of its own, so that every other kernel keeps
// its arguments.
struct AtmosXqParams : AtmosParams {
    QuotPair r_grav, r_cv_d, r_MSLP, r_tau;
};
static constexpr int ATMOS_NHOSTCONST = 7;
static constexpr int ATMOS_MAX_TRACERS = 8;
__host__ __device__ inline int atmos_ntracers(const int32_t *ip) { return (ip[15] >> 8) & 0xff; }
// the parameter block of a law with tracers: the tracer-free block, then delta_chi.  (A type of its
// own, so that the tracer-free kernels keep their arguments.)
template <int NT>
struct AtmosTracerParams : AtmosParams {
    double dchi[NT];
};
template <int NT>
struct AtmosParamsOf {
    using type = AtmosTracerParams<NT>;
};
template <>
struct AtmosParamsOf<0> {
    using type = AtmosParams;
};

// XQ: quotients by a uniform divisor and by a density used more than once share a reciprocal
// (exact_quotient.h: the bits of `/` in four instructions).  The shorter instruction stream lets the
// scheduler keep more values in flight, and in many instantiations that costs the tendency pass its
// register class (profiles/ab_exact_quotient.txt), so the engine turns it on where it was measured to
// pay and to fit -- the Held-Suarez law at N = 4 -- and every other instantiation keeps the division.
template <bool ORIENT, bool REF, bool HYPER, bool SMAG = false, bool LAWNF = false, int NT = 0, bool XQ = false>
struct DryAtmos : LawDefaults {
    // RoeNumericalFlux / HLLCNumericalFlux live in a variant of their own so that the
    // kernels of every other configuration keep their register budget
    static constexpr bool LAW_NF = LAWNF;
    static_assert(!(SMAG && HYPER), "gradient-variable order of this combination is not laid out");
    static_assert(!SMAG || ORIENT, "SmagorinskyLilly needs an orientation (buoyancy correction)");
    static_assert(NT >= 0 && NT <= ATMOS_MAX_TRACERS, "iparam[15] bits 8..15 hold at most ATMOS_MAX_TRACERS tracers");
    static_assert(!(LAWNF && NT > 0), "Roe / HLLC / LMARS have no tracer methods in the reference");
    static_assert(!XQ || NT == 0, "shared reciprocals are laid out for the tracer-free block");
    using Params = std::conditional_t<XQ, AtmosXqParams, typename AtmosParamsOf<NT>::type>;
    static constexpr int NS = 5 + NT;
    static constexpr bool SHARED_RECIPROCALS = XQ;
    // x / m.grav, x / m.cv_d, x / m.MSLP, x / m.tau and x / rho: the division, or with XQ its bits from
    // the shared reciprocal
    __host__ __device__ static double by_grav(const Params &m, double a)
    {
        if constexpr (XQ) return quot(a, m.r_grav);
        else return a / m.grav;
    }
    __host__ __device__ static double by_cv_d(const Params &m, double a)
    {
        if constexpr (XQ) return quot(a, m.r_cv_d);
        else return a / m.cv_d;
    }
    __host__ __device__ static double by_MSLP(const Params &m, double a)
    {
        if constexpr (XQ) return quot(a, m.r_MSLP);
        else return a / m.MSLP;
    }
    __host__ __device__ static double by_tau(const Params &m, double a)
    {
        if constexpr (XQ) return quot(a, m.r_tau);
        else return a / m.tau;
    }
    // a density that divides more than once in a function: one pair with XQ, else the divisor alone
    __host__ __device__ static QuotPair rho_pair(double rho)
    {
        if constexpr (XQ) return quot_pair(rho);
        else return QuotPair{rho, 0.0};
    }
    __host__ __device__ static double by_rho(double a, const QuotPair &d)
    {
        if constexpr (XQ) return quot(a, d);
        else return a / d.b;
    }
    static constexpr int OPHI = 3;
    static constexpr int OREF = OPHI + (ORIENT ? 4 : 0);
    static constexpr int OTURB = OREF + (REF ? 7 : 0);   // turbulence.Delta (SmagorinskyLilly)
    static constexpr int ODELTA = OTURB + (SMAG ? 1 : 0);  // hyperdiffusion.Delta
    static constexpr int OMOIST = ODELTA + (HYPER ? 1 : 0);
    static constexpr int OTRAC = OMOIST + 2;  // tracers.delta_chi[NT]: layout parity, read from Params
    static constexpr int NAUX = OTRAC + NT;
    // Gradient: u, h_tot, [turbulence.theta_v], [hyperdiffusion u_h, h_tot], [tracers.chi]
    static constexpr int OGCHI = 4 + (SMAG ? 1 : 0) + (HYPER ? 4 : 0);
    static constexpr int NGRAD = OGCHI + NT;
    // GradientFlux: grad h_tot, S, [N^2], [grad chi (3, NT)]
    static constexpr int OGFCHI = 9 + (SMAG ? 1 : 0);
    static constexpr int NGF = OGFCHI + 3 * NT;
    static constexpr bool GF_NODE_MAJOR = true;  // (law_defaults.h)
    // The gradient pass holds 3 NGRAD gradient components per node.  With tracers the widest
    // combinations no longer fit the 128 VGPRs of the library's four waves per SIMD: DryBiharmonic
    // takes 132 (NT = 1) and 142 (NT = 2), SmagorinskyLilly with two tracers spilled 12 bytes at 128.
    // They ask for three waves (168 VGPRs); every other combination keeps the library's budget.
    static constexpr int GRAD_MIN_WAVES = NT > 0 && (HYPER || (SMAG && NT >= 2)) ? 3 : 0;
    static constexpr int NGL = HYPER ? 4 : 0;
    static constexpr int NHYP = HYPER ? 12 : 0;
    static constexpr bool HAS_UPDATE_AUX = true;
    __host__ __device__ static bool update_aux_active(const Params &) { return true; }
    // the refresh only writes moisture.theta_v / air_T, which no dry tendency reads, so it
    // can ride in the gradient kernel's first phase instead of costing a pass of its own
    static constexpr bool FUSE_UPDATE_AUX = true;
    static constexpr int NUPD = 2;
    __host__ __device__ static constexpr int upd_aux(int i) { return OMOIST + i; }
    // gradient_argument and update_aux are pure functions of the node's (Q, aux): inside
    // cmdg_lsrk_run the fused update may form both for the next stage (kernels.h GradArgHandoff)
    static constexpr bool GRADARG_HANDOFF = true;
    // ... and may leave the refresh out of every such update but the run's last: theta_v / air_T
    // (upd_aux) are read by no pointwise function of this law in any pass -- flux, source,
    // gradient_argument (which forms theta_v itself where it needs it), boundary_state (which
    // writes its own copy) -- so nothing sees them before the run's last hand-off update has
    // written them again (aux_read counts the columns a pass does read; update_aux checks that
    // they fit among the others).
    static constexpr bool GRADARG_REFRESH_UNREAD = true;
    static constexpr bool HAS_SOURCE = true;
    // sin / cos of the latitude (heldsuarez.jl:134,147-149 recomputes them every call; they
    // only depend on aux.coord, so they are evaluated once with the same libm calls)
    static constexpr int NDER = ORIENT ? 2 : 0;
    // Byte accounting (cmdg_query, bench.py): columns of Q and of the auxiliary state the
    // volume code of a pass actually reads -- load_state asks for all of them and the compiler
    // drops the loads nobody uses.  pass: 0 gradients, 1 Laplacian, 2 gradient of Laplacian,
    // 3 tendency.  Gradients: Phi through the internal energy (gradient argument, fused nodal
    // refresh), grad Phi for the horizontal projection of u (DryBiharmonic) or N^2
    // (SmagorinskyLilly).  Gradient of Laplacian: hyperdiffusion.Delta alone (nu_4), no state.
    // Tendency: Phi, grad Phi (gravity, Held-Suarez drag), ref_state rho and p, turbulence.Delta.
    // A tracer adds its state column to the gradient and tendency passes and no auxiliary column:
    // delta_chi comes from Params.
    __host__ __device__ static constexpr int state_read(int pass) { return pass == 1 || pass == 2 ? 0 : NS; }
    __host__ __device__ static constexpr int aux_read(int pass)
    {
        return pass == 0 ? (ORIENT ? 1 + ((HYPER || SMAG) ? 3 : 0) : 0)
               : pass == 1 ? 0
               : pass == 2 ? (HYPER ? 1 : 0)
                           : (ORIENT ? 4 : 0) + (REF ? 2 : 0) + (SMAG ? 1 : 0);
    }
    __host__ __device__ static constexpr int hv_indexmap(int s) { return 4 + s; }
    // tau = (-2 nu) S and D_t = nu / Pr: with nu == 0 the gradient-flux state only multiplies zeros
    static constexpr GradFlux GRADFLUX = SMAG ? GradFlux::always : GradFlux::ask;
    __host__ __device__ static bool needs_gradflux(const Params &m) { return m.visc != 0; }  // (asked without SMAG)
    // auxiliary fields the interior-face fluxes read from the minus side: Phi (potential
    // energy in the thermodynamic state), the reference pressure and, for SmagorinskyLilly,
    // grad Phi (vertical unit vector) and the filter width
    static constexpr int NFAUX = (ORIENT ? 1 : 0) + (REF ? 1 : 0) + (SMAG ? 4 : 0);
    __host__ __device__ static constexpr int face_aux(int i)
    {
        if (SMAG && i >= NFAUX - 4) return i == NFAUX - 1 ? OTURB : OPHI + 1 + (i - (NFAUX - 4));
        return ORIENT ? (i == 0 ? OPHI : OREF + 1) : OREF + 1;
    }

    static void make_params(Params &p, const int32_t *ip, const double *dp)
    {
        p.orient = ip[0];
        p.subtract = ip[2];
        p.kinematic = ip[3];
        p.src = ip[5];
        p.nbc = ip[6];
        for (int i = 0; i < 7; ++i) p.bc[i] = ip[7 + i];
        p.bc[7] = 0;
        p.visc = dp[0];
        p.tau = dp[1];
        p.R_d = dp[2];
        p.cp_d = dp[3];
        p.cv_d = dp[4];
        p.T_0 = dp[5];
        p.grav = dp[6];
        p.Omega = dp[7];
        p.MSLP = dp[8];
        p.day = dp[9];
        p.invPr = dp[11];
        p.C_smag = dp[13];
        p.withdiv = ip[15] & 1;
        p.zero_h = (ip[15] >> 1) & 1;
        if constexpr (NT > 0) {
            for (int k = 0; k < NT; ++k) p.dchi[k] = dp[16 + k];
        }
        derive_params(p);
    }
    static void derive_params(Params &p)
    {
        const double day = p.day, R_d = p.R_d, cp_d = p.cp_d, cv_d = p.cv_d;
        p.k_a = 1 / (40 * day);
        p.k_f = 1 / day;
        p.k_s = 1 / (4 * day);
        p.kappa = R_d / cp_d;
        p.gamma = cp_d / cv_d;
        p.gamma_R = p.gamma * R_d;
        p.R_ratio = R_d / R_d;
        if constexpr (XQ) {
            p.r_grav = quot_pair(p.grav);
            p.r_cv_d = quot_pair(cv_d);
            p.r_MSLP = quot_pair(p.MSLP);
            p.r_tau = quot_pair(p.tau);
        }
    }
    static void host_constants(const Params &p, double *out)
    {
        const double c[ATMOS_NHOSTCONST] = {p.k_a, p.k_f, p.k_s, p.kappa, p.gamma, p.gamma_R, p.R_ratio};
        for (int i = 0; i < ATMOS_NHOSTCONST; ++i) out[i] = c[i];
    }

    // ---- dry thermodynamics ----------------------------------------------------------
    __host__ __device__ static double internal_energy(const Params &, const double *Q, const double *aux)
    {
        const double rho = Q[0];
        const double rhoinv = 1 / rho;
        const double rhoe_kin = rhoinv * (Q[1] * Q[1] + Q[2] * Q[2] + Q[3] * Q[3]) / 2;
        const double e_pot = ORIENT ? aux[OPHI] : -0.0;
        const double rhoe_pot = rho * e_pot;
        const double rhoe_int = Q[4] - rhoe_kin - rhoe_pot;
        return rhoinv * rhoe_int;
    }
    __host__ __device__ static double air_T(const Params &m, double e_int)
    {
        return m.T_0 + by_cv_d(m, e_int);
    }
    __host__ __device__ static double air_p(const Params &m, double T, double rho)
    {
        return m.R_d * rho * T;
    }
    __host__ __device__ static double soundspeed(const Params &m, double T)
    {
        return sqrt(m.gamma_R * T);  // gamma = cp_d / cv_d; sqrt(gamma * R_d * T)
    }

    // ---- vertical finite volume: src/Atmos/Model/prog_prim_conversion.jl:67-78, 114-131, 187-202
    // (DryModel).  Primitives rho, u (3), p; read by fv.h only.
    static constexpr bool HAS_PRIM_CONVERSION = true, HAS_FACE_AUX_STATE = true;
    static constexpr int PRIM_RHO = 0, PRIM_P = 4;
    __host__ __device__ static double prim_gravity(const Params &m) { return m.grav; }
    __device__ static void prognostic_to_primitive(const Params &m, double *prim, const double *Q,
                                                   const double *aux)
    {
        const double rho = Q[0];
        const double T = air_T(m, internal_energy(m, Q, aux));
        prim[0] = rho;
        const QuotPair rp = rho_pair(rho);
#pragma unroll
        for (int d = 0; d < 3; ++d) prim[1 + d] = by_rho(Q[1 + d], rp);
        prim[4] = air_p(m, T, rho);
    }
    // PhaseDry_rho_p: T = p / (R_d rho); total_energy = e_int + e_kin + e_pot
    __device__ static void primitive_to_prognostic(const Params &m, double *Q, const double *prim,
                                                   const double *aux)
    {
        const double rho = prim[0];
        const double T = prim[4] / (m.R_d * rho);
        const double e_int = m.cv_d * (T - m.T_0);
        const double e_kin = (prim[1] * prim[1] + prim[2] * prim[2] + prim[3] * prim[3]) / 2;
        const double e_pot = ORIENT ? aux[OPHI] : 0.0;
        Q[0] = rho;
#pragma unroll
        for (int d = 0; d < 3; ++d) Q[1 + d] = rho * prim[1 + d];
        Q[4] = rho * (e_int + e_kin + e_pot);
    }
    // dz is signed: negative towards the bottom face of the cell
    __device__ static void construct_face_auxiliary_state(const Params &m, double *aux_face,
                                                          const double *aux_cell, double dz)
    {
#pragma unroll
        for (int s = 0; s < NAUX; ++s) aux_face[s] = aux_cell[s];
        if constexpr (ORIENT) aux_face[OPHI] = aux_cell[OPHI] + m.grav * dz / 2;
    }

    // ---- AtmosLESDefault diagnostics: compute_thermo! of a DryModel (src/Diagnostics/thermo.jl:33-49)
    // and the sub-grid enthalpy flux of atmos_les_default_simple_sums! (atmos_les_default.jl:168-170).
    // Columns temp, pres, theta_dry, e_int, h_tot, h_int, d_h_tot[3].  The LES configurations: an
    // orientation that is flat, no hyperdiffusion; MoistAtmos::les_diagnostics reduces to this at
    // q_tot = 0.
    static constexpr bool HAS_LES_DIAGNOSTICS = ORIENT && !HYPER && !LAWNF && NT == 0;
    static constexpr int NDIAG = 7;
    __host__ __device__ static bool les_diagnostics_active(const Params &m) { return m.orient == 1; }
    __device__ static void les_diagnostics(const Params &m, double *D, const double *Q, const double *aux,
                                           const double *gf, double)
    {
        thermo_columns(m, D, Q, aux);
        double nu[3], tau[9];
        turbulence_tensors(m, Q, gf, aux, nu, tau);
        const double Dt = nu[2] * m.invPr;
        D[6] = (-Dt) * gf[2];
    }
    // compute_thermo! of a DryModel: temp, pres, theta_dry, e_int, h_tot, h_int (thermo.jl:33-44); the
    // one place the six expressions are written, for the LES and the GCM groups
    __device__ static void thermo_columns(const Params &m, double *D, const double *Q, const double *aux)
    {
        const double rho = Q[0];
        const double e_tot = Q[4] / rho;
        const double e_int = internal_energy(m, Q, aux);
        const double T = air_T(m, e_int);
        const double p = air_p(m, T, rho);
        const double exner = pow(by_MSLP(m, p), m.kappa);
        const double RT = m.R_d * T;
        D[0] = T;
        D[1] = p;
        D[2] = T / exner;
        D[3] = e_int;
        D[4] = e_tot + RT;
        D[5] = e_int + RT;
    }

    // ---- AtmosGCMDefault diagnostics (src/Diagnostics/atmos_gcm_default.jl): the same six columns,
    // for every configuration with an orientation (a reference state or hyperdiffusion do not enter)
    static constexpr bool STATE_RHO_RHOU = true;
    static constexpr bool HAS_GCM_DIAGNOSTICS = ORIENT && NT == 0;
    __device__ static void gcm_thermo(const Params &m, double *D, const double *Q, const double *aux)
    {
        thermo_columns(m, D, Q, aux);
    }

    // ---- local Courant numbers: src/Atmos/Model/courant.jl:12-83 ------------------------
    // the manufactured-solution pieces (source, InitStateBC) exist in the plain variant only
    static constexpr bool MMS_VARIANT = !ORIENT && !REF && !HYPER && !SMAG && !LAWNF && NT == 0;
    static constexpr bool HAS_COURANT = true;
    static constexpr bool HAS_PENALTY = false;  // update_penalty! is the default no-op
    __device__ static double courant(const Params &m, int kind, const double *Q, const double *aux,
                                     const double *gf, double dx, double dt, double, int direction)
    {
        double k[3] = {0, 0, 0};
        if constexpr (ORIENT) {
#pragma unroll
            for (int d = 0; d < 3; ++d) k[d] = by_grav(m, aux[OPHI + 1 + d]);
        }
        if (kind == 2) {  // diffusive_courant
            double nu[3], tau[9];
            turbulence_tensors(m, Q, gf, aux, nu, tau);
            double normnu;
            if constexpr (!SMAG) {
                normnu = nu[0];  // norm_nu(nu::Real, ...) = nu
            } else {
                const double dk = nu[0] * k[0] + nu[1] * k[1] + nu[2] * k[2];
                if (direction == DIR_VERTICAL) {
                    normnu = dk;
                } else {
                    double v[3];
#pragma unroll
                    for (int d = 0; d < 3; ++d) v[d] = direction == DIR_HORIZONTAL ? nu[d] - dk * k[d] : nu[d];
                    normnu = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
                }
            }
            return dt * normnu / (dx * dx);
        }
        const double dotk = Q[1] * k[0] + Q[2] * k[1] + Q[3] * k[2];
        const QuotPair rp = rho_pair(Q[0]);
        double normu;
        if (direction == DIR_VERTICAL) {
            normu = by_rho(fabs(dotk), rp);
        } else {
            double v[3];
#pragma unroll
            for (int d = 0; d < 3; ++d)
                v[d] = direction == DIR_HORIZONTAL ? by_rho(Q[1 + d] - dotk * k[d], rp)
                                                   : by_rho(Q[1 + d], rp);
            normu = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        }
        if (kind == 0) return dt * normu / dx;
        const double ss = soundspeed(m, air_T(m, internal_energy(m, Q, aux)));
        return dt * (normu + ss) / dx;
    }

    // ---- fluxes ----------------------------------------------------------------------
    __host__ __device__ static void flux_first_order(const Params &m, double *F, const double *Q,
                                            const double *aux, double, int)
    {
        const double rho = Q[0];
        const double T = air_T(m, internal_energy(m, Q, aux));
        const double p = air_p(m, T, rho);
        // three quotients by rho: one pair (its reciprocal is the rhoinv of internal_energy)
        const QuotPair rp = rho_pair(rho);
        double u[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) u[d] = by_rho(Q[1 + d], rp);
#pragma unroll
        for (int d = 0; d < 3; ++d) F[d] = Q[1 + d];
        double pp = p;
        if constexpr (REF) pp = m.subtract ? p - aux[OREF + 1] : p;
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int d = 0; d < 3; ++d)
                F[d + 3 * (1 + c)] = Q[1 + d] * u[c] + (0.0 + (d == c ? pp : 0.0));
#pragma unroll
        for (int d = 0; d < 3; ++d) F[d + 12] = u[d] * Q[4] + u[d] * p;
        // Tracers, Advect (tendencies_tracers.jl:7-11): rho chi[k] u with u = rho u / rho
#pragma unroll
        for (int k = 0; k < NT; ++k)
#pragma unroll
            for (int d = 0; d < 3; ++d) F[d + 3 * (5 + k)] = Q[5 + k] * u[d];
    }
    __device__ static double sym(const double *c, int i, int j)
    {  // SHermitianCompact{3}: (1,1),(2,1),(3,1),(2,2),(3,2),(3,3)
        const int lo = i < j ? i : j, hi = i < j ? j : i;
        return c[lo == 0 ? hi : (lo == 1 ? 2 + hi : 5)];
    }
    // nu (diagonal), tau = (-2 nu) S as a full 3x3 (row d scaled by nu_d):
    // TurbulenceClosures.jl:372-408 (constant viscosity, WithoutDivergence), :476-497 (Smagorinsky)
    __device__ static void turbulence_tensors(const Params &m, const double *Q, const double *gf,
                                              const double *aux, double *nu, double *tau)
    {
        const double *S = gf + 3;
        if constexpr (!SMAG) {
            // m.kinematic is uniform: a scalar branch.  (Left to itself the compiler evaluates the
            // division in every lane and selects per lane; the empty statement keeps it from
            // hoisting the quotient out of its branch.)
            double v = m.visc;
            if (!m.kinematic) {
                __asm__ volatile("");
                v = m.visc / Q[0];
            }
            nu[0] = nu[1] = nu[2] = v;
        } else {
            const double norm2 = S[0] * S[0] + 2 * (S[1] * S[1]) + 2 * (S[2] * S[2]) + S[3] * S[3] +
                                 2 * (S[4] * S[4]) + S[5] * S[5];
            const double normS = sqrt(2 * norm2);
            double k[3];
#pragma unroll
            for (int d = 0; d < 3; ++d) k[d] = by_grav(m, aux[OPHI + 1 + d]);
            const double epsn = nextafter(fabs(normS), INFINITY) - fabs(normS);  // eps(normS)
            const double Ri = gf[9] / (normS * normS + epsn);
            double c = 1.0 - Ri * m.invPr;
            c = c < 0.0 ? 0.0 : (c > 1.0 ? 1.0 : c);
            const double fb2 = sqrt(c);
            const double cd = m.C_smag * aux[OTURB];
            const double nu0 = normS * (cd * cd) + 1e-5;
            const double dk = nu0 * k[0] + nu0 * k[1] + nu0 * k[2];
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const double nv = k[d] * dk, nh = nu0 - nv;
                nu[d] = nh + nv * fb2;
            }
        }
#pragma unroll
        for (int d = 0; d < 3; ++d)
#pragma unroll
            for (int c = 0; c < 3; ++c) tau[d + 3 * c] = (-2 * nu[d]) * sym(S, d, c);
        if constexpr (!SMAG) {
            if (m.withdiv) {  // compute_stress(::WithDivergence, nu, S) (:369-370)
                const double trS = S[0] + S[3] + S[5];
#pragma unroll
                for (int d = 0; d < 3; ++d) tau[d + 3 * d] += (2 * nu[d] / 3) * trS;
            }
        }
    }
    __device__ static void flux_second_order(const Params &m, double *F, const double *Q,
                                             const double *gf, const double *hyp, const double *aux,
                                             double)
    {
        double nu[3], tau[9];
        turbulence_tensors(m, Q, gf, aux, nu, tau);
        const double rho = Q[0];
#pragma unroll
        for (int d = 0; d < 3; ++d) F[d] = 0.0;
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                double x = 0.0 + tau[d + 3 * c] * rho;
                if constexpr (HYPER) x = x + rho * hyp[d + 3 * c];
                F[d + 3 * (1 + c)] = x;
            }
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const double Dt = nu[d] * m.invPr;
            double x = (tau[d] * Q[1] + tau[d + 3] * Q[2] + tau[d + 6] * Q[3]) + (-Dt * gf[d]) * rho;
            if constexpr (HYPER) {
                x = x + hyp[9 + d] * rho;
                x = x + (hyp[d + 0] * Q[1] + hyp[d + 3] * Q[2] + hyp[d + 6] * Q[3]);
            }
            F[d + 12] = x;
        }
        // Tracers, Diffusion (tendencies_tracers.jl:17-22): d_chi = ((-D_t) delta_chi') .* grad chi,
        // then d_chi rho, with the D_t of the energy flux above
        if constexpr (NT > 0) {
#pragma unroll
            for (int k = 0; k < NT; ++k)
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    const double Dt = nu[d] * m.invPr;
                    F[d + 3 * (5 + k)] = (((-Dt) * m.dchi[k]) * gf[OGFCHI + d + 3 * k]) * rho;
                }
        }
    }
    // Held-Suarez forcing coefficients (heldsuarez.jl:116-155)
    __device__ static void init_derived(const Params &, double *der, const double *aux)
    {
        if constexpr (ORIENT) {
            const double phi =
                asin(aux[2] / sqrt(aux[0] * aux[0] + aux[1] * aux[1] + aux[2] * aux[2]));
            der[0] = sin(phi);
            der[1] = cos(phi);
        }
    }
    __host__ __device__ static void hs_coeffs(const Params &m, const double *Q, const double *der,
                                     double T, double &k_v, double &k_T, double &T_equil)
    {
        const double k_a = m.k_a, k_f = m.k_f, k_s = m.k_s;  // 1 / (40 day), 1 / day, 1 / (4 day)
        const double dTy = 60, dthz = 10, T_eq = 315, T_min = 200, sig_b = 7.0 / 10;
        const double p = air_p(m, T, Q[0]);
        const double sig = by_MSLP(m, p);
        const double exner = pow(sig, m.kappa);
        const double dsig = (sig - sig_b) / (1 - sig_b);
        const double hf = dsig > 0 ? dsig : 0;
        const double s = der[0], c = der[1];
        double Te = (T_eq - dTy * (s * s) - dthz * log(sig) * (c * c)) * exner;
        Te = Te > T_min ? Te : T_min;
        T_equil = Te;
        k_T = k_a + (k_s - k_a) * hf * ((c * c) * (c * c));
        k_v = k_f * hf;
    }
    __host__ __device__ static void source(const Params &m, double *S, const double *Q, const double *,
                                  const double *aux, const double *der, double t, int)
    {
        const double rho = Q[0];
        double Sm[3] = {0, 0, 0}, Se = 0;
        bool first = true;
        double T = 0, k_v = 0, k_T = 0, Te = 0;
        if (m.src & 4) {
            T = air_T(m, internal_energy(m, Q, aux));
            hs_coeffs(m, Q, der, T, k_v, k_T, Te);
        }
        if constexpr (ORIENT) {
            if (m.src & 1) {  // Gravity
                double r = rho;
                if constexpr (REF) r = m.subtract ? rho - aux[OREF] : rho;
#pragma unroll
                for (int d = 0; d < 3; ++d) Sm[d] = -r * aux[OPHI + 1 + d];
                first = false;
            }
        }
        if (m.src & 2) {  // Coriolis: -(0, 0, 2 Omega) x rho u
            const double w = 2 * m.Omega;
            const double c[3] = {-(0 * Q[3] - w * Q[2]), -(w * Q[1] - 0 * Q[3]),
                                 -(0 * Q[2] - 0 * Q[1])};
#pragma unroll
            for (int d = 0; d < 3; ++d) Sm[d] = first ? c[d] : Sm[d] + c[d];
            first = false;
        }
        if constexpr (ORIENT) {
            if (m.src & 4) {  // HeldSuarezForcing
                double k[3];
#pragma unroll
                for (int d = 0; d < 3; ++d) k[d] = by_grav(m, aux[OPHI + 1 + d]);
                const double kn = k[0] * Q[1] + k[1] * Q[2] + k[2] * Q[3];
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    const double x = -k_v * (Q[1 + d] - k[d] * kn);
                    Sm[d] = first ? x : Sm[d] + x;
                }
                first = false;
                Se = -k_T * rho * m.cv_d * (T - Te);
            }
        }
        S[0] = 0;
        S[1] = Sm[0];
        S[2] = Sm[1];
        S[3] = Sm[2];
        S[4] = Se;
#pragma unroll
        for (int k = 0; k < NT; ++k) S[5 + k] = 0;  // no tracer source
        if constexpr (MMS_VARIANT) {
            if (m.src & 8) {  // MMSSource{3} (mms_bc_atmos.jl:65-86)
                double Sx[5];
                mms_source(m, t, aux[0], aux[1], aux[2], Sx);
#pragma unroll
                for (int q = 0; q < 5; ++q) S[q] = q == 0 || first ? Sx[q] : S[q] + Sx[q];
            }
        }
    }
    // ---- manufactured solution of mms_bc_atmos.jl (dim = 3; its generating script is
    // mms_solution.jl:10-100): rho = c g + 3, u = v = c g, w = c h, E = c g + 100 with
    // c = cos(pi t), g = sin(pi x) cos(pi y) cos(pi z), h = sin(pi x) cos(pi y) sin(pi z);
    // P = (gamma - 1)(E - rho |u|^2 / 2), tau = 2 mu (eps - tr(eps) / 3), no heat conduction.
    __device__ static void mms_state(double t, double x, double y, double z, double *Q)
    {
        const double pi = 3.14159265358979323846;
        const double c = cos(pi * t), g = sin(pi * x) * cos(pi * y) * cos(pi * z);
        const double h = sin(pi * x) * cos(pi * y) * sin(pi * z);
        const double rho = g * c + 3;
        Q[0] = rho;
        Q[1] = rho * g * c;
        Q[2] = rho * g * c;
        Q[3] = rho * h * c;
        Q[4] = g * c + 100;
    }
    // S = dq/dt + div F(q, grad q), evaluated from the analytic derivatives of g and h
    __device__ static void mms_source(const Params &m, double t, double x, double y, double z,
                                      double *S)
    {
        const double pi = 3.14159265358979323846, pi2 = pi * pi;
        const double gam = m.cp_d / m.cv_d, mu = m.visc;
        const double ct = cos(pi * t), st = sin(pi * t);
        const double sx = sin(pi * x), cx = cos(pi * x), sy = sin(pi * y), cy = cos(pi * y);
        const double sz = sin(pi * z), cz = cos(pi * z);
        const double g = sx * cy * cz, h = sx * cy * sz;
        const double dg[3] = {pi * cx * cy * cz, -pi * sx * sy * cz, -pi * sx * cy * sz};
        const double dh[3] = {pi * cx * cy * sz, -pi * sx * sy * sz, pi * sx * cy * cz};
        // second derivatives, symmetric storage [xx, xy, xz, yy, yz, zz]
        const double Hg[6] = {-pi2 * g, -pi2 * cx * sy * cz, -pi2 * cx * cy * sz,
                              -pi2 * g, pi2 * sx * sy * sz, -pi2 * g};
        const double Hh[6] = {-pi2 * h, -pi2 * cx * sy * sz, pi2 * cx * cy * cz,
                              -pi2 * h, -pi2 * sx * sy * cz, -pi2 * h};
        auto H = [](const double *A, int i, int j) {
            const int lo = i < j ? i : j, hi = i < j ? j : i;
            return A[lo == 0 ? hi : (lo == 1 ? 2 + hi : 5)];
        };
        const double rho = ct * g + 3, rho_t = -pi * st * g, E = ct * g + 100, E_t = -pi * st * g;
        double u[3] = {ct * g, ct * g, ct * h}, u_t[3] = {-pi * st * g, -pi * st * g, -pi * st * h};
        double drho[3], dE[3], du[3][3];  // du[i][j] = d u_i / d x_j
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            drho[j] = ct * dg[j];
            dE[j] = ct * dg[j];
            du[0][j] = ct * dg[j];
            du[1][j] = ct * dg[j];
            du[2][j] = ct * dh[j];
        }
        const double divu = du[0][0] + du[1][1] + du[2][2];
        double lap[3], ddiv[3];  // laplacian of u_i; gradient of div u
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const double *A = i == 2 ? Hh : Hg;
            lap[i] = ct * (H(A, 0, 0) + H(A, 1, 1) + H(A, 2, 2));
            ddiv[i] = ct * (H(Hg, i, 0) + H(Hg, i, 1) + H(Hh, i, 2));
        }
        const double ke = (u[0] * u[0] + u[1] * u[1] + u[2] * u[2]) / 2;
        double dke[3], dP[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) dke[j] = u[0] * du[0][j] + u[1] * du[1][j] + u[2] * du[2][j];
        const double P = (gam - 1) * (E - rho * ke);
#pragma unroll
        for (int j = 0; j < 3; ++j) dP[j] = (gam - 1) * (dE[j] - drho[j] * ke - rho * dke[j]);
        const double udrho = u[0] * drho[0] + u[1] * drho[1] + u[2] * drho[2];
        const double divm = udrho + rho * divu;  // div(rho u)
        S[0] = rho_t + divm;
        double dtau[3];  // d_j tau_ij
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            dtau[i] = mu * (lap[i] + ddiv[i] / 3);
            const double adv = u[0] * du[i][0] + u[1] * du[i][1] + u[2] * du[i][2];
            S[1 + i] = rho_t * u[i] + rho * u_t[i] + u[i] * divm + rho * adv + dP[i] - dtau[i];
        }
        double work = 0;  // d_j (u_i tau_ij)
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            work += u[i] * dtau[i];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const double tau = mu * (du[i][j] + du[j][i]) - (i == j ? 2 * mu / 3 * divu : 0.0);
                work += du[i][j] * tau;
            }
        }
        const double udEP = u[0] * (dE[0] + dP[0]) + u[1] * (dE[1] + dP[1]) + u[2] * (dE[2] + dP[2]);
        S[4] = E_t + (E + P) * divu + udEP - work;
    }
    __host__ __device__ static void gradient_argument(const Params &m, double *G, const double *Q,
                                             const double *aux, double)
    {
        const double rhoinv = 1 / Q[0];
#pragma unroll
        for (int d = 0; d < 3; ++d) G[d] = rhoinv * Q[1 + d];
        const double T = air_T(m, internal_energy(m, Q, aux));
        const double e_tot = Q[4] * (1 / Q[0]);
        G[3] = m.zero_h ? 0.0 : e_tot + m.R_d * T;
        // transform.turbulence.theta_v = aux.moisture.theta_v (:441-449).  The aux entry is
        // the nodal refresh of this same (Q, aux) -- evaluated here so that the fused refresh
        // of neighbouring elements is never read (see FUSE_UPDATE_AUX)
        if constexpr (SMAG) G[4] = theta_v(m, T, Q[0]);
        // transform.tracers.chi = rho chi * rhoinv (tracers.jl:141-150)
#pragma unroll
        for (int k = 0; k < NT; ++k) G[OGCHI + k] = Q[5 + k] * rhoinv;
        if constexpr (HYPER && ORIENT) {
            double u[3], k[3];
#pragma unroll
            for (int d = 0; d < 3; ++d) u[d] = Q[1 + d] * rhoinv;
#pragma unroll
            for (int d = 0; d < 3; ++d) k[d] = by_grav(m, aux[OPHI + 1 + d]);
#pragma unroll
            for (int i = 0; i < 3; ++i) {  // (SDiagonal(1,1,1) - k k') * u
                double acc = 0;
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const double Pij = (i == j ? 1.0 : 0.0) - k[i] * k[j];
                    acc = j == 0 ? Pij * u[j] : acc + Pij * u[j];
                }
                G[4 + i] = acc;
            }
            G[7] = G[3];
        }
    }
    __host__ __device__ static double theta_v(const Params &m, double T, double rho)
    {  // virtual_pottemp of a dry phase (moisture.jl:53-62)
        const double exner = pow(by_MSLP(m, air_p(m, T, rho)), m.kappa);
        return m.R_ratio * (T / exner);
    }
    __device__ static void gradient_flux(const Params &m, double *gf, const double *g,
                                         const double *Q, const double *aux, double t)
    {
        double th = 0;
        if constexpr (SMAG) th = theta_v(m, air_T(m, internal_energy(m, Q, aux)), Q[0]);
        gradient_flux_th(m, gf, g, aux, th);
    }
    // the same with the node's gradient argument at hand: G[4] is theta_v of this (Q, aux), the
    // very expression above (gradient_argument), so the pow is not evaluated again
    static constexpr bool HAS_GRADIENT_FLUX_G = true;
    __device__ static void gradient_flux_g(const Params &m, double *gf, const double *g,
                                           const double *, const double *aux, double,
                                           const double *G)
    {
        gradient_flux_th(m, gf, g, aux, SMAG ? G[SMAG ? 4 : 0] : 0.0);
    }
    __device__ static void gradient_flux_th(const Params &, double *gf, const double *g,
                                            const double *aux, double th)
    {
        if constexpr (SMAG) {  // N^2 = dot(grad theta_v, grad Phi) / theta_v  (:451-466)
            gf[9] = (g[0 + 3 * 4] * aux[OPHI + 1] + g[1 + 3 * 4] * aux[OPHI + 2] +
                     g[2 + 3 * 4] * aux[OPHI + 3]) / th;
        }
#pragma unroll
        for (int d = 0; d < 3; ++d) gf[d] = g[d + 9];
        gf[3] = g[0 + 3 * 0];
        gf[4] = (g[1 + 3 * 0] + g[0 + 3 * 1]) / 2;
        gf[5] = (g[2 + 3 * 0] + g[0 + 3 * 2]) / 2;
        gf[6] = g[1 + 3 * 1];
        gf[7] = (g[2 + 3 * 1] + g[1 + 3 * 2]) / 2;
        gf[8] = g[2 + 3 * 2];
        // diffusive.tracers.grad chi = grad transform.tracers.chi (tracers.jl:151-160)
#pragma unroll
        for (int k = 0; k < NT; ++k)
#pragma unroll
            for (int d = 0; d < 3; ++d) gf[OGFCHI + d + 3 * k] = g[d + 3 * (OGCHI + k)];
    }
    __device__ static void post_gradient_laplacian(const Params &m, double *hyp, const double *gl,
                                                   const double *, const double *aux, double)
    {
        if constexpr (HYPER) {
            const double h = aux[ODELTA] / 2;
            const double nu4 = by_tau(m, (h * h) * (h * h) / 2);
#pragma unroll
            for (int q = 0; q < 12; ++q) hyp[q] = nu4 * gl[q];
        }
    }
    __host__ __device__ static void wavespeed(const Params &m, double *ws, const double *n, const double *Q,
                                     const double *aux, double, int)
    {
        const double rhoinv = 1 / Q[0];
        const double uN =
            fabs(n[0] * (rhoinv * Q[1]) + n[1] * (rhoinv * Q[2]) + n[2] * (rhoinv * Q[3]));
        const double ss = soundspeed(m, air_T(m, internal_energy(m, Q, aux)));
#pragma unroll
        for (int s = 0; s < 5; ++s) ws[s] = uN + ss;
        // wavespeed_tracers! (tracers.jl:162-178): |n . u| alone
#pragma unroll
        for (int k = 0; k < NT; ++k) ws[5 + k] = uN;
    }
    // RoeNumericalFlux (AtmosModel.jl:1003-1130, DryModel only), HLLCNumericalFlux
    // (:1154-1276) and LMARSNumericalFlux (:1515-1600); adds the normal flux to fluxn
    __device__ static double roe_average(double sM, double sP, double vM, double vP)
    {
        return (sM * vM + sP * vP) / (sM + sP);
    }
    __device__ static void numerical_flux_law(const Params &m, int nf, double *fluxn,
                                              const double *n, const double *QM,
                                              const double *auxM, const double *QP,
                                              const double *auxP, double t, int facedir)
    {
        double FM[15], FP[15];
#pragma unroll
        for (int i = 0; i < 15; ++i) FM[i] = FP[i] = -0.0;
        flux_first_order(m, FM, QM, auxM, t, facedir);
        flux_first_order(m, FP, QP, auxP, t, facedir);
        const double rM = QM[0], rP = QP[0];
        double uM[3], uP[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            uM[d] = QM[1 + d] / rM;
            uP[d] = QP[1 + d] / rP;
        }
        const double TM = air_T(m, internal_energy(m, QM, auxM));
        const double TP = air_T(m, internal_energy(m, QP, auxP));
        const double pM = air_p(m, TM, rM), pP = air_p(m, TP, rP);
        const double cM = soundspeed(m, TM), cP = soundspeed(m, TP);
        const double unM = uM[0] * n[0] + uM[1] * n[1] + uM[2] * n[2];
        const double unP = uP[0] * n[0] + uP[1] * n[1] + uP[2] * n[2];
        if (nf == NF_LMARS) {  // AtmosModel.jl:1515-1600, beta = 1
            double ppM = pM, ppP = pP;
            if constexpr (REF)
                if (m.subtract) {
                    ppM -= auxM[OREF + 1];
                    ppP -= auxP[OREF + 1];
                }
            const double hM = m.zero_h ? 0.0 : QM[4] / rM + m.R_d * TM;
            const double hP = m.zero_h ? 0.0 : QP[4] / rP + m.R_d * TP;
            const double beta = 1.0;
            const double u_half = 1.0 / 2 * (unP + unM) - beta * 1 / (rM + rP) / cM * (ppP - ppM);
            const double p_half =
                1.0 / 2 * (ppP + ppM) - beta * ((rM + rP) * cM) / 4 * (unP - unM);
            const bool up = u_half > 0;
            fluxn[0] += (up ? rM : rP) * u_half;
#pragma unroll
            for (int d = 0; d < 3; ++d)
                fluxn[1 + d] += (up ? QM[1 + d] : QP[1 + d]) * u_half + p_half * n[d];
            fluxn[4] += (up ? rM * hM : rP * hP) * u_half;
            return;
        }
        if (nf == NF_ROE) {
            const double nh0 = n[0] / 2, nh1 = n[1] / 2, nh2 = n[2] / 2;
#pragma unroll
            for (int s = 0; s < 5; ++s)
                fluxn[s] += (FM[3 * s] + FP[3 * s]) * nh0 + (FM[3 * s + 1] + FP[3 * s + 1]) * nh1 +
                            (FM[3 * s + 2] + FP[3 * s + 2]) * nh2;
            const double Phi = ORIENT ? auxM[OPHI] : 0.0;
            const double eM = QM[4] / rM, eP = QP[4] / rP;
            const double hM = m.zero_h ? 0.0 : eM + m.R_d * TM;
            const double hP = m.zero_h ? 0.0 : eP + m.R_d * TP;
            const double sM = sqrt(rM), sP = sqrt(rP);
            const double rt = sqrt(rM * rP);
            double ut[3], du[3];
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                ut[d] = roe_average(sM, sP, uM[d], uP[d]);
                du[d] = uP[d] - uM[d];
            }
            const double ht = roe_average(sM, sP, hM, hP);
            const double ct = sqrt(roe_average(sM, sP, cM * cM, cP * cP));
            const double utn = ut[0] * n[0] + ut[1] * n[1] + ut[2] * n[2];
            const double dr = rP - rM, dp = pP - pM;
            const double dun = du[0] * n[0] + du[1] * n[1] + du[2] * n[2];
            const double w1 = fabs(utn - ct) * (dp - rt * ct * dun) / (2 * (ct * ct));
            const double w2 = fabs(utn + ct) * (dp + rt * ct * dun) / (2 * (ct * ct));
            const double w3 = fabs(utn) * (dr - dp / (ct * ct));
            const double w4 = fabs(utn) * rt;
            fluxn[0] -= (w1 + w2 + w3) / 2;
#pragma unroll
            for (int d = 0; d < 3; ++d)
                fluxn[1 + d] -= (w1 * (ut[d] - ct * n[d]) + w2 * (ut[d] + ct * n[d]) + w3 * ut[d] +
                                 w4 * (du[d] - dun * n[d])) / 2;
            const double utut = ut[0] * ut[0] + ut[1] * ut[1] + ut[2] * ut[2];
            const double utdu = ut[0] * du[0] + ut[1] * du[1] + ut[2] * du[2];
            fluxn[4] -= (w1 * (ht - ct * utn) + w2 * (ht + ct * utn) +
                         w3 * (utut / 2 + Phi - m.T_0 * m.cv_d) + w4 * (utdu - utn * dun)) / 2;
            return;
        }
        double fnM[5], fnP[5];
#pragma unroll
        for (int s = 0; s < 5; ++s) {
            fnM[s] = FM[3 * s] * n[0] + FM[3 * s + 1] * n[1] + FM[3 * s + 2] * n[2];
            fnP[s] = FP[3 * s] * n[0] + FP[3 * s + 1] * n[1] + FP[3 * s + 2] * n[2];
        }
        const double SM = fmin(unM - cM, unP - cP), SP = fmax(unM + cM, unP + cP);
        const double S0 = (pP - pM + rM * unM * (SM - unM) - rP * unP * (SP - unP)) /
                          (rM * (SM - unM) - rP * (SP - unP));
        const double p0 =
            (pP + pM + rM * (SM - unM) * (S0 - unM) + rP * (SP - unP) * (S0 - unP)) / 2;
        double mp = p0;
        if constexpr (REF)
            if (m.subtract) mp = p0 - (auxM[OREF + 1] + auxP[OREF + 1]) / 2;
        const double pD[5] = {0.0, mp * n[0], mp * n[1], mp * n[2], p0 * S0};
        if (0 <= SM) {
#pragma unroll
            for (int s = 0; s < 5; ++s) fluxn[s] += fnM[s];
        } else if (0 <= S0) {
#pragma unroll
            for (int s = 0; s < 5; ++s)
                fluxn[s] += (S0 * (SM * QM[s] - fnM[s]) + SM * pD[s]) / (SM - S0);
        } else if (0 <= SP) {
#pragma unroll
            for (int s = 0; s < 5; ++s)
                fluxn[s] += (S0 * (SP * QP[s] - fnP[s]) + SP * pD[s]) / (SP - S0);
        } else {
#pragma unroll
            for (int s = 0; s < 5; ++s) fluxn[s] += fnP[s];
        }
    }
    // DryModel atmos_nodal_update_auxiliary_state! (moisture.jl:53-62)
    __device__ static void update_aux(const Params &m, const double *Q, double *aux, double)
    {
        static_assert(!GRADARG_REFRESH_UNREAD ||
                          (upd_aux(0) == OTRAC - NUPD && aux_read(0) <= OTRAC - NUPD &&
                           aux_read(2) <= OTRAC - NUPD && aux_read(3) <= OTRAC - NUPD),
                      "a pass that reads moisture.theta_v / air_T needs the refresh in every update");
        const double T = air_T(m, internal_energy(m, Q, aux));
        aux[OMOIST] = theta_v(m, T, Q[0]);
        aux[OMOIST + 1] = T;
    }
    __device__ static void boundary_state(const Params &m, int kind, int bctag, double *QP,
                                          double *auxP, const double *n, const double *QM,
                                          const double *, double t, const double *, const double *)
    {
        // InitStateBC (bc_initstate.jl:12-26): the exact solution.  Only the plain variant of
        // the functor carries it, so the production kernels pay no registers for it
        if constexpr (MMS_VARIANT) {
            if (m.bc[bctag - 1] == 2) {
                mms_state(t, auxP[0], auxP[1], auxP[2], QP);
                return;
            }
        }
        // ImpermeableTracer (bc_tracer.jl): rho chi on the plus side stays the copy of the minus side
        if (m.bc[bctag - 1] == 1) {  // Impenetrable(FreeSlip) + Insulating
            const double dn = QM[1] * n[0] + QM[2] * n[1] + QM[3] * n[2];
            const double f = kind == BS_FIRST ? 2 * dn : dn;
#pragma unroll
            for (int d = 0; d < 3; ++d) QP[1 + d] -= f * n[d];
        }
        update_aux(m, QP, auxP, t);
    }
    // normal_boundary_flux_second_order! of AtmosBC: FreeSlip and Insulating add nothing.
    // InitStateBC takes the generic boundary_flux_second_order! (NumericalFluxes.jl:925-967):
    // boundary_state! puts the exact solution on the plus side (bc_initstate.jl:28-46), the
    // gradient flux there is the copy of the minus side, then flux_second_order! of that side.
    __device__ static void boundary_flux_second_order(const Params &m, int bctag, double *F,
                                                      double *QP, double *gfP, double *hypP,
                                                      double *auxP, const double *,
                                                      const double *, const double *,
                                                      const double *, const double *,
                                                      double t, const double *, const double *,
                                                      const double *)
    {
        if constexpr (MMS_VARIANT) {
            if (m.bc[bctag - 1] != 2) return;
            mms_state(t, auxP[0], auxP[1], auxP[2], QP);
            double FPl[15];
#pragma unroll
            for (int q = 0; q < 15; ++q) FPl[q] = -0.0;
            flux_second_order(m, FPl, QP, gfP, hypP, auxP, t);
#pragma unroll
            for (int q = 0; q < 15; ++q) F[q] += FPl[q];
        }
    }
};

}  // namespace cmdg
