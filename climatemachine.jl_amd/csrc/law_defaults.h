// The interface of a balance-law functor -- the `P` of the pass kernels (kernels.h, fv.h) and of
// EngineT<P, Nq, Nqv> (engine.h) -- written down in one place.  A law is a struct of static members
// that derives from LawDefaults: it defines the mandatory members, and of the optional ones those
// in which it differs from the default.  The kernels read every member as plain `P::X`.
//
// MANDATORY (LawDefaults has none of them: leaving one out is a compile error)
//   using Params                      the parameter block handed to every pointwise function (by value
//                                     in the kernel arguments: trivially copyable)
//   static constexpr int NS           number_states(Prognostic)
//                        NAUX         number_states(Auxiliary)
//                        NGRAD        number_states(Gradient)
//                        NGF          number_states(GradientFlux)
//   static void make_params(Params &, const int32_t *iparam, const double *dparam)
//                                     host: the block out of cmdg_desc::iparam / dparam
//   static constexpr GradFlux GRADFLUX = GradFlux::never / GradFlux::always
//     or  __host__ __device__ static bool needs_gradflux(const Params &)
//                                     does flux_second_order read the gradient-flux state at all (a
//                                     zero viscosity only multiplies it by zero): if not, the passes
//                                     take the instantiations that neither form nor read it.  A law
//                                     whose answer is a constant states it, and the engine instantiates
//                                     the pass kernels of that answer alone; only a law whose answer
//                                     depends on its parameters defines the function (GRADFLUX is then
//                                     the default, GradFlux::ask).  Read through needs_gradflux<P>(prm).
//   __device__ static void flux_first_order(const Params &, double *F, const double *Q,
//                                           const double *aux, double t, int direction)
//                                     flux_first_order!: F[d + 3 s] += ...
//   __device__ static void wavespeed(const Params &, double *ws, const double *n, const double *Q,
//                                    const double *aux, double t, int direction)
//                                     wavespeed: ws[s], one per state (Rusanov)
//
// OPTIONAL: the members of LawDefaults below, each with its default and the function of the
// reference it stands for.  The pointwise hooks default to a variadic no-op, because `Params`
// differs per law.  A function of the same name in the law hides the base's whole overload set, so
// one with a wrong signature is still a compile error at the kernel's call site, never a silent
// fall-through to the no-op.
//
// Members a kernel names only under a flag have no default (the `if constexpr` on the flag discards
// the call): numerical_flux_law (LAW_NF), flux_wavespeed (HAS_FLUX_WAVESPEED), gradient_flux_g
// (HAS_GRADIENT_FLUX_G), prognostic_to_primitive / primitive_to_prognostic (HAS_PRIM_CONVERSION),
// construct_face_auxiliary_state (HAS_FACE_AUX_STATE; PRIM_RHO / PRIM_P / prim_gravity go with the
// conversion).  The entropy-stable passes (esdg.h) ask for
// more -- NENT, state_to_entropy_variables, state_to_entropy, volume_flux, surface_* -- of the one
// law they serve (physics_esdg_dryatmos.h).
#pragma once

namespace cmdg {

// what a law knows at compile time about its gradient-flux state (GRADFLUX below)
enum class GradFlux { ask, never, always };

struct LawDefaults {
    // does flux_second_order read the gradient-flux state: never, always, or ask
    // needs_gradflux(prm) of the law at run time.  The engine names the pass kernels of the answers
    // that are left (engine.h pick_tendency, pick_gradients).
    static constexpr GradFlux GRADFLUX = GradFlux::ask;
    // ---- sizes ---------------------------------------------------------------------------------
    static constexpr int NGL = 0;    // number_states(GradientLaplacian): fields whose Laplacian is formed
    static constexpr int NHYP = 0;   // number_states(Hyperdiffusive)
    // gradient argument entry of Laplacian field s (the reference's hyperdiffusion index map)
    __host__ __device__ static constexpr int hv_indexmap(int) { return 0; }
    // auxiliary columns the interior-face fluxes read from both sides: NFAUX of them, face_aux(i)
    // their column numbers (boundary faces get the whole minus-side auxiliary state)
    static constexpr int NFAUX = 0;
    __host__ __device__ static constexpr int face_aux(int) { return 0; }
    // time-invariant per-node fields the library keeps for `source` (init_derived fills them once)
    static constexpr int NDER = 0;
    template <class... A>
    __device__ static void init_derived(A &&...)  // (prm, der, aux)
    {
    }

    // ---- pointwise hooks: no-ops ---------------------------------------------------------------
    template <class... A>
    __device__ static void flux_second_order(A &&...)  // flux_second_order! (prm, F, Q, gf, hyp, aux, t)
    {
    }
    static constexpr bool HAS_SOURCE = false;
    template <class... A>
    __device__ static void source(A &&...)  // source! (prm, S, Q, gf, aux, der, t, direction)
    {
    }
    template <class... A>
    __device__ static void gradient_argument(A &&...)  // compute_gradient_argument! (prm, G, Q, aux, t)
    {
    }
    template <class... A>
    __device__ static void gradient_flux(A &&...)  // compute_gradient_flux! (prm, gf, gradG, Q, aux, t)
    {
    }
    // compute_gradient_flux! of a node whose gradient ARGUMENT is at hand (the volume node's own, the
    // minus side of a face): a law whose gradient flux needs a quantity that is also an entry of its
    // argument (the dry atmosphere's theta_v under SmagorinskyLilly, a pow) says true and defines
    // gradient_flux_g(prm, gf, gradG, Q, aux, t, G), which the gradient pass then calls instead.
    static constexpr bool HAS_GRADIENT_FLUX_G = false;
    template <class... A>
    __device__ static void post_gradient_laplacian(A &&...)  // transform_post_gradient_laplacian!
    {                                                        // (prm, hyp, gradlap, Q, aux, t)
    }
    // update_penalty! of the Rusanov flux (prm, pen, n, QM, QP), called when HAS_PENALTY
    static constexpr bool HAS_PENALTY = false;
    template <class... A>
    __device__ static void update_penalty(A &&...)
    {
    }
    // boundary_state! for the first-order and the gradient numerical flux (prm, kind = BS_FIRST /
    // BS_GRADIENT, bctag, QP, auxP, n, QM, auxM, t, Q1, aux1): the default leaves the plus side the
    // copy of the minus side it arrives as
    template <class... A>
    __device__ static void boundary_state(A &&...)
    {
    }
    // normal_boundary_flux_second_order!: boundary_state! for the second-order flux, then the law's
    // flux_second_order of the plus side into F (prm, bctag, F, QP, gfP, hypP, auxP, n, QM, gfM, hypM,
    // auxM, t, Q1, gf1, aux1).  The default adds nothing: right for a law without a second-order
    // flux or without boundaries.
    template <class... A>
    __device__ static void boundary_flux_second_order(A &&...)
    {
    }
    template <class... A>
    __device__ static void boundary_state_divergence(A &&...)  // boundary_state! of numerical_boundary_
    {  // flux_divergence! (prm, bctag, gradP, auxP, n, gradM, auxM, t)
    }
    template <class... A>
    __device__ static void boundary_state_higher_order(A &&...)  // ... of numerical_boundary_flux_higher_
    {  // order! (prm, bctag, QP, auxP, lapP, n, QM, auxM, lapM, t)
    }

    // ---- nodal auxiliary refresh: nodal_update_auxiliary_state! ---------------------------------
    // HAS_UPDATE_AUX: update_aux(prm, Q, aux, t) exists; update_aux_active(prm): this parameter
    // block needs it.  NUPD / upd_aux(i): the columns it rewrites (NUPD = 0: all of them).
    // FUSE_UPDATE_AUX: none of those columns is read by a kernel of the evaluation that refreshes
    // them, so the refresh rides in the gradient pass instead of a launch of its own.
    static constexpr bool HAS_UPDATE_AUX = false, FUSE_UPDATE_AUX = false;
    static constexpr int NUPD = 0;
    __host__ __device__ static constexpr int upd_aux(int) { return 0; }
    template <class... A>
    __host__ __device__ static bool update_aux_active(A &&...)
    {
        return false;
    }
    template <class... A>
    __device__ static void update_aux(A &&...)
    {
    }

    // ---- courant(local_courant, ...) -------------------------------------------------------------
    // (prm, kind, Q, aux, gf, dx, dt, t, direction); cmdg_courant refuses a law without HAS_COURANT
    static constexpr bool HAS_COURANT = false;
    template <class... A>
    __device__ static double courant(A &&...)
    {
        return 0.0;
    }

    // ---- AtmosLESDefault diagnostics (diagnostics.h; src/Diagnostics/thermo.jl:33-68) ------------
    // les_diagnostics(prm, D, Q, aux, gf, t) fills the NDIAG nodal columns of compute_thermo! and the
    // two sub-grid terms; LES_MOIST: the law carries the EquilMoist columns and sums;
    // les_diagnostics_active(prm): this parameter block is an LES configuration.  cmdg_les_* refuse a
    // law without HAS_LES_DIAGNOSTICS.
    static constexpr bool HAS_LES_DIAGNOSTICS = false, LES_MOIST = false;
    static constexpr int NDIAG = 0;
    template <class... A>
    __host__ __device__ static bool les_diagnostics_active(A &&...)
    {
        return true;
    }
    template <class... A>
    __device__ static void les_diagnostics(A &&...)
    {
    }

    // ---- AtmosGCMDefault diagnostics (src/Diagnostics/atmos_gcm_default.jl, diagnostic_fields.jl) ---
    // STATE_RHO_RHOU: the prognostic state begins rho, rho u[3], so that VectorGradients / Vorticity can
    // form u = rho u / rho (cmdg_vector_gradients refuses any other law).  HAS_GCM_DIAGNOSTICS:
    // gcm_thermo(prm, d, Q, aux) fills temp, pres, theta_dry, e_int, h_tot, h_int of compute_thermo!
    // (thermo.jl:33-44); cmdg_gcm_nodal refuses a law without it.
    static constexpr bool STATE_RHO_RHOU = false, HAS_GCM_DIAGNOSTICS = false;
    template <class... A>
    __device__ static void gcm_thermo(A &&...)
    {
    }

    // ---- first-order numerical flux --------------------------------------------------------------
    // A law may offer flux_first_order and wavespeed of one state in one call, flux_wavespeed(prm, F,
    // ws, n, Q, aux, t, direction): both need the same thermodynamic state, and the moist law's costs
    // a saturation adjustment.  The Rusanov flux then calls it instead of the pair.
    static constexpr bool HAS_FLUX_WAVESPEED = false;
    // The law carries numerical_flux_first_order! methods of its own (Roe, HLLC, ...):
    // numerical_flux_law(prm, nf, fluxn, n, QM, auxM, QP, auxP, t, direction) serves nf >= NF_ROE.
    static constexpr bool LAW_NF = false;

    // ---- layout and tuning -----------------------------------------------------------------------
    // The library keeps the law's state_gradient_flux node-major, (NGF, Np, nelem), like
    // Qhypervisc_grad (cmdg_common.h).  The dry atmosphere takes it (10 columns gathered on the plus
    // side of every face node; the moist law was measured and keeps the reference layout,
    // physics_moist.h); laws whose hooks work on the array in the reference layout do not.
    static constexpr bool GF_NODE_MAJOR = false;
    // Waves per SIMD the register allocator is to aim for in the gradient pass: light laws gain
    // residency with a budget of their own.  0: the library's CMDG_GRAD_MINW.
    static constexpr int GRAD_MIN_WAVES = 0;
    // gradient_argument and update_aux are pure functions of the node's (Q, aux) whose time argument
    // is unused: inside cmdg_lsrk_run the fused update may form both for the next stage (kernels.h
    // GradArgHandoff, which also asks for NGL > 0 and a fused refresh).
    static constexpr bool GRADARG_HANDOFF = false;
    // ... and the columns the refresh writes are read by none of the law's pointwise functions in any
    // pass: the hand-off launches of a run but the last then neither call update_aux nor store the
    // columns.  Every other law refreshes in every update.
    static constexpr bool GRADARG_REFRESH_UNREAD = false;
    // Byte accounting (cmdg_query): columns of Q / of the auxiliary state the volume code of a pass
    // reads.  pass: 0 gradients, 1 Laplacian, 2 gradient of Laplacian, 3 tendency.  Negative: every
    // column (NS / NAUX).
    __host__ __device__ static constexpr int state_read(int) { return -1; }
    __host__ __device__ static constexpr int aux_read(int) { return -1; }

    // ---- vertical finite volume (fv.h; src/BalanceLaws/prog_prim_conversion.jl) ------------------
    // prognostic_to_primitive / primitive_to_prognostic(prm, out, in, aux); default: the identity
    static constexpr bool HAS_PRIM_CONVERSION = false;
    // construct_face_auxiliary_state(prm, aux_face, aux_cell, dz); default: the copy
    static constexpr bool HAS_FACE_AUX_STATE = false;
    // HBFVReconstruction (src/Atmos/Model/reconstructions.jl): a law whose primitives name a density
    // and a pressure says which entries they are and defines prim_gravity(prm); PRIM_P < 0: the law
    // has no pressure primitive and cmdg_create_dgfv refuses the wrapper on it
    static constexpr int PRIM_RHO = -1, PRIM_P = -1;
    template <class... A>
    __host__ __device__ static double prim_gravity(A &&...)
    {
        return 0.0;
    }
};

// What the law says about its gradient flux, for the engine: a law without gradient-flux states never
// reads them, whatever else it says.
template <class P>
inline constexpr GradFlux gradflux_of = P::NGF > 0 ? P::GRADFLUX : GradFlux::never;
// ... and the answer for one parameter block: the one place that calls P::needs_gradflux
template <class P>
__host__ __device__ inline bool needs_gradflux(const typename P::Params &prm)
{
    static_assert(P::NGF > 0 || P::GRADFLUX != GradFlux::always,
                  "a law with no gradient-flux states (NGF == 0) cannot always read them");
    if constexpr (gradflux_of<P> == GradFlux::ask)
        return P::needs_gradflux(prm);
    else
        return gradflux_of<P> == GradFlux::always;
}

}  // namespace cmdg
