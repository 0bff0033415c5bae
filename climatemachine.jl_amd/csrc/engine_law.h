// The law layer of the engine: EngineLaw<P, NQ, NQV> holds the parameter block of one balance law and
// answers for it whatever needs no pass kernel -- the nodal launches (kernels_nodal.h), the
// introspection of cmdg_query, the arguments and the profiling bracket of a pass.  It instantiates no
// DG pass kernel: an engine class on top of it names the ones its handles can launch (EngineT of
// engine.h all four passes, EngineFV of engine_fv.h the horizontal gradient and tendency kernels,
// EngineESDG of engine_esdg.hip none), and a pass a class cannot reach fails the evaluation.
#pragma once
#include <stdio.h>

#include "engine_base.h"
#include "kernels_nodal.h"

namespace cmdg {

template <class P>
using PassKernel = void (*)(PassArgs<P>);

template <class P, int NQ_, int NQV_ = NQ_>
struct EngineLaw : EngineBase {
    typename P::Params prm;
    // The hand-off as the engine sees it: the law and order have it (GradArgHandoff) and the law may run
    // without its gradient flux (handoff_eligible) -- one that always reads it never hands anything on.
    // The refresh can be elided only where there is a hand-off.
    static constexpr bool HO = GradArgHandoff<P, NQ_, NQV_>::value && gradflux_of<P> != GradFlux::always;
    static constexpr bool ELIDE = HO && GradArgHandoff<P, NQ_, NQV_>::elide_refresh;
    // what every factory copies from the law (an ESDG handle then counts its reference columns in)
    void init_law(const cmdg_desc *d)
    {
        NQ = NQ_;
        NQV = NQV_;
        ns = P::NS;
        naux = P::NAUX;
        ngrad = P::NGRAD;
        ngf = P::NGF;
        ngl = P::NGL;
        nhyp = P::NHYP;
        P::make_params(prm, d->iparam, d->dparam);
    }
    // send0 / send1: the send buffers of what an exterior launch produces (halo_dev)
    PassArgs<P> make_args(const RhsCtx &c, const int64_t *elems, int64_t n, int dir, bool exterior, double *send0,
                          double *send1) const
    {
        PassArgs<P> a;
        a.prm = prm;
        a.g = g;
        a.elems = elems;
        a.nelems = n;
        a.Q = c.Qin;
        a.aux = aux;
        a.aux_rw = aux;
        a.derived = derived;
        a.gf = gf;
        a.hypgrad = hypgrad;
        a.hypdiv = hypdiv;
        a.tendency = c.tendency;
        a.Qout = c.Qout;
        a.garg = garg;
        a.lapr = lapr;
        a.hypdiv_out = c.hypdiv_out;
        a.t = c.t;
        a.tptr = c.tptr;
        a.alpha = c.alpha;
        a.beta = c.beta;
        a.rkb_dt = c.rkb_dt;
        a.rka_next = c.rka_next;
        a.direction = dir;
        a.model_dir = direction;
        a.nf_first = nf_first;
        a.h = halo_dev(exterior, send0, send1);
        return a;
    }
    using Kernel = PassKernel<P>;
    struct Pass {
        const char *range, *range_ext;  // roctx range of the interior / exterior launch
        int prof, prof_ext;             // ... and its profiling id
    };
    static constexpr Pass GRADIENTS{"cmdg:gradients", "cmdg:gradients:exterior", CMDG_K_GRADIENTS, CMDG_K_GRADIENTS_EXT};
    static constexpr Pass DIVGRAD{"cmdg:divgrad", "cmdg:divgrad:exterior", CMDG_K_DIVGRAD, CMDG_K_DIVGRAD_EXT};
    static constexpr Pass GRADLAP{"cmdg:gradlap", "cmdg:gradlap:exterior", CMDG_K_GRADLAP, CMDG_K_GRADLAP_EXT};
    static constexpr Pass TENDENCY{"cmdg:tendency", "cmdg:tendency:exterior", CMDG_K_TENDENCY, CMDG_K_TENDENCY_EXT};
    // What every launch of a pass shares: nothing for an empty element list, else the roctx range and
    // the profiling bracket of the interior or exterior launch around what `enqueue` puts on st.
    template <class Enqueue>
    int in_pass(const Pass &p, int64_t n, bool exterior, hipStream_t st, Enqueue enqueue)
    {
        if (n <= 0) return CMDG_OK;
        Range range_(exterior ? p.range_ext : p.range);
        prof_begin(exterior ? p.prof_ext : p.prof, st);
        const int r = enqueue();
        prof_end(st);
        return r;
    }
    // The kernel a picker names for the flags of a launch goes on the stream.  A combination it does
    // not name (null) fails the evaluation and launches nothing: `flags` says what was asked for.
    template <class... A>
    int launch_picked(Kernel k, unsigned blocks, unsigned threads, hipStream_t st, const PassArgs<P> &args,
                      const char *pass, const char *flags, A... values)
    {
        if (!k) {
            char what[160];
            snprintf(what, sizeof what, flags, values...);
            return fail(CMDG_ERR_UNSUPPORTED, std::string("the ") + pass + " pass has no kernel of this law for " +
                                                  what + ": the engine class does not instantiate it");
        }
        hipLaunchKernelGGL(k, dim3(blocks), dim3(threads), 0, st, args);
        return CMDG_OK;
    }
    // a pass no handle of the engine class can reach
    int no_pass(const char *pass, const char *model)
    {
        return fail(CMDG_ERR_UNSUPPORTED, std::string("the ") + pass + " pass is not compiled for " + model + " handles");
    }
    void launch_update_aux(const RhsCtx &c, int64_t e0, int64_t e1) override
    {
        if constexpr (P::HAS_UPDATE_AUX) {
            if (e1 <= e0 || !P::update_aux_active(prm)) return;
            const int64_t n = (e1 - e0) * KDims<NQ_, NQV_>::Np;
            prof_begin(CMDG_K_UPDATE_AUX, s_comp);
            hipLaunchKernelGGL((k_update_aux<P, NQ_, NQV_>), dim3((unsigned)((n + 255) / 256)), dim3(256),
                               0, s_comp, prm, c.Qin, aux, d_activedofs, c.t, e0, e1);
            prof_end(s_comp);
        }
    }
    int launch_courant(int mode, int kind, const double *Q, double dt, double t, int dir,
                       double *out_elem) override
    {
        constexpr int NT = KDims<NQ_, NQV_>::Np <= 128 ? 128 : 256;
        if (mode == 1 && !P::HAS_COURANT)
            return fail(CMDG_ERR_UNSUPPORTED, "this balance law defines no local Courant number");
        if (mode == 0)
            hipLaunchKernelGGL((k_courant<P, NQ_, NQV_, 0>), dim3((unsigned)nreal), dim3(NT), 0, s_comp, prm,
                               g.vgeo, g.nvgeo, Q, aux, gf, kind, dt, t, dir, out_elem);
        else
            hipLaunchKernelGGL((k_courant<P, NQ_, NQV_, 1>), dim3((unsigned)nreal), dim3(NT), 0, s_comp, prm,
                               g.vgeo, g.nvgeo, Q, aux, gf, kind, dt, t, dir, out_elem);
        return CMDG_OK;
    }
    int launch_les_nodal(const double *Q, double t, double *D, int *ndiag, int *moist) override
    {
        if constexpr (P::HAS_LES_DIAGNOSTICS) {
            if (!P::les_diagnostics_active(prm))
                return fail(CMDG_ERR_UNSUPPORTED, "AtmosLESDefault diagnostics: this configuration of the law is "
                                                  "not an LES one (flat orientation)");
            *ndiag = P::NDIAG;
            *moist = P::LES_MOIST;
            if (!D) return CMDG_OK;
            const int64_t n = nreal * KDims<NQ_, NQV_>::Np;
            if (n <= 0) return CMDG_OK;
            hipLaunchKernelGGL((k_les_nodal<P, NQ_, NQV_>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s_comp,
                               prm, Q, aux, gf, (int)(gf_live() && gf != nullptr), t, nreal, D);
            return CMDG_OK;
        } else {
            return fail(CMDG_ERR_UNSUPPORTED, "AtmosLESDefault diagnostics: this balance law defines no LES "
                                              "diagnostics (the dry and the moist atmosphere laws do)");
        }
    }
    int launch_vector_gradients(const double *Q, double *vgrad) override
    {
        if constexpr (P::STATE_RHO_RHOU && NQV_ >= 2) {
            if (nreal > 0)
                hipLaunchKernelGGL((k_vector_gradients<NQ_, NQV_>), dim3((unsigned)nreal), dim3(KDims<NQ_, NQV_>::Np),
                                   0, s_comp, Q, P::NS, g.vgeo, g.nvgeo, g.D, g.Dv, vgrad);
            return CMDG_OK;
        } else {
            return fail(CMDG_ERR_UNSUPPORTED, "VectorGradients: the state of this balance law does not begin rho, "
                                              "rho u[3] (the dry and the moist atmosphere laws' do)");
        }
    }
    int launch_gcm_nodal(const double *Q, double, double *G, double *u) override
    {
        if constexpr (P::HAS_GCM_DIAGNOSTICS && NQV_ >= 2) {
            if (nreal > 0)
                hipLaunchKernelGGL((k_gcm_nodal<P, NQ_, NQV_>), dim3((unsigned)nreal), dim3(KDims<NQ_, NQV_>::Np), 0,
                                   s_comp, prm, Q, aux, g.vgeo, g.nvgeo, g.D, g.Dv, G, u);
            return CMDG_OK;
        } else if constexpr (P::LES_MOIST) {
            return fail(CMDG_ERR_UNSUPPORTED, "AtmosGCMDefault diagnostics: the moist columns are not built (the "
                                              "moist law here is the flat LES configuration, and the group "
                                              "requires a cubed sphere)");
        } else {
            return fail(CMDG_ERR_UNSUPPORTED, "AtmosGCMDefault diagnostics: this balance law defines no GCM "
                                              "diagnostics (the dry atmosphere law with an orientation does)");
        }
    }
    bool has_update_aux() const override { return P::HAS_UPDATE_AUX && P::update_aux_active(prm); }
    bool law_needs_gradflux() const override { return needs_gradflux<P>(prm); }
    bool gf_node_major() const override { return cmdg::gf_node_major<P>; }
    bool fused_update_aux() const override { return P::HAS_UPDATE_AUX && P::FUSE_UPDATE_AUX; }
    bool garg_capable() const override { return HO && !needs_gradflux<P>(prm); }
    bool refresh_elidable() const override { return ELIDE; }
    int law_nder() const override { return P::HAS_SOURCE ? P::NDER : 0; }
    int law_nupd() const override { return P::HAS_UPDATE_AUX ? P::NUPD : 0; }
    int tendency_epb() const override { return TendencyShape<P, NQ_, NQV_>::EPB; }
    // (a law that does not count them reads every column, law_defaults.h)
    int law_state_read(int pass) const override { return P::state_read(pass) < 0 ? P::NS : P::state_read(pass); }
    int law_aux_read(int pass) const override { return P::aux_read(pass) < 0 ? P::NAUX : P::aux_read(pass); }
    int init_derived() override
    {
        if constexpr (P::NDER > 0) {
            const int64_t n = nelem * KDims<NQ_, NQV_>::Np;
            if (derived.alloc((size_t)n * P::NDER) != hipSuccess)
                return fail(CMDG_ERR_HIP, "hipMalloc(derived) failed");
            hipLaunchKernelGGL((k_init_derived<P, NQ_, NQV_>), dim3((unsigned)((n + 255) / 256)), dim3(256),
                               0, s_comp, prm, aux, derived, nelem);
            if (hipStreamSynchronize(s_comp) != hipSuccess)
                return fail(CMDG_ERR_HIP, "k_init_derived failed");
        }
        return CMDG_OK;
    }
};

}  // namespace cmdg
