// The template layer of the engine: EngineT<P, NQ, NQV> launches the pass kernels (kernels.h) of one
// balance law at one polynomial order for the host engine of engine_base.h.  The engine_*.hip units
// and the generated plug-ins (plugins.py) include this header; everything else includes engine_base.h.
#pragma once
#include "engine_base.h"
#include "kernels.h"

namespace cmdg {

// ---------------------------------------------------------------------------------
template <class P, int NQ_, int NQV_ = NQ_>
struct EngineT : EngineBase {
    typename P::Params prm;
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
    // ---- the four passes ---------------------------------------------------------------------
    using Kernel = void (*)(PassArgs<P>);
    static constexpr bool HO = GradArgHandoff<P, NQ_, NQV_>::value;
    static constexpr bool ELIDE = GradArgHandoff<P, NQ_, NQV_>::elide_refresh;
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
    void in_pass(const Pass &p, int64_t n, bool exterior, hipStream_t st, Enqueue enqueue)
    {
        if (n <= 0) return;
        Range range_(exterior ? p.range_ext : p.range);
        prof_begin(exterior ? p.prof_ext : p.prof, st);
        enqueue();
        prof_end(st);
    }
    // The instantiation of a pass kernel for the flags of a launch.  A combination the law does not
    // instantiate (GradArgHandoff) is not named for it; the flags never ask for one (handoff_eligible).
    static Kernel pick_gradients(bool gf_live, bool garg_in)
    {
        if constexpr (HO)  // (handoff_eligible: no gradient flux, no ghosts)
            if (garg_in) return k_gradients<P, NQ_, NQV_, false, true>;
        return gf_live ? k_gradients<P, NQ_, NQV_, true> : k_gradients<P, NQ_, NQV_, false>;
    }
    template <bool LSRK, bool GF>
    static Kernel tendency_recv(bool recv)
    {
        return recv ? k_tendency<P, NQ_, NQV_, LSRK, GF, true> : k_tendency<P, NQ_, NQV_, LSRK, GF, false>;
    }
    static Kernel pick_tendency(bool lsrk, bool gf, bool recv, GargOut out)
    {
        if constexpr (HO)  // (handoff_eligible: fused update, no gradient flux, no ghosts)
            if (out != GargOut::none) {
                if constexpr (ELIDE)
                    if (out == GargOut::records) return k_tendency<P, NQ_, NQV_, true, false, false, true, false>;
                return k_tendency<P, NQ_, NQV_, true, false, false, true>;
            }
        if (lsrk) return gf ? tendency_recv<true, true>(recv) : tendency_recv<true, false>(recv);
        return gf ? tendency_recv<false, true>(recv) : tendency_recv<false, false>(recv);
    }
    // The Laplacian and gradient-of-Laplacian passes of an evaluation that reads the records (c.garg_in)
    // hand the Laplacians on as ring-ordered records (cmdg_common.h ring_slot); the second gathers
    // them through facePr.
    // fused (RhsCtx::lap_fused): the launch does the work of the gradient pass as well, which is then
    // not launched (k_lapfused).
    static Kernel pick_divgrad(bool ring, bool fused)
    {
        if constexpr (HO) {
            if (ring && fused) return k_lapfused<P, NQ_, NQV_>;
            if (ring) return k_divgrad<P, NQ_, NQV_, true>;
        }
        return k_divgrad<P, NQ_, NQV_>;
    }
    static Kernel pick_gradlap(bool ring)
    {
        if constexpr (HO)
            if (ring) return k_gradlap<P, NQ_, NQV_, true>;
        return k_gradlap<P, NQ_, NQV_>;
    }
    void launch_gradients(const RhsCtx &c, const int64_t *elems, int64_t n, bool exterior, hipStream_t st) override
    {
        if (c.lap_fused) return;  // (formed inside the Laplacian launch)
        in_pass(GRADIENTS, n, exterior, st, [&] {
            const PassArgs<P> args = make_args(c, elems, n, diffusion_direction, exterior,
                                               gf_live() ? slot[SLOT_GF].sendbuf : nullptr,
                                               ngl > 0 ? slot[SLOT_HG].sendbuf : nullptr);
            hipLaunchKernelGGL(pick_gradients(gf_live(), c.garg_in), dim3((unsigned)n), dim3(KDims<NQ_, NQV_>::NT), 0,
                               st, args);
        });
    }
    void launch_divgrad(const RhsCtx &c, const int64_t *elems, int64_t n, bool exterior, hipStream_t st) override
    {
        in_pass(DIVGRAD, n, exterior, st, [&] {
            PassArgs<P> args = make_args(c, elems, n, diffusion_direction, exterior, slot[SLOT_HD].sendbuf, nullptr);
            const bool fused = HO && c.garg_in && c.lap_fused;
            if (fused) {  // (the tables of k_lapfused travel in two arguments the pass does not read)
                args.g.facePr = d_lapI;
                args.derived = d_lapT;
            }
            hipLaunchKernelGGL(pick_divgrad(c.garg_in, fused), dim3((unsigned)n), dim3(KDims<NQ_, NQV_>::NT), 0, st, args);
        });
    }
    void launch_gradlap(const RhsCtx &c, const int64_t *elems, int64_t n, bool exterior, hipStream_t st) override
    {
        in_pass(GRADLAP, n, exterior, st, [&] {
            PassArgs<P> args = make_args(c, elems, n, diffusion_direction, exterior, slot[SLOT_HG].sendbuf, nullptr);
            if (c.garg_in) args.g.faceP = g.facePr;
            hipLaunchKernelGGL(pick_gradlap(c.garg_in), dim3((unsigned)n), dim3(KDims<NQ_, NQV_>::NT), 0, st, args);
        });
    }
    void launch_tendency(const RhsCtx &c, const int64_t *elems, int64_t n, bool exterior, hipStream_t st) override
    {
        in_pass(TENDENCY, n, exterior, st, [&] {
            using SH = TendencyShape<P, NQ_, NQV_>;
            PassArgs<P> args = make_args(c, elems, n, direction, exterior, c.lsrk ? slot[SLOT_Q].sendbuf : nullptr, nullptr);
            const bool recv = args.h.ghostslot != nullptr && exterior;  // (interior elements have no ghost neighbour)
            if (!recv) args.h.ghostslot = nullptr;
            hipLaunchKernelGGL(pick_tendency(c.lsrk, P::needs_gradflux(prm), recv, c.garg_out),
                               dim3((unsigned)SH::blocks(n)), dim3(SH::NT), 0, st, args);
        });
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
    bool law_needs_gradflux() const override { return P::needs_gradflux(prm); }
    bool gf_node_major() const override { return cmdg::gf_node_major<P>; }
    bool fused_update_aux() const override { return P::HAS_UPDATE_AUX && P::FUSE_UPDATE_AUX; }
    bool garg_capable() const override { return HO && !P::needs_gradflux(prm); }
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

template <class P, int NQ_, int NQV_ = NQ_>
EngineBase *make_engine(const cmdg_desc *d)
{
    auto *e = new EngineT<P, NQ_, NQV_>();
    e->NQ = NQ_;
    e->NQV = NQV_;
    e->ns = P::NS;
    e->naux = P::NAUX;
    e->ngrad = P::NGRAD;
    e->ngf = P::NGF;
    e->ngl = P::NGL;
    e->nhyp = P::NHYP;
    P::make_params(e->prm, d->iparam, d->dparam);
    return e;
}

// The laws compiled in are the rows of one table (create.hip LAWS), their factories are declared in
// laws.h and defined per physics family in the engine_*.hip units.

}  // namespace cmdg
