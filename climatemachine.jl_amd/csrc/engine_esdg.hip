// Engine of an ESDGModel handle (cmdg_create_esdg) and its instantiations for the dry atmosphere of
// the entropy-stable tests (physics_esdg_dryatmos.h).  The orchestration is EngineBase::rhs_segment
// unchanged: the law has no gradient, gradient-flux or hyperdiffusive states, so an evaluation is
// one exchange of Q with the interior element list launched before the ghosts arrive and the
// exterior list after -- (esdg::ESDGModel)(tendency, Q, _, t, alpha, beta), ESDGModel.jl:110-316,
// whose volume launches read no ghost and commute with the end of the exchange.  The tendency of
// either list is the one launch of esdg.h, so the class sits on the law layer and compiles no DG pass
// kernel: the three passes an ESDGModel evaluation never reaches fail.
#include "engine_law.h"
#include "laws.h"
#include "esdg.h"

namespace cmdg {

template <class P, int NQ_>
struct EngineESDG : EngineLaw<P, NQ_, NQ_> {
    using Base = EngineLaw<P, NQ_, NQ_>;
    using Kernel = void (*)(EsdgArgs<P>);
    cmdg_esdg_desc ed{};

    template <int VF>
    static Kernel pick_surface(int sf)
    {
        switch (sf) {
        case ESDG_NONE: return k_esdg_tendency<P, NQ_, VF, ESDG_NONE>;
        case ESDG_EC: return k_esdg_tendency<P, NQ_, VF, ESDG_EC>;
        case ESDG_RUSANOV: return k_esdg_tendency<P, NQ_, VF, ESDG_RUSANOV>;
        case ESDG_EC_PENALTY: return k_esdg_tendency<P, NQ_, VF, ESDG_EC_PENALTY>;
        default: return k_esdg_tendency<P, NQ_, VF, ESDG_MATRIX>;
        }
    }
    Kernel pick() const
    {
        switch (ed.volume_flux) {
        case ESDG_NONE: return pick_surface<ESDG_NONE>(ed.surface_flux);
        case ESDG_EC: return pick_surface<ESDG_EC>(ed.surface_flux);
        case ESDG_CENTRAL: return pick_surface<ESDG_CENTRAL>(ed.surface_flux);
        default: return pick_surface<ESDG_KG>(ed.surface_flux);
        }
    }
    int launch_gradients(const RhsCtx &, const int64_t *, int64_t, bool, hipStream_t) override
    {
        return this->no_pass("gradient", "ESDGModel");
    }
    int launch_divgrad(const RhsCtx &, const int64_t *, int64_t, bool, hipStream_t) override
    {
        return this->no_pass("Laplacian", "ESDGModel");
    }
    int launch_gradlap(const RhsCtx &, const int64_t *, int64_t, bool, hipStream_t) override
    {
        return this->no_pass("gradient-of-Laplacian", "ESDGModel");
    }
    int launch_tendency(const RhsCtx &c, const int64_t *elems, int64_t n, bool exterior, hipStream_t st) override
    {
        if (n <= 0) return CMDG_OK;
        Range range_(exterior ? "cmdg:esdg_tendency:exterior" : "cmdg:esdg_tendency");
        this->prof_begin(CMDG_K_ESDG_TENDENCY, st);
        EsdgArgs<P> a;
        a.prm = this->prm;
        a.g = this->g;
        a.elems = elems;
        a.nelems = n;
        a.Q = c.Qin;
        a.aux = this->aux;
        a.naux = this->naux;
        a.tendency = c.tendency;
        a.t = c.t;
        a.alpha = c.alpha;
        a.beta = c.beta;
        hipLaunchKernelGGL(pick(), dim3((unsigned)n), dim3(KDims<NQ_, NQ_>::NT), 0, st, a);
        this->prof_end(st);
        return CMDG_OK;
    }
    // advective_courant / nondiffusive_courant of the law (DryAtmos.jl:758-793); the minimum node
    // distance (mode 0) is the grid's
    template <class PA>
    void launch_courant_t(int kind, const double *Q, double dt, double t, int dir, double *out_elem)
    {
        constexpr int NT = KDims<NQ_, NQ_>::Np <= 128 ? 128 : 256;
        hipLaunchKernelGGL((k_courant<PA, NQ_, NQ_, 1>), dim3((unsigned)this->nreal), dim3(NT), 0, this->s_comp,
                           this->prm, this->g.vgeo, this->g.nvgeo, Q, this->aux, this->gf, kind, dt, t, dir, out_elem);
    }
    int launch_courant(int mode, int kind, const double *Q, double dt, double t, int dir, double *out_elem) override
    {
        if (mode == 0) return Base::launch_courant(mode, kind, Q, dt, t, dir, out_elem);
        if (kind != CMDG_ADVECTIVE_COURANT && kind != CMDG_NONDIFFUSIVE_COURANT)
            return this->fail(CMDG_ERR_UNSUPPORTED, "courant: the DryAtmosModel of the entropy-stable discretisation "
                                                    "defines the advective and the nondiffusive Courant number only");
        if (this->naux == EsdgDryAtmosRef::NAUX)
            launch_courant_t<EsdgDryAtmosRef>(kind, Q, dt, t, dir, out_elem);
        else
            launch_courant_t<P>(kind, Q, dt, t, dir, out_elem);
        return CMDG_OK;
    }
    int launch_entropy(const double *Q, double *beta, double *eta) override
    {
        constexpr int Np = KDims<NQ_, NQ_>::Np;
        const int64_t n = this->nreal * Np;
        if (n > 0)
            hipLaunchKernelGGL((k_esdg_entropy<P, Np>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, this->s_comp,
                               this->prm, Q, this->aux, this->naux, beta, eta, this->nreal);
        return this->launch_status("k_esdg_entropy");
    }
};

template <class P, int NQ_>
static EngineBase *make_engine_esdg_t(const cmdg_desc *d, const cmdg_esdg_desc *ed)
{
    static_assert(P::NGRAD == 0 && P::NGF == 0 && P::NGL == 0 && P::NHYP == 0, "an ESDGModel has one pass");
    auto *e = new EngineESDG<P, NQ_>();
    e->init_law(d);
    e->naux += d->iparam[1] != 0 ? 4 : 0;
    e->esdg = true;
    e->ed = *ed;
    e->prm.Mcut = ed->Mcut;
    e->prm.low_mach = ed->low_mach != 0;
    e->prm.kep = ed->kinetic_energy_preserving != 0;
    return e;
}

int counts_esdg_dryatmos(const int32_t *ip, int32_t out[6])
{
    out[0] = 5;
    out[1] = 4 + (ip[1] != 0 ? 4 : 0);
    out[2] = out[3] = out[4] = out[5] = 0;
    return CMDG_OK;
}

EngineBase *make_engine_esdg(const cmdg_desc *d, const cmdg_esdg_desc *ed, std::string &err)
{
    switch (d->N[0]) {
    case 3: return make_engine_esdg_t<EsdgDryAtmos, 4>(d, ed);
    case 4: return make_engine_esdg_t<EsdgDryAtmos, 5>(d, ed);
    default:
        err = "cmdg_create_esdg: the flux-differencing kernel is compiled for polynomial orders 3 and 4";
        return nullptr;
    }
}

}  // namespace cmdg
