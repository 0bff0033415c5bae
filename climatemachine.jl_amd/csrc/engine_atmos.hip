// Engine instantiations for the dry atmosphere law (physics_atmos.h).
#include "engine.h"
#include "laws.h"
#include "physics_atmos.h"
#include "with_constant.h"

namespace cmdg {

int counts_atmos(const int32_t *ip, int32_t out[6])
{
    const bool orient = ip[0] != 0, ref = ip[1] != 0, hyp = ip[4] != 0, smag = ip[14] == 1;
    const int nt = atmos_ntracers(ip);  // NTracers: rho chi, chi, grad chi (3 each), delta_chi
    if (nt > ATMOS_MAX_TRACERS) return CMDG_ERR_UNSUPPORTED;
    out[0] = 5 + nt;
    out[1] = 3 + (orient ? 4 : 0) + (ref ? 7 : 0) + (smag ? 1 : 0) + (hyp ? 1 : 0) + 2 + nt;
    out[2] = 4 + (smag ? 1 : 0) + (hyp ? 4 : 0) + nt;
    out[3] = 9 + (smag ? 1 : 0) + 3 * nt;
    out[4] = hyp ? 4 : 0;
    out[5] = hyp ? 12 : 0;
    return CMDG_OK;
}

// what make_params derives from the parameter block (the same for every variant of the functor)
int host_constants_atmos(const int32_t *ip, const double *dp, double out[7])
{
    static_assert(ATMOS_NHOSTCONST == 7, "cmdg_atmos_host_constants documents seven");
    using P = DryAtmos<false, false, false>;
    P::Params prm;
    P::make_params(prm, ip, dp);
    P::host_constants(prm, out);
    return CMDG_OK;
}

template <int NQ>
static EngineBase *pick(const cmdg_desc *d, std::string &err)
{
    const bool orient = d->iparam[0] != 0, ref = d->iparam[1] != 0, hyp = d->iparam[4] != 0;
    bool mms = (d->iparam[5] & 8) != 0;
    for (int i = 0; i < d->iparam[6] && i < 7; ++i) mms = mms || d->iparam[7 + i] == 2;
    if (mms && (orient || ref || hyp || d->iparam[14] != 0)) {
        err = "DryAtmos: MMSSource / InitStateBC are compiled for NoOrientation, NoReferenceState, "
              "constant viscosity only";
        return nullptr;
    }
    if (d->nf_first >= NF_ROE) {  // the law's own Roe / HLLC methods
        if constexpr (NQ == 5) {
            if (!orient && !ref && !hyp && d->iparam[14] == 0 && !mms)
                return make_engine<DryAtmos<false, false, false, false, true>, NQ>(d);
            if (orient && ref && !hyp && d->iparam[14] == 0)
                return make_engine<DryAtmos<true, true, false, false, true>, NQ>(d);
        }
        err = "DryAtmos: Roe / HLLC / LMARS numerical fluxes are compiled for N = 4, constant "
              "viscosity, without orientation and reference state or with both";
        return nullptr;
    }
    if (d->iparam[14] == 1) {  // SmagorinskyLilly (AtmosLES configurations)
        if (orient && ref && !hyp) return make_engine<DryAtmos<true, true, false, true>, NQ>(d);
        err = "DryAtmos: SmagorinskyLilly is compiled with orientation + reference state, no hyperdiffusion";
        return nullptr;
    }
    if (d->iparam[14] != 0) {
        err = "DryAtmos: unknown turbulence closure";
        return nullptr;
    }
    if (!orient && !ref && !hyp) return make_engine<DryAtmos<false, false, false>, NQ>(d);
    if (!orient && ref) {
        // a reference state that is carried, not subtracted (the reference subtracts for
        // HydrostaticState alone, tendencies_momentum.jl): the isentropic vortex's, for its linear model
        if constexpr (NQ == 5) {
            if (!hyp && d->iparam[2] == 0) return make_engine<DryAtmos<false, true, false>, NQ>(d);
        }
        err = "DryAtmos: a reference state without an orientation is compiled for N = 4, not subtracted "
              "(subtract_off = false), without hyperdiffusion";
        return nullptr;
    }
    // Held-Suarez: shared reciprocals (XQ) at N = 4, where every kernel keeps its register class
    if (orient && ref && hyp) return make_engine<DryAtmos<true, true, true, false, false, 0, NQ == 5>, NQ>(d);
    if (orient && ref && !hyp) return make_engine<DryAtmos<true, true, false>, NQ>(d);
    if (orient && !ref && !hyp) return make_engine<DryAtmos<true, false, false>, NQ>(d);
    err = "DryAtmos: this orientation/ref-state/hyperdiffusion combination is not compiled in";
    return nullptr;
}

// a descriptor with tracers never reaches the five-state engines of pick: the units of their own
// (engine_atmos_tracers<NT>.hip) serve it or nobody here does
static EngineBase *pick_tracers(const cmdg_desc *d, int nt, std::string &err)
{
    bool mms = (d->iparam[5] & 8) != 0;
    for (int i = 0; i < d->iparam[6] && i < 7; ++i) mms = mms || d->iparam[7 + i] == 2;
    if (nt > ATMOS_MAX_TRACERS) {
        err = "DryAtmos: at most 8 tracers";
        return nullptr;
    }
    if (mms) {
        err = "DryAtmos: MMSSource / InitStateBC are not defined for a model with tracers";
        return nullptr;
    }
    if (d->nf_first >= NF_ROE) {
        err = "DryAtmos: the Roe / HLLC / LMARS numerical fluxes have no tracer methods (tracers need Rusanov or "
              "the central flux)";
        return nullptr;
    }
    if (d->iparam[14] != 0 && d->iparam[14] != 1) {
        err = "DryAtmos: unknown turbulence closure";
        return nullptr;
    }
    if (nt == 1) return make_engine_atmos_tracers1(d, err);
    if (nt == 2) return make_engine_atmos_tracers2(d, err);
    err = "DryAtmos: 1 or 2 tracers are compiled in (more: plugins.build_dry_atmos(ntracers=...))";
    return nullptr;
}

EngineBase *make_engine_atmos(const cmdg_desc *d, std::string &err)
{
    if (const int nt = atmos_ntracers(d->iparam)) return pick_tracers(d, nt, err);
    if (d->iparam[4] != 0 && d->iparam[0] == 0) {
        err = "DryAtmos: hyperdiffusion needs an orientation";
        return nullptr;
    }
    // element-per-workgroup kernels: one element's working set lives in LDS (N = 6 with
    // hyperdiffusion: 90 KB of the CU's 160 KB)
    EngineBase *e = nullptr;
    if (!with_constant<2, 6>(d->N[0], [&](auto n) { e = pick<n() + 1>(d, err); }))
        err = "DryAtmos: polynomial order not compiled in (have N = 2..6)";
    return e;
}

}  // namespace cmdg
