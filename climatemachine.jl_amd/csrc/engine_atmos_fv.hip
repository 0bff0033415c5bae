// DGFVModel engine instantiations for the dry atmosphere law (physics_atmos.h, engine_fv.h): the two
// combinations the reference runs a DGFVModel on (test/Numerics/DGMethods/Euler/
// fvm_isentropicvortex.jl, fvm_balance.jl; experiments/TestCase/*_fvm.jl), with the law's own
// numerical fluxes compiled in.
#include "engine_fv.h"
#include "laws.h"
#include "physics_atmos.h"

namespace cmdg {

EngineBase *make_engine_atmos_fv(const cmdg_desc *d, const cmdg_fv_desc *fv, std::string &err)
{
    static const char *const have = "DGFVModel DryAtmos: compiled in are N_h = 4, constant viscosity, no "
                                    "hyperdiffusion, without orientation and reference state or with both";
    const bool orient = d->iparam[0] != 0, ref = d->iparam[1] != 0, hyp = d->iparam[4] != 0;
    bool mms = (d->iparam[5] & 8) != 0;
    for (int i = 0; i < d->iparam[6] && i < 7; ++i) mms = mms || d->iparam[7 + i] == 2;
    if (atmos_ntracers(d->iparam) != 0) {
        err = std::string("DGFVModel DryAtmos: a model with tracers is not compiled in (the primitive conversion "
                          "carries rho, u, p); ") + have;
        return nullptr;
    }
    if (hyp) {
        err = std::string("DGFVModel: a law with hyperdiffusive states is not supported (DGFVModel.jl:91); ") + have;
        return nullptr;
    }
    if (d->iparam[14] != 0) {
        err = std::string("DGFVModel DryAtmos: SmagorinskyLilly is not compiled in; ") + have;
        return nullptr;
    }
    if (d->N[0] != 4) {
        err = std::string("DGFVModel DryAtmos: this horizontal polynomial order is not compiled in; ") + have;
        return nullptr;
    }
    if (!mms && !orient && !ref) return make_engine_fv<DryAtmos<false, false, false, false, true>, 5>(d, fv);
    if (!mms && orient && ref) return make_engine_fv<DryAtmos<true, true, false, false, true>, 5>(d, fv);
    err = std::string("DGFVModel DryAtmos: this orientation / reference state combination is not compiled in; ") + have;
    return nullptr;
}

}  // namespace cmdg
