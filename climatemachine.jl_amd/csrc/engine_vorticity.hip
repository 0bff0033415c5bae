// Engine instantiations for the VorticityModel of the AtmosGCMDefault diagnostics (physics_vorticity.h):
// the orders of the dry atmosphere law whose velocity it differentiates, one order in every direction.
#include "engine.h"
#include "laws.h"
#include "physics_vorticity.h"
#include "with_constant.h"

namespace cmdg {

int counts_vorticity(const int32_t *, int32_t out[6])
{
    out[0] = VorticityLaw::NS;
    out[1] = VorticityLaw::NAUX;
    out[2] = out[3] = out[4] = out[5] = 0;
    return CMDG_OK;
}

EngineBase *make_engine_vorticity(const cmdg_desc *d, std::string &err)
{
    EngineBase *e = nullptr;
    if (d->N[2] != d->N[0] || !with_constant<2, 6>(d->N[0], [&](auto n) { e = make_engine<VorticityLaw, n() + 1>(d); }))
        err = "VorticityModel: polynomial order not compiled in (have N = 2..6, one order in every direction)";
    return e;
}

}  // namespace cmdg
