// Engine instantiations of the dry atmosphere law with NTracers (physics_atmos.h, NT > 0): the body of
// the engine_atmos_tracers<NT>.hip units, one per tracer count so that engine_atmos.o stays what it is.
// N = 4: no orientation and no reference state, orientation + reference state without and with
// DryBiharmonic, and SmagorinskyLilly; N = 5 (NT = 1 only): orientation + reference state, the
// acoustic wave.  Every other combination is a plug-in's (plugins.build_dry_atmos(ntracers=...)).
#pragma once
#include "engine.h"
#include "laws.h"
#include "physics_atmos.h"

namespace cmdg {

template <int NT, bool N5>
static EngineBase *pick_atmos_tracers(const cmdg_desc *d, std::string &err)
{
    const bool orient = d->iparam[0] != 0, ref = d->iparam[1] != 0, hyp = d->iparam[4] != 0;
    const bool smag = d->iparam[14] == 1;
    if (d->N[0] == 4) {
        if (smag) {
            if (orient && ref && !hyp) return make_engine<DryAtmos<true, true, false, true, false, NT>, 5>(d);
        } else {
            if (!orient && !ref && !hyp) return make_engine<DryAtmos<false, false, false, false, false, NT>, 5>(d);
            if (orient && ref && !hyp) return make_engine<DryAtmos<true, true, false, false, false, NT>, 5>(d);
            if (orient && ref && hyp) return make_engine<DryAtmos<true, true, true, false, false, NT>, 5>(d);
        }
    }
    if constexpr (N5) {
        if (d->N[0] == 5 && !smag && orient && ref && !hyp)
            return make_engine<DryAtmos<true, true, false, false, false, NT>, 6>(d);
    }
    err = "DryAtmos with tracers: compiled in are N = 4 with 1 or 2 tracers (no orientation and no reference "
          "state; orientation + reference state, with or without hyperdiffusion or SmagorinskyLilly) and N = 5 "
          "with 1 tracer (orientation + reference state)";
    return nullptr;
}

}  // namespace cmdg
