// Engine instantiations for AtmosAcousticGravityLinearModel (physics_atmos_linear.h).  The law
// shares the full model's auxiliary array.  Of the dry law the count comes from the full model's
// parameter block: orientation and reference state are required, hyperdiffusion or
// SmagorinskyLilly add one column each, a tracer of the full model one more (the linear model itself
// carries none: five states, AtmosModel.jl:399-406).  Of the moist LES law (CMDG_PHYSICS_MOIST_LINEAR_AG) it is
// always MoistAtmos's 19, at the orders the moist law is compiled for.
#include "engine.h"
#include "laws.h"
#include "physics_atmos_linear.h"

namespace cmdg {

static int naux_of_full(const int32_t *ip)
{
    int32_t c[6];
    counts_atmos(ip, c);
    return c[1];
}

int counts_atmos_linear(const int32_t *ip, int32_t out[6])
{
    out[0] = 5;
    out[1] = naux_of_full(ip);
    out[2] = out[3] = out[4] = out[5] = 0;
    return CMDG_OK;
}

template <int NQ>
static EngineBase *pick(const cmdg_desc *d, std::string &err)
{
    switch (naux_of_full(d->iparam)) {
    case 16: return make_engine<AtmosLinearAG<16>, NQ>(d);  // no hyperdiffusion, no Smagorinsky
    case 17: return make_engine<AtmosLinearAG<17>, NQ>(d);  // DryBiharmonic (Held-Suarez), or one tracer
    // the count is a stride only: the law reads Phi, grad Phi and the reference state, which precede
    // every optional column.  One or two tracers (delta_chi columns) on top of the above:
    case 18: return make_engine<AtmosLinearAG<18>, NQ>(d);
    case 19: return make_engine<AtmosLinearAG<19>, NQ>(d);
    default:
        err = "AtmosAcousticGravityLinearModel: the full model's auxiliary layout is not compiled in "
              "(have orientation + reference state, with or without hyperdiffusion or SmagorinskyLilly, and "
              "up to two tracers on top: 16 to 19 columns)";
        return nullptr;
    }
}

EngineBase *make_engine_atmos_linear(const cmdg_desc *d, std::string &err)
{
    if (d->iparam[0] == 0 || d->iparam[1] == 0) {
        err = "AtmosAcousticGravityLinearModel needs a model with an orientation and a reference state";
        return nullptr;
    }
    if (d->nf_first != CMDG_RUSANOV && d->nf_first != CMDG_CENTRAL_FIRST_ORDER) {
        err = "AtmosAcousticGravityLinearModel: Rusanov or central first-order flux only";
        return nullptr;
    }
    switch (d->N[0]) {
    case 4: return pick<5>(d, err);
    case 5: return pick<6>(d, err);
    default:
        err = "AtmosAcousticGravityLinearModel: polynomial order not compiled in (have N = 4, 5)";
        return nullptr;
    }
}

int counts_atmos_acoustic(const int32_t *ip, int32_t out[6]) { return counts_atmos_linear(ip, out); }

EngineBase *make_engine_atmos_acoustic(const cmdg_desc *d, std::string &err)
{
    if (d->iparam[0] != 0 || d->iparam[1] == 0 || d->iparam[4] != 0 || d->iparam[14] != 0) {
        err = "AtmosAcousticLinearModel is compiled for a dry model with NoOrientation and a reference state "
              "(no hyperdiffusion, constant viscosity)";
        return nullptr;
    }
    if (d->nf_first != CMDG_RUSANOV && d->nf_first != CMDG_CENTRAL_FIRST_ORDER) {
        err = "AtmosAcousticLinearModel: Rusanov or central first-order flux only";
        return nullptr;
    }
    if (d->N[0] != 4) {
        err = "AtmosAcousticLinearModel: polynomial order not compiled in (have N = 4)";
        return nullptr;
    }
    return make_engine<AtmosLinearAG<12, false, false>, 5>(d);
}

int counts_moist_linear(const int32_t *, int32_t out[6])
{
    out[0] = 6;
    out[1] = 19;
    out[2] = out[3] = out[4] = out[5] = 0;
    return CMDG_OK;
}

EngineBase *make_engine_moist_linear(const cmdg_desc *d, std::string &err)
{
    // moist.py descriptor(): iparam[4] marks NoOrientation + NoReferenceState
    if (d->iparam[4] != 0) {
        err = "AtmosAcousticGravityLinearModel needs a moist model with an orientation and a reference "
              "state (this one has no_orientation)";
        return nullptr;
    }
    if (d->nf_first != CMDG_RUSANOV && d->nf_first != CMDG_CENTRAL_FIRST_ORDER) {
        err = "AtmosAcousticGravityLinearModel (EquilMoist): Rusanov or central first-order flux only";
        return nullptr;
    }
    switch (d->N[0]) {
    case 4: return make_engine<AtmosLinearAG<19, true>, 5>(d);
    case 6: return make_engine<AtmosLinearAG<19, true>, 7>(d);
    default:
        err = "AtmosAcousticGravityLinearModel (EquilMoist): polynomial order not compiled in (have N = 4, 6)";
        return nullptr;
    }
}

}  // namespace cmdg
