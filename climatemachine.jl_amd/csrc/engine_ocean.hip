// Engine instantiations for the hydrostatic Boussinesq ocean law (physics_ocean.h) and the
// PressureGradientModel used by the reference-state initialisation (physics_pgrad.h).
#include "engine.h"
#include "laws.h"
#include "physics_ocean.h"
#include "physics_ocean01.h"
#include "physics_pgrad.h"
#include "physics_sw.h"
#include "with_constant.h"

namespace cmdg {

// a law whose functor fixes its counts (no gradient-Laplacian or hyperdiffusive states)
template <class P>
static int law_counts(int32_t out[6])
{
    out[0] = P::NS;
    out[1] = P::NAUX;
    out[2] = P::NGRAD;
    out[3] = P::NGF;
    out[4] = out[5] = 0;
    return CMDG_OK;
}

// make_engine<P, N + 1> for LO <= N <= HI (NQ = N + 1 is a template parameter of every kernel)
template <class P, int LO, int HI>
static EngineBase *make_for_order(const cmdg_desc *d, std::string &err, const char *refusal)
{
    EngineBase *e = nullptr;
    if (!with_constant<LO, HI>(d->N[0], [&](auto n) { e = make_engine<P, n() + 1>(d); })) err = refusal;
    return e;
}

int counts_ocean(const int32_t *, int32_t out[6]) { return law_counts<HydroBoussinesq>(out); }

EngineBase *make_engine_ocean(const cmdg_desc *d, std::string &err)
{
    return make_for_order<HydroBoussinesq, 2, 5>(
        d, err, "HydrostaticBoussinesq: polynomial order not compiled in (have N = 2..5)");
}

int counts_sw(const int32_t *ip, int32_t out[6])
{
    out[0] = 3;
    out[1] = 5;
    out[2] = ShallowWater::NGRAD;
    out[3] = ShallowWater::NGF;
    out[4] = out[5] = 0;
    (void)ip;
    return CMDG_OK;
}

EngineBase *make_engine_sw(const cmdg_desc *d, std::string &err)
{
    if (d->iparam[1] != 0) {
        err = "ShallowWaterModel: LinearDrag is not compiled in (ConstantViscosity only)";
        return nullptr;
    }
    if (d->N[2] != d->N[0]) {
        // the one-layer extrusion of the 2-D grid needs no resolution along the extrusion:
        // two nodes (N_v = 1) carry the same 2-D arithmetic at 2/5 of the work
        if (d->N[0] == 4 && d->N[2] == 1) return make_engine<ShallowWater, 5, 2>(d);
        err = "ShallowWaterModel: mixed polynomial orders compiled in: (4, 1)";
        return nullptr;
    }
    return make_for_order<ShallowWater, 2, 5>(
        d, err, "ShallowWaterModel: polynomial order not compiled in (have N = 2..5)");
}

// src/Ocean/SplitExplicit01: OceanModel, Continuity3dModel, BarotropicModel (N = 4, the order
// of its reference tests; the barotropic model also with two nodes along the extrusion)
int counts_ocean_se01(const int32_t *, int32_t out[6]) { return law_counts<OceanSE01>(out); }
int counts_continuity3d_se01(const int32_t *, int32_t out[6]) { return law_counts<Continuity3dSE01>(out); }
int counts_barotropic_se01(const int32_t *, int32_t out[6]) { return law_counts<BarotropicSE01>(out); }

EngineBase *make_engine_se01(const cmdg_desc *d, std::string &err)
{
    if (d->N[0] != 4) {
        err = "SplitExplicit01 laws: polynomial order not compiled in (have N = 4)";
        return nullptr;
    }
    if (d->physics_id == CMDG_PHYSICS_BAROTROPIC_SE01) {
        if (d->N[2] == 1) return make_engine<BarotropicSE01, 5, 2>(d);
        if (d->N[2] == 4) return make_engine<BarotropicSE01, 5>(d);
        err = "BarotropicModel: extrusion order 1 or 4";
        return nullptr;
    }
    if (d->N[2] != 4) {
        err = "SplitExplicit01 laws: one polynomial order in all directions";
        return nullptr;
    }
    if (d->physics_id == CMDG_PHYSICS_OCEAN_SE01) return make_engine<OceanSE01, 5>(d);
    return make_engine<Continuity3dSE01, 5>(d);
}

int counts_pgrad(const int32_t *, int32_t out[6])
{
    out[0] = 3;
    out[1] = 1;
    out[2] = out[3] = out[4] = out[5] = 0;
    return CMDG_OK;
}

EngineBase *make_engine_pgrad(const cmdg_desc *d, std::string &err)
{
    return make_for_order<PressureGradient, 1, 7>(
        d, err, "PressureGradientModel: polynomial order not compiled in (have N = 1..7)");
}

}  // namespace cmdg
