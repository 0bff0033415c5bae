// Engine instantiations for the AdvectionDiffusion law (physics_advdiff.h).
#include "engine_fv.h"
#include "laws.h"
#include "physics_advdiff.h"
#include "with_constant.h"

namespace cmdg {

int counts_advdiff(const int32_t *ip, int32_t out[6])
{
    if (ip[0] != 1) return CMDG_ERR_UNSUPPORTED;  // num_equations
    const bool adv = ip[1], diff = ip[2], hyp = ip[3];
    out[0] = 1;
    out[1] = 3 + (adv ? 3 : 0) + (diff ? 9 : 0) + (hyp ? 9 : 0);
    out[2] = (diff || hyp) ? 1 : 0;
    out[3] = diff ? 3 : 0;
    out[4] = hyp ? 1 : 0;
    out[5] = hyp ? 3 : 0;
    return CMDG_OK;
}

template <int NQ>
static EngineBase *pick(const cmdg_desc *d, std::string &err)
{
    const bool adv = d->iparam[1], diff = d->iparam[2], hyp = d->iparam[3];
    if (adv && diff && !hyp) return make_engine<AdvDiff<true, true, false>, NQ>(d);
    if (!adv && !diff && hyp) return make_engine<AdvDiff<false, false, true>, NQ>(d);
    if (adv && !diff && !hyp) return make_engine<AdvDiff<true, false, false>, NQ>(d);
    if (!adv && diff && !hyp) return make_engine<AdvDiff<false, true, false>, NQ>(d);
    if (!adv && diff && hyp) return make_engine<AdvDiff<false, true, true>, NQ>(d);
    err = "AdvectionDiffusion: this advection/diffusion/hyperdiffusion combination is not compiled in";
    return nullptr;
}

EngineBase *make_engine_advdiff(const cmdg_desc *d, std::string &err)
{
    if (d->iparam[0] != 1) {
        err = "AdvectionDiffusion: num_equations != 1 is not compiled in";
        return nullptr;
    }
    if (d->N[2] != d->N[0]) {
        // polynomialorder = (N_h, N_v): the pairs of variable_degree_advection_diffusion.jl:300
        const bool adv = d->iparam[1], diff = d->iparam[2], hyp = d->iparam[3];
        if (adv && diff && !hyp) {
            if (d->N[0] == 4 && d->N[2] == 2) return make_engine<AdvDiff<true, true, false>, 5, 3>(d);
            if (d->N[0] == 2 && d->N[2] == 4) return make_engine<AdvDiff<true, true, false>, 3, 5>(d);
        }
        err = "AdvectionDiffusion: mixed polynomial orders compiled in are (4,2) and (2,4), "
              "advection + diffusion";
        return nullptr;
    }
    EngineBase *e = nullptr;  // NQ = N + 1 is a template parameter of every kernel
    if (!with_constant<1, 7>(d->N[0], [&](auto n) { e = pick<n() + 1>(d, err); }))
        err = "AdvectionDiffusion: polynomial order not compiled in (have N = 1..7)";
    return e;
}

// DGFVModel handles: advection, and advection + diffusion, at N_h = 4 and N_h = 1
template <int NQ>
static EngineBase *pick_fv(const cmdg_desc *d, const cmdg_fv_desc *fv, std::string &err)
{
    const bool adv = d->iparam[1], diff = d->iparam[2], hyp = d->iparam[3];
    if (hyp) {
        err = "DGFVModel: a law with hyperdiffusive states is not supported (DGFVModel.jl:91)";
        return nullptr;
    }
    if (adv && diff) return make_engine_fv<AdvDiff<true, true, false>, NQ>(d, fv);
    if (adv && !diff) return make_engine_fv<AdvDiff<true, false, false>, NQ>(d, fv);
    err = "DGFVModel AdvectionDiffusion: advection, or advection + diffusion, are compiled in";
    return nullptr;
}

EngineBase *make_engine_advdiff_fv(const cmdg_desc *d, const cmdg_fv_desc *fv, std::string &err)
{
    if (d->iparam[0] != 1) {
        err = "AdvectionDiffusion: num_equations != 1 is not compiled in";
        return nullptr;
    }
    switch (d->N[0]) {
    case 1: return pick_fv<2>(d, fv, err);
    case 4: return pick_fv<5>(d, fv, err);
    default:
        err = "DGFVModel AdvectionDiffusion: horizontal polynomial orders compiled in are 1 and 4";
        return nullptr;
    }
}

}  // namespace cmdg
