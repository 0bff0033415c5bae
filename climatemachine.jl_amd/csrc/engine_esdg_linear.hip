// Engine instantiations for DryAtmosAcousticGravityLinearModel (physics_esdg_dryatmos_linear.h): an
// ordinary DGModel law through the pass kernels of kernels.h, at the orders an ESDGModel handle is
// compiled for.  It shares the ESDG model's auxiliary array, whose reference-state columns it needs.
#include "band_solve.h"
#include "engine.h"
#include "laws.h"
#include "physics_esdg_dryatmos_linear.h"

namespace cmdg {

int counts_esdg_dryatmos_linear(const int32_t *, int32_t out[6])
{
    out[0] = EsdgDryAtmosLinearAG::NS;
    out[1] = EsdgDryAtmosLinearAG::NAUX;
    out[2] = out[3] = out[4] = out[5] = 0;
    return CMDG_OK;
}

EngineBase *make_engine_esdg_dryatmos_linear(const cmdg_desc *d, std::string &err)
{
    if (d->iparam[1] == 0) {
        err = "DryAtmosAcousticGravityLinearModel needs a model with a reference state";
        return nullptr;
    }
    if (d->nf_first != CMDG_RUSANOV && d->nf_first != CMDG_CENTRAL_FIRST_ORDER) {
        err = "DryAtmosAcousticGravityLinearModel: Rusanov or central first-order flux only";
        return nullptr;
    }
    if (d->N[0] != d->N[2]) {
        err = "DryAtmosAcousticGravityLinearModel: mixed polynomial orders are not compiled in";
        return nullptr;
    }
    switch (d->N[0]) {
    case 3: return make_engine<EsdgDryAtmosLinearAG, 4>(d);
    case 4: return make_engine<EsdgDryAtmosLinearAG, 5>(d);
    default:
        err = "DryAtmosAcousticGravityLinearModel: polynomial order not compiled in (have N = 3, 4)";
        return nullptr;
    }
}

// The column solver's substitution at this law's own order, N = 3 (the other laws start at N = 4): a
// window of 20 doubles per lane, in registers like the others (scratch 0).
void band_solve_nqv4_ns5(dim3 grid, dim3 block, hipStream_t st, double *X, const double *B, const double *A,
                         int64_t ncol, int nvert, int nqh2)
{
    hipLaunchKernelGGL((k_band_solve<4, EsdgDryAtmosLinearAG::NS>), grid, block, 0, st, X, B, A, ncol, nvert, nqh2);
}

}  // namespace cmdg
