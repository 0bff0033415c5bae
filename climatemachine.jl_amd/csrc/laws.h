// The factories and the counts functions of the laws compiled in, one pair per physics id: defined per
// physics family in the engine_*.hip units, looked up through the table of create.hip (LAWS).  A factory
// returns NULL with the reason in err for a descriptor its family does not serve.  Internal.
#pragma once
#include <string>

#include "engine_base.h"

namespace cmdg {

EngineBase *make_engine_advdiff(const cmdg_desc *d, std::string &err);
EngineBase *make_engine_advdiff_fv(const cmdg_desc *d, const cmdg_fv_desc *fv, std::string &err);
EngineBase *make_engine_atmos(const cmdg_desc *d, std::string &err);
EngineBase *make_engine_atmos_tracers1(const cmdg_desc *d, std::string &err);  // (NTracers: one unit per count)
EngineBase *make_engine_atmos_tracers2(const cmdg_desc *d, std::string &err);
EngineBase *make_engine_atmos_fv(const cmdg_desc *d, const cmdg_fv_desc *fv, std::string &err);
EngineBase *make_engine_ocean(const cmdg_desc *d, std::string &err);
EngineBase *make_engine_pgrad(const cmdg_desc *d, std::string &err);
EngineBase *make_engine_sw(const cmdg_desc *d, std::string &err);
EngineBase *make_engine_moist(const cmdg_desc *d, std::string &err);
EngineBase *make_engine_se01(const cmdg_desc *d, std::string &err);  // (the three SplitExplicit01 ids)
EngineBase *make_engine_atmos_linear(const cmdg_desc *d, std::string &err);
EngineBase *make_engine_moist_linear(const cmdg_desc *d, std::string &err);
EngineBase *make_engine_atmos_acoustic(const cmdg_desc *d, std::string &err);
EngineBase *make_engine_esdg(const cmdg_desc *d, const cmdg_esdg_desc *ed, std::string &err);
EngineBase *make_engine_esdg_dryatmos_linear(const cmdg_desc *d, std::string &err);
EngineBase *make_engine_vorticity(const cmdg_desc *d, std::string &err);

// out: num_state_conservative, auxiliary, gradient, gradient_flux, gradient_laplacian, hyperdiffusive
int counts_advdiff(const int32_t *iparam, int32_t out[6]);
int counts_atmos(const int32_t *iparam, int32_t out[6]);
int counts_ocean(const int32_t *iparam, int32_t out[6]);
int counts_pgrad(const int32_t *iparam, int32_t out[6]);
int counts_sw(const int32_t *iparam, int32_t out[6]);
int counts_moist(const int32_t *iparam, int32_t out[6]);
int counts_ocean_se01(const int32_t *iparam, int32_t out[6]);
int counts_continuity3d_se01(const int32_t *iparam, int32_t out[6]);
int counts_barotropic_se01(const int32_t *iparam, int32_t out[6]);
int counts_atmos_linear(const int32_t *iparam, int32_t out[6]);
int counts_moist_linear(const int32_t *iparam, int32_t out[6]);
int counts_atmos_acoustic(const int32_t *iparam, int32_t out[6]);
int counts_esdg_dryatmos(const int32_t *iparam, int32_t out[6]);
int counts_esdg_dryatmos_linear(const int32_t *iparam, int32_t out[6]);
int counts_vorticity(const int32_t *iparam, int32_t out[6]);
int host_constants_atmos(const int32_t *iparam, const double *dparam, double out[7]);

}  // namespace cmdg
