// Dry atmosphere law with two tracers (engine_atmos_tracers.h).
#include "engine_atmos_tracers.h"

namespace cmdg {

EngineBase *make_engine_atmos_tracers2(const cmdg_desc *d, std::string &err) { return pick_atmos_tracers<2, false>(d, err); }

}  // namespace cmdg
