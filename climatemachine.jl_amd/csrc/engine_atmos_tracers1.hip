// Dry atmosphere law with one tracer (engine_atmos_tracers.h).
#include "engine_atmos_tracers.h"

namespace cmdg {

EngineBase *make_engine_atmos_tracers1(const cmdg_desc *d, std::string &err) { return pick_atmos_tracers<1, true>(d, err); }

}  // namespace cmdg
