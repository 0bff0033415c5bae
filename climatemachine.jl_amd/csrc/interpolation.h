// Interpolation of DG states onto box and latitude-longitude grids (cmdg_interp_* of
// include/cmdg.h); implemented in interpolation.hip, which also holds those entries.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/cmdg.h"

namespace cmdg {
struct InterpObj;
// st == nullptr selects the default stream of the object's device and waits for the work; the
// caller has made the right device current otherwise.  On failure err holds the reason.
int interp_create(const cmdg_interp_desc *d, InterpObj **out, std::string &err);
void interp_destroy(InterpObj *o);
int interp_device(const InterpObj *o);
int interp_apply(const InterpObj *o, const double *Q, int nstate, int64_t nelemQ, double *v, hipStream_t st,
                 bool wait, std::string &err);
int interp_project(const InterpObj *o, double *v, int nstate, const int32_t *uvwi, hipStream_t st, bool wait,
                   std::string &err);
int interp_scatter(const InterpObj *const *o, int n, const double *const *v, int nstate, double *fiv,
                   hipStream_t st, bool wait, std::string &err);
// the finishing pass of the AtmosGCMDefault group: projection, quotients and scatter of the 13 variables
int interp_gcm_finish(const InterpObj *const *o, int n, const double *const *vG, const double *const *vB,
                      double *fiv, hipStream_t st, bool wait, std::string &err);
}  // namespace cmdg
