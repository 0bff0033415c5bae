// Reductions of state arrays (cmdg_reduce_*): the device part lives in reductions.hip, the ABI
// entries and the RCCL all-gather follow it there.  Free functions that take the engine: nothing here
// changes the layout of EngineBase (the scratch of a handle is kept in a table of reductions.hip).
#pragma once
#include <string>

#include "../../include/cmdg.h"

namespace cmdg {
struct EngineBase;

// argument checks that need no handle (op, p, nstate, state subset)
int reduce_check(const cmdg_reduce_desc *d, std::string &err);
// values per rank: per_state ? chosen states : 1
int reduce_nout(const cmdg_reduce_desc *d);
// enqueues both stages on e->s_comp; *d_result: nout (hi, lo) pairs on the device, valid until the
// next reduction of this engine
int reduce_device(EngineBase *e, const cmdg_reduce_desc *d, const double *A, const double *B,
                  const double **d_result);
// a device buffer of n doubles owned by the engine's reduction scratch (the all-gather target)
int reduce_gather_buffer(EngineBase *e, size_t n, double **buf);
// pinned host staging of n doubles owned by the same scratch
int reduce_host_buffer(EngineBase *e, size_t n, double **buf);
// nranks x nout partials -> nout finished values (cmdg_reduce_combine)
int reduce_combine(const cmdg_reduce_desc *d, const double *partials, int nranks, double *out,
                   std::string &err);
// frees the scratch of an engine that is being destroyed (its device current)
void reduce_release(EngineBase *e);
}  // namespace cmdg
