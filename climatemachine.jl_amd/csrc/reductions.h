// Reductions of state arrays (cmdg_reduce_*): the device part lives in reductions.hip, the ABI
// entries and the RCCL all-gather follow it there.  Free functions that take the engine: nothing here
// changes the layout of EngineBase (the scratch of a handle is kept in a table of reductions.hip).
#pragma once
#include <string>

#include "../../include/cmdg.h"

#include <hip/hip_runtime.h>
#include <math.h>

namespace cmdg {
struct EngineBase;

// ---- double-double primitives (reductions.hip, diagnostics.hip) -------------------------------
// exact only in a unit compiled with -ffp-contract=off and no fast-math (Makefile)
struct DD {
    double hi, lo;
};
__host__ __device__ inline DD two_sum(double a, double b)
{
    const double s = a + b, bb = s - a;
    return {s, (a - (s - bb)) + (b - bb)};
}
__host__ __device__ inline DD fast_two_sum(double a, double b)  // |a| >= |b|
{
    const double s = a + b;
    return {s, b - (s - a)};
}
__device__ inline DD two_prod(double a, double b)
{
    const double p = a * b;
    return {p, fma(a, b, -p)};
}
// accurate double-double addition (both components' errors carried)
__host__ __device__ inline DD dd_add(DD a, DD b)
{
    DD s = two_sum(a.hi, b.hi);
    const DD t = two_sum(a.lo, b.lo);
    s.lo += t.hi;
    s = fast_two_sum(s.hi, s.lo);
    s.lo += t.lo;
    return fast_two_sum(s.hi, s.lo);
}
// (hi + lo) * b; exact when lo == 0 (TwoProd)
__device__ inline DD dd_mul_d(DD a, double b)
{
    DD p = two_prod(a.hi, b);
    p.lo = fma(a.lo, b, p.lo);
    return fast_two_sum(p.hi, p.lo);
}
// (hi + lo) + b for a double b
__host__ __device__ inline DD dd_add_d(DD a, double b)
{
    DD s = two_sum(a.hi, b);
    s.lo += a.lo;
    return fast_two_sum(s.hi, s.lo);
}

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
