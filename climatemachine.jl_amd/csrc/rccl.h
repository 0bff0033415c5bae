// RCCL, resolved lazily so that single-GPU use has no link-time dependency.  halo.hip resolves the
// entry points (rccl::load) and uses most of them; ~EngineBase (CommDestroy) and cmdg_reduce
// (AllGather) are the callers outside it.  An entry point is NULL until load() has succeeded.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

namespace cmdg {
namespace rccl {
typedef struct { char internal[128]; } uid_t;
typedef int (*GetUniqueId_t)(uid_t *);
typedef int (*CommInitRank_t)(void **, int, uid_t, int);
typedef int (*CommDestroy_t)(void *);
typedef int (*GroupStart_t)();
typedef int (*GroupEnd_t)();
typedef int (*Send_t)(const void *, size_t, int, int, void *, hipStream_t);
typedef int (*Recv_t)(void *, size_t, int, int, void *, hipStream_t);
typedef const char *(*GetErrorString_t)(int);
typedef int (*AllGather_t)(const void *, void *, size_t, int, void *, hipStream_t);
extern GetUniqueId_t GetUniqueId;
extern CommInitRank_t CommInitRank;
extern CommDestroy_t CommDestroy;
extern GroupStart_t GroupStart;
extern GroupEnd_t GroupEnd;
extern Send_t Send;
extern Recv_t Recv;
extern GetErrorString_t GetErrorString;
extern AllGather_t AllGather;
constexpr int kDouble = 8;  // ncclFloat64 / ncclDouble
bool load(std::string &err);
}  // namespace rccl
}  // namespace cmdg
