// Stand-in for <hip/hip_runtime.h> in host_owners.cpp: the calls csrc/owned.h makes, counted and
// logged, so that the owner types can be exercised (and run under sanitizers) without a device.
#pragma once
#include <stddef.h>
#include <stdlib.h>

#include <set>
#include <string>
#include <vector>

typedef int hipError_t;
constexpr hipError_t hipSuccess = 0, hipErrorInvalidValue = 1;
typedef struct stub_event *hipEvent_t;
typedef struct stub_stream *hipStream_t;
constexpr unsigned hipEventDefault = 0, hipEventDisableTiming = 2, hipStreamNonBlocking = 1;

namespace stub {
inline std::set<void *> live;            // what was handed out and not yet released
inline std::vector<std::string> log;     // "free", "event", "stream" in the order of release
inline int bad_release = 0;              // releases of something not live (a double free)
inline void *make() { return *live.insert(malloc(1)).first; }
inline hipError_t release(void *p, const char *what)
{
    if (!live.erase(p)) return ++bad_release, hipErrorInvalidValue;
    free(p);
    log.push_back(what);
    return hipSuccess;
}
}  // namespace stub

inline hipError_t hipMalloc(void **p, size_t) { return *p = stub::make(), hipSuccess; }
inline hipError_t hipFree(void *p) { return stub::release(p, "free"); }
inline hipError_t hipMemsetAsync(void *p, int, size_t, hipStream_t) { return stub::live.count(p) ? hipSuccess : hipErrorInvalidValue; }
inline hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) { return *e = (hipEvent_t)stub::make(), hipSuccess; }
inline hipError_t hipEventDestroy(hipEvent_t e) { return stub::release(e, "event"); }
inline hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned) { return *s = (hipStream_t)stub::make(), hipSuccess; }
inline hipError_t hipStreamCreateWithPriority(hipStream_t *s, unsigned, int) { return *s = (hipStream_t)stub::make(), hipSuccess; }
inline hipError_t hipStreamDestroy(hipStream_t s) { return stub::release(s, "stream"); }
