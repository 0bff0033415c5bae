// Move-only owners of what a handle allocates on the device: a member of one of these types is
// released by its own destructor, in the reverse of the order of declaration, so a function that
// returns early and a destructor that forgets a member leak nothing.  Each is one pointer wide and
// converts to the raw handle, so launches, copies and pointer arithmetic read as with a raw member.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include <utility>

namespace cmdg {

// one raw handle H, released once with RELEASE
template <class H, hipError_t (*RELEASE)(H)>
class Owned {
  protected:
    H h = nullptr;

  public:
    Owned() = default;
    Owned(Owned &&o) noexcept : h(std::exchange(o.h, nullptr)) {}
    Owned &operator=(Owned &&o) noexcept
    {
        if (this != &o) {
            reset();
            h = std::exchange(o.h, nullptr);
        }
        return *this;
    }
    ~Owned() { reset(); }
    H get() const { return h; }
    operator H() const { return h; }
    void reset()
    {
        if (h) (void)RELEASE(std::exchange(h, nullptr));
    }
};

template <class T>
inline hipError_t dev_free(T *p) { return hipFree(p); }

// every create / alloc releases what the owner held before
template <class T>
struct DevBuf : Owned<T *, dev_free<T>> {
    hipError_t alloc(size_t n)  // n elements
    {
        this->reset();
        return hipMalloc((void **)&this->h, sizeof(T) * n);
    }
    // ... filled with zeros by st: the fill is ordered before whatever st is given next, and before
    // nothing else (a hipMemset on the null stream is not ordered against non-blocking streams)
    hipError_t alloc_zeroed(size_t n, hipStream_t st)
    {
        const hipError_t r = alloc(n);
        return r != hipSuccess ? r : hipMemsetAsync(this->h, 0, sizeof(T) * n, st);
    }
};

struct Event : Owned<hipEvent_t, hipEventDestroy> {
    hipError_t create(unsigned flags = hipEventDefault)
    {
        reset();
        return hipEventCreateWithFlags(&h, flags);
    }
};

struct Stream : Owned<hipStream_t, hipStreamDestroy> {
    hipError_t create(unsigned flags)
    {
        reset();
        return hipStreamCreateWithFlags(&h, flags);
    }
    hipError_t create(unsigned flags, int priority)
    {
        reset();
        return hipStreamCreateWithPriority(&h, flags, priority);
    }
};

}  // namespace cmdg
