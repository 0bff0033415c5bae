// Host check of csrc/with_constant.h and csrc/owned.h, without a device: built for the CPU against
// stub/hip/hip_runtime.h, meant to run under -fsanitize=address,undefined (test_host_owners.py).
//   c++ -std=c++17 -fsanitize=address,undefined -Istub -I../../climatemachine.jl_amd/csrc host_owners.cpp
#include <stdio.h>

#include "owned.h"
#include "with_constant.h"

using namespace cmdg;

static int failures = 0;
#define CHECK(x) \
    if (!(x)) ++failures, printf("FAILED line %d: %s\n", __LINE__, #x)

static void dispatch()
{
    for (int v = -1; v <= 10; ++v) {
        int seen = 0, calls = 0;
        const bool ok = with_constant<2, 8>(v, [&](auto n) {
            static_assert(decltype(n)::value >= 2 && decltype(n)::value <= 8, "instantiated outside the range");
            seen = n();
            ++calls;
        });
        CHECK(ok == (v >= 2 && v <= 8));
        CHECK(calls == (ok ? 1 : 0) && seen == (ok ? v : 0));
    }
    // nested, as the column operators use it: 2..8 x 1..4 and nothing else
    int pairs = 0;
    for (int a = 0; a <= 9; ++a)
        for (int b = 0; b <= 5; ++b) {
            bool inner = false;
            const bool outer = with_constant<2, 8>(a, [&](auto x) {
                inner = with_constant<1, 4>(b, [&](auto y) {
                    CHECK(x() == a && y() == b);
                    ++pairs;
                });
            });
            CHECK(outer == (a >= 2 && a <= 8) && inner == (outer && b >= 1 && b <= 4));
        }
    CHECK(pairs == 7 * 4);
    CHECK((!with_constant<3, 2>(3, [](auto) {})));  // empty range
}

struct Holder {  // members are released in the reverse of their declaration: the stream last
    Stream s;
    DevBuf<double> a, b;
    Event e;
};

static void owners()
{
    {
        DevBuf<double> a;
        CHECK(!a && a.get() == nullptr);
        a.reset();  // empty: nothing to release
        CHECK(a.alloc(4) == hipSuccess && a && stub::live.size() == 1);
        double *raw = a;
        CHECK(raw == a.get() && a + 1 == raw + 1);
        DevBuf<double> b(std::move(a));  // move: one owner
        CHECK(!a && b.get() == raw && stub::live.size() == 1);
        a = std::move(b);
        CHECK(!b && a.get() == raw);
        a = std::move(a);  // self-assignment keeps the buffer
        CHECK(a.get() == raw && stub::live.size() == 1);
        CHECK(b.alloc_zeroed(2, nullptr) == hipSuccess && stub::live.size() == 2);
        b = std::move(a);  // the target's buffer is released first
        CHECK(stub::live.size() == 1 && b.get() == raw);
        CHECK(b.alloc(8) == hipSuccess && stub::live.size() == 1);  // re-alloc releases the old one
        b.reset();
        b.reset();  // twice: released once
        CHECK(stub::live.empty());
        CHECK(a.alloc(1) == hipSuccess);
    }  // a released by its destructor, b and the moved-from objects release nothing
    CHECK(stub::live.empty() && stub::bad_release == 0);
    {
        Event e, f;
        Stream s, t;
        CHECK(e.create() == hipSuccess && e.create(hipEventDisableTiming) == hipSuccess && stub::live.size() == 1);
        f = std::move(e);
        CHECK(!e && f);
        CHECK(s.create(hipStreamNonBlocking) == hipSuccess && t.create(hipStreamNonBlocking, -1) == hipSuccess);
        s = std::move(t);  // set_stream_priority: the old stream goes, the new one stays
        CHECK(!t && s && stub::live.size() == 2);
    }
    CHECK(stub::live.empty() && stub::bad_release == 0);
    stub::log.clear();
    {
        Holder h;
        CHECK(h.s.create(hipStreamNonBlocking) == hipSuccess && h.a.alloc(1) == hipSuccess &&
              h.b.alloc(1) == hipSuccess && h.e.create() == hipSuccess);
        Holder g(std::move(h));  // a moved-from holder releases nothing
    }
    CHECK((stub::log == std::vector<std::string>{"event", "free", "free", "stream"}));
    CHECK(stub::live.empty() && stub::bad_release == 0);
}

int main()
{
    dispatch();
    owners();
    printf(failures ? "%d check(s) failed\n" : "host owners: ok\n", failures);
    return failures != 0;
}
