// The three steps of csrc/exact_quotient.h (quot_steps, with std::fma) against `/` on the host,
// bit for bit.  Operands: the dry law's uniform divisors against numerators over many binades,
// 10^6 random normal pairs (fixed seed), divisors whose significand is all ones or next to a power
// of two, and numerators within an ulp of exact multiples of the divisor.  +-0, +-inf and NaN are
// left to the device test: on the host quot is `/` itself.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "exact_quotient.h"

using cmdg::quot_pair;
using cmdg::quot_steps;

static uint64_t bits(double x)
{
    uint64_t u;
    std::memcpy(&u, &x, 8);
    return u;
}
static double from_bits(uint64_t u)
{
    double x;
    std::memcpy(&x, &u, 8);
    return x;
}

static long checked = 0, failed = 0;
static void check(double a, double b)
{
    const volatile double want = a / b;
    const double got = quot_steps(a, quot_pair(b));
    ++checked;
    if (bits(got) != bits(want)) {
        if (failed < 10) std::printf("MISMATCH a=%a b=%a: steps %a, / %a\n", a, b, got, (double)want);
        ++failed;
    }
    // quot on the host is the division itself
    if (bits(cmdg::quot(a, quot_pair(b))) != bits(want)) ++failed;
}

int main()
{
    std::mt19937_64 rng(20250117);
    // a normal double with a random significand and an exponent in [-lim, lim]
    auto rnd = [&](int lim) {
        const uint64_t m = rng() & ((1ull << 52) - 1);
        const int e = int(rng() % uint64_t(2 * lim + 1)) - lim;
        const uint64_t s = rng() & 1;
        return from_bits((s << 63) | (uint64_t(1023 + e) << 52) | m);
    };

    // the uniform divisors of the dry law with the library's defaults (planet parameters of
    // CLIMAParameters 0.1: grav, cv_d = cp_d - R_d, MSLP) and the hyperdiffusion time scales in use
    const double R_d = 8.3144598 / 28.97e-3, cp_d = R_d / (2.0 / 7);
    const std::vector<double> uniform = {9.81, cp_d - R_d, 1e5, 101325.0, 3600.0, 8 * 3600.0, 86400.0,
                                         1.0, 2.0, 3.0, 0.7, 1 - 7.0 / 10};
    for (double b : uniform)
        for (int i = 0; i < 20000; ++i) check(rnd(200), b);

    for (int i = 0; i < 1000000; ++i) check(rnd(300), rnd(300));

    // divisors: all-ones significand, 1 + k ulp, 2 - k ulp, and a few bits set at either end
    std::vector<double> hard;
    for (int e = -3; e <= 3; ++e) {
        const uint64_t ex = uint64_t(1023 + e) << 52;
        for (uint64_t k = 0; k < 8; ++k) {
            hard.push_back(from_bits(ex | (((1ull << 52) - 1) - k)));
            hard.push_back(from_bits(ex | k));
            hard.push_back(from_bits(ex | (((1ull << 52) - 1) >> k)));
            hard.push_back(from_bits(ex | (((1ull << 52) - 1) << (4 * k) & ((1ull << 52) - 1))));
        }
    }
    for (double b : hard) {
        for (int i = 0; i < 2000; ++i) check(rnd(100), b);
        for (double a : hard) check(a, b);
    }

    // numerators within an ulp of an exact multiple: a = RN(k b) and its two neighbours
    for (int i = 0; i < 100000; ++i) {
        const double b = i % 2 ? rnd(50) : hard[size_t(rng() % hard.size())];
        const double k = i % 3 ? double(int64_t(rng() % 4096) + 1) : rnd(30);
        const double a = k * b;
        check(a, b);
        check(from_bits(bits(a) + 1), b);
        check(from_bits(bits(a) - 1), b);
    }

    std::printf("%ld quotients, %ld mismatches\n", checked, failed);
    if (failed) return 1;
    std::printf("host exact quotient: ok\n");
    return 0;
}
