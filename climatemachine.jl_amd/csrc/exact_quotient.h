// The correctly rounded fp64 quotient a / b from a reciprocal that several quotients share.
//
// The reference divides; a * (1 / b) differs from a / b in the last bit for many operand pairs and
// the bit-for-bit tests reject it.  What is formed here is RN(a / b) itself, by a shorter road than
// the compiler's expansion of `/` (v_div_scale x 2, v_rcp, five v_fma, v_div_fmas, v_div_fixup).
//
// Theorem (Markstein, "Computation of elementary functions on the IBM RISC System/6000 processor",
// IBM J. Res. Dev. 34, 1990; Muller et al., Handbook of Floating-Point Arithmetic, section 4.7):
// with y = RN(1 / b), q0 = RN(a y), r = fma(-b, q0, a) and q = fma(r, y, q0), q = RN(a / b).
// q0 is within an ulp of a / b, so r is exact; r y then corrects q0 with one rounding.  This is
// the tail of the compiler's own sequence.
// Preconditions:
//   - y is the correctly rounded reciprocal.  quot_pair forms it with a full division; the uniform
//     pairs of a parameter block come from one IEEE division on the host.
//   - a, b, a / b, 1 / b and r stay in the normal range: nothing overflows, and r = a - b q0, about
//     2^-53 |a|, does not underflow (|a| > 2^-968 or so).  v_div_scale guards the compiler's
//     sequence against that; nothing does here.
// A numerator that is +-0, +-inf or NaN, or a divisor that is, goes through v_div_fixup_f64 as in
// the compiler's sequence, which gives the signed zero, the infinity or the NaN of a / b whatever
// the three steps left.
// Why the balance laws' operands qualify: divisors are the density (order 1e-3 .. 1) and planetary
// constants (grav, cv_d, MSLP, tau: 1 .. 1e5); numerators are momenta, energies, pressures and
// grad Phi, which are either exactly zero (a state at rest: the fix-up) or many hundreds of binades
// above 2^-968.
//
// On the host (the __host__ __device__ law functions, make_params) quot is plain a / b: the same
// bits by IEEE, with no precondition.  quot_steps is the generic text of the three steps; the host
// test compiles it with std::fma against `/`.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define CMDG_XQ_HD __host__ __device__
#else
#define CMDG_XQ_HD
#endif

namespace cmdg {

struct QuotPair {
    double b, y;  // the divisor and RN(1 / b)
};

CMDG_XQ_HD inline QuotPair quot_pair(double b) { return QuotPair{b, 1.0 / b}; }

// explicit fma calls: they stay fused under -ffp-contract=off, and nothing else here may fuse
CMDG_XQ_HD inline double quot_steps(double a, const QuotPair &d)
{
    const double q0 = a * d.y;
    const double r = std::fma(-d.b, q0, a);
    return std::fma(r, d.y, q0);
}

CMDG_XQ_HD inline double quot(double a, const QuotPair &d)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_div_fixup(quot_steps(a, d), d.b, a);
#else
    return a / d.b;
#endif
}

}  // namespace cmdg
