// bb_device_round.hpp -- the .NET Framework rounding and the scalar tests of the Branch & Bound
// path on the device, shared by the single-tree kernels (bb_kernels.hip) and the batched B&B
// (bb_batch_kernels.hip).  Host copies of the same rules live in bb_engine.hip.
#pragma once

#include "engine_common.hpp"

#include <climits>

#pragma clang fp contract(off)

namespace lpr {

constexpr double kBBEps = 1e-6;  // BranchAndBound.epsilon (:493)

// ------------------------------------------------------------------ .NET Framework rounding
// Math.Round(double) -- COMDouble::Round (round half to even through floor(x + 0.5)).
// (The runtime's own text is `if (x == (double)(long long)x) return x; t = x + 0.5; f = floor(t);
// if (f == t && fmod(t, 2.0) != 0) f -= 1.0; return copysign(f, x)`.  The two tests are restated
// without the 64-bit integer conversion and without fmod -- "x is integral" is floor(x) == x for
// every finite x (above 2^52 every double is), "t is odd" is "t / 2 is not integral", exact because
// halving is -- which is 4x fewer instructions on the device and bit-identical: checked against
// the literal form over 2e8 random and edge operands on the CPU.)
__device__ __forceinline__ double dn_round_int(double x) {
    if (isnan(x) || isinf(x)) return x;
    if (floor(x) == x) return x;
    const double t = x + 0.5;
    double f = floor(t);
    const double h = t * 0.5;
    if (f == t && floor(h) != h) f -= 1.0;
    return copysign(f, x);
}
// Math.Round(double, 4) -- Math.InternalRound: scale, round, unscale; identity for |x| >= 1e16.
__device__ __forceinline__ double dn_round4(double x) {
    if (fabs(x) < 1e16) {
        x = x * 10000.0;
        x = dn_round_int(x);
        x = ieee_div(x, 10000.0);
    }
    return x;
}

// RoundNumber(RoundNumber(x)): the C# rounds a value again wherever a rounded tableau is handed on
// (:702 then :655 / :747).  Below 1e11 the second call returns its argument (x * 1e4 is within half
// a unit of the integer it came from, so it rounds back to it; checked over 2e8 operands); only
// above that is it evaluated.
__device__ __forceinline__ double dn_round4_twice(double x) {
    const double r = dn_round4(x);
    return (fabs(r) < 1e11) ? r : dn_round4(r);
}

// x rounded three times, then DoDualSimplex's -0 -> +0 (what a row of the parent has been through
// when the child's dual simplex starts: :702, :747, :799, :307-313)
__device__ __forceinline__ double dn_round4_thrice_clean(double x) {
    double r = dn_round4(x);
    if (!(fabs(r) < 1e11)) r = dn_round4(dn_round4(r));
    if (r == 0.0) r = 0.0;
    return r;
}

// IsInteger (:595-599): Math.Round(v, 4) within epsilon of Math.Round of itself.
__device__ __forceinline__ bool dn_is_integer(double v) {
    const double r = dn_round4(v);
    return fabs(r - dn_round_int(r)) <= kBBEps;
}

// `(int)d` of the C# (:870-871) as the x64 JIT of .NET Framework 4.7.2 compiles it (cvttsd2si): a
// value outside int's range, or NaN, gives 0x80000000.
__device__ __forceinline__ int dn_to_int32(double x) {
    if (!(x > -2147483649.0 && x < 2147483648.0)) return INT_MIN;
    return (int)x;
}

}  // namespace lpr
