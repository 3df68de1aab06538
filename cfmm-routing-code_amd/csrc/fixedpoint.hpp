// The arithmetic of the reproducible mode's 96-bit fixed point (kernels.hpp: Scatter<true>, det_fold_kernel), free of device
// builtins so that the host compiler builds it alone: tests/test_fixedpoint_host.py checks it against Python integers, the
// device suite checks the device's compile of the same lines against the same integers (cfmm_debug_scatter_limbs).
#pragma once
#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CFMM_FX_HD __host__ __device__ inline __attribute__((always_inline))     // (__forceinline__ spelt out: a host program that hipcc builds need not include the HIP runtime's header)
#else
#define CFMM_FX_HD inline
#endif

namespace cfmm {

struct FixedLimbs { unsigned a0, a1; int a2; };        // value = a2 2^64 + a1 2^32 + a0,  0 <= a0, a1 < 2^32

// floor(yf) as three limbs, for yf = y * 2^F already scaled (a power of two: exact).  Exact for both signs and every |yf| < 2^95;
// det_scales (cfmm_hip.hip) keeps |yf| < 2^84, the head-room bound of the mode (10 bits below the sign of the 96-bit image).
// Only the fraction of yf is dropped (towards -inf).  Every step is exactly representable:
//   t = floor(yf) is an integer of at most 53 significant bits; q = floor(t / 2^32) keeps a prefix of them; a0 = t - q 2^32 is the
//   integer in [0, 2^32) congruent to t, a multiple of ulp(t): at most 32 bits.  Likewise q -> (a2, a1).  The three conversions see
//   integers inside their types' ranges, whatever the sign of yf.
// (Taking the TOP limb first -- a2 = floor(yf 2^-64), r = yf - a2 2^64 -- is not exact: for small negative yf, r = 2^64 + yf lies
// where doubles are 2^11 apart, and rounds up to 2^64 itself for -2^10 < yf < 0.)
CFMM_FX_HD FixedLimbs fixed_split(double yf)
{
    const double t = floor(yf);
    const double q = floor(t * 0x1p-32);
    const double a0 = fma(-q, 0x1p32, t);
    const double a2 = floor(q * 0x1p-32);
    const double a1 = fma(-a2, 0x1p32, q);
    return {(unsigned)a0, (unsigned)a1, (int)a2};
}

// l2 2^64 + l1 2^32 + l0 of three limb SUMS as a signed 128-bit integer hi 2^64 + lo.  l0 and l1 are sums of limbs in [0, 2^32):
// UNSIGNED, exact up to 2^32 contributions of 2^32 - 1 each; l2 is a wrapped SIGNED 64-bit sum, negative when the value is.
// Unsigned 128-bit arithmetic: wraps, never overflows (l2 2^64 drops the sign extension of l2, as it must).
struct Fixed128 { long long hi; unsigned long long lo; };
CFMM_FX_HD Fixed128 fixed_combine(unsigned long long l0, unsigned long long l1, unsigned long long l2)
{
    typedef unsigned __int128 u128;
    const u128 t = ((u128)l2 << 64) + ((u128)l1 << 32) + (u128)l0;
    return {(long long)(unsigned long long)(t >> 64), (unsigned long long)t};
}

}  // namespace cfmm
