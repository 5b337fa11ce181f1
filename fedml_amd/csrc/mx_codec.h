// mx_codec.h -- the quantizer arithmetic of the Microscaling formats (include/fedagg_mx.h), on the bits
// of a float32 and in integers only, so that it rounds as the header's mathematics says on any
// processor: the shared exponent of a block from the bits of its amax, and an element's E4M3 / E2M1
// code.  Compiles as device code for mx.hip and as plain C++.  Not part of the ABI.
#pragma once

#include <cstdint>

#ifdef __HIPCC__
#define FA_MX_HD __host__ __device__ __forceinline__
#else
#define FA_MX_HD inline
#endif

namespace fa_detail {

// Per element format: mantissa bits, the exponent of the least normal value (the subnormals share
// its ulp), the exponent of the largest value, the largest finite magnitude's code, the sign's bit.
template <int FMT> struct MxFmt;
template <> struct MxFmt<0> { enum { MB = 3, QMIN = -6, EMAX = 8, MAXC = 0x7E, SB = 7 }; };  // E4M3
template <> struct MxFmt<1> { enum { MB = 1, QMIN = 0, EMAX = 2, MAXC = 0x7, SB = 3 }; };    // E2M1

FA_MX_HD int mx_msb(uint32_t m) { return 31 - __builtin_clz(m); }  // m != 0

// E = clamp(floor(log2 amax) - emax, -127, 127) from the bits of a finite amax >= 0; amax = 0: -127.
// A subnormal amax counts by its true exponent.  (The upper clamp never binds: E <= 127 - emax.)
template <int FMT>
FA_MX_HD int mx_shared_exp(uint32_t amax_bits) {
  const int ef = (int)(amax_bits >> 23);
  if (amax_bits == 0) return -127;
  const int fl = ef ? ef - 127 : mx_msb(amax_bits) - 149;
  const int e = fl - (int)MxFmt<FMT>::EMAX;
  return e < -127 ? -127 : e;
}

// The code of a finite x (its bits) in a block of shared exponent E: the sign, and the magnitude
// nearest to |x| / 2^E, ties to the even mantissa, saturated at the format's maximum.
// |x| = M * 2^(s + E) with an integer M < 2^24; q is the exponent of the result's binade, at least
// QMIN; the magnitude is round(M / 2^sh) ulps of 2^(q - MB).  Codes are monotone in the magnitude, so
// the binade's base code plus the rounded count carries into the next binade by itself.  sh >= 1
// always: a normal x has M's top bit at 23, so sh >= 23 - MB >= 20; a subnormal x has s = -149 - E <=
// -22 and lies below 2^QMIN, so q = QMIN and sh = QMIN - MB - s >= 13.  From sh = 25 on the count is 0,
// so sh is capped where the 32-bit arithmetic still holds.
template <int FMT>
FA_MX_HD uint32_t mx_code(uint32_t xbits, int E) {
  using F = MxFmt<FMT>;
  const uint32_t a = xbits & 0x7FFFFFFFu, ef = a >> 23;
  const uint32_t M = ef ? ((a & 0x7FFFFFu) | 0x800000u) : a;
  const int s = (int)(ef ? ef : 1u) - 150 - E;
  const int top = (M ? mx_msb(M) : 0) + s;
  const int q = top > (int)F::QMIN ? top : (int)F::QMIN;
  int sh = q - (int)F::MB - s;
  sh = sh > 31 ? 31 : sh;
  const uint32_t r = (M + ((1u << (sh - 1)) - 1u) + ((M >> sh) & 1u)) >> sh;  // ties to even
  uint32_t c = ((uint32_t)(q - (int)F::QMIN + 1) << F::MB) + r - (1u << F::MB);
  c = c > (uint32_t)F::MAXC ? (uint32_t)F::MAXC : c;
  return c | ((xbits >> 31) << F::SB);
}

}  // namespace fa_detail
