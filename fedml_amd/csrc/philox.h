// philox.h -- the one device copy of the counter-based generator's block function (include/fedagg_dp.h
// states the words), shared by the noise kernels (noise.hip) and the randomized Hadamard rotation's
// signs (hadamard.hip).  Not part of the ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "fa_internal.h"

namespace fa_detail {

// Philox4x32-10 of counter (lo32(b), hi32(b), seg, round) under key (k0, k1).
__device__ __forceinline__ u32x4 noise_block(uint32_t k0, uint32_t k1, uint64_t b, uint32_t seg, uint32_t round) {
  constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
  uint32_t c0 = (uint32_t)b, c1 = (uint32_t)(b >> 32), c2 = seg, c3 = round;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(M0, c0), lo0 = M0 * c0;
    const uint32_t hi1 = __umulhi(M1, c2), lo1 = M1 * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += W0;
    k1 += W1;
  }
  return u32x4{c0, c1, c2, c3};
}

}  // namespace fa_detail
