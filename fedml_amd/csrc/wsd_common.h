// wsd_common.h -- the reduction shared by the fused sum-and-squared-distance kernels (wsum_dist.hip:
// float tensors; quant_dist.hip: block-quantized int8 tensors): a lane's float64 partial summed over its
// 16-lane DPP row, the workgroup's row sums added in row order into its row of the caller's scratch, and
// k_wsd_reduce, which adds the workgroups' rows in a fixed order.  No floating-point atomics anywhere, so
// the same call gives the same bits.  Every translation unit that includes this gets its own copy of the
// kernel (anonymous namespace).  Not part of the ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "fa_internal.h"

namespace fa_detail {
namespace {

constexpr int kKB = 128;  // clients per pass of phase 2 (the LDS block of wave sums)
constexpr int kRows = kBlock / 16;  // 16-lane DPP rows per workgroup

// Sum over the lane's 16-lane row, left in every lane of the row: four DPP exchanges (xor 1, xor 2 by
// quad_perm, then row_half_mirror and row_mirror), plain VALU, in a fixed order.  The rows of a wave
// are NOT combined here (that would take cross-row permutes through the LDS crossbar, and a wait
// each): the row leaders store to LDS and the workgroup's 16 row sums are added in row order.
template <int CTRL>
__device__ __forceinline__ double dpp_add(double v) {
  const u32x2 b = __builtin_bit_cast(u32x2, v);
  const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)b[0], CTRL, 0xF, 0xF, true);
  const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)b[1], CTRL, 0xF, 0xF, true);
  return v + __builtin_bit_cast(double, u32x2{lo, hi});
}
__device__ __forceinline__ double row_sum(double v) {
  v = dpp_add<0xB1>(v);   // quad_perm [1, 0, 3, 2]
  v = dpp_add<0x4E>(v);   // quad_perm [2, 3, 0, 1]
  v = dpp_add<0x141>(v);  // row_half_mirror
  v = dpp_add<0x140>(v);  // row_mirror
  return v;
}

// the workgroup's row sums of clients [b0, b0 + bn) -> its row of partials, rows added in row order
__device__ __forceinline__ void flush_rows(double (&red)[kRows][2 * kKB], int b0, int bn, int k,
                                           double* __restrict__ part) {
  __syncthreads();
  for (int t = (int)threadIdx.x; t < 2 * kKB; t += kBlock) {
    const int i = b0 + (t < kKB ? t : t - kKB);
    if (i < b0 + bn) {
      double s = red[0][t];
#pragma unroll
      for (int w = 1; w < kRows; ++w) s += red[w][t];
      part[t < kKB ? i : k + i] = s;
    }
  }
  __syncthreads();
}

// stats[e] = the sum over the chunks' rows of partial[row][e] in a fixed order (k_gram_reduce's
// split, robust.hip): a workgroup of 16 waves takes 16 consecutive entries and splits the rows 64
// ways (128-byte row reads, each lane its rows in row order), then one lane per entry adds the 64
// split sums in split order through LDS.
constexpr int kRW = 16, kRE = 16, kRS = kRW * 64 / kRE;
__global__ void __launch_bounds__(64 * kRW)
k_wsd_reduce(const double* __restrict__ partial, int64_t nparts, int n2k, double* __restrict__ stats) {
  __shared__ double red[kRW * 64];
  const int el = threadIdx.x % kRE, rs = threadIdx.x / kRE;
  const int e = blockIdx.x * kRE + el;
  const bool on = e < n2k;
  const int ec = on ? e : n2k - 1;
  double s = 0.0;
  int64_t b = rs;
  for (; b + 7 * kRS < nparts; b += 8 * kRS) {  // 8 loads in flight, added in row order
    double x[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) x[u] = partial[(b + u * kRS) * n2k + ec];
#pragma unroll
    for (int u = 0; u < 8; ++u) s += x[u];
  }
  for (; b < nparts; b += kRS) s += partial[b * n2k + ec];
  red[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x < kRE && on) {
    double t = 0.0;
    for (int u = 0; u < kRS; ++u) t += red[u * kRE + threadIdx.x];
    stats[e] = t;
  }
}

// the 2k sums of `tiles` workgroups' rows of `part` -> d_stats, behind the kernel that wrote them
inline void wsd_reduce_launch(hipStream_t st, const double* part, int64_t tiles, int k, void* d_stats) {
  hipLaunchKernelGGL(k_wsd_reduce, dim3((unsigned)((2 * k + kRE - 1) / kRE)), dim3(64 * kRW), 0, st, part, tiles, 2 * k,
                     (double*)d_stats);
}

}  // namespace
}  // namespace fa_detail
