// trimmed.hip -- MI355X (gfx950) kernels + C ABI of the coordinate-wise trimmed mean
// (include/fedagg_robust.h: fa_coord_trimmed_mean, fa_coord_trimmed_mean_tiled; Yin et al. 2018).
//
// Per coordinate: sort the K client values ascending (-0.0 below +0.0, NaN above +inf), drop the b
// smallest and b largest, sum the rest in rank order in float64 starting FROM the first kept value,
// divide by K - 2b, round once to float32 (and once more to bf16 / f16).  The sum's order is part of
// the contract: a float64 sum of float32 values is not always exact.
//
// Same family as the median kernels (median.hip), whose helpers (median_common.h), host path
// (median_host.h), sorting networks (median_nets.h) and addressing it shares; here the network is a
// FULL sort, since every kept rank is needed.  The float networks run on IEEE 754-2019 minimum / maximum: -0 < +0, and one NaN turns every
// output NaN -- so a NaN result (a NaN in the column, or +inf and -inf both kept) sends that column to
// the in-order path trimmed_col(), which places NaNs as the largest values.
//   K <= 64          k_tmean_off: one lane per coordinate, B = K rounded up to 8 keys in registers
//   K in (64, 128]   k_tmean_2l:  two lanes per coordinate, N = B/2 keys each, exchange through LDS
//   K > 128, float64 k_tmean_rank: trimmed_col() for every column (correct, not fast)
#include <hip/hip_runtime.h>

#include <cstdint>

#include "fa_internal.h"
#include "fedagg_robust.h"
#include "median_common.h"
#include "median_host.h"
#include "trimmed_nets.h"

using namespace fa_detail;

namespace {

// q -> out[e]: float64 as is; float32 one rounding; bf16 / f16 float64 -> float32 -> 16 bits, each
// round-to-nearest-even (what torch's q.to(float32).to(dtype) does)
template <int DT>
__device__ __forceinline__ void tm_store(void* out, int64_t e, double q) {
  if constexpr (DT == FA_DTYPE_F64) {
    ((double*)out)[e] = q;
  } else if constexpr (DT == FA_DTYPE_F32) {
    ((float*)out)[e] = (float)q;
  } else if constexpr (DT == FA_DTYPE_BF16) {
    const float f = (float)q;
    const unsigned u = __float_as_uint(f);
    ((unsigned short*)out)[e] = f != f ? (unsigned short)0x7FC0 : (unsigned short)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
  } else {
    ((unsigned short*)out)[e] = __builtin_bit_cast(unsigned short, (_Float16)(float)q);
  }
}

// Total order of a column's values as a 64-bit key: numeric order on non-NaN values, -0.0 just below
// +0.0, every NaN (any sign or payload) the largest key.  (The uint32 fkey alone would put a
// negative-signed NaN below -inf.)
__device__ __forceinline__ unsigned long long dkey(double x) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(x);
  return x != x ? ~0ull : u ^ ((unsigned long long)((long long)u >> 63) | 0x8000000000000000ull);
}

// In-order path: the kept ranks' float64 sum of one column, by repeated selection of the next
// (key, client index) after the last one taken -- (K - b) passes over the K values, O(K^2) loads.
// Equal keys are taken in client order (they are equal values, or NaNs, so the sum does not depend on
// it).  Client j's element: at(in[j], ub) + c elements.
template <int DT>
__device__ double trimmed_col(const void* const* in, int64_t ub, int64_t c, int k, int b) {
  unsigned long long ck = 0;
  int ci = -1;
  double acc = 0.0;
  for (int r = 0; r < k - b; ++r) {
    unsigned long long bk = 0;
    int bi = -1;
    double bv = 0.0;
    for (int j = 0; j < k; ++j) {
      const double v = load_d<DT>(at(in[j], ub), c);
      const unsigned long long kj = dkey(v);
      const bool after = r == 0 || kj > ck || (kj == ck && j > ci);
      if (after && (bi < 0 || kj < bk)) { bk = kj; bi = j; bv = v; }
    }
    ck = bk;
    ci = bi;
    if (r == b) acc = bv;
    else if (r > b) acc = acc + bv;
  }
  return acc;
}

// the column's result from the fast path's sum; NaN -> the in-order path decides
template <int DT>
__device__ __forceinline__ void tm_finish(double acc, const void* const* in, int64_t ub, int64_t c, int k, int b,
                                          int64_t e, void* out) {
  const double cnt = (double)(k - 2 * b);
  double q = acc / cnt;
  if (q != q) q = trimmed_col<DT>(in, ub, c, k, b) / cnt;
  tm_store<DT>(out, e, q);
}

// One lane per coordinate, K <= 64 (k_median_off's structure): the column's K pointers (scalar
// loads), all B element loads (clamped, unconditional, SGPR base + one shared 32-bit offset) before any
// is consumed; slots [k, B) become +inf sentinels, which land above every real rank; SortNet<B>; then
// the float64 walk over x[b .. k-1-b], branch-free over the unrolled registers (b, k are uniform:
// every step is a select).  b <= (k-1)/2 < (B+1)/2, so the first-value select stops there.
template <int DT, int B, int W = (B > 56 ? 3 : (B > 32 ? 4 : 5))>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(W)))
k_tmean_off(const MSeg* __restrict__ segs, int nseg, const void* const* __restrict__ ptrs, int k, int b) {
  const int64_t tile = blockIdx.x;
  const MSeg sg = segs[nseg > 1 ? find_seg(segs, nseg, tile) : 0];
  const int64_t e0 = (tile - sg.tile_start) * kBlock, e = e0 + threadIdx.x;
  const bool live = e < sg.numel;
  const int64_t ec = live ? e : sg.numel - 1;
  const void* const* in = ptrs + sg.ptr_base;
  const int64_t ub = col_base<MedT<DT>::kBytes>(e0, sg.tstride);
  const unsigned boff = (unsigned)(ec - e0) * (unsigned)MedT<DT>::kBytes;
  float x[B];
#pragma unroll
  for (int i = 0; i < B; ++i) x[i] = MedT<DT>::load_off(at(in[min(i, k - 1)], ub), boff);
#pragma unroll
  for (int i = B - 8; i < B; ++i) x[i] = i < k ? x[i] : __builtin_inff();  // k > B - 8
  SortNet<B>::run(x);  // a NaN input turns every output NaN
  const int ke = k - b;
  double acc = 0.0;
#pragma unroll
  for (int r = 0; r < B; ++r) {
    const double v = (double)x[r];
    if (r < (B + 1) / 2) acc = r == b ? v : (r > b && r < ke ? acc + v : acc);
    else acc = r < ke ? acc + v : acc;
  }
  if (!live) return;
  tm_finish<DT>(acc, in, ub, e - e0, k, b, e, sg.out);
}

// Two lanes per coordinate, K in (64, 128] (k_median_2l's structure): waves 0-1 of the workgroup hold
// clients 0..N-1 of 128 columns, waves 2-3 clients N..2N-1 (B = 2N = K rounded up to 8; +inf sentinels
// in the upper half's last slots).  Each lane sorts its N keys (A below, C above).  The upper lanes
// put C in LDS; the lower lane forms, for every j, lo = min(A[j], C[N-1-j]) (kept in A[j]'s register:
// the column's N smallest keys, an up-then-down sequence) and hi = max(A[j], C[N-1-j]) (written back
// over C[N-1-j]: the N largest, down-then-up in C's index), so ONE N x 512 B buffer serves both
// directions.  Both lanes then sort their N keys with a bitonic merger in registers (trimmed_nets.h).
// The lower lane sums its kept ranks -- rank b, where the sum starts, is always below N -- and hands the
// running float64 to the upper lane through LDS, which continues over ranks N .. k-1-b and stores.
// Three barriers; no lane leaves before the last.
constexpr int kTm2lCols = kBlock / 2;  // columns per workgroup
template <int DT, int N>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(N > 40 ? 4 : 5)))
k_tmean_2l(const MSeg* __restrict__ segs, int nseg, const void* const* __restrict__ ptrs, int k, int b) {
  __shared__ u32x4 xs[N / 4][kTm2lCols];
  __shared__ double accs[kTm2lCols];
  const int h = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kTm2lCols);  // half: wave-uniform
  const int c = (int)threadIdx.x % kTm2lCols;
  const int64_t tile = blockIdx.x;
  const MSeg sg = segs[nseg > 1 ? find_seg(segs, nseg, tile) : 0];
  const int64_t e0 = (tile - sg.tile_start) * kTm2lCols, e = e0 + c;
  const bool live = e < sg.numel;
  const int64_t ec = live ? e : sg.numel - 1;
  const void* const* in = ptrs + sg.ptr_base;
  const int64_t ub = col_base<MedT<DT>::kBytes>(e0, sg.tstride);
  const unsigned boff = (unsigned)(ec - e0) * (unsigned)MedT<DT>::kBytes;
  const int base = N * h;
  float x[N];
#pragma unroll
  for (int t = 0; t < N; ++t) x[t] = MedT<DT>::load_off(at(in[min(base + t, k - 1)], ub), boff);
#pragma unroll
  for (int t = N - 8; t < N; ++t) x[t] = base + t < k ? x[t] : __builtin_inff();  // k > 2N - 8: upper half only
  SortNet<N>::run(x);  // a NaN input turns every sorted output NaN
  if (h == 1) {
#pragma unroll
    for (int q = 0; q < N / 4; ++q)
      xs[q][c] = u32x4{__float_as_uint(x[4 * q]), __float_as_uint(x[4 * q + 1]), __float_as_uint(x[4 * q + 2]),
                       __float_as_uint(x[4 * q + 3])};
  }
  __syncthreads();
  if (h == 0) {
#pragma unroll
    for (int q = 0; q < N / 4; ++q) {
      const u32x4 cq = xs[q][c];
      const float c0 = __uint_as_float(cq.x), c1 = __uint_as_float(cq.y), c2 = __uint_as_float(cq.z),
                  c3 = __uint_as_float(cq.w);
      const float a0 = x[N - 1 - 4 * q], a1 = x[N - 2 - 4 * q], a2 = x[N - 3 - 4 * q], a3 = x[N - 4 - 4 * q];
      x[N - 1 - 4 * q] = kmin(a0, c0);
      x[N - 2 - 4 * q] = kmin(a1, c1);
      x[N - 3 - 4 * q] = kmin(a2, c2);
      x[N - 4 - 4 * q] = kmin(a3, c3);
      xs[q][c] = u32x4{__float_as_uint(kmax(a0, c0)), __float_as_uint(kmax(a1, c1)), __float_as_uint(kmax(a2, c2)),
                       __float_as_uint(kmax(a3, c3))};
    }
  }
  __syncthreads();
  const int ke = k - b;
  if (h == 0) {
    BitonicLo<N>::run(x);  // ranks 0 .. N-1
    double acc = 0.0;
#pragma unroll
    for (int r = 0; r < N; ++r) {
      const double v = (double)x[r];
      acc = r == b ? v : (r > b && r < ke ? acc + v : acc);
    }
    accs[c] = acc;
  } else {
#pragma unroll
    for (int q = 0; q < N / 4; ++q) {
      const u32x4 cq = xs[q][c];
      x[4 * q] = __uint_as_float(cq.x);
      x[4 * q + 1] = __uint_as_float(cq.y);
      x[4 * q + 2] = __uint_as_float(cq.z);
      x[4 * q + 3] = __uint_as_float(cq.w);
    }
    BitonicHi<N>::run(x);  // ranks N .. 2N-1
  }
  __syncthreads();
  if (h == 0 || !live) return;
  double acc = accs[c];
#pragma unroll
  for (int r = 0; r < N; ++r) acc = N + r < ke ? acc + (double)x[r] : acc;
  tm_finish<DT>(acc, in, ub, e - e0, k, b, e, sg.out);
}

// Any K, and float64: the in-order path for every column.
template <int DT>
__global__ void __launch_bounds__(kBlock)
k_tmean_rank(const MSeg* __restrict__ segs, int nseg, const void* const* __restrict__ ptrs, int k, int b) {
  const int64_t tile = blockIdx.x;
  const MSeg sg = segs[nseg > 1 ? find_seg(segs, nseg, tile) : 0];
  const int64_t e0 = (tile - sg.tile_start) * kBlock, e = e0 + threadIdx.x;
  if (e >= sg.numel) return;
  const void* const* in = ptrs + sg.ptr_base;
  const int64_t ub = col_base<elem_bytes<DT>()>(e0, sg.tstride);
  const double acc = trimmed_col<DT>(in, ub, e - e0, k, b);
  tm_store<DT>(sg.out, e, acc / (double)(k - 2 * b));
}

// lanes per column: 2 for K in (64, 128] (not float64), else 1
int tmean_lanes(int dtype, int k) { return dtype != FA_DTYPE_F64 && k > 64 && k <= 128 ? 2 : 1; }

template <int DT>
void launch_tmean(int k, int b, dim3 grid, hipStream_t st, const MSeg* ds, int nseg, const void* const* dp) {
  if constexpr (DT != FA_DTYPE_F64) {
    switch ((k + 7) / 8) {  // B = K rounded up to 8; two lanes: N = B / 2 keys per lane
#define FA_T1(Q) \
  case Q: hipLaunchKernelGGL((k_tmean_off<DT, 8 * Q>), grid, dim3(kBlock), 0, st, ds, nseg, dp, k, b); return;
#define FA_T2(Q) \
  case Q: hipLaunchKernelGGL((k_tmean_2l<DT, 4 * Q>), grid, dim3(kBlock), 0, st, ds, nseg, dp, k, b); return;
      FA_T1(1) FA_T1(2) FA_T1(3) FA_T1(4) FA_T1(5) FA_T1(6) FA_T1(7) FA_T1(8)
      FA_T2(9) FA_T2(10) FA_T2(11) FA_T2(12) FA_T2(13) FA_T2(14) FA_T2(15) FA_T2(16)
#undef FA_T1
#undef FA_T2
      default: break;
    }
  }
  hipLaunchKernelGGL((k_tmean_rank<DT>), grid, dim3(kBlock), 0, st, ds, nseg, dp, k, b);
}

int tmean_impl(const ColArgs& a, int32_t trim) {
  if (const int rc = col_check_args(a)) return rc;
  const int k = a.k;
  if (trim < 0 || 2 * (int64_t)trim >= k)
    return fail(FA_ERR_INVALID, "%s: trim must satisfy 0 <= trim and 2 * trim < k (trim %d, k %d)", a.fn, trim, k);
  return col_launch(a, tmean_lanes(a.dtype, k) == 2 ? kTm2lCols : kBlock,
                    [&](dim3 grid, hipStream_t st, const MSeg* ds, int nseg, const void* const* dp) {
                      switch (a.dtype) {
                        case FA_DTYPE_F32: launch_tmean<FA_DTYPE_F32>(k, trim, grid, st, ds, nseg, dp); break;
                        case FA_DTYPE_BF16: launch_tmean<FA_DTYPE_BF16>(k, trim, grid, st, ds, nseg, dp); break;
                        case FA_DTYPE_F16: launch_tmean<FA_DTYPE_F16>(k, trim, grid, st, ds, nseg, dp); break;
                        default: launch_tmean<FA_DTYPE_F64>(k, trim, grid, st, ds, nseg, dp); break;
                      }
                    });
}

}  // namespace

extern "C" {

int fa_coord_trimmed_mean(fa_ctx* ctx, int dtype, int32_t num_segments, const int64_t* seg_numel, int32_t k,
                          int32_t trim, const void* const* d_in, void* const* d_out, void* hip_stream) {
  return tmean_impl({"fa_coord_trimmed_mean", ctx, dtype, num_segments, seg_numel, k, d_in, 0, d_out, hip_stream}, trim);
}

int fa_coord_trimmed_mean_tiled(fa_ctx* ctx, int dtype, int32_t num_segments, const int64_t* seg_numel, int32_t k,
                                int32_t trim, const void* const* d_in, int64_t tile_stride, void* const* d_out,
                                void* hip_stream) {
  if (ctx && tile_stride <= 0) return fail(FA_ERR_INVALID, "fa_coord_trimmed_mean_tiled: tile_stride must be > 0");
  return tmean_impl({"fa_coord_trimmed_mean_tiled", ctx, dtype, num_segments, seg_numel, k, d_in, tile_stride, d_out,
                     hip_stream},
                    trim);
}

}  // extern "C"
