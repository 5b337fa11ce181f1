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
// Below them, on the same sorts, loads and store: the mean around the median (fa_coord_mean_around_median,
// fa_coord_mean_around_median_tiled; Bulyan's second stage) -- k_mam_off, k_mam_2l, k_mam_rank.
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

// ---------------------------------------------------------------------------------------------------
// Mean around the median (fa_coord_mean_around_median[_tiled]; Bulyan's second stage, El Mhamdi et al.
// 2018): per coordinate the mean of the `keep` values nearest to the lower median m = s[h],
// h = (k-1)/2 -- a window of `keep` consecutive ranks that holds h.  Its start (the header's step 4):
// lo = lomin + #{ r in [lomin, lomax) : dist(s[r]) > dist(s[r + keep]) }, lomin = max(0, h - keep + 1),
// lomax = min(h, k - keep), dist(v) = |(double)v - (double)m| (0 if v == m, +inf if v is NaN).  Then the
// trimmed mean's float64 walk over ranks lo .. lo + keep - 1 and its store.
//
// The fast paths hold m finite and no NaN (the float networks turn a column with a NaN all NaN, m
// included), where dist() is the plain float64 subtraction: v == m gives 0 and an infinite v gives
// +inf by themselves.  Every other column -- m not finite, or a NaN result -- goes to mam_col().

__device__ __forceinline__ double mam_dist(double v, double m) {
  return v == m ? 0.0 : (v != v ? (double)__builtin_inff() : __builtin_fabs(v - m));
}

// In-order path: a cursor over the column's ranks, by trimmed_col()'s repeated selection of the next
// (key, client index) -- K loads per step.  r: the rank of v, -1 before the first step.
struct RankCur {
  unsigned long long ck;
  int ci, r;
  double v;
};

template <int DT>
__device__ void rank_next(RankCur& cu, const void* const* in, int64_t ub, int64_t c, int k) {
  unsigned long long bk = 0;
  int bi = -1;
  double bv = 0.0;
  for (int j = 0; j < k; ++j) {
    const double v = load_d<DT>(at(in[j], ub), c);
    const unsigned long long kj = dkey(v);
    const bool after = cu.r < 0 || kj > cu.ck || (kj == cu.ck && j > cu.ci);
    if (after && (bi < 0 || kj < bk)) { bk = kj; bi = j; bv = v; }
  }
  cu.ck = bk;
  cu.ci = bi;
  cu.v = bv;
  ++cu.r;
}

// One column's result q by the header's steps, O(K^2) loads: the median, then two cursors `keep` ranks
// apart for the window's start, then the walk.
template <int DT>
__device__ double mam_col(const void* const* in, int64_t ub, int64_t c, int k, int keep) {
  const int h = (k - 1) / 2, lomin = max(0, h - keep + 1), lomax = min(h, k - keep);
  RankCur a{0, -1, -1, 0.0};
  while (a.r < h) rank_next<DT>(a, in, ub, c, k);
  const double m = a.v;
  if (m != m) return m;
  int lo = lomin;
  if (lomin < lomax) {
    RankCur p{0, -1, -1, 0.0}, q = a;  // lomin + keep > h: the upper cursor starts from the median's
    while (p.r < lomin) rank_next<DT>(p, in, ub, c, k);
    while (q.r < lomin + keep) rank_next<DT>(q, in, ub, c, k);
    for (int r = lomin;;) {
      lo += mam_dist(p.v, m) > mam_dist(q.v, m) ? 1 : 0;
      if (++r == lomax) break;
      rank_next<DT>(p, in, ub, c, k);
      rank_next<DT>(q, in, ub, c, k);
    }
  }
  RankCur s{0, -1, -1, 0.0};
  while (s.r < lo) rank_next<DT>(s, in, ub, c, k);
  double acc = s.v;
  for (int r = 1; r < keep; ++r) {
    rank_next<DT>(s, in, ub, c, k);
    acc = acc + s.v;
  }
  return acc / (double)keep;
}

// the column's result from the fast path's sum and median
template <int DT>
__device__ __forceinline__ void mam_finish(double acc, bool fast, const void* const* in, int64_t ub, int64_t c, int k,
                                           int keep, int64_t e, void* out) {
  double q = acc / (double)keep;
  if (!fast || q != q) q = mam_col<DT>(in, ub, c, k, keep);
  tm_store<DT>(out, e, q);
}

// rank r's share of the walk over ranks lo .. lo + keep - 1 (lo per lane): the value inside the window,
// -0.0 outside, which a float64 sum that starts at -0.0 passes through unchanged -- so the sum equals
// the header's, which starts FROM s[lo], bit for bit.
__device__ __forceinline__ double mam_term(float v, int r, int lo, int keep) {
  return (double)((unsigned)(r - lo) < (unsigned)keep ? v : -0.0f);
}

// One lane per coordinate, K <= 64: k_tmean_off's loads, sentinels and SortNet<B>; then the median (a
// uniform select over ranks < B/2), the partners y[r] = s[r + keep] by a uniform barrel shift of the
// sorted registers (bit_length(B-1) stages of moves under scalar conditions: a non-empty range has
// keep < k <= B), the count over r < h <= B/2 - 1 under the uniform range predicate, and the walk.
// No dynamic register index, no scratch for it.
template <int DT, int B, int W = (B > 56 ? 3 : (B > 32 ? 4 : 5))>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(W)))
k_mam_off(const MSeg* __restrict__ segs, int nseg, const void* const* __restrict__ ptrs, int k, int keep) {
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
  const int h = (k - 1) >> 1, lomin = max(0, h - keep + 1), lomax = min(h, k - keep);
  constexpr int R = B / 2 - 1;  // r < h <= B/2 - 1
  float m = x[0];
#pragma unroll
  for (int r = 1; r <= R; ++r) m = r == h ? x[r] : m;
  float y[B];
#pragma unroll
  for (int i = 0; i < B; ++i) y[i] = x[i];
#pragma unroll
  for (int s = 1; s < B; s <<= 1) {
    const bool on = (keep & s) != 0;
#pragma unroll
    for (int i = 0; i < B; ++i) y[i] = on ? (i + s < B ? y[i + s] : __builtin_inff()) : y[i];
  }
  const double dm = (double)m;
  int lo = lomin;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const bool gt = __builtin_fabs((double)x[r] - dm) > __builtin_fabs((double)y[r] - dm);
    lo += (r >= lomin && r < lomax && gt) ? 1 : 0;
  }
  double acc = -0.0;
#pragma unroll
  for (int r = 0; r < B; ++r) acc = acc + mam_term(x[r], r, lo, keep);
  if (!live) return;
  mam_finish<DT>(acc, __builtin_fabsf(m) < __builtin_inff(), in, ub, e - e0, k, keep, e, sg.out);
}

// Two lanes per coordinate, K in (64, 128]: k_tmean_2l through the mergers (the lower lane then holds
// ranks 0 .. N-1, the upper ranks N .. 2N-1).  k > 2N - 8, so the median rank h is one of N-4 .. N-1,
// in the lower lane, and every partner rank r + keep >= h + 1 >= N - 3.  Once every upper lane has
// read its keys back (a barrier: the table's layout differs from the exchange buffer's it reuses), the
// ranks N-4 .. 2N-1 are published as fl[rank - (N-4)][column] -- the lower lane its last four keys, the
// upper lane all of its own; consecutive lanes on consecutive banks -- and the lower lane reads each
// partner at a uniform row.  It counts, sums its part of the window and hands the running float64 and
// lo (-1: the median is not finite) to the upper lane through LDS, which continues in rank order and
// stores.  Five barriers; no lane leaves before the last.
template <int DT, int N>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(N > 40 ? 4 : 5)))
k_mam_2l(const MSeg* __restrict__ segs, int nseg, const void* const* __restrict__ ptrs, int k, int keep) {
  __shared__ u32x4 xs[N / 4 + 1][kTm2lCols];  // the exchange buffer, then the table of N + 4 ranks
  __shared__ double accs[kTm2lCols];
  __shared__ int los[kTm2lCols];
  const int hf = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kTm2lCols);  // half: wave-uniform
  const int c = (int)threadIdx.x % kTm2lCols;
  const int64_t tile = blockIdx.x;
  const MSeg sg = segs[nseg > 1 ? find_seg(segs, nseg, tile) : 0];
  const int64_t e0 = (tile - sg.tile_start) * kTm2lCols, e = e0 + c;
  const bool live = e < sg.numel;
  const int64_t ec = live ? e : sg.numel - 1;
  const void* const* in = ptrs + sg.ptr_base;
  const int64_t ub = col_base<MedT<DT>::kBytes>(e0, sg.tstride);
  const unsigned boff = (unsigned)(ec - e0) * (unsigned)MedT<DT>::kBytes;
  const int base = N * hf;
  float x[N];
#pragma unroll
  for (int t = 0; t < N; ++t) x[t] = MedT<DT>::load_off(at(in[min(base + t, k - 1)], ub), boff);
#pragma unroll
  for (int t = N - 8; t < N; ++t) x[t] = base + t < k ? x[t] : __builtin_inff();  // k > 2N - 8: upper half only
  SortNet<N>::run(x);  // a NaN input turns every sorted output NaN
  if (hf == 1) {
#pragma unroll
    for (int q = 0; q < N / 4; ++q)
      xs[q][c] = u32x4{__float_as_uint(x[4 * q]), __float_as_uint(x[4 * q + 1]), __float_as_uint(x[4 * q + 2]),
                       __float_as_uint(x[4 * q + 3])};
  }
  __syncthreads();
  if (hf == 0) {
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
  if (hf == 0) {
    BitonicLo<N>::run(x);  // ranks 0 .. N-1
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
  __syncthreads();  // every read of the exchange buffer is done
  float* fl = (float*)xs;  // [N + 4][kTm2lCols]: ranks N-4 .. 2N-1
  if (hf == 0) {
#pragma unroll
    for (int t = 0; t < 4; ++t) fl[t * kTm2lCols + c] = x[N - 4 + t];
  } else {
#pragma unroll
    for (int t = 0; t < N; ++t) fl[(4 + t) * kTm2lCols + c] = x[t];
  }
  __syncthreads();
  if (hf == 0) {
    const int h = (k - 1) >> 1, lomin = max(0, h - keep + 1), lomax = min(h, k - keep);
    float m = x[N - 4];
#pragma unroll
    for (int r = N - 3; r < N; ++r) m = r == h ? x[r] : m;
    const double dm = (double)m;
    int lo = lomin;
#pragma unroll
    for (int r = 0; r < N - 1; ++r) {  // r < h <= N - 1
      if (r >= lomin && r < lomax) {  // uniform: a branch, so only the range's partners are read
        const float p = fl[(r + keep - (N - 4)) * kTm2lCols + c];  // row in [1, N + 3]
        lo += __builtin_fabs((double)x[r] - dm) > __builtin_fabs((double)p - dm) ? 1 : 0;
      }
    }
    double acc = -0.0;
#pragma unroll
    for (int r = 0; r < N; ++r) acc = acc + mam_term(x[r], r, lo, keep);
    accs[c] = acc;
    los[c] = __builtin_fabsf(m) < __builtin_inff() ? lo : -1;
  }
  __syncthreads();
  if (hf == 0 || !live) return;
  double acc = accs[c];
  const int lo = los[c];
#pragma unroll
  for (int r = 0; r < N; ++r) acc = acc + mam_term(x[r], N + r, lo, keep);
  mam_finish<DT>(acc, lo >= 0, in, ub, e - e0, k, keep, e, sg.out);
}

// Any K, and float64: the in-order path for every column.
template <int DT>
__global__ void __launch_bounds__(kBlock)
k_mam_rank(const MSeg* __restrict__ segs, int nseg, const void* const* __restrict__ ptrs, int k, int keep) {
  const int64_t tile = blockIdx.x;
  const MSeg sg = segs[nseg > 1 ? find_seg(segs, nseg, tile) : 0];
  const int64_t e0 = (tile - sg.tile_start) * kBlock, e = e0 + threadIdx.x;
  if (e >= sg.numel) return;
  const void* const* in = ptrs + sg.ptr_base;
  const int64_t ub = col_base<elem_bytes<DT>()>(e0, sg.tstride);
  tm_store<DT>(sg.out, e, mam_col<DT>(in, ub, e - e0, k, keep));
}

template <int DT>
void launch_mam(int k, int keep, dim3 grid, hipStream_t st, const MSeg* ds, int nseg, const void* const* dp) {
  if constexpr (DT != FA_DTYPE_F64) {
    switch ((k + 7) / 8) {  // as launch_tmean
#define FA_M1(Q) \
  case Q: hipLaunchKernelGGL((k_mam_off<DT, 8 * Q>), grid, dim3(kBlock), 0, st, ds, nseg, dp, k, keep); return;
#define FA_M2(Q) \
  case Q: hipLaunchKernelGGL((k_mam_2l<DT, 4 * Q>), grid, dim3(kBlock), 0, st, ds, nseg, dp, k, keep); return;
      FA_M1(1) FA_M1(2) FA_M1(3) FA_M1(4) FA_M1(5) FA_M1(6) FA_M1(7) FA_M1(8)
      FA_M2(9) FA_M2(10) FA_M2(11) FA_M2(12) FA_M2(13) FA_M2(14) FA_M2(15) FA_M2(16)
#undef FA_M1
#undef FA_M2
      default: break;
    }
  }
  hipLaunchKernelGGL((k_mam_rank<DT>), grid, dim3(kBlock), 0, st, ds, nseg, dp, k, keep);
}

int mam_impl(const ColArgs& a, int32_t keep) {
  if (const int rc = col_check_args(a)) return rc;
  const int k = a.k;
  if (keep < 1 || keep > k)
    return fail(FA_ERR_INVALID, "%s: keep must satisfy 1 <= keep <= k (keep %d, k %d)", a.fn, keep, k);
  return col_launch(a, tmean_lanes(a.dtype, k) == 2 ? kTm2lCols : kBlock,
                    [&](dim3 grid, hipStream_t st, const MSeg* ds, int nseg, const void* const* dp) {
                      switch (a.dtype) {
                        case FA_DTYPE_F32: launch_mam<FA_DTYPE_F32>(k, keep, grid, st, ds, nseg, dp); break;
                        case FA_DTYPE_BF16: launch_mam<FA_DTYPE_BF16>(k, keep, grid, st, ds, nseg, dp); break;
                        case FA_DTYPE_F16: launch_mam<FA_DTYPE_F16>(k, keep, grid, st, ds, nseg, dp); break;
                        default: launch_mam<FA_DTYPE_F64>(k, keep, grid, st, ds, nseg, dp); break;
                      }
                    });
}

}  // namespace

extern "C" {

int fa_coord_mean_around_median(fa_ctx* ctx, int dtype, int32_t num_segments, const int64_t* seg_numel, int32_t k,
                                int32_t keep, const void* const* d_in, void* const* d_out, void* hip_stream) {
  return mam_impl({"fa_coord_mean_around_median", ctx, dtype, num_segments, seg_numel, k, d_in, 0, d_out, hip_stream},
                  keep);
}

int fa_coord_mean_around_median_tiled(fa_ctx* ctx, int dtype, int32_t num_segments, const int64_t* seg_numel,
                                      int32_t k, int32_t keep, const void* const* d_in, int64_t tile_stride,
                                      void* const* d_out, void* hip_stream) {
  if (ctx && tile_stride <= 0)
    return fail(FA_ERR_INVALID, "fa_coord_mean_around_median_tiled: tile_stride must be > 0");
  return mam_impl({"fa_coord_mean_around_median_tiled", ctx, dtype, num_segments, seg_numel, k, d_in, tile_stride,
                   d_out, hip_stream},
                  keep);
}

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
