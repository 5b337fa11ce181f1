// median.hip -- MI355X (gfx950) kernels + C ABI of the coordinate-wise median over the clients
// (include/fedagg_robust.h: fa_coord_median, fa_coord_median_tiled).
//
// torch.median over the client axis is a SELECTION, so the result is one of the inputs, bit for bit.  One lane owns one coordinate: it loads the K client
// values (all loads in flight at once), maps them to order-preserving uint32 keys (unsigned order
// == numeric order, -0.0 just below +0.0), pads to B = K rounded up to 8 with low/high sentinels
// that put the lower median at rank (B-1)/2, and selects that rank with a pruned odd-even merge
// network (median_nets.h: 283 min/max for B = 32, 1,233 for B = 72, 2,299 for B = 128, vs 480 /
// 3,584 / 3,584 for a full bitonic sort of the next power of two).  ATen's exact rules are kept: a NaN
// anywhere in the column returns the FIRST NaN; among equal values the client index decides, which only matters for +-0 -- both cases (a NaN
// seen, or a zero selected) take a short in-order rescan of the column.
// K <= 128 runs the network; larger K and float64 a rank-counting kernel (O(K^2) per coordinate).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>

#include "fa_internal.h"
#include "fedagg_robust.h"
#include "median_common.h"
#include "median_host.h"
#include "median_nets.h"

using namespace fa_detail;

namespace {

// gld / gld_nt / gld_nt_off, MedT, fkey, MSeg, col_base, at: median_common.h (shared with trimmed.hip)

// Rare cases, resolved by an in-order rescan of the column: a NaN anywhere -> ATen returns the
// FIRST NaN; a zero selected -> the selected rank r falls in the block of (equal) zeros, which ATen
// orders by client index -> the (r - #negatives)-th zero in client order.
// Client i's element of this lane: at(in[i], ub) + boff (col_base); the result goes to out[e].
template <int DT>
__device__ __forceinline__ void store_rare(const void* const* in, int64_t ub, unsigned boff, int k, int64_t e, int r,
                                           bool nan, void* out) {
  if (nan) {
    for (int i = 0; i < k; ++i) {
      const float x = MedT<DT>::load_off(at(in[i], ub), boff);
      if (x != x) { MedT<DT>::store_bits_off(out, e, at(in[i], ub), boff); return; }
    }
  }
  int negc = 0;
  for (int i = 0; i < k; ++i) negc += MedT<DT>::load_off(at(in[i], ub), boff) < 0.0f;
  int seen = 0;
  for (int i = 0; i < k; ++i) {
    const float x = MedT<DT>::load_off(at(in[i], ub), boff);
    if (x == 0.0f) {
      if (seen == r - negc) { MedT<DT>::store_bits_off(out, e, at(in[i], ub), boff); return; }
      ++seen;
    }
  }
}

// One coordinate in uint32 keys (k_median_pk's odd last coordinate).  Loads: the column's K client
// pointers first (scalar loads), then all B element loads (clamped, unconditional) before any is
// consumed.  Keys: the K real keys, then
// L = (B-1)/2 - (K-1)/2 low sentinels (0, below every non-NaN key) and high sentinels
// (0xFFFFFFFF) for the rest, so the lower median of the reals is rank (B-1)/2 of all B keys --
// which the pruned network select_mid<B> (median_nets.h) computes.  B = K rounded up to 8.
template <int DT, int B>
__device__ __forceinline__ void median_col(const void* const* in, int64_t ub, unsigned boff, int k, int64_t e,
                                           bool live, void* out) {
  const void* p[B];
#pragma unroll
  for (int i = 0; i < B; ++i) p[i] = at(in[min(i, k - 1)], ub);
  float x[B];
#pragma unroll
  for (int i = 0; i < B; ++i) x[i] = MedT<DT>::load_off(p[i], boff);  // clamped: every load unconditional
  const int lo_end = k + (B - 1) / 2 - ((k - 1) >> 1);          // sentinels [k, lo_end) are low
  unsigned key[B];
  bool nan = false;
#pragma unroll
  for (int i = 0; i < B; ++i) {
    nan = nan || (i < k && x[i] != x[i]);
    key[i] = i < k ? fkey(x[i]) : (i < lo_end ? 0u : 0xFFFFFFFFu);
  }
  const unsigned kr = select_mid<B>(key);
  if (!live) return;
  const int r = (k - 1) >> 1;
  if (nan || kr == kPosZeroKey || kr == kNegZeroKey) store_rare<DT>(in, ub, boff, k, e, r, nan, out);
  else MedT<DT>::store(out, e, fkey_inv(kr));
}

// Branch-free form (r02), for every segment size: median_col's form, as a whole kernel, compiled
// `i < k ? key : sentinel` and `nan || ...` (k a runtime value) into an exec-mask branch with its
// own s_waitcnt per client -- ~3,000 scalar and branch instructions ahead of B = 128's 2,175
// min/max -- and kept a 64-bit VGPR address per client (B = 128: 158 VGPRs).  Here the sentinels are
// uniform selects (no branch) and every load is `uniform base (SGPRs) + ONE shared 32-bit byte offset` (global_load ... saddr).  Measured (r02j): K = 128 1.58 -> 1.45 ms,
// K = 96 1.11 -> 0.88, K = 64 0.62 -> 0.59, K = 32 0.278 -> 0.272 ms; bit-exact (same network).
// EXACT (k == B, no sentinels): the selects are dropped at compile time (K = 128: 1.53 -> 1.45 ms).
// Float keys (r03): the network runs on the loaded floats with IEEE 754-2019 minimum / maximum
// (median_nets.h, v_minimum3_f32 / v_maximum3_f32): their order is the uint32 keys' order on every
// non-NaN value (-0 < +0 included), so the same bits are selected, and a NaN anywhere in the column
// makes the selected value NaN (every input reaches the selected output) -- no per-key conversion
// or NaN test (5-6 VALU a key in the uint32-key form, commit 9aaf2ea).  Sentinels are -inf / +inf (a
// tie with a real infinity selects the same bits).  Interleaved A/B (profiles/r03ac): K = 64 0.606 ->
// 0.535 ms, K = 32 unchanged.
template <int DT, int B, bool EXACT, int W = (B > 64 ? 2 : (B > 56 ? 3 : (B > 32 ? 4 : 5)))>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(W)))
k_median_off(const MSeg* __restrict__ segs, int nseg, const void* const* __restrict__ ptrs, int k) {
  if constexpr (EXACT) k = B;
  const int64_t tile = blockIdx.x;
  const MSeg sg = segs[nseg > 1 ? find_seg(segs, nseg, tile) : 0];
  const int64_t e0 = (tile - sg.tile_start) * kBlock, e = e0 + threadIdx.x;
  const bool live = e < sg.numel;
  const int64_t ec = live ? e : sg.numel - 1;
  const void* const* in = ptrs + sg.ptr_base;
  const int64_t ub = col_base<MedT<DT>::kBytes>(e0, sg.tstride);
  const unsigned boff = (unsigned)(ec - e0) * (unsigned)MedT<DT>::kBytes;
  const int lo_end = k + (B - 1) / 2 - ((k - 1) >> 1);  // sentinels [k, lo_end) low, [lo_end, B) high
  float x[B];
#pragma unroll
  for (int i = 0; i < B; ++i) x[i] = MedT<DT>::load_off(at(in[min(i, k - 1)], ub), boff);
  if constexpr (!EXACT) {
#pragma unroll
    for (int i = 0; i < B; ++i) x[i] = i < k ? x[i] : (i < lo_end ? -__builtin_inff() : __builtin_inff());
  }
  const float kr = select_mid<B>(x);
  if (!live) return;
  const int r = (k - 1) >> 1;
  const bool nan = kr != kr;
  if (nan || kr == 0.0f) store_rare<DT>(in, ub, boff, k, e, r, nan, sg.out);
  else MedT<DT>::store(sg.out, e, kr);
}

// Two lanes per column, K in (64, 128] (r02).  k_median_off at B = 128 holds 128 keys per lane:
// 256 VGPRs with spills, 2 waves per SIMD (1 wave without spills was slower still: K = 128 1.49 ->
// 1.99 ms), so HBM latency is exposed between the network's phases.  Here a column's B = 2N keys
// (B = K rounded up to 8, as k_median_off) are split between two lanes of different waves: waves 0-1
// of the workgroup hold clients 0..N-1 of 128 columns, waves 2-3 clients N..2N-1 of the same columns
// (the half index is wave-uniform, so every load keeps the SGPR-base + 32-bit-offset form).  Each lane
// sorts its N keys (SortNet<N>, median_nets.h: 1,086 min/max for N = 64, the same work as half of
// B = 128's pruned selection network), the upper lanes hand their sorted keys to the lower lanes
// through LDS, and the lower median -- rank N-1 of the 2N keys -- is max_j min(A[j], C[N-1-j]) (the N
// pairwise minima of a sorted A and a reversed sorted C are the N smallest keys).  Padding as
// k_median_off, all of it in the upper half, sentinels -inf / +inf.  Float keys as k_median_off (r03):
// a NaN in either half turns that half's sorted keys NaN and so the merged value (r02's uint32 keys
// found a NaN as a sorted key outside [key(-inf), key(+inf)]; K = 100 1.009 -> 0.955 ms, K = 128
// within 1 %, profiles/r03ac).  N keys + the merge fit 128 VGPRs
// (4 waves per SIMD).  Same keys and rare-case rules as k_median_off: bit-exact.
// xcd: always 0.  It chose the XCD-contiguous tile map in an A/B measurement that was not kept; the
// argument and its select stay because the kernel without them -- the same instructions from the
// segment lookup on -- measured K = 128 3-13 % slower and K = 100 2-9 % faster in interleaved runs
// (profiles/median_refactor), and this kernel is to run as it did.
constexpr int k2lCols = kBlock / 2;  // columns per workgroup
template <int DT, int N, bool EXACT>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(N <= 40 ? 8 : N <= 48 ? 6 : 5)))
k_median_2l(const MSeg* __restrict__ segs, int nseg, const void* const* __restrict__ ptrs, int k, int xcd) {
  constexpr int B = 2 * N;
  if constexpr (EXACT) k = B;
  __shared__ u32x4 xs[N / 4][k2lCols];  // the upper lanes' N sorted keys, [quad][column]
  const int h = __builtin_amdgcn_readfirstlane((int)threadIdx.x / k2lCols);  // half: wave-uniform
  const int c = (int)threadIdx.x % k2lCols;
  const int64_t tile = xcd ? xcd_tile_map(blockIdx.x, gridDim.x) : (int64_t)blockIdx.x;
  const MSeg sg = segs[nseg > 1 ? find_seg(segs, nseg, tile) : 0];
  const int64_t e0 = (tile - sg.tile_start) * k2lCols, e = e0 + c;
  const bool live = e < sg.numel;
  const int64_t ec = live ? e : sg.numel - 1;
  const void* const* in = ptrs + sg.ptr_base;
  const int64_t ub = col_base<MedT<DT>::kBytes>(e0, sg.tstride);
  const unsigned boff = (unsigned)(ec - e0) * (unsigned)MedT<DT>::kBytes;
  const int base = N * h;
  const int lo_end = k + (B - 1) / 2 - ((k - 1) >> 1);  // slots [k, lo_end) low sentinels, [lo_end, B) high
  float x[N];
#pragma unroll
  for (int t = 0; t < N; ++t) x[t] = MedT<DT>::load_off(at(in[min(base + t, k - 1)], ub), boff);
  if constexpr (!EXACT) {
#pragma unroll
    for (int t = N - 8; t < N; ++t)  // K > B - 8: only the upper half's last 8 slots can hold sentinels
      x[t] = base + t < k ? x[t] : (base + t < lo_end ? -__builtin_inff() : __builtin_inff());
  }
  SortNet<N>::run(x);  // a NaN input turns every sorted output NaN
  if (h == 1) {
#pragma unroll
    for (int q = 0; q < N / 4; ++q)
      xs[q][c] = u32x4{__float_as_uint(x[4 * q]), __float_as_uint(x[4 * q + 1]), __float_as_uint(x[4 * q + 2]),
                       __float_as_uint(x[4 * q + 3])};
  }
  __syncthreads();
  if (h == 1) return;
  float kr = -__builtin_inff();
#pragma unroll
  for (int q = 0; q < N / 4; ++q) {
    const u32x4 b = xs[q][c];
    kr = kmax(kr, kmin(x[N - 1 - 4 * q], __uint_as_float(b.x)));
    kr = kmax(kr, kmin(x[N - 2 - 4 * q], __uint_as_float(b.y)));
    kr = kmax(kr, kmin(x[N - 3 - 4 * q], __uint_as_float(b.z)));
    kr = kmax(kr, kmin(x[N - 4 - 4 * q], __uint_as_float(b.w)));
  }
  if (!live) return;
  const int r = (k - 1) >> 1;
  const bool nan = kr != kr;
  if (nan || kr == 0.0f) store_rare<DT>(in, ub, boff, k, e, r, nan, sg.out);
  else MedT<DT>::store(sg.out, e, kr);
}

// 16-bit types, two coordinates per lane: one 4-byte load per client, the two 16-bit keys packed in
// one register and the same network on v_pk_min_u16 / v_pk_max_u16 (half the loads and min/max
// instructions of one coordinate per lane).  Needs 4-byte aligned client and output pointers (the
// host checks); a column pair cut by the segment end takes the one-coordinate path.
__device__ __forceinline__ unsigned k16(unsigned u) { return u ^ ((u & 0x8000u) ? 0xFFFFu : 0x8000u); }
__device__ __forceinline__ unsigned k16_inv(unsigned k) { return (k & 0x8000u) ? (k & 0x7FFFu) : (~k & 0xFFFFu); }
template <int DT> __device__ __forceinline__ bool nan16(unsigned u) {
  return (u & 0x7FFFu) > (DT == FA_DTYPE_BF16 ? 0x7F80u : 0x7C00u);
}

template <int DT, int B>
__global__ void __launch_bounds__(kBlock)
k_median_pk(const MSeg* __restrict__ segs, int nseg, const void* const* __restrict__ ptrs, int k) {
  const int64_t tile = blockIdx.x;
  const MSeg sg = segs[nseg > 1 ? find_seg(segs, nseg, tile) : 0];
  const int64_t e0 = (tile - sg.tile_start) * kBlock * 2, e = e0 + threadIdx.x * 2;
  if (e >= sg.numel) return;
  const void* const* in = ptrs + sg.ptr_base;
  const int64_t ub = col_base<2>(e0, sg.tstride);
  const unsigned boff = (unsigned)(e - e0) * 2u;
  if (e + 1 == sg.numel) {  // odd segment length: the last coordinate alone
    median_col<DT, B>(in, ub, boff, k, e, true, sg.out);
    return;
  }
  const void* p[B];
#pragma unroll
  for (int i = 0; i < B; ++i) p[i] = at(in[min(i, k - 1)], ub);
  unsigned w[B];
#pragma unroll
  for (int i = 0; i < B; ++i) w[i] = gld_nt_off<unsigned>(p[i], boff);
  const int lo_end = k + (B - 1) / 2 - ((k - 1) >> 1);
  fa_u16x2 key[B];
  bool nan0 = false, nan1 = false;
#pragma unroll
  for (int i = 0; i < B; ++i) {
    const unsigned lo = w[i] & 0xFFFFu, hi = w[i] >> 16;
    nan0 = nan0 || (i < k && nan16<DT>(lo));
    nan1 = nan1 || (i < k && nan16<DT>(hi));
    const unsigned short sent = i < lo_end ? (unsigned short)0 : (unsigned short)0xFFFF;
    key[i] = i < k ? fa_u16x2{(unsigned short)k16(lo), (unsigned short)k16(hi)} : fa_u16x2{sent, sent};
  }
  const fa_u16x2 kr = select_mid<B>(key);
  const int r = (k - 1) >> 1;
  const unsigned k0 = kr.x, k1 = kr.y;
  const bool rare0 = nan0 || k0 == 0x8000u || k0 == 0x7FFFu;  // NaN seen / a zero selected
  const bool rare1 = nan1 || k1 == 0x8000u || k1 == 0x7FFFu;
  if (!rare0 && !rare1) {
    ((unsigned*)sg.out)[e >> 1] = k16_inv(k0) | (k16_inv(k1) << 16);
    return;
  }
  if (rare0) store_rare<DT>(in, ub, boff, k, e, r, nan0, sg.out);
  else ((unsigned short*)sg.out)[e] = (unsigned short)k16_inv(k0);
  if (rare1) store_rare<DT>(in, ub, boff + 2u, k, e + 1, r, nan1, sg.out);
  else ((unsigned short*)sg.out)[e + 1] = (unsigned short)k16_inv(k1);
}

// Any K (and float64): rank counting, ATen's order (value, client index), NaN first.
template <int DT>
__device__ __forceinline__ void copy_bits(void* out, int64_t e, const void* src, int64_t c) {
  if constexpr (DT == FA_DTYPE_F64) ((unsigned long long*)out)[e] = ((const unsigned long long*)src)[c];
  else MedT<DT>::store_bits_off(out, e, src, (unsigned)c * (unsigned)MedT<DT>::kBytes);
}

template <int DT>
__global__ void __launch_bounds__(kBlock)
k_median_rank(const MSeg* __restrict__ segs, int nseg, const void* const* __restrict__ ptrs, int k) {
  const int64_t tile = blockIdx.x;
  const MSeg sg = segs[nseg > 1 ? find_seg(segs, nseg, tile) : 0];
  const int64_t e0 = (tile - sg.tile_start) * kBlock, e = e0 + threadIdx.x;
  if (e >= sg.numel) return;
  const void* const* in = ptrs + sg.ptr_base;
  const int64_t ub = col_base<elem_bytes<DT>()>(e0, sg.tstride);
  const int64_t c = e - e0;
  for (int i = 0; i < k; ++i) {
    const double xi = load_d<DT>(at(in[i], ub), c);
    if (xi != xi) { copy_bits<DT>(sg.out, e, at(in[i], ub), c); return; }
  }
  const int r = (k - 1) >> 1;
  for (int i = 0; i < k; ++i) {
    const double xi = load_d<DT>(at(in[i], ub), c);
    int less = 0, eq_before = 0;
    for (int j = 0; j < k; ++j) {
      const double xj = load_d<DT>(at(in[j], ub), c);
      less += xj < xi;
      eq_before += (xj == xi) && (j < i);
    }
    if (less + eq_before == r) { copy_bits<DT>(sg.out, e, at(in[i], ub), c); return; }
  }
}

// Lanes per column for K in (64, 128]: 2 = k_median_2l (every K there: r02y measured K = 65 and 96
// within 2 % either way, the rest faster; at B = 40..64 the split measured 0-11 % slower, r02ab), 1 = one
// lane (k_median_off).  FA_MEDIAN_LANES forces a form (read at every call: the tests run both).
// (r03: a four-lanes-per-column form measured 19-30 % slower than k_median_2l and was removed)
int median_lanes(int dtype, int k, bool packed) {
  if (dtype == FA_DTYPE_F64 || packed || k <= 64 || k > 128) return 1;
  const char* e = getenv("FA_MEDIAN_LANES");
  return e && atoi(e) == 1 ? 1 : 2;
}

template <int DT>
void launch_median(int k, bool packed, int lanes, dim3 grid, hipStream_t st, const MSeg* ds, int nseg,
                   const void* const* dp) {
  if constexpr (DT != FA_DTYPE_F64) {
    switch ((k + 7) / 8) {  // bucket B = K rounded up to 8 (median_nets.h); two lanes: N = B / 2 keys per lane
#define FA_MB(Q)                                                                                        \
  case Q:                                                                                             \
    if constexpr (DT != FA_DTYPE_F32 && Q <= 8) /* packed: K <= 64 (see median_impl) */               \
      if (packed) {                                                                                   \
        hipLaunchKernelGGL((k_median_pk<DT, 8 * Q>), grid, dim3(kBlock), 0, st, ds, nseg, dp, k);      \
        return;                                                                                       \
      }                                                                                               \
    if constexpr (Q > 8)                                                                              \
      if (lanes == 2) {                                                                               \
        if (k == 8 * Q)                                                                               \
          hipLaunchKernelGGL((k_median_2l<DT, 4 * Q, true>), grid, dim3(kBlock), 0, st, ds, nseg, dp, k, 0); \
        else                                                                                          \
          hipLaunchKernelGGL((k_median_2l<DT, 4 * Q, false>), grid, dim3(kBlock), 0, st, ds, nseg, dp, k, 0); \
        return;                                                                                       \
      }                                                                                               \
    if (k == 8 * Q)                                                                                   \
      hipLaunchKernelGGL((k_median_off<DT, 8 * Q, true>), grid, dim3(kBlock), 0, st, ds, nseg, dp, k);  \
    else                                                                                              \
      hipLaunchKernelGGL((k_median_off<DT, 8 * Q, false>), grid, dim3(kBlock), 0, st, ds, nseg, dp, k); \
    return;
      FA_MB(1) FA_MB(2) FA_MB(3) FA_MB(4) FA_MB(5) FA_MB(6) FA_MB(7) FA_MB(8)
      FA_MB(9) FA_MB(10) FA_MB(11) FA_MB(12) FA_MB(13) FA_MB(14) FA_MB(15) FA_MB(16)
#undef FA_MB
      default: break;
    }
  }
  hipLaunchKernelGGL((k_median_rank<DT>), grid, dim3(kBlock), 0, st, ds, nseg, dp, k);
}

int median_impl(const ColArgs& a) {
  if (const int rc = col_check_args(a)) return rc;
  const int k = a.k;
  // bf16 / f16 with 4-byte aligned pointers, K <= 64: two coordinates per lane (k_median_pk;
  // bf16 K = 16 / 32 / 64: 0.127 / 0.251 / 0.655 -> 0.106 / 0.205 / 0.572 ms.  K = 128 took 2.44 ms
  // packed vs 1.51 ms one per lane: 128 live keys + 128 pointers exceed the register file)
  bool packed = (a.dtype == FA_DTYPE_BF16 || a.dtype == FA_DTYPE_F16) && k <= 64;
  for (int s = 0; s < a.num_segments && packed; ++s) {
    if (a.seg_numel[s] <= 0) continue;
    packed = a.d_out[s] && (uintptr_t)a.d_out[s] % 4 == 0;
    for (int i = 0; i < k && packed; ++i) packed = (uintptr_t)a.d_in[(int64_t)s * k + i] % 4 == 0;
  }
  const int lanes = median_lanes(a.dtype, k, packed);
  return col_launch(a, packed ? 2 * kBlock : lanes == 2 ? k2lCols : kBlock,
                    [&](dim3 grid, hipStream_t st, const MSeg* ds, int nseg, const void* const* dp) {
                      switch (a.dtype) {
                        case FA_DTYPE_F32: launch_median<FA_DTYPE_F32>(k, packed, lanes, grid, st, ds, nseg, dp); break;
                        case FA_DTYPE_BF16: launch_median<FA_DTYPE_BF16>(k, packed, lanes, grid, st, ds, nseg, dp); break;
                        case FA_DTYPE_F16: launch_median<FA_DTYPE_F16>(k, packed, lanes, grid, st, ds, nseg, dp); break;
                        default: launch_median<FA_DTYPE_F64>(k, packed, lanes, grid, st, ds, nseg, dp); break;
                      }
                    });
}

}  // namespace

extern "C" {

int fa_coord_median(fa_ctx* ctx, int dtype, int32_t num_segments, const int64_t* seg_numel, int32_t k,
                    const void* const* d_in, void* const* d_out, void* hip_stream) {
  return median_impl({"fa_coord_median", ctx, dtype, num_segments, seg_numel, k, d_in, 0, d_out, hip_stream});
}

int fa_coord_median_tiled(fa_ctx* ctx, int dtype, int32_t num_segments, const int64_t* seg_numel, int32_t k,
                          const void* const* d_in, int64_t tile_stride, void* const* d_out, void* hip_stream) {
  if (ctx && tile_stride <= 0) return fail(FA_ERR_INVALID, "fa_coord_median_tiled: tile_stride must be > 0");
  return median_impl(
      {"fa_coord_median_tiled", ctx, dtype, num_segments, seg_numel, k, d_in, tile_stride, d_out, hip_stream});
}

}  // extern "C"
