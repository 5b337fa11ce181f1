// quant_col.hip -- MI355X (gfx950) kernels + C ABI of the coordinate-wise defenses over block-quantized int8
// ("q8") client uploads (include/fedagg_quant_col.h): fa_coord_median_q8, fa_coord_trimmed_mean_q8 and
// fa_coord_mean_around_median_q8.  The contracts are the header's; the sorting networks are median.hip's and
// trimmed.hip's (median_nets.h, trimmed_nets.h), unchanged.
//
// Ownership.  A float column kernel loads 4 bytes per client and lane; a lane that loaded one int8 per client
// would issue a quarter of the bytes per load instruction, and the q8 sum is bound by its load rate.  So a
// lane owns FOUR consecutive columns: per client it loads ONE dword of q (non-temporal, uniform base + 32-bit
// offset), all loads issued before any is used, and keeps the raw dwords in registers.  It then runs four
// rounds, one per byte position (a rolled loop: one copy of the network in the instruction cache): sign-extend
// the byte, convert, multiply by the block's scale -- the float32 keys x = rnd((float)q * scale) -- run the
// network and the operator's epilogue.  The four results leave in one 16-byte store.
//   K <= 64         k_q8col_1l: a workgroup owns a slot of 1,024 columns, a lane B = K rounded up to 8 keys
//   K in (64, 128]  k_q8col_2l: a workgroup owns 512 columns; waves 0-1 hold clients 0..N-1 (N = B/2), waves
//                   2-3 clients N..2N-1 of the same columns; halves sort, then exchange through LDS as
//                   k_median_2l / k_tmean_2l / k_mam_2l do
// Slots start at multiples of 512 columns from the segment start, so a lane's four columns share one block at
// every B >= 16.
//
// Scales.  The slot's scales -- (columns / B, at least 1) blocks x B clients -- are staged once in LDS,
// [block][client] with an odd client stride (no bank conflict between the lanes of different blocks); a key's
// scale is one ds_read at an immediate offset from the lane's block row, a broadcast where lanes share a
// block.  K scales per lane in registers next to K raw dwords and B keys would not fit the register budget,
// and 64 scales plus 64 pointers do not fit the scalar registers either, so one LDS path serves every B.
//
// NaN.  A NaN key (a NaN scale, or q = 0 under an infinite scale) is handled in registers, with no in-order
// rescan: the sums' keys map NaN to +inf and count the column's NaNs, cn.  Sorted, the NaNs are the ranks
// k - cn .. k - 1 (above every real +inf, which carries the same value), so the window [a, b) holds a NaN iff
// b > k - cn, the mean around the median's dist() is +inf at such a rank, and +inf with -inf kept gives NaN in
// the float64 sum by itself.  Whole blocks turn NaN together, so a rescan would run on whole waves.  The
// median needs none of it: IEEE minimum / maximum carry a NaN to the selected output.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "blockq_host.h"
#include "elem.h"
#include "fa_internal.h"
#include "fedagg_quant.h"
#include "median_common.h"
#include "median_nets.h"
#include "trimmed_nets.h"

using namespace fa_detail;

namespace {

enum { kMedian = 0, kTmean = 1, kMam = 2 };

constexpr int kSlot = FA_Q8_COL_SLOT;  // columns per workgroup, one lane per column group
constexpr int kHalf = kBlock / 2;      // two lanes per column group: lanes per half,
constexpr int kSlot2 = 4 * kHalf;      // and columns per workgroup
constexpr int kScLds = 64 * 65;        // staged scales: 64 blocks x (64 | 1) clients, or 32 x (128 | 1)
static_assert(kSlot == 4 * kBlock && kSlot2 * 2 == kSlot, "a lane owns four columns");

typedef float f32x4 __attribute__((ext_vector_type(4)));
using G4f = __attribute__((address_space(1))) f32x4;

// What a workgroup knows of its slot.  COLS: its columns.
template <int COLS>
struct Slot {
  MSeg sg;
  const void* const* q;   // the segment's K data pointers
  const void* const* sc;  // and scale pointers
  int fl;                 // kDataAligned | kOutAligned
  int64_t e0;             // the slot's first column
  unsigned rem;           // its live columns, 1 .. COLS

  __device__ Slot(const MSeg* segs, int nseg, const void* const* qptrs, const void* const* sptrs, const int* flags) {
    const int64_t tile = blockIdx.x;
    const int si = nseg > 1 ? find_seg(segs, nseg, tile) : 0;
    sg = segs[si];
    q = qptrs + sg.ptr_base;
    sc = sptrs + sg.ptr_base;
    fl = flags[si];
    e0 = (tile - sg.tile_start) * COLS;
    rem = (unsigned)(sg.numel - e0 < COLS ? sg.numel - e0 : COLS);
  }
};

// ssc[j * (BP | 1) + i] = the scale of client min(i, k - 1) for the slot's block j, i < BP (the padded client
// count), blocks clamped to the segment's last; returns the lane's row, for columns c4 .. c4 + 3 of the slot
template <int BP, int COLS>
__device__ __forceinline__ int stage_scales(float* ssc, const Slot<COLS>& s, unsigned c4, int k, int shift) {
  constexpr int KP = BP | 1;
  constexpr int LOGC = COLS == 1024 ? 10 : 9;
  static_assert((1 << LOGC) == COLS && ((COLS >> 4) - 1) * KP + BP <= kScLds, "the staged scales fit");
  const int lognb = max(0, LOGC - shift);
  const int64_t sb0 = s.e0 >> shift, last = (s.sg.numel - 1) >> shift;
  for (int idx = (int)threadIdx.x; idx < (BP << lognb); idx += kBlock) {
    const int i = idx >> lognb, j = idx & ((1 << lognb) - 1);
    ssc[j * KP + i] = gld<float>(s.sc[min(i, k - 1)], min(sb0 + j, last));
  }
  __syncthreads();
  return (int)((((unsigned)s.e0 & ((1u << shift) - 1u)) + c4) >> shift) * KP;
}

// The lane's raw dwords of clients base .. base + N - 1 (clamped to the last client): byte j = column c4 + j.
// A whole slot of a segment with 4-byte aligned q: one dword load per client; else byte loads at clamped
// columns into the same registers.
template <int N, int COLS>
__device__ __forceinline__ void load_raw(unsigned (&raw)[N], const Slot<COLS>& s, int base, int k, unsigned c4) {
  if ((s.fl & kDataAligned) && s.rem == COLS) {  // workgroup-uniform
#pragma unroll
    for (int t = 0; t < N; ++t) raw[t] = gld_nt_off<unsigned>(at(s.q[min(base + t, k - 1)], s.e0), c4);
  } else {
    unsigned o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = min(c4 + j, s.rem - 1);
#pragma unroll
    for (int t = 0; t < N; ++t) {
      const void* p = at(s.q[min(base + t, k - 1)], s.e0);
      raw[t] = (unsigned)gld_nt_off<unsigned char>(p, o[0]) | ((unsigned)gld_nt_off<unsigned char>(p, o[1]) << 8) |
               ((unsigned)gld_nt_off<unsigned char>(p, o[2]) << 16) | ((unsigned)gld_nt_off<unsigned char>(p, o[3]) << 24);
    }
  }
}

// The keys of byte position sh / 8: x[t] = rnd((float)q * scale) of client base + t; slots at or past client k
// (the last 8 only: k > the padded count - 8) become -inf below lo_end and +inf from it.  CNT: NaN keys become
// +inf and are counted in cn.
template <int N, bool CNT>
__device__ __forceinline__ void make_keys(float (&x)[N], const unsigned (&raw)[N], const float* ls, int sh, int base,
                                          int k, int lo_end, int& cn) {
#pragma unroll
  for (int t = 0; t < N; ++t) x[t] = op_mul((float)((int)(raw[t] << (24 - sh)) >> 24), ls[t]);
#pragma unroll
  for (int t = N - 8; t < N; ++t)
    x[t] = base + t < k ? x[t] : (base + t < lo_end ? -__builtin_inff() : __builtin_inff());
  if constexpr (CNT) {
#pragma unroll
    for (int t = 0; t < N; ++t) {
      const bool n = x[t] != x[t];
      cn += n ? 1 : 0;
      x[t] = n ? __builtin_inff() : x[t];
    }
  }
}

// the four results of columns c4 .. c4 + 3 of the slot
template <int COLS>
__device__ __forceinline__ void store4(const Slot<COLS>& s, unsigned c4, const float (&res)[4]) {
  if (c4 >= s.rem) return;
  float* out = (float*)s.sg.out + s.e0 + c4;
  if ((s.fl & kOutAligned) && c4 + 4 <= s.rem) {
    __builtin_nontemporal_store(f32x4{res[0], res[1], res[2], res[3]}, (G4f*)out);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (c4 + j < s.rem) out[j] = res[j];
  }
}

// dist() of fedagg_robust.h's mean around the median for the value v of a rank that holds no NaN
__device__ __forceinline__ double q8_dist(float v, float m, double dm) {
  return v == m ? 0.0 : __builtin_fabs((double)v - dm);
}

// One lane per column group, K <= 64.  arg: the trim (kTmean) or the keep (kMam).
template <int OP, int B, int W>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(W)))
k_q8col_1l(const MSeg* __restrict__ segs, int nseg, const void* const* __restrict__ qptrs,
           const void* const* __restrict__ sptrs, const int* __restrict__ flags, int k, int shift, int arg) {
  __shared__ float ssc[kScLds];
  const Slot<kSlot> s(segs, nseg, qptrs, sptrs, flags);
  const unsigned c4 = threadIdx.x * 4u;
  unsigned raw[B];
  load_raw<B>(raw, s, 0, k, c4);  // in flight over the staging of the scales
  const float* ls = ssc + stage_scales<B>(ssc, s, c4, k, shift);
  const int h = (k - 1) >> 1;
  float res[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 1
  for (int b = 0; b < 4; ++b) {
    float x[B], v;
    int cn = 0;
    if constexpr (OP == kMedian) {
      // k_median_off's sentinels: the lower median of the reals is rank (B-1)/2 of all B keys
      make_keys<B, false>(x, raw, ls, 8 * b, 0, k, k + (B - 1) / 2 - h, cn);
      v = select_mid<B>(x);
    } else {
      make_keys<B, true>(x, raw, ls, 8 * b, 0, k, k, cn);
      SortNet<B>::run(x);
      if constexpr (OP == kTmean) {  // k_tmean_off's walk over x[trim .. k-1-trim]
        const int ke = k - arg;
        double acc = 0.0;
#pragma unroll
        for (int r = 0; r < B; ++r) {
          const double d = (double)x[r];
          if (r < (B + 1) / 2) acc = r == arg ? d : (r > arg && r < ke ? acc + d : acc);
          else acc = r < ke ? acc + d : acc;
        }
        v = cn > arg ? __builtin_nanf("") : (float)(acc / (double)(k - 2 * arg));
      } else {  // k_mam_off's median, barrel shift, count and walk; dist() exact for every column
        const int keep = arg, kn = k - cn, lomin = max(0, h - keep + 1), lomax = min(h, k - keep);
        constexpr int R = B / 2 - 1;  // r < h <= B/2 - 1
        float m = x[0];
#pragma unroll
        for (int r = 1; r <= R; ++r) m = r == h ? x[r] : m;
        float y[B];
#pragma unroll
        for (int i = 0; i < B; ++i) y[i] = x[i];
#pragma unroll
        for (int st = 1; st < B; st <<= 1) {
          const bool on = (keep & st) != 0;
#pragma unroll
          for (int i = 0; i < B; ++i) y[i] = on ? (i + st < B ? y[i + st] : __builtin_inff()) : y[i];
        }
        const double dm = (double)m;
        int lo = lomin;
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const double dy = r + keep >= kn ? (double)__builtin_inff() : q8_dist(y[r], m, dm);
          lo += (r >= lomin && r < lomax && q8_dist(x[r], m, dm) > dy) ? 1 : 0;
        }
        double acc = -0.0;
#pragma unroll
        for (int r = 0; r < B; ++r) acc = acc + mam_term(x[r], r, lo, keep);
        v = (h >= kn || lo + keep > kn) ? __builtin_nanf("") : (float)(acc / (double)keep);
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) res[j] = b == j ? v : res[j];
  }
  store4(s, c4, res);
}

// The two-lane forms' exchange (k_tmean_2l): each half's lane holds its N sorted keys (A below, C above).  The
// upper lanes put C in LDS; the lower lane keeps lo = min(A[j], C[N-1-j]) and writes hi = max back over
// C[N-1-j]; then the lower lane holds ranks 0 .. N-1 and the upper lane ranks N .. 2N-1, ascending.  Two
// barriers; column c's rows of xs are touched by its two lanes only.
template <int N>
__device__ __forceinline__ void merge_2l(float (&x)[N], u32x4 (*xs)[kHalf], int hf, int c) {
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
    BitonicLo<N>::run(x);
  } else {
#pragma unroll
    for (int q = 0; q < N / 4; ++q) {
      const u32x4 cq = xs[q][c];
      x[4 * q] = __uint_as_float(cq.x);
      x[4 * q + 1] = __uint_as_float(cq.y);
      x[4 * q + 2] = __uint_as_float(cq.z);
      x[4 * q + 3] = __uint_as_float(cq.w);
    }
    BitonicHi<N>::run(x);
  }
}

// Two lanes per column group, K in (64, 128]; B = 2N = K rounded up to 8, the padding in the upper half.
// Every barrier is reached by all lanes in every round.  The lane that ends a round with the result (the
// lower one for the median, the upper one for the sums) stores.
template <int OP, int N, int W>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(W)))
k_q8col_2l(const MSeg* __restrict__ segs, int nseg, const void* const* __restrict__ qptrs,
           const void* const* __restrict__ sptrs, const int* __restrict__ flags, int k, int shift, int arg) {
  constexpr int B = 2 * N;
  __shared__ float ssc[kScLds];
  __shared__ u32x4 xs[N / 4 + (OP == kMam ? 1 : 0)][kHalf];  // the exchange buffer; kMam: then N + 4 ranks
  __shared__ double accs[kHalf];
  __shared__ int los[kHalf], cns[kHalf];
  const int hf = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kHalf);  // half: wave-uniform
  const int c = (int)threadIdx.x % kHalf;
  const Slot<kSlot2> s(segs, nseg, qptrs, sptrs, flags);
  const unsigned c4 = (unsigned)c * 4u;
  const int base = N * hf;
  unsigned raw[N];
  load_raw<N>(raw, s, base, k, c4);
  const float* ls = ssc + stage_scales<B>(ssc, s, c4, k, shift) + base;
  const int h = (k - 1) >> 1;  // one of N-4 .. N-1: k > 2N - 8
  float res[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 1
  for (int b = 0; b < 4; ++b) {
    float x[N], v = 0.0f;
    int cn = 0;
    if constexpr (OP == kMedian) {  // k_median_2l: rank N-1 of the 2N keys = max_j min(A[j], C[N-1-j])
      make_keys<N, false>(x, raw, ls, 8 * b, base, k, k + (B - 1) / 2 - h, cn);
      SortNet<N>::run(x);  // a NaN input turns every sorted output NaN
      if (hf == 1) {
#pragma unroll
        for (int q = 0; q < N / 4; ++q)
          xs[q][c] = u32x4{__float_as_uint(x[4 * q]), __float_as_uint(x[4 * q + 1]), __float_as_uint(x[4 * q + 2]),
                           __float_as_uint(x[4 * q + 3])};
      }
      __syncthreads();
      if (hf == 0) {
        v = -__builtin_inff();
#pragma unroll
        for (int q = 0; q < N / 4; ++q) {
          const u32x4 cq = xs[q][c];
          v = kmax(v, kmin(x[N - 1 - 4 * q], __uint_as_float(cq.x)));
          v = kmax(v, kmin(x[N - 2 - 4 * q], __uint_as_float(cq.y)));
          v = kmax(v, kmin(x[N - 3 - 4 * q], __uint_as_float(cq.z)));
          v = kmax(v, kmin(x[N - 4 - 4 * q], __uint_as_float(cq.w)));
        }
      }
      __syncthreads();  // the next round's keys overwrite xs
    } else {
      make_keys<N, true>(x, raw, ls, 8 * b, base, k, k, cn);
      SortNet<N>::run(x);
      merge_2l<N>(x, xs, hf, c);
      if constexpr (OP == kTmean) {  // k_tmean_2l: the lower lane sums its kept ranks, the upper continues
        const int ke = k - arg;
        if (hf == 0) {
          double acc = 0.0;
#pragma unroll
          for (int r = 0; r < N; ++r) {
            const double d = (double)x[r];
            acc = r == arg ? d : (r > arg && r < ke ? acc + d : acc);
          }
          accs[c] = acc;
          cns[c] = cn;
        }
        __syncthreads();
        if (hf == 1) {
          double acc = accs[c];
#pragma unroll
          for (int r = 0; r < N; ++r) acc = N + r < ke ? acc + (double)x[r] : acc;
          v = cn + cns[c] > arg ? __builtin_nanf("") : (float)(acc / (double)(k - 2 * arg));
        }
      } else {  // k_mam_2l: ranks N-4 .. 2N-1 published as fl[rank - (N-4)][column], partners at uniform rows
        const int keep = arg;
        __syncthreads();  // every read of the exchange buffer is done
        float* fl = (float*)xs;
        if (hf == 0) {
#pragma unroll
          for (int t = 0; t < 4; ++t) fl[t * kHalf + c] = x[N - 4 + t];
        } else {
#pragma unroll
          for (int t = 0; t < N; ++t) fl[(4 + t) * kHalf + c] = x[t];
          cns[c] = cn;
        }
        __syncthreads();
        if (hf == 0) {
          const int kn = k - cn - cns[c], lomin = max(0, h - keep + 1), lomax = min(h, k - keep);
          float m = x[N - 4];
#pragma unroll
          for (int r = N - 3; r < N; ++r) m = r == h ? x[r] : m;
          const double dm = (double)m;
          int lo = lomin;
#pragma unroll
          for (int r = 0; r < N - 1; ++r) {  // r < h <= N - 1
            if (r >= lomin && r < lomax) {   // uniform: a branch, so only the range's partners are read
              const float p = fl[(r + keep - (N - 4)) * kHalf + c];  // row in [1, N + 3]
              const double dp = r + keep >= kn ? (double)__builtin_inff() : q8_dist(p, m, dm);
              lo += q8_dist(x[r], m, dm) > dp ? 1 : 0;
            }
          }
          double acc = -0.0;
#pragma unroll
          for (int r = 0; r < N; ++r) acc = acc + mam_term(x[r], r, lo, keep);
          accs[c] = acc;
          los[c] = (h >= kn || lo + keep > kn) ? -1 : lo;  // -1: the result is NaN
        }
        __syncthreads();
        if (hf == 1) {
          double acc = accs[c];
          const int lo = los[c];
#pragma unroll
          for (int r = 0; r < N; ++r) acc = acc + mam_term(x[r], N + r, lo, keep);
          v = lo < 0 ? __builtin_nanf("") : (float)(acc / (double)keep);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) res[j] = b == j ? v : res[j];
  }
  if (hf == (OP == kMedian ? 0 : 1)) store4(s, c4, res);
}

// waves per SIMD by the keys a lane holds next to as many raw dwords (DESIGN, block-quantized family)
// the mean around the median also holds the shifted copy of its keys (one lane) or the partners' loop (two)
constexpr int w1(int op, int b) {
  return op == kMam ? (b > 40 ? 1 : (b > 16 ? 2 : 3)) : (b > 32 ? 2 : (b > 24 ? 3 : 4));
}
constexpr int w2(int op, int n) { return op == kMam || n > 48 ? 2 : 3; }

template <int OP>
void launch_q8col(int k, int arg, dim3 grid, hipStream_t st, const MSeg* ds, int nseg, const void* const* dq,
                  const void* const* dsc, const int* dfl, int shift) {
  switch ((k + 7) / 8) {  // B = K rounded up to 8; two lanes: N = B / 2 keys per lane
#define FA_C1(Q)                                                                                            \
  case Q:                                                                                                   \
    hipLaunchKernelGGL((k_q8col_1l<OP, 8 * Q, w1(OP, 8 * Q)>), grid, dim3(kBlock), 0, st, ds, nseg, dq, dsc, dfl, k, \
                       shift, arg);                                                                         \
    return;
#define FA_C2(Q)                                                                                            \
  case Q:                                                                                                   \
    hipLaunchKernelGGL((k_q8col_2l<OP, 4 * Q, w2(OP, 4 * Q)>), grid, dim3(kBlock), 0, st, ds, nseg, dq, dsc, dfl, k, \
                       shift, arg);                                                                         \
    return;
    FA_C1(1) FA_C1(2) FA_C1(3) FA_C1(4) FA_C1(5) FA_C1(6) FA_C1(7) FA_C1(8)
    FA_C2(9) FA_C2(10) FA_C2(11) FA_C2(12) FA_C2(13) FA_C2(14) FA_C2(15) FA_C2(16)
#undef FA_C1
#undef FA_C2
    default: break;  // k > FA_Q8_COL_MAX_K: refused before the launch
  }
}

constexpr BlockFmt kQ8{"q", FA_Q8_BLOCK_MIN, FA_Q8_BLOCK_MAX, 0};

template <int OP, class ArgCheck>
int q8col_entry(const char* fn, fa_ctx* ctx, int32_t num_segments, const int64_t* seg_numel, int32_t k, int32_t block,
                int32_t arg, const void* const* d_q, const void* const* d_scale, void* const* d_out, void* hip_stream,
                ArgCheck check_arg) {
  return block_col_entry(fn, kQ8, k > 64 ? kSlot2 : kSlot, FA_Q8_COL_MAX_K, ctx, num_segments, seg_numel, k, block, d_q,
                         d_scale, d_out, hip_stream, check_arg,
                         [&](dim3 grid, hipStream_t st, const MSeg* ds, int n, const void* const* dq,
                             const void* const* dsc, const int* dfl, int shift) {
                           launch_q8col<OP>(k, arg, grid, st, ds, n, dq, dsc, dfl, shift);
                         });
}

}  // namespace

extern "C" {

int fa_coord_median_q8(fa_ctx* ctx, int32_t num_segments, const int64_t* seg_numel, int32_t k, int32_t block,
                       const void* const* d_q, const void* const* d_scale, void* const* d_out, void* hip_stream) {
  return q8col_entry<kMedian>("fa_coord_median_q8", ctx, num_segments, seg_numel, k, block, 0, d_q, d_scale, d_out,
                              hip_stream, [] { return (int)FA_OK; });
}

int fa_coord_trimmed_mean_q8(fa_ctx* ctx, int32_t num_segments, const int64_t* seg_numel, int32_t k, int32_t block,
                             int32_t trim, const void* const* d_q, const void* const* d_scale, void* const* d_out,
                             void* hip_stream) {
  return q8col_entry<kTmean>("fa_coord_trimmed_mean_q8", ctx, num_segments, seg_numel, k, block, trim, d_q, d_scale,
                             d_out, hip_stream, [&] {
                               if (trim < 0 || 2 * (int64_t)trim >= k)
                                 return fail(FA_ERR_INVALID,
                                             "fa_coord_trimmed_mean_q8: trim must satisfy 0 <= trim and 2 * trim < k "
                                             "(trim %d, k %d)", trim, k);
                               return (int)FA_OK;
                             });
}

int fa_coord_mean_around_median_q8(fa_ctx* ctx, int32_t num_segments, const int64_t* seg_numel, int32_t k,
                                   int32_t block, int32_t keep, const void* const* d_q, const void* const* d_scale,
                                   void* const* d_out, void* hip_stream) {
  return q8col_entry<kMam>("fa_coord_mean_around_median_q8", ctx, num_segments, seg_numel, k, block, keep, d_q, d_scale,
                           d_out, hip_stream, [&] {
                             if (keep < 1 || keep > k)
                               return fail(FA_ERR_INVALID,
                                           "fa_coord_mean_around_median_q8: keep must satisfy 1 <= keep <= k "
                                           "(keep %d, k %d)", keep, k);
                             return (int)FA_OK;
                           });
}

}  // extern "C"
