// quant_dist.hip -- MI355X (gfx950) kernels + C ABI of the fused sum and squared distances over
// block-quantized int8 ("q8") client updates (include/fedagg_quant_dist.h: fa_weighted_sum_sqdist_q8,
// fa_centered_sum_sqdist_q8): one pass of the smoothed Weiszfeld iteration (geometric median) or of
// centered clipping, straight from the uploaded bytes.  The contract and its op order are the header's.
//
// The shape is k_wsum_q8's (quant.hip): a workgroup owns ONE 4-KiB slot of q per client = 4,096
// elements; a lane holds 16 consecutive elements per client, one 16-byte load and exactly one scale
// because B >= 16.  Phase 1 forms the lane's 16 float32 values of out (or takes the center's), phase 2
// every client's two float64 partials against them: the differences in float32, squared and summed in
// float64 FMAs; the squared norm as the exact integer sum of the 16 q^2 (four v_dot4_i32_i8) times
// (double)scale^2, one conversion and two multiplies per client instead of 16 conversions and 16 FMAs.
// Each partial takes one DPP row reduction, the 16 row leaders write LDS, the rows are added in row order
// into the workgroup's row of the scratch (wsd_common.h, shared with wsum_dist.hip) and k_wsd_reduce adds
// the rows: no floating-point atomics.
//
// k_wsdq_reg, K <= 32 (KM = K rounded up to 8): every client's 16 bytes and scale, 5 VGPRs per client,
// are loaded non-temporally before the first is consumed and stay in registers between the phases: the
// input is read once.  Clients past k repeat client k - 1 and are masked by selects, so no branch depends
// on the client index.  The distance-only mode has no second walk to save and takes k_wsdq.  k_wsdq, any K: phase 1 is k_wsum_q8's loop with kU clients in flight, phase 2
// walks the clients again (K x 4 KiB per workgroup) in LDS blocks of 128 clients.  A ragged last slot and
// a segment whose q pointers, output or center are not all 16-byte aligned take coalesced byte loads
// with a `live` mask in both kernels: the same arithmetic per element of out, the same bits.
// Kept and lost forms, with their numbers: DESIGN.md.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>

#include "elem.h"
#include "fa_internal.h"
#include "fedagg_quant.h"
#include "blockq_host.h"
#include "median_common.h"
#include "wsd_common.h"

using namespace fa_detail;

namespace {

constexpr int kQ = 16;                       // elements per lane: 16 bytes of q
constexpr int64_t E = (int64_t)kBlock * kQ;  // a slot's elements (FA_TILE_BYTES of q)
static_assert(E == FA_Q8_DIST_SLOT && E == FA_TILE_BYTES, "a slot of q is one tile");
constexpr int kU = 8;   // clients whose loads are in flight together (whole aligned slots)
constexpr int kUE = 1;  // the same on the byte path (16 q and 16 scale registers per client)
enum { kPlain = 0, kCenter = 1, kDist = 2 };  // what a pass forms

using G4 = __attribute__((address_space(1))) u32x4;

// One client's 16 elements of this lane.  VEC: 16 consecutive elements, one scale; else the byte path's
// 16 elements a wave's width apart, each with its own block's scale.
template <bool VEC>
struct QRaw;
template <>
struct QRaw<true> {
  u32x4 r;
  float s;
  __device__ __forceinline__ float q(int j) const {  // one v_cvt_f32_i32 with a byte select
    return (float)(int)(signed char)(r[j >> 2] >> (8 * (j & 3)));
  }
  __device__ __forceinline__ float sc(int) const { return s; }
};
template <>
struct QRaw<false> {
  signed char x[kQ];
  float s[kQ];
  __device__ __forceinline__ float q(int j) const { return (float)(int)x[j]; }
  __device__ __forceinline__ float sc(int j) const { return s[j]; }
};

// Where this lane's 16 elements of a slot lie: uniform slot bases plus 32-bit lane offsets.
template <bool VEC>
struct QLane {
  int64_t e0;                  // the slot's first element = its byte offset in q
  int shift;
  unsigned off[VEC ? 1 : kQ];  // VEC: the lane's first element in the slot; else its (clamped) elements
  unsigned live;               // bit j: element j lies inside the segment

  __device__ __forceinline__ void init(const MSeg& sg, int64_t tl, int sh) {
    const int tid = (int)threadIdx.x;
    e0 = tl * E;
    shift = sh;
    if constexpr (VEC) {
      off[0] = (unsigned)tid * kQ;
      live = ~0u;
    } else {
      const unsigned rem = (unsigned)(sg.numel - e0 < E ? sg.numel - e0 : E);
      live = 0;
#pragma unroll
      for (int j = 0; j < kQ; ++j) {
        const unsigned e = (unsigned)(j * kBlock + tid);
        if (e < rem) live |= 1u << j;
        off[j] = e < rem ? e : rem - 1;  // clamped: every load unconditional
      }
    }
  }
  __device__ __forceinline__ void load(QRaw<VEC>& c, const void* q, const void* sc) const {
    const void* qb = (const char*)q + e0;
    const void* sb = (const float*)sc + (e0 >> shift);  // E is a multiple of B
    if constexpr (VEC) {
      c.r = gld_nt_off<u32x4>(qb, off[0]);
      c.s = gld_nt_off<float>(sb, (off[0] >> shift) * 4u);
    } else {
#pragma unroll
      for (int j = 0; j < kQ; ++j) {
        c.x[j] = gld_nt_off<signed char>(qb, off[j]);
        c.s[j] = gld_nt_off<float>(sb, (off[j] >> shift) * 4u);
      }
    }
  }
  // the lane's elements of a flat float32 tensor (the center, out): the same lane reads and writes an element
  __device__ __forceinline__ void load_f32(float (&v)[kQ], const void* p) const {
    const float* b = (const float*)p + e0;
    if constexpr (VEC) {
#pragma unroll
      for (int w = 0; w < 4; ++w) El<FA_DTYPE_F32>::unpack(*(const G4*)(b + off[0] + 4 * w), &v[4 * w]);
    } else {
#pragma unroll
      for (int j = 0; j < kQ; ++j) v[j] = gld<float>(b, off[j]);
    }
  }
  __device__ __forceinline__ void store_f32(const float (&v)[kQ], void* p) const {
    float* b = (float*)p + e0;
    if constexpr (VEC) {
#pragma unroll
      for (int w = 0; w < 4; ++w) *(u32x4*)(b + off[0] + 4 * w) = El<FA_DTYPE_F32>::pack(&v[4 * w]);
    } else {
#pragma unroll
      for (int j = 0; j < kQ; ++j)
        if (live >> j & 1u) b[off[j]] = v[j];
    }
  }
};

// acc += client i's 16 terms (w = (float)coef[i]).  kPlain: t = rnd(q * c), c = rnd(scale * w) once per
// block; kCenter: t = rnd(rnd(rnd(q * scale) - center) * w).  on == false leaves acc as it is (a select).
template <bool VEC, int CM>
__device__ __forceinline__ void q8d_add(float (&acc)[kQ], const QRaw<VEC>& c, const float (&cen)[kQ], float w,
                                        bool on) {
#pragma unroll
  for (int j = 0; j < kQ; ++j) {
    float t;
    if constexpr (CM == kCenter) t = op_mul(op_sub(op_mul(c.q(j), c.sc(j)), cen[j]), w);
    else t = op_mul(c.q(j), op_mul(c.sc(j), w));
    const float nxt = op_add(acc[j], t);
    acc[j] = on ? nxt : acc[j];
  }
}

// the sum of the 16 q^2 of 16 bytes, exact (<= 16 * 128^2)
__device__ __forceinline__ int q8_sumsq(u32x4 r) {
  int s = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) s = __builtin_amdgcn_sdot4((int)r[w], (int)r[w], s, false);
  return s;
}

// One client's two partials of this lane against ref (the registers' out, or the center).
template <bool VEC>
__device__ __forceinline__ void q8d_stats(const QRaw<VEC>& c, const float (&ref)[kQ], unsigned live, double& d2,
                                          double& ss) {
  d2 = 0.0;
  ss = 0.0;
#pragma unroll
  for (int j = 0; j < kQ; ++j) {
    const float x = op_mul(c.q(j), c.sc(j));
    const double dd = (double)op_sub(x, ref[j]);
    if (VEC || (live >> j & 1u)) {
      d2 = __builtin_fma(dd, dd, d2);
      if constexpr (!VEC) ss = __builtin_fma((double)x, (double)x, ss);
    }
  }
  if constexpr (VEC) {
    const double sd = (double)c.s;
    ss = (double)q8_sumsq(c.r) * (sd * sd);  // sd * sd is exact; 0 * NaN and 0 * Inf stay non-finite
  }
}

// the lane's partials of the client in LDS column `col`: one DPP row sum each, the row leader stores
__device__ __forceinline__ void q8d_put(double (&red)[kRows][2 * kKB], int col, double d2, double ss, bool on) {
  d2 = row_sum(d2);
  ss = row_sum(ss);
  if (on && ((int)threadIdx.x & 15) == 0) {
    red[(int)threadIdx.x >> 4][col] = d2;
    red[(int)threadIdx.x >> 4][kKB + col] = ss;
  }
}

// Generic form of one slot, any k.  CM: kPlain, the weighted sum; kCenter, out = rnd(center + the ordered
// sum of the clipped differences); kDist, out IS the center: no first walk and no store.
template <bool VEC, int CM>
__device__ __forceinline__ void q8d_slot(const MSeg& sg, int64_t tl, const void* const* __restrict__ q,
                                         const void* const* __restrict__ sc, const void* __restrict__ center,
                                         const double* __restrict__ coef, int k, int shift, double* __restrict__ part,
                                         double (&red)[kRows][2 * kKB]) {
  constexpr int U = VEC ? kU : kUE;
  QLane<VEC> ln;
  ln.init(sg, tl, shift);
  float cen[kQ] = {};
  if constexpr (CM != kPlain) ln.load_f32(cen, center);
  float acc[kQ];
#pragma unroll
  for (int j = 0; j < kQ; ++j) acc[j] = CM == kDist ? cen[j] : -0.0f;  // -0 + t == t bitwise for every t
  if constexpr (CM != kDist) {
    for (int i0 = 0; i0 < k; i0 += U) {
      QRaw<VEC> c[U];
#pragma unroll
      for (int u = 0; u < U; ++u) ln.load(c[u], q[min(i0 + u, k - 1)], sc[min(i0 + u, k - 1)]);
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (i0 + u < k) q8d_add<VEC, CM>(acc, c[u], cen, (float)coef[i0 + u], true);  // wave-uniform
    }
    if constexpr (CM == kCenter) {
#pragma unroll
      for (int j = 0; j < kQ; ++j) acc[j] = op_add(cen[j], acc[j]);
    }
    ln.store_f32(acc, sg.out);
  }
  // phase 2: the two sums of every client against the registers' out, kKB clients per LDS block
  for (int b0 = 0; b0 < k; b0 += kKB) {
    const int bn = min(kKB, k - b0);
    for (int i0 = b0; i0 < b0 + bn; i0 += U) {
      QRaw<VEC> c[U];
#pragma unroll
      for (int u = 0; u < U; ++u) ln.load(c[u], q[min(i0 + u, b0 + bn - 1)], sc[min(i0 + u, b0 + bn - 1)]);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (i0 + u < b0 + bn) {  // wave-uniform
          double d2, ss;
          q8d_stats<VEC>(c[u], acc, ln.live, d2, ss);
          q8d_put(red, i0 + u - b0, d2, ss, true);
        }
      }
    }
    flush_rows(red, b0, bn, k, part);
  }
}

// What every kernel here starts with: the workgroup's segment, slot, tables and row of the scratch.
struct QWork {
  MSeg sg;
  int64_t tl;
  const void* const* q;
  const void* const* sc;
  const void* center;
  double* part;
  bool vec;  // a whole slot of a segment whose q pointers, output and center are 16-byte aligned
  __device__ __forceinline__ QWork(const MSeg* __restrict__ segs, int nseg, const void* const* __restrict__ qptrs,
                                   const void* const* __restrict__ sptrs, const void* const* __restrict__ cens,
                                   const int* __restrict__ flags, int k, double* __restrict__ partial) {
    const int64_t tile = xcd_tile_map(blockIdx.x, gridDim.x);
    const int si = nseg > 1 ? find_seg(segs, nseg, tile) : 0;
    sg = segs[si];
    tl = tile - sg.tile_start;
    q = qptrs + sg.ptr_base;
    sc = sptrs + sg.ptr_base;
    center = cens[si];
    part = partial + tile * (2 * (int64_t)k);
    vec = (flags[si] & kDataAligned) && (tl + 1) * E <= sg.numel;  // workgroup-uniform
  }
};

// qptrs / sptrs: [segment][client] (MSeg.ptr_base); cens[j] / flags[j]: the center and kDataAligned of
// the table's segment j; partial: one row of 2k float64 per workgroup.
template <int CM>
__global__ void __launch_bounds__(kBlock)
k_wsdq(const MSeg* __restrict__ segs, int nseg, const void* const* __restrict__ qptrs,
       const void* const* __restrict__ sptrs, const void* const* __restrict__ cens, const int* __restrict__ flags,
       const double* __restrict__ coef, int k, int shift, double* __restrict__ partial) {
  __shared__ double red[kRows][2 * kKB];
  const QWork w(segs, nseg, qptrs, sptrs, cens, flags, k, partial);
  if (w.vec) q8d_slot<true, CM>(w.sg, w.tl, w.q, w.sc, w.center, coef, k, shift, w.part, red);
  else q8d_slot<false, CM>(w.sg, w.tl, w.q, w.sc, w.center, coef, k, shift, w.part, red);
}

// Single-read form, k <= KM: the slot's KM x 20 bytes of every lane stay in registers between the phases.
template <int KM, int CM>
__global__ void __launch_bounds__(kBlock)
k_wsdq_reg(const MSeg* __restrict__ segs, int nseg, const void* const* __restrict__ qptrs,
           const void* const* __restrict__ sptrs, const void* const* __restrict__ cens, const int* __restrict__ flags,
           const double* __restrict__ coef, int k, int shift, double* __restrict__ partial) {
  static_assert(KM <= kKB, "one LDS block holds every client");
  __shared__ double red[kRows][2 * kKB];
  const QWork w(segs, nseg, qptrs, sptrs, cens, flags, k, partial);
  if (!w.vec) {
    q8d_slot<false, CM>(w.sg, w.tl, w.q, w.sc, w.center, coef, k, shift, w.part, red);
    return;
  }
  QLane<true> ln;
  ln.init(w.sg, w.tl, shift);
  QRaw<true> c[KM];
#pragma unroll
  for (int i = 0; i < KM; ++i) ln.load(c[i], w.q[min(i, k - 1)], w.sc[min(i, k - 1)]);
  float cen[kQ] = {};
  if constexpr (CM != kPlain) ln.load_f32(cen, w.center);
  float acc[kQ];
#pragma unroll
  for (int j = 0; j < kQ; ++j) acc[j] = CM == kDist ? cen[j] : -0.0f;
  if constexpr (CM != kDist) {
#pragma unroll
    for (int i = 0; i < KM; ++i) q8d_add<true, CM>(acc, c[i], cen, (float)coef[min(i, k - 1)], i < k);
    if constexpr (CM == kCenter) {
#pragma unroll
      for (int j = 0; j < kQ; ++j) acc[j] = op_add(cen[j], acc[j]);
    }
    ln.store_f32(acc, w.sg.out);
  }
#pragma unroll
  for (int i = 0; i < KM; ++i) {
    // the bytes are converted again here: without the barrier the compiler keeps phase 1's 16 floats per
    // client alive instead (KM x 16 more VGPRs, and spills from KM = 24 on)
    asm volatile("" : "+v"(c[i].r));
    double d2, ss;
    q8d_stats<true>(c[i], acc, ~0u, d2, ss);
    q8d_put(red, i, d2, ss, i < k);
  }
  flush_rows(red, 0, k, k, w.part);
}

constexpr int kRegMaxK = 32;  // clients the single-read form holds in registers (KM = 40 .. 64)

bool wsdq_reg_enabled() {  // FA_WSDQ_REG=0: the generic kernel for every K (A/B); read per call
  const char* e = getenv("FA_WSDQ_REG");
  return !(e && e[0] == '0');
}

template <int CM>
void wsdq_launch(int k, dim3 grid, hipStream_t st, const MSeg* ds, int n, const void* const* dp, const void* const* dsc,
                 const int* dfl, const void* const* dcen, const double* dc, int shift, double* part) {
  const dim3 block(kBlock);
  // kDist walks the clients once in either form; the generic kernel's 8 clients in flight at 124 VGPRs ran
  // level with or ahead of KM x 5 held registers, so the register form is not built for it
  if constexpr (CM != kDist) {
    if (k <= kRegMaxK && wsdq_reg_enabled()) {
      switch ((k + 7) / 8) {  // KM = K rounded up to 8
#define FA_QR(Q) \
  case Q: hipLaunchKernelGGL((k_wsdq_reg<8 * Q, CM>), grid, block, 0, st, ds, n, dp, dsc, dcen, dfl, dc, k, shift, part); break;
        FA_QR(1) FA_QR(2) FA_QR(3) FA_QR(4)
#undef FA_QR
      }
      return;
    }
  }
  hipLaunchKernelGGL((k_wsdq<CM>), grid, block, 0, st, ds, n, dp, dsc, dcen, dfl, dc, k, shift, part);
}

constexpr BlockFmt kQ8{"q", FA_Q8_BLOCK_MIN, FA_Q8_BLOCK_MAX, 0};

int wsdq_impl(const char* fn, bool centered, fa_ctx* ctx, int32_t num_segments, const int64_t* seg_numel, int32_t k,
              int32_t block, const void* const* d_q, const void* const* d_scale, const void* const* d_center,
              const double* coef, void* const* d_out, void* d_stats, void* d_scratch, size_t scratch_bytes,
              void* hip_stream) {
  const int mode = !centered ? kPlain : coef ? kCenter : kDist;
  return block_dist_entry(
      fn, kQ8, E, ctx, centered, num_segments, seg_numel, k, block, d_q, d_scale, d_center, coef, d_out, d_stats,
      d_scratch, scratch_bytes, hip_stream,
      [&](dim3 grid, hipStream_t st, const MSeg* ds, int n, const void* const* dp, const void* const* dsc,
          const int* dfl, const void* const* dcen, const double* dc, int shift, int64_t tiles) {
        double* part = (double*)d_scratch;
        switch (mode) {
          case kPlain: wsdq_launch<kPlain>(k, grid, st, ds, n, dp, dsc, dfl, dcen, dc, shift, part); break;
          case kCenter: wsdq_launch<kCenter>(k, grid, st, ds, n, dp, dsc, dfl, dcen, dc, shift, part); break;
          default: wsdq_launch<kDist>(k, grid, st, ds, n, dp, dsc, dfl, dcen, dc, shift, part); break;
        }
        wsd_reduce_launch(st, part, tiles, k, d_stats);
      });
}

}  // namespace

extern "C" {

int fa_weighted_sum_sqdist_q8(fa_ctx* ctx, int32_t num_segments, const int64_t* seg_numel, int32_t k, int32_t block,
                              const void* const* d_q, const void* const* d_scale, const double* coef,
                              void* const* d_out, void* d_stats, void* d_scratch, size_t scratch_bytes,
                              void* hip_stream) {
  return wsdq_impl("fa_weighted_sum_sqdist_q8", false, ctx, num_segments, seg_numel, k, block, d_q, d_scale, nullptr,
                   coef, d_out, d_stats, d_scratch, scratch_bytes, hip_stream);
}

int fa_centered_sum_sqdist_q8(fa_ctx* ctx, int32_t num_segments, const int64_t* seg_numel, int32_t k, int32_t block,
                              const void* const* d_q, const void* const* d_scale, const void* const* d_center,
                              const double* coef, void* const* d_out, void* d_stats, void* d_scratch,
                              size_t scratch_bytes, void* hip_stream) {
  return wsdq_impl("fa_centered_sum_sqdist_q8", true, ctx, num_segments, seg_numel, k, block, d_q, d_scale, d_center,
                   coef, d_out, d_stats, d_scratch, scratch_bytes, hip_stream);
}

size_t fa_weighted_sum_sqdist_q8_scratch_bytes(int32_t num_segments, const int64_t* seg_numel, int32_t k) {
  if (k <= 0 || num_segments <= 0 || !seg_numel) return 0;
  int64_t tiles = 0;
  for (int s = 0; s < num_segments; ++s) {
    if (seg_numel[s] < 0) return 0;
    tiles += (seg_numel[s] + E - 1) / E;
  }
  if (tiles > 0x7FFFFFFFll) return 0;
  return (size_t)tiles * 2 * (size_t)k * sizeof(double);
}

}  // extern "C"
