// quant.hip -- MI355X (gfx950) kernels + C ABI of the block-quantized int8 ("q8") client updates
// (include/fedagg_quant.h): fa_weighted_sum_q8, the fused dequantize-and-sum, and fa_quantize_q8, the
// device quantizer that produces the format.  The contracts and their op order are the header's.
//
// k_wsum_q8: the weighted-sum family's shape -- a workgroup owns ONE 4-KiB slot of q per client, which
// is 4,096 elements; a lane reads 16 bytes per client (non-temporal), 16 consecutive elements that all
// fall in one block because B >= 16, so one scale per lane and client, with the coefficient folded into
// it once.  kU clients' loads are issued before any is consumed.  A lane ends with 16 float32
// accumulators = 64 consecutive bytes of the output; a wave passes them through LDS (a 4 x 4 transpose
// of 16-byte chunks between the lanes of a quad of quads, bank-conflict free) so that every store
// instruction writes 1 KiB of consecutive bytes, 16 per lane.  Segments whose q pointers are not all
// 16-byte aligned, and a segment's ragged last slot, take byte loads with the same arithmetic per
// element (the same bits); an output that is only 4-byte aligned takes element stores.
//
// k_quantize_q8: a workgroup owns 4,096 elements, a lane 16 consecutive ones (one 16-byte store of q).
// A block of B elements spans B / 16 <= 64 lanes of ONE wave, so the block's amax is a butterfly
// max inside the wave, taken on the bits of |x|: for non-negative floats the integer order is the float
// order, subnormals included, and every NaN and Inf lies at or above 0x7f800000 -- one reduction gives
// both the amax and the non-finite flag.  Not on the server's hot path.  Numbers: DESIGN.md.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "elem.h"
#include "fa_internal.h"
#include "fedagg_quant.h"
#include "median_common.h"
#include "median_host.h"

using namespace fa_detail;

namespace {

constexpr int kQ = 16;                       // elements per lane: 16 bytes of q
constexpr int64_t E = (int64_t)kBlock * kQ;  // a slot's elements (FA_TILE_BYTES of q)
static_assert(E == FA_TILE_BYTES, "a slot of q is one tile");
constexpr int kU = 8;   // clients whose loads are in flight together (whole aligned slots)
constexpr int kUE = 2;  // the same on the byte path (16 q and 16 scale registers per client)

using G4 = __attribute__((address_space(1))) u32x4;

enum { kQAligned = 1, kOutAligned = 2 };  // per-segment flags of k_wsum_q8

__device__ __forceinline__ float q8_coef(float scale, const double* __restrict__ coef, int i, bool mulw) {
  return mulw ? op_mul(scale, (float)coef[i]) : scale;
}

// acc += the 16 elements of one client's 16 bytes, each (float)q * c
__device__ __forceinline__ void q8_consume(float (&acc)[kQ], u32x4 r, float c) {
#pragma unroll
  for (int w = 0; w < 4; ++w) {
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const float x = (float)(int)(signed char)(r[w] >> (8 * b));  // one v_cvt_f32_i32 with a byte select
      acc[4 * w + b] = op_add(acc[4 * w + b], op_mul(x, c));
    }
  }
}

// A whole slot of a segment whose q pointers are 16-byte aligned.  sm: kBlock * 4 chunks (VOUT only).
template <bool MULW, bool VOUT>
__device__ __forceinline__ void q8_sum_vec(const MSeg& sg, int64_t tl, const void* const* __restrict__ q,
                                           const void* const* __restrict__ sc, const double* __restrict__ coef, int k,
                                           int shift, u32x4* sm) {
  constexpr int U = kU;
  const int tid = (int)threadIdx.x;
  // uniform slot base + the lane's 32-bit byte offset
  const int64_t s0 = tl * E;                   // the slot's first element = its byte offset in q
  const unsigned qoff = (unsigned)tid * kQ;    // the lane's first element in the slot
  const unsigned soff = (qoff >> shift) * 4u;  // its block's scale (E is a multiple of B)
  const int64_t e0 = s0 + qoff;
  float acc[kQ];
#pragma unroll
  for (int j = 0; j < kQ; ++j) acc[j] = -0.0f;  // -0 + t == t bitwise for every t
  // the group of clients i0 .. i0 + U - 1, clamped to the last client: every load unconditional
  auto load = [&](u32x4 (&r)[U], float (&s)[U], int i0) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = min(i0 + u, k - 1);
      r[u] = gld_nt_off<u32x4>((const char*)q[i] + s0, qoff);
      s[u] = gld_nt_off<float>((const float*)sc[i] + (s0 >> shift), soff);
    }
  };
  auto eat = [&](const u32x4 (&r)[U], const float (&s)[U], int i0) {
    if (i0 + U <= k) {  // a whole group: no guard between the clients
#pragma unroll
      for (int u = 0; u < U; ++u) q8_consume(acc, r[u], q8_coef(s[u], coef, i0 + u, MULW));
    } else {
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (i0 + u < k) q8_consume(acc, r[u], q8_coef(s[u], coef, i0 + u, MULW));  // wave-uniform
    }
  };
  for (int i0 = 0; i0 < k; i0 += U) {
    u32x4 r[U];
    float s[U];
    load(r, s, i0);  // every load of the group is issued before the first client's arithmetic
    eat(r, s, i0);
  }

  float* out = (float*)sg.out;
  if constexpr (VOUT) {
    // chunk (lane l, j) = the lane's floats 4j .. 4j+3 goes to slot 4 * tid + ((j + l / 4) & 3): the 16
    // lanes that one LDS pass serves hit 16 different 16-byte bank groups, on the write and on the read
    const int l = tid & 63, wave0 = tid & ~63;
#pragma unroll
    for (int j = 0; j < 4; ++j) sm[4 * tid + ((j + (l >> 2)) & 3)] = El<FA_DTYPE_F32>::pack(acc + 4 * j);
    __syncthreads();
    // store j of a wave: its chunks 64 j .. 64 j + 63, one per lane = 1 KiB of consecutive bytes
    char* wout = (char*)(out + tl * E + (int64_t)wave0 * kQ);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = j * 64 + l, sl = c >> 2, sj = c & 3;
      const u32x4 v = sm[4 * (wave0 + sl) + ((sj + (sl >> 2)) & 3)];
      __builtin_nontemporal_store(v, (G4*)(wout + (int64_t)c * 16));
    }
  } else {
#pragma unroll
    for (int j = 0; j < kQ; ++j) out[e0 + j] = acc[j];
  }
}

// Any slot: byte loads, element j of lane l is the slot's element j * kBlock + l (coalesced).
template <bool MULW>
__device__ __forceinline__ void q8_sum_elem(const MSeg& sg, int64_t tl, const void* const* __restrict__ q,
                                            const void* const* __restrict__ sc, const double* __restrict__ coef, int k,
                                            int shift) {
  const int tid = (int)threadIdx.x;
  // the slot's base is uniform; a lane's elements are 32-bit offsets into it (E is a multiple of B)
  const int64_t e0 = tl * E;
  const unsigned rem = (unsigned)(sg.numel - e0 < E ? sg.numel - e0 : E);
  unsigned off[kQ], live = 0;
#pragma unroll
  for (int j = 0; j < kQ; ++j) {
    const unsigned e = (unsigned)(j * kBlock + tid);
    if (e < rem) live |= 1u << j;
    off[j] = e < rem ? e : rem - 1;  // clamped: every load unconditional
  }
  float acc[kQ];
#pragma unroll
  for (int j = 0; j < kQ; ++j) acc[j] = -0.0f;
  for (int i0 = 0; i0 < k; i0 += kUE) {
    signed char x[kUE][kQ];
    float s[kUE][kQ];
#pragma unroll
    for (int u = 0; u < kUE; ++u) {
      const int i = min(i0 + u, k - 1);
      const void* qb = (const char*)q[i] + e0;
      const void* sb = (const float*)sc[i] + (e0 >> shift);
#pragma unroll
      for (int j = 0; j < kQ; ++j) {
        x[u][j] = gld_nt_off<signed char>(qb, off[j]);
        s[u][j] = gld_nt_off<float>(sb, (off[j] >> shift) * 4u);
      }
    }
#pragma unroll
    for (int u = 0; u < kUE; ++u) {
      if (i0 + u < k) {  // wave-uniform
#pragma unroll
        for (int j = 0; j < kQ; ++j)
          acc[j] = op_add(acc[j], op_mul((float)(int)x[u][j], q8_coef(s[u][j], coef, i0 + u, MULW)));
      }
    }
  }
  float* out = (float*)sg.out;
#pragma unroll
  for (int j = 0; j < kQ; ++j)
    if (live >> j & 1u) out[e0 + j * kBlock + tid] = acc[j];
}

// qptrs / sptrs: [segment][client] (MSeg.ptr_base); flags[j]: kQAligned | kOutAligned of segment j.
// 4 waves per SIMD (128 VGPRs): kU clients of 20 bytes per lane in flight on each
template <bool MULW>
__global__ void __launch_bounds__(kBlock, 4)
k_wsum_q8(const MSeg* __restrict__ segs, int nseg, const void* const* __restrict__ qptrs,
          const void* const* __restrict__ sptrs, const int* __restrict__ flags, const double* __restrict__ coef, int k,
          int shift) {
  __shared__ u32x4 sm[kBlock * 4];
  const int64_t tile = xcd_tile_map(blockIdx.x, gridDim.x);
  const int si = nseg > 1 ? find_seg(segs, nseg, tile) : 0;
  const MSeg sg = segs[si];
  const int64_t tl = tile - sg.tile_start;
  const void* const* q = qptrs + sg.ptr_base;
  const void* const* sc = sptrs + sg.ptr_base;
  const int fl = flags[si];
  // workgroup-uniform: the barrier of the vector-store path is reached by all lanes or none
  if ((fl & kQAligned) && (tl + 1) * E <= sg.numel) {
    if (fl & kOutAligned) q8_sum_vec<MULW, true>(sg, tl, q, sc, coef, k, shift, sm);
    else q8_sum_vec<MULW, false>(sg, tl, q, sc, coef, k, shift, sm);
  } else {
    q8_sum_elem<MULW>(sg, tl, q, sc, coef, k, shift);
  }
}

// One slot of the quantizer.  VEC: a whole slot, input and q 16-byte aligned.
template <int DT, bool VEC>
__device__ __forceinline__ void q8_quant_slot(const MSeg& sg, int64_t tl, const void* __restrict__ in,
                                              float* __restrict__ scale, int shift) {
  using T = El<DT>;
  using S = typename T::S;
  const int tid = (int)threadIdx.x;
  const int64_t e0 = tl * E + (int64_t)tid * kQ;  // the lane's first element
  float x[kQ];
  if constexpr (VEC) {
#pragma unroll
    for (int v = 0; v < kQ / T::V; ++v) {
      const u32x4 r = __builtin_nontemporal_load((const G4*)((const char*)in + e0 * T::SZ + v * 16));
      T::unpack(r, x + v * T::V);
    }
  } else {
#pragma unroll
    for (int j = 0; j < kQ; ++j) {
      const int64_t e = e0 + j;
      const float v = T::from_bits(gld<S>(in, e < sg.numel ? e : sg.numel - 1));  // clamped: unconditional
      x[j] = e < sg.numel ? v : 0.0f;  // past the end: no part in the amax
    }
  }
  // the bits of |x|: integer order == float order, NaN and Inf at or above 0x7f800000
  unsigned m = 0;
#pragma unroll
  for (int j = 0; j < kQ; ++j) m = max(m, __float_as_uint(x[j]) & 0x7FFFFFFFu);
  const int lanes = 1 << (shift - 4);  // of one block: 1 .. 64, a power of two, inside one wave
  for (int o = 1; o < lanes; o <<= 1) m = max(m, (unsigned)__shfl_xor((int)m, o));
  const bool bad = m >= 0x7F800000u;
  const float s = bad ? __uint_as_float(0x7FC00000u) : op_div(__uint_as_float(m), 127.0f);
  const bool zero = bad || s == 0.0f;
  int qi[kQ];
#pragma unroll
  for (int j = 0; j < kQ; ++j) {
    const float r = __builtin_rintf(op_div(x[j], s));  // ties to even
    qi[j] = zero ? 0 : (int)fminf(fmaxf(r, -127.0f), 127.0f);
  }
  if ((tid & (lanes - 1)) == 0 && e0 < sg.numel) scale[e0 >> shift] = s;
  signed char* q = (signed char*)sg.out;
  if constexpr (VEC) {
    u32x4 w;
#pragma unroll
    for (int v = 0; v < 4; ++v)
      w[v] = ((unsigned)qi[4 * v] & 0xFFu) | (((unsigned)qi[4 * v + 1] & 0xFFu) << 8) |
             (((unsigned)qi[4 * v + 2] & 0xFFu) << 16) | ((unsigned)qi[4 * v + 3] << 24);
    __builtin_nontemporal_store(w, (G4*)((char*)q + e0));
  } else {
#pragma unroll
    for (int j = 0; j < kQ; ++j)
      if (e0 + j < sg.numel) q[e0 + j] = (signed char)qi[j];
  }
}

// ins[j]: the input of the table's segment j (MSeg.ptr_base); scales[j]: its scales; MSeg.out: its q;
// MSeg.aligned: input and q are 16-byte aligned.
template <int DT>
__global__ void __launch_bounds__(kBlock)
k_quantize_q8(const MSeg* __restrict__ segs, int nseg, const void* const* __restrict__ ins,
              void* const* __restrict__ scales, int shift) {
  const int64_t tile = blockIdx.x;
  const int si = nseg > 1 ? find_seg(segs, nseg, tile) : 0;
  const MSeg sg = segs[si];
  const int64_t tl = tile - sg.tile_start;
  const void* in = ins[sg.ptr_base];
  float* scale = (float*)scales[si];
  if (sg.aligned && (tl + 1) * E <= sg.numel) q8_quant_slot<DT, true>(sg, tl, in, scale, shift);
  else q8_quant_slot<DT, false>(sg, tl, in, scale, shift);
}

// log2 of a valid block size, or -1
int q8_shift(int32_t block) {
  if (block < FA_Q8_BLOCK_MIN || block > FA_Q8_BLOCK_MAX || (block & (block - 1))) return -1;
  int s = 0;
  while ((1 << s) < block) ++s;
  return s;
}
inline bool al4(const void* p) { return ((uintptr_t)p & 3u) == 0; }

}  // namespace

extern "C" {

int fa_weighted_sum_q8(fa_ctx* ctx, int mode, int32_t num_segments, const int64_t* seg_numel, int32_t k, int32_t block,
                       const void* const* d_q, const void* const* d_scale, const double* coef, void* const* d_out,
                       void* hip_stream) {
  const char* fn = "fa_weighted_sum_q8";
  if (!ctx) return fail(FA_ERR_INVALID, "%s: ctx is NULL", fn);
  const int shift = q8_shift(block);
  if (shift < 0)
    return fail(FA_ERR_INVALID, "%s: block %d is not a power of two in [%d, %d]", fn, block, FA_Q8_BLOCK_MIN,
                FA_Q8_BLOCK_MAX);
  if (k <= 0 || num_segments <= 0) return fail(FA_ERR_INVALID, "%s: k and num_segments must be positive", fn);
  if (!seg_numel || !d_q || !d_scale || !d_out) return fail(FA_ERR_INVALID, "%s: a table is NULL", fn);
  if (!coef && mode != FA_MODE_SUM) return fail(FA_ERR_INVALID, "%s: coef is NULL (allowed for FA_MODE_SUM only)", fn);
  if (mode != FA_MODE_MUL_W && mode != FA_MODE_SUM)
    return fail(FA_ERR_DTYPE, "%s: mode %d not supported (FA_MODE_MUL_W, FA_MODE_SUM)", fn, mode);
  int nseg = 0;
  int64_t tiles = 0;
  for (int s = 0; s < num_segments; ++s) {
    if (seg_numel[s] < 0) return fail(FA_ERR_INVALID, "%s: segment %d has negative numel", fn, s);
    if (seg_numel[s] == 0) continue;
    if (!d_out[s] || !al4(d_out[s]))
      return fail(FA_ERR_INVALID, "%s: segment %d: output NULL or not 4-byte aligned", fn, s);
    for (int i = 0; i < k; ++i) {
      const int64_t t = (int64_t)s * k + i;
      if (!d_q[t]) return fail(FA_ERR_INVALID, "%s: segment %d client %d: q NULL", fn, s, i);
      if (!d_scale[t] || !al4(d_scale[t]))
        return fail(FA_ERR_INVALID, "%s: segment %d client %d: scale NULL or not 4-byte aligned", fn, s, i);
    }
    ++nseg;
    tiles += (seg_numel[s] + E - 1) / E;
  }
  if (tiles > 0x7FFFFFFFll) return fail(FA_ERR_INVALID, "%s: too many tiles", fn);
  if (nseg == 0) return FA_OK;

  // the payload: the k coefficients, the non-empty segments' scale pointers ([segment][client], as
  // the q table), and one flag word per segment
  const ColArgs a{fn, ctx, FA_DTYPE_F32, num_segments, seg_numel, k, d_q, 0, d_out, hip_stream};
  const size_t coef_bytes = sizeof(double) * (size_t)k;
  const size_t ptr_bytes = sizeof(void*) * (size_t)nseg * k;
  const size_t fl_off = coef_bytes + ptr_bytes;
  const size_t extra = fl_off + ((sizeof(int) * (size_t)nseg + 7) & ~size_t(7));
  return col_stage_launch(
      a, E, nseg, tiles, extra,
      [&](void* h) {
        for (int i = 0; i < k; ++i) ((double*)h)[i] = coef ? coef[i] : 0.0;
        const void** hs = (const void**)((char*)h + coef_bytes);
        int* hfl = (int*)((char*)h + fl_off);
        int j = 0;
        for (int s = 0; s < num_segments; ++s) {
          if (!seg_numel[s]) continue;
          bool qal = true;
          for (int i = 0; i < k; ++i) {
            hs[(int64_t)j * k + i] = d_scale[(int64_t)s * k + i];
            qal = qal && al16(d_q[(int64_t)s * k + i]);
          }
          hfl[j] = (qal ? kQAligned : 0) | (al16(d_out[s]) ? kOutAligned : 0);
          ++j;
        }
        if (nseg & 1) hfl[nseg] = 0;  // the padding is staged too
      },
      [&](dim3 grid, hipStream_t st, const MSeg* ds, int n, const void* const* dp, const void* payload) {
        const char* pl = (const char*)payload;
        const double* dc = (const double*)pl;
        const void* const* dsc = (const void* const*)(pl + coef_bytes);
        const int* dfl = (const int*)(pl + fl_off);
        const dim3 blk(kBlock);
        if (mode == FA_MODE_MUL_W) hipLaunchKernelGGL((k_wsum_q8<true>), grid, blk, 0, st, ds, n, dp, dsc, dfl, dc, k, shift);
        else hipLaunchKernelGGL((k_wsum_q8<false>), grid, blk, 0, st, ds, n, dp, dsc, dfl, dc, k, shift);
      });
}

int fa_quantize_q8(fa_ctx* ctx, int dtype, int32_t num_segments, const int64_t* seg_numel, int32_t block,
                   const void* const* d_in, void* const* d_q, void* const* d_scale, void* hip_stream) {
  const char* fn = "fa_quantize_q8";
  if (!ctx) return fail(FA_ERR_INVALID, "%s: ctx is NULL", fn);
  const int shift = q8_shift(block);
  if (shift < 0)
    return fail(FA_ERR_INVALID, "%s: block %d is not a power of two in [%d, %d]", fn, block, FA_Q8_BLOCK_MIN,
                FA_Q8_BLOCK_MAX);
  if (num_segments <= 0) return fail(FA_ERR_INVALID, "%s: num_segments must be positive", fn);
  if (!seg_numel || !d_in || !d_q || !d_scale) return fail(FA_ERR_INVALID, "%s: a table is NULL", fn);
  if (dtype != FA_DTYPE_F32 && dtype != FA_DTYPE_BF16 && dtype != FA_DTYPE_F16)
    return fail(FA_ERR_DTYPE, "%s: dtype %d not supported (F32, BF16, F16)", fn, dtype);
  const uintptr_t in_mask = dtype == FA_DTYPE_F32 ? 3u : 1u;
  int nseg = 0;
  int64_t tiles = 0;
  for (int s = 0; s < num_segments; ++s) {
    if (seg_numel[s] < 0) return fail(FA_ERR_INVALID, "%s: segment %d has negative numel", fn, s);
    if (seg_numel[s] == 0) continue;
    if (!d_in[s] || ((uintptr_t)d_in[s] & in_mask))
      return fail(FA_ERR_INVALID, "%s: segment %d: input NULL or not aligned to its element", fn, s);
    if (!d_q[s]) return fail(FA_ERR_INVALID, "%s: segment %d: q NULL", fn, s);
    if (!d_scale[s] || !al4(d_scale[s]))
      return fail(FA_ERR_INVALID, "%s: segment %d: scale NULL or not 4-byte aligned", fn, s);
    ++nseg;
    tiles += (seg_numel[s] + E - 1) / E;
  }
  if (tiles > 0x7FFFFFFFll) return fail(FA_ERR_INVALID, "%s: too many tiles", fn);
  if (nseg == 0) return FA_OK;

  // the table: one "client" per segment (the input), the output is q; the payload: the scale pointers
  const ColArgs a{fn, ctx, dtype, num_segments, seg_numel, 1, d_in, 0, d_q, hip_stream};
  return col_stage_launch(
      a, E, nseg, tiles, sizeof(void*) * (size_t)nseg,
      [&](void* h) {
        for (int s = 0, j = 0; s < num_segments; ++s)
          if (seg_numel[s]) ((void**)h)[j++] = d_scale[s];
      },
      [&](dim3 grid, hipStream_t st, const MSeg* ds, int n, const void* const* dp, const void* payload) {
        void* const* dsc = (void* const*)payload;
        const dim3 blk(kBlock);
        switch (dtype) {
          case FA_DTYPE_F32: hipLaunchKernelGGL((k_quantize_q8<FA_DTYPE_F32>), grid, blk, 0, st, ds, n, dp, dsc, shift); break;
          case FA_DTYPE_BF16: hipLaunchKernelGGL((k_quantize_q8<FA_DTYPE_BF16>), grid, blk, 0, st, ds, n, dp, dsc, shift); break;
          default: hipLaunchKernelGGL((k_quantize_q8<FA_DTYPE_F16>), grid, blk, 0, st, ds, n, dp, dsc, shift); break;
        }
      });
}

}  // extern "C"
