// mx.hip -- MI355X (gfx950) kernels + C ABI of the OCP Microscaling ("mx") client updates
// (include/fedagg_mx.h): fa_weighted_sum_mx, the fused decode-and-sum of MXFP8 (E4M3) and MXFP4 (E2M1)
// clients, and fa_quantize_mx, the device quantizer that produces the format.  The contracts and their
// op order are the header's; the host path is blockq_host.h's, shared with q8 and q1.
//
// k_wsum_mx: the block-compressed family's shape -- a workgroup of 256 lanes owns ONE 4-KiB slot of
// data per client, a lane reads 16 bytes per client (non-temporal), and kU clients' loads are issued
// before any is consumed.  For FP4 a lane's 16 bytes are 32 elements = exactly one block, so one scale
// byte per lane and client and 32 accumulators; the slot is 8,192 elements.  For FP8 they are 16
// elements = half a block, a pair of lanes shares a scale byte, the slot is 4,096 elements.  The scale
// bytes reach the lanes as ONE BYTE LOAD per lane and client (a slot's 256 or 128 consecutive bytes, at
// any alignment; the pair of an FP8 block reads the same byte): no cross-lane step, no second path.
//
// The decode is the hardware's: v_cvt_scalef32_pk_f32_fp8 / _fp4 turn two codes into two float32 with
// the block's power of two applied on the way; their scale operand is the float whose exponent field
// is X, (unsigned)X << 23.  Run over every scale byte and every code in every byte and nibble position
// they give the header's value bit for bit -- X = 0 (2^-127), X = 255 (NaN), subnormal results (kept),
// E4M3 overflow (Inf), E4M3 NaN, the low nibble first -- so no case is patched by a select
// (tests/test_gpu_mx.py::test_decode_exhaustive is that check).  Per client element: half a conversion,
// one multiply by the client's coefficient (MUL_W) and one add, each rounded once.  The coefficient
// cannot be folded into the scale as q8's contract does: the header's value is the float32 sum over the
// DECODED tensors, two roundings.  The multiply and the add are packed float32, written on the register
// pairs the conversions return (pk_term_add): a v_pk_mul_f32 by the coefficient (its low half used twice,
// op_sel_hi) and a v_pk_add_f32 into an accumulator pair, each half rounded once as the scalar ops
// would -- 1.5 vector ops per client element plus the per-client ones (1.6 FP4 / 1.75 FP8 in the
// assembly, against 2.6 / 2.75 of the scalar form).  Measured against the scalar build: DESIGN.md.
//
// A lane ends with 16 (FP8) or 32 (FP4) accumulators = 64 or 128 consecutive output bytes; a workgroup
// passes them through 16 or 32 KiB of LDS (q8's 4 x 4 rotation of 16-byte chunks, and its 8 x 8
// extension between pairs of lanes for FP4, bank-conflict free on the write and on the read) so that
// every store instruction of a wave writes 1 KiB of consecutive bytes.  Segments whose data pointers
// are not all 16-byte aligned, and a segment's ragged last slot, take byte loads in passes of 4,096
// elements: element j of lane l is the pass's element 256 j + l, an FP4 lane shifts its nibble down (l
// and the element have the same parity) -- the same conversion per element, so the same bits.  An
// output that is only 4-byte aligned takes element stores.
//
// k_quantize_mx: a workgroup owns one slot of the sum, a lane 32 (FP4) or 16 (FP8) consecutive
// elements = 16 bytes of codes.  The block's amax is taken on the bits of |x| (integer order == float
// order, every NaN and Inf at or above 0x7f800000: one maximum gives the amax and the non-finite flag)
// inside the lane, with one shuffle between the two lanes of an FP8 block.  The exponent and the codes
// are mx_codec.h's integer arithmetic, which rounds as the header says by construction; the hardware's
// float32 -> FP8 / FP4 conversions are not used.  Not on the server's hot path.  Numbers: DESIGN.md.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "blockq_host.h"
#include "elem.h"
#include "fa_internal.h"
#include "fedagg_mx.h"
#include "median_common.h"
#include "mx_codec.h"

using namespace fa_detail;

namespace {

constexpr int kU = 8;         // clients whose loads are in flight together (whole aligned slots)
constexpr int kUE = 2;        // the same on the byte path (16 data and 16 scale registers per client)
constexpr int kPass = 16;     // elements per lane of one pass of the byte path
constexpr int64_t kPassE = (int64_t)kBlock * kPass;
static_assert(kU == FA_MX_GROUP, "fedagg_mx.h states the group");

using G4 = __attribute__((address_space(1))) u32x4;
using f32x2 = float __attribute__((ext_vector_type(2)));

// acc + d * {c, c} (MUL_W) or acc + d on the register pair a conversion returns: v_pk_mul_f32 and
// v_pk_add_f32, each half rounded once as the scalar ops would (-ffp-contract=off keeps them apart).
template <bool MULW>
__device__ __forceinline__ f32x2 pk_term_add(f32x2 acc, f32x2 d, float c) {
  if constexpr (MULW) d = d * (f32x2){c, c};
  return acc + d;
}

// Per format: kQ elements in a lane's 16 bytes, kC 16-byte output chunks per lane, kRot the lanes that
// share a rotation of the LDS transpose (kC * kRot = 16), EPB elements per data byte, the lane's
// scale byte in its slot.
template <int FMT> struct Mx;
template <> struct Mx<FA_MX_FP8> {
  static constexpr int kQ = 16, kC = 4, kRotShift = 2, EPB = 1;
  static constexpr int64_t E = FA_MX_FP8_SLOT;
  __device__ static unsigned scale_index(int tid) { return (unsigned)tid >> 1; }
  // acc += the 16 elements of one client's 16 bytes
  template <bool MULW>
  __device__ static void consume(f32x2 (&acc)[kQ / 2], u32x4 r, float sf, float c) {
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      acc[2 * w] = pk_term_add<MULW>(acc[2 * w], __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(r[w], sf, false), c);
      acc[2 * w + 1] = pk_term_add<MULW>(acc[2 * w + 1], __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(r[w], sf, true), c);
    }
  }
  // one element from its byte
  __device__ static float one(unsigned byte, int, float sf) {
    return __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(byte, sf, false)[0];
  }
};
template <> struct Mx<FA_MX_FP4> {
  static constexpr int kQ = 32, kC = 8, kRotShift = 1, EPB = 2;
  static constexpr int64_t E = FA_MX_FP4_SLOT;
  __device__ static unsigned scale_index(int tid) { return (unsigned)tid; }
  template <bool MULW>
  __device__ static void consume(f32x2 (&acc)[kQ / 2], u32x4 r, float sf, float c) {
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      acc[4 * w] = pk_term_add<MULW>(acc[4 * w], __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(r[w], sf, 0), c);
      acc[4 * w + 1] = pk_term_add<MULW>(acc[4 * w + 1], __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(r[w], sf, 1), c);
      acc[4 * w + 2] = pk_term_add<MULW>(acc[4 * w + 2], __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(r[w], sf, 2), c);
      acc[4 * w + 3] = pk_term_add<MULW>(acc[4 * w + 3], __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(r[w], sf, 3), c);
    }
  }
  // the element in the byte's nibble `odd`: shifted to the low nibble, the first of the pair
  __device__ static float one(unsigned byte, int odd, float sf) {
    return __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(byte >> (4 * odd), sf, 0)[0];
  }
};

// the conversions' scale operand: the float whose exponent field is the E8M0 byte
__device__ __forceinline__ float mx_scale(unsigned char x) { return __uint_as_float((unsigned)x << 23); }

// A whole slot of a segment whose data pointers are 16-byte aligned.  sm: kBlock * kC chunks (VOUT only).
template <int FMT, bool MULW, bool VOUT>
__device__ __forceinline__ void mx_sum_vec(const MSeg& sg, int64_t tl, const void* const* __restrict__ data,
                                           const void* const* __restrict__ sc, const double* __restrict__ coef, int k,
                                           u32x4* sm) {
  using F = Mx<FMT>;
  constexpr int U = kU, Q = F::kQ, C = F::kC;
  const int tid = (int)threadIdx.x;
  // uniform slot bases (a slot is FA_TILE_BYTES of data and E / 32 scale bytes) + the lane's 32-bit offsets
  const int64_t d0 = tl * FA_TILE_BYTES, x0 = tl * (F::E / FA_MX_BLOCK);
  const unsigned doff = (unsigned)tid * 16u, xoff = F::scale_index(tid);
  f32x2 acc[Q / 2];
#pragma unroll
  for (int j = 0; j < Q / 2; ++j) acc[j] = (f32x2){-0.0f, -0.0f};  // -0 + t == t bitwise for every t
  for (int i0 = 0; i0 < k; i0 += U) {
    u32x4 r[U];
    unsigned char x[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {  // the group's clients, clamped to the last one: every load unconditional
      const int i = min(i0 + u, k - 1);
      r[u] = gld_nt_off<u32x4>((const char*)data[i] + d0, doff);
      x[u] = gld_nt_off<unsigned char>((const char*)sc[i] + x0, xoff);
    }
    if (i0 + U <= k) {  // a whole group: no guard between the clients
#pragma unroll
      for (int u = 0; u < U; ++u)
        F::template consume<MULW>(acc, r[u], mx_scale(x[u]), MULW ? (float)coef[i0 + u] : 0.0f);
    } else {
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (i0 + u < k)  // wave-uniform
          F::template consume<MULW>(acc, r[u], mx_scale(x[u]), MULW ? (float)coef[i0 + u] : 0.0f);
    }
  }

  float* out = (float*)sg.out + tl * F::E;
  if constexpr (VOUT) {
    // chunk (lane l, j) = the lane's floats 4j .. 4j+3 goes to slot C * tid + ((j + l / kRot) & (C - 1)):
    // the 16 lanes that one LDS pass serves hit 16 different 16-byte bank groups, on the write and on the read
    constexpr int RS = F::kRotShift;
    const int l = tid & 63, wave0 = tid & ~63;
#pragma unroll
    for (int j = 0; j < C; ++j) {
      const f32x2 a = acc[2 * j], b = acc[2 * j + 1];
      sm[C * tid + ((j + (l >> RS)) & (C - 1))] =
          u32x4{__float_as_uint(a[0]), __float_as_uint(a[1]), __float_as_uint(b[0]), __float_as_uint(b[1])};
    }
    __syncthreads();
    // store j of a wave: its chunks 64 j .. 64 j + 63, one per lane = 1 KiB of consecutive bytes
    char* wout = (char*)(out + (int64_t)wave0 * Q);
#pragma unroll
    for (int j = 0; j < C; ++j) {
      const int c = j * 64 + l, sl = c / C, sj = c % C;
      const u32x4 v = sm[C * (wave0 + sl) + ((sj + (sl >> RS)) & (C - 1))];
      __builtin_nontemporal_store(v, (G4*)(wout + (int64_t)c * 16));
    }
  } else {
#pragma unroll
    for (int j = 0; j < Q; ++j) out[(unsigned)tid * Q + j] = acc[j >> 1][j & 1];
  }
}

// Any slot: byte loads, in passes of kPassE elements; element j of lane l is the pass's element
// j * kBlock + l (coalesced), so an FP4 lane's elements all sit in the nibble of l's parity.
template <int FMT, bool MULW>
__device__ __forceinline__ void mx_sum_elem(const MSeg& sg, int64_t tl, const void* const* __restrict__ data,
                                            const void* const* __restrict__ sc, const double* __restrict__ coef,
                                            int k) {
  using F = Mx<FMT>;
  const int tid = (int)threadIdx.x;
  for (int64_t e0 = tl * F::E; e0 < (tl + 1) * F::E && e0 < sg.numel; e0 += kPassE) {  // workgroup-uniform
    const unsigned rem = (unsigned)(sg.numel - e0 < kPassE ? sg.numel - e0 : kPassE);
    unsigned off[kPass], live = 0;
#pragma unroll
    for (int j = 0; j < kPass; ++j) {
      const unsigned e = (unsigned)(j * kBlock + tid);
      if (e < rem) live |= 1u << j;
      off[j] = e < rem ? e : rem - 1;  // clamped: every load unconditional
    }
    float acc[kPass];
#pragma unroll
    for (int j = 0; j < kPass; ++j) acc[j] = -0.0f;
    for (int i0 = 0; i0 < k; i0 += kUE) {
      unsigned char b[kUE][kPass], x[kUE][kPass];
#pragma unroll
      for (int u = 0; u < kUE; ++u) {
        const int i = min(i0 + u, k - 1);
        const void* db = (const char*)data[i] + e0 / F::EPB;  // e0 is a multiple of 4,096
        const void* xb = (const char*)sc[i] + e0 / FA_MX_BLOCK;
#pragma unroll
        for (int j = 0; j < kPass; ++j) {
          b[u][j] = gld_nt_off<unsigned char>(db, off[j] / F::EPB);
          x[u][j] = gld_nt_off<unsigned char>(xb, off[j] / FA_MX_BLOCK);
        }
      }
#pragma unroll
      for (int u = 0; u < kUE; ++u) {
        if (i0 + u < k) {  // wave-uniform
          const float c = MULW ? (float)coef[i0 + u] : 0.0f;
#pragma unroll
          for (int j = 0; j < kPass; ++j) {
            const float d = F::one(b[u][j], off[j] & 1u, mx_scale(x[u][j]));
            acc[j] = op_add(acc[j], MULW ? op_mul(d, c) : d);
          }
        }
      }
    }
    float* out = (float*)sg.out + e0;
#pragma unroll
    for (int j = 0; j < kPass; ++j)
      if (live >> j & 1u) out[j * kBlock + tid] = acc[j];
  }
}

// dptrs / sptrs: [segment][client] (MSeg.ptr_base); flags[j]: kDataAligned | kOutAligned of segment j.
// FP8: 4 waves per SIMD (128 VGPRs), kU clients of 17 bytes per lane in flight on each.  FP4: 3 waves (168
// VGPRs, 161 used): at 128 the compiler spills 44 - 220 bytes per lane inside the client loop.
template <int FMT, bool MULW>
__global__ void __launch_bounds__(kBlock, FMT == FA_MX_FP4 ? 3 : 4)
k_wsum_mx(const MSeg* __restrict__ segs, int nseg, const void* const* __restrict__ dptrs,
          const void* const* __restrict__ sptrs, const int* __restrict__ flags, const double* __restrict__ coef, int k) {
  __shared__ u32x4 sm[kBlock * Mx<FMT>::kC];
  const int64_t tile = xcd_tile_map(blockIdx.x, gridDim.x);
  const int si = nseg > 1 ? find_seg(segs, nseg, tile) : 0;
  const MSeg sg = segs[si];
  const int64_t tl = tile - sg.tile_start;
  const void* const* d = dptrs + sg.ptr_base;
  const void* const* sc = sptrs + sg.ptr_base;
  const int fl = flags[si];
  // workgroup-uniform: the barrier of the vector-store path is reached by all lanes or none
  if ((fl & kDataAligned) && (tl + 1) * Mx<FMT>::E <= sg.numel) {
    if (fl & kOutAligned) mx_sum_vec<FMT, MULW, true>(sg, tl, d, sc, coef, k, sm);
    else mx_sum_vec<FMT, MULW, false>(sg, tl, d, sc, coef, k, sm);
  } else {
    mx_sum_elem<FMT, MULW>(sg, tl, d, sc, coef, k);
  }
}

// One slot of the quantizer.  VEC: a whole slot, input and data 16-byte aligned.
template <int FMT, int DT, bool VEC>
__device__ __forceinline__ void mx_quant_slot(const MSeg& sg, int64_t tl, const void* __restrict__ in,
                                              unsigned char* __restrict__ scale) {
  using F = Mx<FMT>;
  using T = El<DT>;
  using S = typename T::S;
  constexpr int Q = F::kQ;
  const int tid = (int)threadIdx.x;
  const int64_t e0 = tl * F::E + (int64_t)tid * Q;  // the lane's first element
  float x[Q];
  if constexpr (VEC) {
#pragma unroll
    for (int v = 0; v < Q / T::V; ++v) {
      const u32x4 r = __builtin_nontemporal_load((const G4*)((const char*)in + e0 * T::SZ + v * 16));
      T::unpack(r, x + v * T::V);
    }
  } else {
#pragma unroll
    for (int j = 0; j < Q; ++j) {
      const int64_t e = e0 + j;
      const float v = T::from_bits(gld<S>(in, e < sg.numel ? e : sg.numel - 1));  // clamped: unconditional
      x[j] = e < sg.numel ? v : 0.0f;  // past the end: no part in the amax, a zero code
    }
  }
  // the bits of |x|: integer order == float order, NaN and Inf at or above 0x7f800000
  unsigned m = 0;
#pragma unroll
  for (int j = 0; j < Q; ++j) m = max(m, __float_as_uint(x[j]) & 0x7FFFFFFFu);
  if constexpr (Q < FA_MX_BLOCK) m = max(m, (unsigned)__shfl_xor((int)m, 1));  // FP8: the block's other half
  const bool bad = m >= 0x7F800000u;
  const int E = bad ? 128 : mx_shared_exp<FMT>(m);
  // 16 bytes of codes: FP8 one per byte, FP4 the even element in the low nibble
  constexpr int CB = 8 / F::EPB;  // bits per code
  u32x4 w;
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    unsigned word = 0;
#pragma unroll
    for (int t = 0; t < Q / 4; ++t) word |= mx_code<FMT>(__float_as_uint(x[v * (Q / 4) + t]), E) << (CB * t);
    w[v] = bad ? 0u : word;
  }
  if ((tid * Q) % FA_MX_BLOCK == 0 && e0 < sg.numel) scale[e0 / FA_MX_BLOCK] = (unsigned char)(E + 127);
  unsigned char* d = (unsigned char*)sg.out + e0 / F::EPB;
  if constexpr (VEC) {
    __builtin_nontemporal_store(w, (G4*)d);
  } else {
#pragma unroll
    for (int b = 0; b < 16; ++b)
      if (e0 + b * F::EPB < sg.numel) d[b] = (unsigned char)(w[b >> 2] >> (8 * (b & 3)));
  }
}

// ins[j]: the input of the table's segment j (MSeg.ptr_base); scales[j]: its scale bytes; MSeg.out: its
// data; MSeg.aligned: input and data are 16-byte aligned.
template <int FMT, int DT>
__global__ void __launch_bounds__(kBlock)
k_quantize_mx(const MSeg* __restrict__ segs, int nseg, const void* const* __restrict__ ins,
              void* const* __restrict__ scales) {
  const int64_t tile = blockIdx.x;
  const int si = nseg > 1 ? find_seg(segs, nseg, tile) : 0;
  const MSeg sg = segs[si];
  const int64_t tl = tile - sg.tile_start;
  const void* in = ins[sg.ptr_base];
  unsigned char* scale = (unsigned char*)scales[si];
  if (sg.aligned && (tl + 1) * Mx<FMT>::E <= sg.numel) mx_quant_slot<FMT, DT, true>(sg, tl, in, scale);
  else mx_quant_slot<FMT, DT, false>(sg, tl, in, scale);
}

// data and scale bytes at any alignment; the block is fixed
constexpr BlockFmt kMx{"data", FA_MX_BLOCK, FA_MX_BLOCK, 0, 0};

inline int fmt_check(const char* fn, fa_ctx* ctx, int fmt) {
  if (!ctx) return fail(FA_ERR_INVALID, "%s: ctx is NULL", fn);
  if (fmt != FA_MX_FP8 && fmt != FA_MX_FP4)
    return fail(FA_ERR_INVALID, "%s: fmt %d is not FA_MX_FP8 or FA_MX_FP4", fn, fmt);
  return FA_OK;
}

template <int FMT>
void launch_sum(int mode, dim3 grid, hipStream_t st, const MSeg* ds, int n, const void* const* dp,
                const void* const* dsc, const int* dfl, const double* dc, int k) {
  const dim3 blk(kBlock);
  if (mode == FA_MODE_MUL_W) hipLaunchKernelGGL((k_wsum_mx<FMT, true>), grid, blk, 0, st, ds, n, dp, dsc, dfl, dc, k);
  else hipLaunchKernelGGL((k_wsum_mx<FMT, false>), grid, blk, 0, st, ds, n, dp, dsc, dfl, dc, k);
}

template <int FMT>
void launch_quant(int dtype, dim3 grid, hipStream_t st, const MSeg* ds, int n, const void* const* dp,
                  void* const* dsc) {
  const dim3 blk(kBlock);
  switch (dtype) {
    case FA_DTYPE_F32: hipLaunchKernelGGL((k_quantize_mx<FMT, FA_DTYPE_F32>), grid, blk, 0, st, ds, n, dp, dsc); break;
    case FA_DTYPE_BF16: hipLaunchKernelGGL((k_quantize_mx<FMT, FA_DTYPE_BF16>), grid, blk, 0, st, ds, n, dp, dsc); break;
    default: hipLaunchKernelGGL((k_quantize_mx<FMT, FA_DTYPE_F16>), grid, blk, 0, st, ds, n, dp, dsc); break;
  }
}

}  // namespace

// The argument checks after fmt, the staged tables and the payload are blockq_host.h's.
extern "C" {

int fa_weighted_sum_mx(fa_ctx* ctx, int fmt, int mode, int32_t num_segments, const int64_t* seg_numel, int32_t k,
                       const void* const* d_data, const void* const* d_scale, const double* coef, void* const* d_out,
                       void* hip_stream) {
  const char* fn = "fa_weighted_sum_mx";
  if (const int rc = fmt_check(fn, ctx, fmt)) return rc;
  return block_sum_entry(
      fn, kMx, fmt == FA_MX_FP4 ? Mx<FA_MX_FP4>::E : Mx<FA_MX_FP8>::E, ctx, mode, num_segments, seg_numel, k,
      FA_MX_BLOCK, d_data, d_scale, coef, d_out, hip_stream,
      [&](dim3 grid, hipStream_t st, const MSeg* ds, int n, const void* const* dp, const void* const* dsc,
          const int* dfl, const double* dc, int) {
        if (fmt == FA_MX_FP4) launch_sum<FA_MX_FP4>(mode, grid, st, ds, n, dp, dsc, dfl, dc, k);
        else launch_sum<FA_MX_FP8>(mode, grid, st, ds, n, dp, dsc, dfl, dc, k);
      });
}

int fa_quantize_mx(fa_ctx* ctx, int fmt, int dtype, int32_t num_segments, const int64_t* seg_numel,
                   const void* const* d_in, void* const* d_data, void* const* d_scale, void* hip_stream) {
  const char* fn = "fa_quantize_mx";
  if (const int rc = fmt_check(fn, ctx, fmt)) return rc;
  return block_quant_entry(
      fn, kMx, fmt == FA_MX_FP4 ? Mx<FA_MX_FP4>::E : Mx<FA_MX_FP8>::E, ctx, dtype, num_segments, seg_numel,
      FA_MX_BLOCK, d_in, d_data, d_scale, hip_stream,
      [&](dim3 grid, hipStream_t st, const MSeg* ds, int n, const void* const* dp, void* const* dsc, int) {
        if (fmt == FA_MX_FP4) launch_quant<FA_MX_FP4>(dtype, grid, st, ds, n, dp, dsc);
        else launch_quant<FA_MX_FP8>(dtype, grid, st, ds, n, dp, dsc);
      });
}

}  // extern "C"
