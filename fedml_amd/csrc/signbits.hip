// signbits.hip -- MI355X (gfx950) kernels + C ABI of the 1-bit sign-compressed ("q1") client updates
// (include/fedagg_sign.h): fa_weighted_sum_q1, the fused decompress-and-sum; fa_sign_vote_q1, the
// majority vote on bit-sliced counters; fa_quantize_q1, the device quantizer that produces the format.
// The contracts and their op order are the header's; the host path is blockq_host.h's, shared with q8.
//
// k_wsum_q1: at 1/8 byte per element the ordered float sum is bound by the vector units, not by HBM, so
// the design is about instructions per client element.  A lane takes ONE 32-bit word per client: 32
// consecutive elements, which share one scale because B >= 32; a 256-lane workgroup owns 8,192 elements
// (1 KiB of bits per client).  A dword per lane is coalesced at any 4-byte alignment, so there is one
// load path.  kU clients' words and scales are in flight before any is consumed.  Per client word: the
// coefficient is folded into the scale (MUL_W), and the word is inverted when that c is negative, so
// that per element the term is "the low 31 bits of c under bit j of the word": one shift that brings
// bit j to bit 31 and one v_and_or_b32 ((shifted & 0x80000000) | |c|), then the add -- 3 vector ops per
// client element (2 for j = 31, which needs no shift).  The device code of this file is built without
// packed-FP32 instructions (DEVFLAGS_signbits in the Makefile).  A v_pk_add_f32 would round each half
// once and so keep the contract, but in the assembly the packed build is the worse one: it pairs the
// adds and then builds the terms with separate v_and_b32 and v_or_b32, 3.3 instead of 2.8 vector ops
// per client element, on 138 instead of 127 VGPRs (3 instead of 4 waves per SIMD).  The packed build
// was not run on the device.  A lane ends with 32 accumulators = 128 consecutive output bytes; a
// workgroup passes them through 32 KiB of LDS (an 8 x 8 rotation of 16-byte chunks between pairs of
// lanes, bank-conflict free on the write and on the read) so that every store instruction of a wave
// writes 1 KiB of consecutive bytes.  A ragged last slot, and an output that is only 4-byte aligned,
// take the same arithmetic with clamped loads and guarded element stores (the same bits).
//
// k_sign_vote_q1: integer until the last store.  A lane takes 16 bytes per client (128 elements), a
// workgroup 32,768 elements (4 KiB of bits per client).  The count of set bits per element lives in 12
// BIT-SLICED planes: plane p is a 32-bit word that holds bit p of the count for 32 elements, four words
// (one 16-byte load) side by side.  Eight clients at a time go through a carry-save tree (7 full
// adders, 2 three-input v_bitop3_b32 each) into the ones / twos / fours planes, and only the one carry
// word of weight 8 ripples through planes 3 .. 11: about 8 ops per client word, a quarter of an op per
// client element.  The decision never forms a per-element count: the planes
// are compared bitwise, most significant first, against the constants lo = (k - threshold) / 2 and
// hi = (k + threshold + 1) / 2, which gives a "positive" (neg <= lo) and a "negative" (neg >= hi) mask
// word per 32 elements.  The masks go through 8 KiB of LDS; then lane t of store i handles the 16-byte
// chunk 256 i + t of the slot's output: it reads the two mask words its 4 elements belong to (8
// neighbouring lanes read the same word, a broadcast) and builds each float from its two bits, so every
// store instruction of a wave writes 1 KiB of consecutive bytes.  Segments whose bits or output are
// not 16-byte aligned, and ragged last slots, take word loads at clamped indices and guarded stores.
//
// k_quantize_q1: a workgroup owns 8,192 elements, a lane 32 consecutive ones = one word of bits.  The
// lane reduces its 32 |x| as the balanced tree; a block of B elements spans B / 32 <= 32 lanes of ONE
// wave, and an xor-butterfly over them continues exactly that tree (an add is commutative, so both
// lanes of a pair hold the same bits).  The non-finite flag is a butterfly max on the bits of |x|, as
// in k_quantize_q8.  Not on the server's hot path.  Registers, LDS, instruction counts: DESIGN.md.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "blockq_host.h"
#include "elem.h"
#include "fa_internal.h"
#include "fedagg_sign.h"
#include "median_common.h"

using namespace fa_detail;

namespace {

constexpr int kW = 32;                        // elements per word = per lane of the sum and the quantizer
constexpr int64_t ES = (int64_t)kBlock * kW;  // their slot's elements
constexpr int kU = 8;                         // clients whose loads are in flight together
constexpr int kVW = 4;                        // words per lane and client of the vote: one 16-byte load
constexpr int64_t EV = (int64_t)kBlock * kVW * 32;  // the vote's slot
constexpr int kPlanes = 12;                   // bits of a count <= FA_Q1_VOTE_MAX_K
static_assert(ES == FA_Q1_SUM_SLOT && EV == FA_Q1_VOTE_SLOT && kU == FA_Q1_GROUP, "fedagg_sign.h states the split");
static_assert(FA_Q1_VOTE_MAX_K < (1 << kPlanes), "a count fits the planes");
static_assert(ES % FA_Q1_BLOCK_MAX == 0, "a slot starts a block");

using G4 = __attribute__((address_space(1))) u32x4;

// acc += one client's 32 elements: c under the word's bits
__device__ __forceinline__ void q1_consume(float (&acc)[kW], unsigned w, float c) {
  const unsigned cb = __float_as_uint(c);
  const unsigned wp = w ^ (unsigned)((int)cb >> 31);  // c < 0: a set bit gives +|c|
#pragma unroll
  for (int j = 0; j < kW; ++j) {
    const unsigned t = (cb & 0x7FFFFFFFu) | ((wp << (31 - j)) & 0x80000000u);  // v_lshlrev + v_and_or
    acc[j] = op_add(acc[j], __uint_as_float(t));
  }
}

// One slot.  FULL: a whole slot with a 16-byte aligned output (sm: kBlock * 8 chunks, FULL only).
template <bool MULW, bool FULL>
__device__ __forceinline__ void q1_sum_slot(const MSeg& sg, int64_t tl, const void* const* __restrict__ bits,
                                            const void* const* __restrict__ sc, const double* __restrict__ coef,
                                            int k, int shift, u32x4* sm) {
  constexpr int U = kU;
  const int tid = (int)threadIdx.x;
  const int64_t s0 = tl * ES;  // the slot's first element; its first word is tl * kBlock
  const unsigned rem = FULL ? (unsigned)ES : (unsigned)(sg.numel - s0 < ES ? sg.numel - s0 : ES);
  // the lane's word, clamped to the slot's last one: every load unconditional
  const unsigned wi = FULL ? (unsigned)tid : min((unsigned)tid, ((rem + 31u) >> 5) - 1u);
  const unsigned woff = wi * 4u;
  const unsigned soff = ((wi * (unsigned)kW) >> shift) * 4u;  // its block's scale (ES is a multiple of B)
  float acc[kW];
#pragma unroll
  for (int j = 0; j < kW; ++j) acc[j] = -0.0f;  // -0 + t == t bitwise for every t
  for (int i0 = 0; i0 < k; i0 += U) {
    unsigned r[U];
    float s[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {  // the group's clients, clamped to the last one
      const int i = min(i0 + u, k - 1);
      r[u] = gld_nt_off<unsigned>((const unsigned*)bits[i] + tl * kBlock, woff);
      s[u] = gld_nt_off<float>((const float*)sc[i] + (s0 >> shift), soff);
    }
    if (i0 + U <= k) {  // a whole group: no guard between the clients
#pragma unroll
      for (int u = 0; u < U; ++u) q1_consume(acc, r[u], MULW ? op_mul(s[u], (float)coef[i0 + u]) : s[u]);
    } else {
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (i0 + u < k) q1_consume(acc, r[u], MULW ? op_mul(s[u], (float)coef[i0 + u]) : s[u]);  // wave-uniform
    }
  }

  float* out = (float*)sg.out + s0;
  if constexpr (FULL) {
    // chunk (lane l, j) = the lane's floats 4j .. 4j+3 goes to slot 8 * tid + ((j + l / 2) & 7): the 16
    // lanes that one LDS pass serves hit 16 different 16-byte bank groups, on the write and on the read
    const int l = tid & 63, wave0 = tid & ~63;
#pragma unroll
    for (int j = 0; j < 8; ++j) sm[8 * tid + ((j + (l >> 1)) & 7)] = El<FA_DTYPE_F32>::pack(acc + 4 * j);
    __syncthreads();
    // store j of a wave: its chunks 64 j .. 64 j + 63, one per lane = 1 KiB of consecutive bytes
    char* wout = (char*)(out + (int64_t)wave0 * kW);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = j * 64 + l, sl = c >> 3, sj = c & 7;
      const u32x4 v = sm[8 * (wave0 + sl) + ((sj + (sl >> 1)) & 7)];
      __builtin_nontemporal_store(v, (G4*)(wout + (int64_t)c * 16));
    }
  } else {
    const unsigned e = (unsigned)tid * kW;
#pragma unroll
    for (int j = 0; j < kW; ++j)
      if (e + j < rem) out[e + j] = acc[j];
  }
}

// bptrs / sptrs: [segment][client] (MSeg.ptr_base); flags[j]: kOutAligned of segment j.
template <bool MULW>
__global__ void __launch_bounds__(kBlock)
k_wsum_q1(const MSeg* __restrict__ segs, int nseg, const void* const* __restrict__ bptrs,
          const void* const* __restrict__ sptrs, const int* __restrict__ flags, const double* __restrict__ coef, int k,
          int shift) {
  __shared__ u32x4 sm[kBlock * 8];
  const int64_t tile = xcd_tile_map(blockIdx.x, gridDim.x);
  const int si = nseg > 1 ? find_seg(segs, nseg, tile) : 0;
  const MSeg sg = segs[si];
  const int64_t tl = tile - sg.tile_start;
  const void* const* b = bptrs + sg.ptr_base;
  const void* const* sc = sptrs + sg.ptr_base;
  // workgroup-uniform: the barrier of the vector-store path is reached by all lanes or none
  if ((flags[si] & kOutAligned) && (tl + 1) * ES <= sg.numel) q1_sum_slot<MULW, true>(sg, tl, b, sc, coef, k, shift, sm);
  else q1_sum_slot<MULW, false>(sg, tl, b, sc, coef, k, shift, sm);
}

// ---------------------------------------------------------------------------------------------------
// the vote

// full adder on whole words: (hi, lo) = a + b + c per bit position
__device__ __forceinline__ void csa(u32x4& hi, u32x4& lo, u32x4 a, u32x4 b, u32x4 c) {
  const u32x4 u = a ^ b;
  hi = (a & b) | (u & c);
  lo = u ^ c;
}

// P += the bits of clients 0 .. k-1 of this lane's kVW words.  VEC: one 16-byte load per client at byte
// offset off[0]; else word loads at the clamped byte offsets off[0 .. 3].
template <bool VEC>
__device__ __forceinline__ void vote_count(u32x4 (&P)[kPlanes], const void* const* __restrict__ bits, int64_t word0,
                                           const unsigned (&off)[kVW], int k) {
  constexpr int U = kU;
  for (int i0 = 0; i0 < k; i0 += U) {
    u32x4 r[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = min(i0 + u, k - 1);
      const void* base = (const unsigned*)bits[i] + word0;
      if constexpr (VEC) {
        r[u] = gld_nt_off<u32x4>(base, off[0]);
      } else {
#pragma unroll
        for (int v = 0; v < kVW; ++v) r[u][v] = gld_nt_off<unsigned>(base, off[v]);
      }
    }
#pragma unroll
    for (int u = 1; u < U; ++u)
      if (i0 + u >= k) r[u] = u32x4{0, 0, 0, 0};  // wave-uniform: a client past the last adds nothing
    u32x4 ta, tb, fa, fb, c;
    csa(ta, P[0], P[0], r[0], r[1]);
    csa(tb, P[0], P[0], r[2], r[3]);
    csa(fa, P[1], P[1], ta, tb);
    csa(ta, P[0], P[0], r[4], r[5]);
    csa(tb, P[0], P[0], r[6], r[7]);
    csa(fb, P[1], P[1], ta, tb);
    csa(c, P[2], P[2], fa, fb);
#pragma unroll
    for (int p = 3; p < kPlanes; ++p) {  // the carry of weight 8 ripples up
      const u32x4 t = P[p] & c;
      P[p] ^= c;
      c = t;
    }
  }
}

// lt: count < v, eq: count == v, per bit position, for a wave-uniform v
__device__ __forceinline__ void vote_compare(const u32x4 (&P)[kPlanes], unsigned v, u32x4& lt, u32x4& eq) {
  lt = u32x4{0, 0, 0, 0};
  eq = ~lt;
#pragma unroll
  for (int p = kPlanes - 1; p >= 0; --p) {
    const unsigned cw = 0u - ((v >> p) & 1u);  // all ones where v has bit p
    lt |= eq & ~P[p] & cw;
    eq &= ~(P[p] ^ cw);
  }
}

// lo = (k - threshold) / 2: net >= threshold <=> neg <= lo;  hi = (k + threshold + 1) / 2: net <=
// -threshold <=> neg >= hi.  lo < hi, so no element is both.  MSeg.aligned: bits and output are 16-byte aligned.
__global__ void __launch_bounds__(kBlock)
k_sign_vote_q1(const MSeg* __restrict__ segs, int nseg, const void* const* __restrict__ bptrs, int k, unsigned lo,
               unsigned hi, float step) {
  __shared__ u32x4 sm[kBlock * 2];  // the positive masks, then the negative ones
  const int tid = (int)threadIdx.x;
  const int64_t tile = xcd_tile_map(blockIdx.x, gridDim.x);
  const int si = nseg > 1 ? find_seg(segs, nseg, tile) : 0;
  const MSeg sg = segs[si];
  const int64_t tl = tile - sg.tile_start;
  const void* const* b = bptrs + sg.ptr_base;
  const int64_t s0 = tl * EV;
  const unsigned rem = (unsigned)(sg.numel - s0 < EV ? sg.numel - s0 : EV);
  const int64_t word0 = tl * (kBlock * kVW);
  u32x4 P[kPlanes];
#pragma unroll
  for (int p = 0; p < kPlanes; ++p) P[p] = u32x4{0, 0, 0, 0};
  unsigned off[kVW];
  if (sg.aligned && rem == EV) {
    off[0] = (unsigned)tid * 16u;
    vote_count<true>(P, b, word0, off, k);
  } else {
    const unsigned last = ((rem + 31u) >> 5) - 1u;  // the slot's last word
#pragma unroll
    for (int v = 0; v < kVW; ++v) off[v] = min((unsigned)tid * kVW + v, last) * 4u;
    vote_count<false>(P, b, word0, off, k);
  }
  u32x4 lt, eq;
  vote_compare(P, lo, lt, eq);
  sm[tid] = lt | eq;
  vote_compare(P, hi, lt, eq);
  sm[kBlock + tid] = ~lt;
  __syncthreads();

  const unsigned* pos = (const unsigned*)sm;
  const unsigned* neg = pos + kBlock * kVW;
  const unsigned sb = __float_as_uint(step);
  float* out = (float*)sg.out + s0;
  constexpr int kStores = (int)(EV / 4 / kBlock);  // 16-byte chunks per lane
#pragma unroll 4
  for (int it = 0; it < kStores; ++it) {
    const unsigned c = (unsigned)it * kBlock + tid, e = 4u * c;  // the chunk and its first element
    if ((unsigned)it * kBlock * 4u >= rem) break;                // workgroup-uniform
    const unsigned sh = e & 31u;
    const unsigned nw = neg[c >> 3] >> sh, aw = (pos[c >> 3] >> sh) | nw;
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned any = 0u - ((aw >> j) & 1u);  // all ones where the element votes
      v[j] = __uint_as_float(any & (sb ^ ((nw << (31 - j)) & 0x80000000u)));
    }
    if (sg.aligned && e + 3 < rem) {
      __builtin_nontemporal_store(El<FA_DTYPE_F32>::pack(v), (G4*)(out + e));
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (e + j < rem) out[e + j] = v[j];
    }
  }
}

// ---------------------------------------------------------------------------------------------------
// the quantizer

// One slot.  VEC: a whole slot, input 16-byte aligned.
template <int DT, bool VEC>
__device__ __forceinline__ void q1_quant_slot(const MSeg& sg, int64_t tl, const void* __restrict__ in,
                                              float* __restrict__ scale, int shift) {
  using T = El<DT>;
  using S = typename T::S;
  const int tid = (int)threadIdx.x;
  const int64_t e0 = tl * ES + (int64_t)tid * kW;  // the lane's first element
  float x[kW];
  if constexpr (VEC) {
#pragma unroll
    for (int v = 0; v < kW / T::V; ++v) {
      const u32x4 r = __builtin_nontemporal_load((const G4*)((const char*)in + e0 * T::SZ + v * 16));
      T::unpack(r, x + v * T::V);
    }
  } else {
#pragma unroll
    for (int j = 0; j < kW; ++j) {
      const int64_t e = e0 + j;
      const float v = T::from_bits(gld<S>(in, e < sg.numel ? e : sg.numel - 1));  // clamped: unconditional
      x[j] = e < sg.numel ? v : 0.0f;  // past the end: a +0 leaf and a clear bit
    }
  }
  unsigned m = 0, word = 0;
  float a[kW];
#pragma unroll
  for (int j = 0; j < kW; ++j) {
    const unsigned u = __float_as_uint(x[j]);
    m = max(m, u & 0x7FFFFFFFu);  // the bits of |x|: NaN and Inf at or above 0x7f800000
    word |= (u >> 31) << j;
    a[j] = __uint_as_float(u & 0x7FFFFFFFu);
  }
  // the balanced tree: the lane's 32 leaves, then the block's lanes
#pragma unroll
  for (int w = kW / 2; w >= 1; w >>= 1) {
#pragma unroll
    for (int j = 0; j < w; ++j) a[j] = op_add(a[2 * j], a[2 * j + 1]);
  }
  float sum = a[0];
  const int lanes = 1 << (shift - 5);  // of one block: 1 .. 32, a power of two, inside one wave
  for (int o = 1; o < lanes; o <<= 1) {
    m = max(m, (unsigned)__shfl_xor((int)m, o));
    sum = op_add(sum, __shfl_xor(sum, o));
  }
  const bool bad = m >= 0x7F800000u;
  const int64_t b0 = (e0 >> shift) << shift;  // the block's first element
  const int64_t left = sg.numel - b0;
  const float count = (float)(left < ((int64_t)1 << shift) ? (left > 1 ? left : 1) : (int64_t)1 << shift);
  const float s = bad ? __uint_as_float(0x7FC00000u) : op_div(sum, count);
  if (e0 < sg.numel) {
    if ((tid & (lanes - 1)) == 0) scale[e0 >> shift] = s;
    ((unsigned*)sg.out)[e0 >> 5] = bad ? 0u : word;
  }
}

// ins[j]: the input of the table's segment j (MSeg.ptr_base); scales[j]: its scales; MSeg.out: its bits;
// MSeg.aligned: input and bits are 16-byte aligned.
template <int DT>
__global__ void __launch_bounds__(kBlock)
k_quantize_q1(const MSeg* __restrict__ segs, int nseg, const void* const* __restrict__ ins,
              void* const* __restrict__ scales, int shift) {
  const int64_t tile = blockIdx.x;
  const int si = nseg > 1 ? find_seg(segs, nseg, tile) : 0;
  const MSeg sg = segs[si];
  const int64_t tl = tile - sg.tile_start;
  const void* in = ins[sg.ptr_base];
  float* scale = (float*)scales[si];
  if (sg.aligned && (tl + 1) * ES <= sg.numel) q1_quant_slot<DT, true>(sg, tl, in, scale, shift);
  else q1_quant_slot<DT, false>(sg, tl, in, scale, shift);
}

constexpr BlockFmt kQ1{"bits", FA_Q1_BLOCK_MIN, FA_Q1_BLOCK_MAX, 3};

}  // namespace

extern "C" {

int fa_weighted_sum_q1(fa_ctx* ctx, int mode, int32_t num_segments, const int64_t* seg_numel, int32_t k, int32_t block,
                       const void* const* d_bits, const void* const* d_scale, const double* coef, void* const* d_out,
                       void* hip_stream) {
  return block_sum_entry(
      "fa_weighted_sum_q1", kQ1, ES, ctx, mode, num_segments, seg_numel, k, block, d_bits, d_scale, coef, d_out,
      hip_stream,
      [&](dim3 grid, hipStream_t st, const MSeg* ds, int n, const void* const* dp, const void* const* dsc,
          const int* dfl, const double* dc, int shift) {
        const dim3 blk(kBlock);
        if (mode == FA_MODE_MUL_W) hipLaunchKernelGGL((k_wsum_q1<true>), grid, blk, 0, st, ds, n, dp, dsc, dfl, dc, k, shift);
        else hipLaunchKernelGGL((k_wsum_q1<false>), grid, blk, 0, st, ds, n, dp, dsc, dfl, dc, k, shift);
      });
}

int fa_quantize_q1(fa_ctx* ctx, int dtype, int32_t num_segments, const int64_t* seg_numel, int32_t block,
                   const void* const* d_in, void* const* d_bits, void* const* d_scale, void* hip_stream) {
  return block_quant_entry(
      "fa_quantize_q1", kQ1, ES, ctx, dtype, num_segments, seg_numel, block, d_in, d_bits, d_scale, hip_stream,
      [&](dim3 grid, hipStream_t st, const MSeg* ds, int n, const void* const* dp, void* const* dsc, int shift) {
        const dim3 blk(kBlock);
        switch (dtype) {
          case FA_DTYPE_F32: hipLaunchKernelGGL((k_quantize_q1<FA_DTYPE_F32>), grid, blk, 0, st, ds, n, dp, dsc, shift); break;
          case FA_DTYPE_BF16: hipLaunchKernelGGL((k_quantize_q1<FA_DTYPE_BF16>), grid, blk, 0, st, ds, n, dp, dsc, shift); break;
          default: hipLaunchKernelGGL((k_quantize_q1<FA_DTYPE_F16>), grid, blk, 0, st, ds, n, dp, dsc, shift); break;
        }
      });
}

int fa_sign_vote_q1(fa_ctx* ctx, int32_t num_segments, const int64_t* seg_numel, int32_t k, const void* const* d_bits,
                    int32_t threshold, double step, void* const* d_out, void* hip_stream) {
  const char* fn = "fa_sign_vote_q1";
  if (!ctx) return fail(FA_ERR_INVALID, "%s: ctx is NULL", fn);
  if (k <= 0 || k > FA_Q1_VOTE_MAX_K || num_segments <= 0)
    return fail(FA_ERR_INVALID, "%s: k must be in [1, %d] and num_segments positive (k = %d)", fn, FA_Q1_VOTE_MAX_K, k);
  if (!seg_numel || !d_bits || !d_out) return fail(FA_ERR_INVALID, "%s: a table is NULL", fn);
  if (threshold < 1 || threshold > k)
    return fail(FA_ERR_INVALID, "%s: threshold %d is not in [1, k = %d]", fn, threshold, k);
  int nseg = 0;
  int64_t tiles = 0;
  for (int s = 0; s < num_segments; ++s) {
    if (seg_numel[s] < 0) return fail(FA_ERR_INVALID, "%s: segment %d has negative numel", fn, s);
    if (seg_numel[s] == 0) continue;
    if (!d_out[s] || !al4(d_out[s]))
      return fail(FA_ERR_INVALID, "%s: segment %d: output NULL or not 4-byte aligned", fn, s);
    for (int i = 0; i < k; ++i)
      if (!data_ok(kQ1, d_bits[(int64_t)s * k + i]))
        return fail(FA_ERR_INVALID, "%s: segment %d client %d: bits NULL or not 4-byte aligned", fn, s, i);
    ++nseg;
    tiles += (seg_numel[s] + EV - 1) / EV;
  }
  if (tiles > 0x7FFFFFFFll) return fail(FA_ERR_INVALID, "%s: too many tiles", fn);
  if (nseg == 0) return FA_OK;
  const ColArgs a{fn, ctx, FA_DTYPE_F32, num_segments, seg_numel, k, d_bits, 0, d_out, hip_stream};
  const unsigned lo = (unsigned)(k - threshold) / 2u, hi = (unsigned)(k + threshold + 1) / 2u;
  return col_stage_launch(
      a, EV, nseg, tiles, 0, [](void*) {},
      [&](dim3 grid, hipStream_t st, const MSeg* ds, int n, const void* const* dp, const void*) {
        hipLaunchKernelGGL(k_sign_vote_q1, grid, dim3(kBlock), 0, st, ds, n, dp, k, lo, hi, (float)step);
      });
}

}  // extern "C"
