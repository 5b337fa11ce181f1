// quant_gram.hip -- MI355X (gfx950) kernels + C ABI of the q8 Gram matrix and pairwise squared distances
// (include/fedagg_quant_gram.h: fa_pairwise_gram_q8): Krum's device pass straight on block-quantized int8
// uploads.  The contract and its op order are the header's.
//
// G_ij = sum_b s_i[b] s_j[b] I_ij[b]: the integer part I of a block is exact in int32 on
// v_mfma_i32_16x16x64_i8, the two scales go in through float64 with one fma per block, pair and lane.
//
// k_gram_q8: a workgroup (8 waves) owns a run of consecutive units (kUnit elements of one segment, all k
// clients; the split is the header's, a function of the segment sizes alone).  It walks the run in stages
// of W elements (W by k, so that a stage is <= 32 KB of q): the k clients' int8 rows of a stage lie in
// LDS row-major, row stride W + 16 bytes (the 16 rows that one 16-byte operand read touches then fall in
// 16 different bank groups), next to the stage's scales widened to float64, [block][client].  Two stages
// in LDS: the loads of stage s + 1 are issued into registers before the MFMAs of stage s and written
// after them, one barrier per stage.  Rows k .. 16 nt - 1 and everything past a segment's end are zero.
// The nt (nt + 1) / 2 upper-triangular pairs of 16-client tiles are dealt to the waves round-robin
// (pair p to wave p % 8: one pair for k <= 16, 36 pairs = at most 5 per wave for k = 128; PW, the
// pairs per wave, is the template parameter, so every accumulator has a fixed register).  Per pair the
// wave keeps 4 int32 and 4 float64 accumulators per lane; a block of B elements is B / 64 MFMAs into
// the int32 ones (across stages when B > W), then one scale step: acc64 = fma(s_i s_j, (double)I, acc64).
// Per-workgroup float64 slabs ([pair][16][16]) go to the scratch; k_gram_reduce adds them in a fixed
// order and writes both triangles of G; k_gram_dist forms D from G's bits (gram_common.h, shared with the
// q1 Gram kernel of signgram.hip, as are the work split and the staged tables).
// Numbers and the resource use: DESIGN.md (block-quantized family).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "fa_internal.h"
#include "fedagg_quant.h"
#include "blockq_host.h"
#include "gram_common.h"
#include "median_common.h"

using namespace fa_detail;

namespace {

constexpr int kGramThreads = 512, kGramWaves = kGramThreads / 64;
constexpr int kUnit = FA_Q8_GRAM_UNIT;
constexpr int kNI = 4;        // 16-byte items of q per thread and stage: 2,048 items = 32 KB at most
constexpr int kPad = 16;      // bytes between the rows of a stage
constexpr int kMaxPW = 5;     // 36 pairs on 8 waves
// the largest of 2 * 16 nt * (W + kPad) bytes of q (nt = 4, W = 512) + 2 * max(1, W / 64) * 16 nt float64 scales
constexpr int kGramLds = 2 * 128 * (256 + kPad) + 8192;
static_assert(kGramLds >= 2 * 64 * (512 + kPad) + 8192 && kGramLds >= 2 * 32 * (1024 + kPad) + 8192,
              "LDS of every plan");
static_assert(2 * kGramLds <= 160 * 1024, "two workgroups per CU");

typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr BlockFmt kQ8Gram{"q", FA_Q8_GRAM_BLOCK_MIN, FA_Q8_BLOCK_MAX, 0};

struct GramPlan { int nt, npairs, pw, W; };
GramPlan gram_plan(int k) {
  GramPlan p;
  p.nt = (k + 15) / 16;
  p.npairs = p.nt * (p.nt + 1) / 2;
  p.pw = (p.npairs + kGramWaves - 1) / kGramWaves;
  p.W = p.nt <= 2 ? 1024 : p.nt <= 4 ? 512 : FA_Q8_GRAM_STAGE_MIN;
  return p;
}

template <int PW>
__global__ void __launch_bounds__(kGramThreads)
k_gram_q8(const GSeg* __restrict__ segs, int nseg, const void* const* __restrict__ qptrs,
          const void* const* __restrict__ sptrs, int k, int nt, int W, int shift, int64_t nunits,
          double* __restrict__ partial) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[kGramLds];
  const int R = 16 * nt, S = W + kPad, B = 1 << shift;
  const int nbs = (W >> shift) > 0 ? (W >> shift) : 1;  // blocks (or the one part of a block) per stage
  unsigned char* lq = smem;                      // [2][R][S]
  double* lsc = (double*)(smem + 2 * R * S);     // [2][nbs][R]
  const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
  const int npairs = nt * (nt + 1) / 2;

  // staging roles, the same in every stage: item n is 16 bytes of client irow[n]; one scale per thread
  const int C = W / 16;
  int irow[kNI], icol[kNI];
  bool iact[kNI];
#pragma unroll
  for (int n = 0; n < kNI; ++n) {
    const int idx = t + n * kGramThreads;
    irow[n] = idx / C;
    icol[n] = idx % C;
    iact[n] = irow[n] < k;
  }
  const bool sact = t < nbs * R && t % R < k;
  const int sblk = t / R, srow = t % R;

  // rows k .. R - 1 of both buffers, q and scales, are zero; no stage writes them
  for (int idx = t; idx < 2 * (R - k) * (S / 4); idx += kGramThreads) {
    const int b = idx / ((R - k) * (S / 4)), r = idx / (S / 4) % (R - k), c = idx % (S / 4);
    ((unsigned*)lq)[((b * R + k + r) * S) / 4 + c] = 0u;
  }
  for (int idx = t; idx < 2 * nbs * R; idx += kGramThreads)
    if (idx % R >= k) lsc[idx] = 0.0;

  // the loader's position: unit lu of segment sg, stage at element le0 of the segment
  const int64_t u0 = nunits * blockIdx.x / gridDim.x, u1 = nunits * (blockIdx.x + 1) / gridDim.x;
  int64_t lu = u0, le0 = 0;
  int cseg = -1;
  GSeg sg{};
  const void* qp[kNI];
  const void* sp = nullptr;
  auto enter_unit = [&]() {
    const int sidx = nseg > 1 ? find_seg(segs, nseg, lu) : 0;
    if (sidx != cseg) {  // one set of pointer loads per segment
      cseg = sidx;
      sg = segs[sidx];
#pragma unroll
      for (int n = 0; n < kNI; ++n) qp[n] = iact[n] ? qptrs[sg.ptr_base + irow[n]] : nullptr;
      sp = sact ? sptrs[sg.ptr_base + srow] : nullptr;
    }
    le0 = (lu - sg.tile_start) * kUnit;
  };
  auto advance = [&]() {  // to the next stage of the unit that starts inside the segment, or the next unit
    le0 += W;
    if ((le0 & (kUnit - 1)) == 0 || le0 >= sg.numel) {
      ++lu;
      if (lu < u1) enter_unit();
    }
  };
  u32x4 rq[kNI];
  double rs = 0.0;
  auto load = [&]() {
#pragma unroll
    for (int n = 0; n < kNI; ++n) {
      rq[n] = u32x4{0u, 0u, 0u, 0u};
      if (!iact[n]) continue;
      const int64_t e = le0 + 16 * icol[n], left = sg.numel - e;
      if (left >= 16 && sg.aligned) {
        rq[n] = __builtin_nontemporal_load((const __attribute__((address_space(1))) u32x4*)((const char*)qp[n] + e));
      } else if (left > 0) {  // byte loads: the same 16 bytes, zeros past the segment's end
#pragma unroll
        for (int v = 0; v < 16; ++v)
          if (v < left) rq[n][v / 4] |= (unsigned)gld<unsigned char>(qp[n], e + v) << (8 * (v % 4));
      }
    }
    if (sact) {
      const int64_t b = (le0 >> shift) + sblk, nblk = (sg.numel + B - 1) >> shift;
      rs = b < nblk ? (double)gld<float>(sp, b) : 0.0;
    }
  };
  auto put = [&](int buf) {
#pragma unroll
    for (int n = 0; n < kNI; ++n)
      if (iact[n]) *(u32x4*)(lq + (buf * R + irow[n]) * S + 16 * icol[n]) = rq[n];
    if (sact) lsc[(buf * nbs + sblk) * R + srow] = rs;
  };

  // the wave's pairs
  int pti[PW], ptj[PW];
  i32x4 iacc[PW];
  double dacc[PW][4];
#pragma unroll
  for (int u = 0; u < PW; ++u) {
    pti[u] = ptj[u] = 0;
    if (wave + u * kGramWaves < npairs) pair_tiles(wave + u * kGramWaves, nt, pti[u], ptj[u]);
    iacc[u] = i32x4{0, 0, 0, 0};
#pragma unroll
    for (int r = 0; r < 4; ++r) dacc[u][r] = 0.0;
  }
  // v_mfma_i32_16x16x64_i8, D = A B + C with A 16 x 64, B 64 x 16 (int8) and C, D 16 x 16 (int32):
  //   A: lane l holds row l % 16, 16 consecutive k of the 64 in its 4 VGPRs, the group chosen by l / 16;
  //   B: lane l holds column l % 16, the same k group;
  //   D: lane l, VGPR r holds D[4 (l / 16) + r][l % 16].
  // Both operands are read from the same 16 bytes, 16 (l / 16) .. + 15 of the 64-element step, of their
  // client's row, so every k meets itself whichever order the hardware gives the 16 bytes of a group.
  const int kq = lane >> 4, lr = lane & 15;
  auto compute = [&](int buf, int64_t e0, int64_t numel) {
#pragma unroll
    for (int u = 0; u < PW; ++u) {
      if (wave + u * kGramWaves >= npairs) continue;  // wave-uniform
      const unsigned char* pa = lq + (buf * R + 16 * pti[u] + lr) * S + 16 * kq;
      const unsigned char* pb = lq + (buf * R + 16 * ptj[u] + lr) * S + 16 * kq;
      for (int j = 0; j < W; j += 64) {
        const i32x4 a = *(const i32x4*)(pa + j), b = *(const i32x4*)(pb + j);
        iacc[u] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, iacc[u], 0, 0, 0);
        const int64_t e = e0 + j + 64;
        if ((e & (B - 1)) == 0 || e >= numel) {  // the block ends here: its scale step
          const double* sc = lsc + (buf * nbs + (j >> shift)) * R;
          const double sj = sc[16 * ptj[u] + lr];
#pragma unroll
          for (int r = 0; r < 4; ++r)
            dacc[u][r] = __builtin_fma(sc[16 * pti[u] + 4 * kq + r] * sj, (double)iacc[u][r], dacc[u][r]);
          iacc[u] = i32x4{0, 0, 0, 0};
          if (e >= numel) break;
        }
      }
    }
  };

  bool have = u0 < u1;
  int64_t ce0 = 0, cnumel = 0;
  if (have) {
    enter_unit();
    load();
    put(0);
    ce0 = le0;
    cnumel = sg.numel;
    advance();
  }
  __syncthreads();
  for (int buf = 0; have; buf ^= 1) {
    const bool more = lu < u1;
    if (more) load();  // in flight during the MFMAs
    compute(buf, ce0, cnumel);
    if (more) {
      put(buf ^ 1);  // buffer buf ^ 1 was last read before the previous barrier
      ce0 = le0;
      cnumel = sg.numel;
      advance();
    }
    __syncthreads();
    have = more;
  }

  double* out = partial + (int64_t)blockIdx.x * npairs * 256;
#pragma unroll
  for (int u = 0; u < PW; ++u) {
    const int p = wave + u * kGramWaves;
    if (p >= npairs) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) out[p * 256 + (4 * kq + r) * 16 + lr] = dacc[u][r];
  }
}

}  // namespace

extern "C" {

size_t fa_pairwise_gram_q8_scratch_bytes(int32_t num_segments, const int64_t* seg_numel, int32_t k) {
  if (k < 1 || k > FA_Q8_GRAM_MAX_K || num_segments <= 0 || !seg_numel) return 0;
  for (int s = 0; s < num_segments; ++s)
    if (seg_numel[s] < 0) return 0;
  const int64_t nwg = gram_workgroups(gram_units(num_segments, seg_numel, kUnit), FA_Q8_GRAM_MIN_UNITS,
                                      FA_Q8_GRAM_MAX_WORKGROUPS);
  return sizeof(double) * ((size_t)nwg * gram_plan(k).npairs * 256 + (size_t)k * k);
}

int fa_pairwise_gram_q8(fa_ctx* ctx, int32_t num_segments, const int64_t* seg_numel, int32_t k, int32_t block,
                        const void* const* d_q, const void* const* d_scale, void* d_gram, void* d_dist,
                        void* d_scratch, size_t scratch_bytes, void* hip_stream) {
  const char* fn = "fa_pairwise_gram_q8";
  if (!ctx) return fail(FA_ERR_INVALID, "%s: ctx is NULL", fn);
  const int shift = block_shift(kQ8Gram, block);
  if (shift < 0) return block_fail(fn, kQ8Gram, block);
  if (k <= 0 || k > FA_Q8_GRAM_MAX_K || num_segments <= 0)
    return fail(FA_ERR_INVALID, "%s: k (1 .. %d) and num_segments must be positive", fn, FA_Q8_GRAM_MAX_K);
  if (!seg_numel || !d_q || !d_scale || !d_dist) return fail(FA_ERR_INVALID, "%s: a table is NULL", fn);
  int nseg = 0;
  for (int s = 0; s < num_segments; ++s) {
    if (seg_numel[s] < 0) return fail(FA_ERR_INVALID, "%s: segment %d has negative numel", fn, s);
    if (seg_numel[s] == 0) continue;
    for (int i = 0; i < k; ++i) {
      const int64_t t = (int64_t)s * k + i;
      if (!d_q[t]) return fail(FA_ERR_INVALID, "%s: segment %d client %d: q NULL", fn, s, i);
      if (!d_scale[t] || !al4(d_scale[t]))
        return fail(FA_ERR_INVALID, "%s: segment %d client %d: scale NULL or not 4-byte aligned", fn, s, i);
    }
    ++nseg;
  }
  const size_t need = fa_pairwise_gram_q8_scratch_bytes(num_segments, seg_numel, k);
  if (!d_scratch || ((uintptr_t)d_scratch & 7u) || scratch_bytes < need)
    return fail(FA_ERR_INVALID, "%s: scratch must hold %zu bytes, 8-byte aligned", fn, need);

  const GramPlan pl = gram_plan(k);
  const int64_t nunits = gram_units(num_segments, seg_numel, kUnit);
  const int nwg = (int)gram_workgroups(nunits, FA_Q8_GRAM_MIN_UNITS, FA_Q8_GRAM_MAX_WORKGROUPS);
  double* slabs = (double*)d_scratch;
  double* gram = d_gram ? (double*)d_gram : slabs + (size_t)nwg * pl.npairs * 256;
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(FA_ERR_HIP, "hipSetDevice(%d) failed", ctx->device);
  hipStream_t st = (hipStream_t)hip_stream;
  GramTables tb;
  if (nseg) {
    const int rc = gram_stage_tables(ctx, num_segments, seg_numel, k, nseg, kUnit, d_q, d_scale, st, &tb);
    if (rc) return rc;
    const dim3 grid((unsigned)nwg), blk(kGramThreads);
#define FA_GRAM(PW) \
  hipLaunchKernelGGL((k_gram_q8<PW>), grid, blk, 0, st, tb.segs, nseg, tb.data, tb.scale, (int)k, pl.nt, pl.W, shift, nunits, \
                     slabs)
    switch (pl.pw) {
      case 1: FA_GRAM(1); break;
      case 2: FA_GRAM(2); break;
      case 3: FA_GRAM(3); break;
      case 4: FA_GRAM(4); break;
      default: FA_GRAM(kMaxPW); break;
    }
#undef FA_GRAM
  }
  gram_reduce_dist(st, slabs, nwg, (int)k, pl.nt, gram, (double*)d_dist);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    if (tb.slot) (void)release(tb.slot, st);
    return fail(FA_ERR_HIP, "%s: %s", fn, hipGetErrorString(e));
  }
  return tb.slot ? release(tb.slot, st) : FA_OK;
}

}  // extern "C"
