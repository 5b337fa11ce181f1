// signgram.hip -- MI355X (gfx950) kernel + C ABI of the q1 Gram matrix and pairwise squared distances
// (include/fedagg_sign_gram.h: fa_pairwise_gram_q1): Krum's device pass straight on 1-bit sign uploads.
// The contract and its op order are the header's.
//
// G_ij = sum_b s_i[b] s_j[b] I_ij[b] with I = n_b - 2 popcount(w_i ^ w_j): at 1/8 byte per element the
// kernel is bound by the vector units, so the design is about instructions per pair and word.  One XOR and
// one accumulating v_bcnt_u32_b32 take 32 elements of a pair, with no expansion of the bits.
//
// k_gram_q1: a workgroup owns a run of consecutive units (kUnit elements of one segment, all k clients;
// the split is the header's, a function of the segment sizes alone).  It walks the run in stages of 16
// words (512 elements): the k clients' words of a stage lie in LDS row-major, row stride 20 words (the 8
// rows that one 16-byte operand read touches, consecutive clients, then fall in 8 different 16-byte bank
// groups), next to the stage's scales widened to float64 once, [block][client] with the client stride
// padded by 2.  Bits past a segment's end are masked when a stage is written, words past it and rows
// k .. R - 1 are zero, so a count only ever sees real elements.  Two stages in LDS: the loads of stage
// s + 1 are issued into registers before the arithmetic of stage s and written after it, one barrier per
// stage.
// LANES OWN PAIRS: a wave takes a 32 x 32 tile of clients as 8 x 8 lanes of 4 x 4 pairs, lane (li, lj)
// the clients li + 8 r against lj + 8 c.  Per group of four words it reads 4 + 4 operands with
// ds_read_b128 (the lanes of a row or a column read one address: a broadcast) and does 64 XORs and 64
// accumulating counts; a block's I is complete in the lane's own integer accumulator when the block ends,
// so no cross-lane step sits before the scale step: I = n_b - 2 pop, one convert, one multiply and one
// fma per owned pair.  The words per block (WPB) are a template parameter, so the block ends are known at
// compile time and a block's first count takes 0 as its addend; only blocks of 1024 (two stages) carry
// the integer accumulators across a stage.  Each of the nt (nt + 1) / 2 upper-triangular pairs of
// 32-client tiles has a wave of its own -- 10 waves for k = 128, where 10 pairs on 8 or on 5 waves would
// leave a wave with twice the work of another -- and the workgroup is launched with as many waves as the
// pairs and the staging (one 16-byte item per thread) need: 2 for k <= 32, 4 for k = 64, 10 for k = 128.
// A wave's tile leaves as four (three on the diagonal) of quant_gram.hip's [16][16] float64 slabs, so the
// reduction and the distance kernel are gram_common.h's, shared with q8.
// Numbers and the resource use: DESIGN.md (1-bit sign family).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "blockq_host.h"
#include "fa_internal.h"
#include "fedagg_sign_gram.h"
#include "gram_common.h"
#include "median_common.h"

using namespace fa_detail;

namespace {

constexpr int kMaxThreads = 640;            // one wave per tile pair: 10 at k = 128
constexpr int kUnit = FA_Q1_GRAM_UNIT;
constexpr int kSW = FA_Q1_GRAM_STAGE / 32;  // words of a client per stage
constexpr int kRowW = kSW + 4;              // words between the rows of a stage
static_assert(kUnit % FA_Q1_BLOCK_MAX == 0 && kUnit % FA_Q1_GRAM_STAGE == 0, "a unit starts a block and a stage");
static_assert(kMaxThreads >= FA_Q1_GRAM_MAX_K * (kSW / 4), "every 16-byte item of a stage has a thread");

constexpr BlockFmt kQ1Gram{"bits", FA_Q1_BLOCK_MIN, FA_Q1_BLOCK_MAX, 3};

struct GramPlan { int nt, npairs, threads, nt16, np16; };
GramPlan gram_plan(int k) {
  GramPlan p;
  p.nt = (k + 31) / 32;
  p.npairs = p.nt * (p.nt + 1) / 2;
  // a wave per pair, a thread per 16-byte item of a stage (that also covers the scales' two threads per client)
  p.threads = 64 * std::max(p.npairs, (k * (kSW / 4) + 63) / 64);
  p.nt16 = 2 * p.nt;
  p.np16 = p.nt16 * (p.nt16 + 1) / 2;
  return p;
}
// blocks of a stage that hold their own scale: 16 words / (B / 32), one for B >= 512
constexpr int stage_blocks(int wpb) { return kSW / wpb; }
size_t gram_lds(int nt, int wpb) {
  const size_t R = 32 * (size_t)nt;
  return 2 * R * kRowW * sizeof(unsigned) + 2 * (size_t)stage_blocks(wpb) * (R + 2) * sizeof(double);
}

// WPB: words per block, 1 .. 8, or 16 = the whole stage for B >= 512 (a block of 1024 ends every other stage)
template <int WPB>
__global__ void __launch_bounds__(kMaxThreads)
k_gram_q1(const GSeg* __restrict__ segs, int nseg, const void* const* __restrict__ bptrs,
          const void* const* __restrict__ sptrs, int k, int nt, int shift, int64_t nunits,
          double* __restrict__ partial) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int NBS = stage_blocks(WPB), PER = NBS < 8 ? NBS : 8, SP = NBS / PER;  // scales per thread, threads per client
  static_assert(SP <= kSW / 4, "the scales' threads are among the items' threads");
  const int R = 32 * nt, RS = R + 2, B = 1 << shift;
  unsigned* lw = (unsigned*)smem;                                      // [2][R][kRowW]
  double* lsc = (double*)(smem + 2 * R * kRowW * sizeof(unsigned));    // [2][NBS][RS]
  const int t = (int)threadIdx.x, nthr = (int)blockDim.x, lane = t & 63, wave = t >> 6;
  const int npairs = nt * (nt + 1) / 2;

  // staging roles, the same in every stage: thread t takes 4 words of client irow; PER scales of client srow
  const int irow = t / (kSW / 4), icol = t % (kSW / 4);
  const bool iact = irow < k;
  const int srow = t / SP, spart = t % SP;
  const bool sact = srow < k;

  // rows k .. R - 1 of both buffers, words and scales (and the scales' two pad columns), are zero
  for (int idx = t; idx < 2 * (R - k) * kRowW; idx += nthr) {
    const int b = idx / ((R - k) * kRowW), r = idx / kRowW % (R - k), c = idx % kRowW;
    lw[(b * R + k + r) * kRowW + c] = 0u;
  }
  for (int idx = t; idx < 2 * NBS * RS; idx += nthr)
    if (idx % RS >= k) lsc[idx] = 0.0;

  // the loader's position: unit lu of segment sg, stage at element le0 of the segment
  const int64_t u0 = nunits * blockIdx.x / gridDim.x, u1 = nunits * (blockIdx.x + 1) / gridDim.x;
  int64_t lu = u0, le0 = 0;
  int cseg = -1;
  GSeg sg{};
  const void* bp = nullptr;
  const void* sp = nullptr;
  auto enter_unit = [&]() {
    const int sidx = nseg > 1 ? find_seg(segs, nseg, lu) : 0;
    if (sidx != cseg) {  // one set of pointer loads per segment
      cseg = sidx;
      sg = segs[sidx];
      bp = iact ? bptrs[sg.ptr_base + irow] : nullptr;
      sp = sact ? sptrs[sg.ptr_base + srow] : nullptr;
    }
    le0 = (lu - sg.tile_start) * kUnit;
  };
  auto advance = [&]() {  // to the next stage of the unit that starts inside the segment, or the next unit
    le0 += FA_Q1_GRAM_STAGE;
    if ((le0 & (kUnit - 1)) == 0 || le0 >= sg.numel) {
      ++lu;
      if (lu < u1) enter_unit();
    }
  };
  u32x4 rq;
  float rs[PER];
  auto load = [&]() {
    rq = u32x4{0u, 0u, 0u, 0u};
    if (iact) {
      const int64_t nw = (sg.numel + 31) >> 5, w = (le0 >> 5) + 4 * icol, left = nw - w;
      if (left >= 4 && sg.aligned) {
        rq = __builtin_nontemporal_load((const __attribute__((address_space(1))) u32x4*)((const unsigned*)bp + w));
      } else {  // dword loads: the same words, zeros past the segment's last
#pragma unroll
        for (int v = 0; v < 4; ++v)
          if (v < left) rq[v] = gld<unsigned>(bp, w + v);
      }
      const int64_t rem = sg.numel - 32 * w;  // real elements from this item's first bit on
      if (rem < 128) {                        // the segment ends here: its last word's other bits do not count
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int64_t r = rem - 32 * v;
          if (r < 32) rq[v] &= r <= 0 ? 0u : (1u << r) - 1u;
        }
      }
    }
    if (sact) {
      const int64_t b0 = (le0 >> shift) + spart * PER, nblk = (sg.numel + B - 1) >> shift;
#pragma unroll
      for (int v = 0; v < PER; ++v) rs[v] = b0 + v < nblk ? gld<float>(sp, b0 + v) : 0.0f;
    }
  };
  auto put = [&](int buf) {
    if (iact) *(u32x4*)(lw + (buf * R + irow) * kRowW + 4 * icol) = rq;
    if (sact) {
#pragma unroll
      for (int v = 0; v < PER; ++v) lsc[(buf * NBS + spart * PER + v) * RS + srow] = (double)rs[v];
    }
  };

  // the wave's tile pair; lane (li, lj) owns the clients li + 8 r of tile pti against lj + 8 c of tile ptj
  const bool cact = wave < npairs;  // wave-uniform: the other waves only stage
  const int li = lane >> 3, lj = lane & 7;
  int pti = 0, ptj = 0;
  if (cact) pair_tiles(wave, nt, pti, ptj);
  int pop[4][4];
  double dacc[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      pop[r][c] = 0;
      dacc[r][c] = 0.0;
    }
  // the block that ends at element eend: acc = fma(s_i s_j, (double)(n_b - 2 pop), acc) for the 16 owned pairs
  auto scale_step = [&](const double* sc, int64_t eend, int64_t numel) {
    const int64_t left = numel - (((eend - 1) >> shift) << shift);  // from the block's first element on
    const int nb = left >= B ? B : left > 0 ? (int)left : 0;        // wave-uniform
    double si[4], sj[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      si[r] = sc[32 * pti + li + 8 * r];
      sj[r] = sc[32 * ptj + lj + 8 * r];
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c)
        dacc[r][c] = __builtin_fma(si[r] * sj[c], (double)(nb - 2 * pop[r][c]), dacc[r][c]);
  };
  auto compute = [&](int buf, int64_t e0, int64_t numel) {
    const unsigned* pa = lw + (buf * R + 32 * pti + li) * kRowW;
    const unsigned* pb = lw + (buf * R + 32 * ptj + lj) * kRowW;
    const double* sc = lsc + buf * NBS * RS;
    constexpr bool kCarry = WPB == kSW;
#pragma unroll
    for (int g = 0; g < kSW / 4; ++g) {
      u32x4 a[4], b[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        a[r] = *(const u32x4*)(pa + 8 * r * kRowW + 4 * g);
        b[r] = *(const u32x4*)(pb + 8 * r * kRowW + 4 * g);
      }
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const int wi = 4 * g + w;
        const bool first = !kCarry && wi % WPB == 0;  // compile time: a block's first count adds to 0
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int c = 0; c < 4; ++c) pop[r][c] = __builtin_popcount(a[r][w] ^ b[c][w]) + (first ? 0 : pop[r][c]);
        if (!kCarry && (wi + 1) % WPB == 0) scale_step(sc + (wi / WPB) * RS, e0 + 32 * (wi + 1), numel);
      }
    }
    if constexpr (kCarry) {
      const int64_t e = e0 + FA_Q1_GRAM_STAGE;
      if ((e & (B - 1)) == 0 || e >= numel) {  // the block ends with this stage
        scale_step(sc, e, numel);
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int c = 0; c < 4; ++c) pop[r][c] = 0;
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
    if (more) load();  // in flight during the counts
    if (cact) compute(buf, ce0, cnumel);
    if (more) {
      put(buf ^ 1);  // buffer buf ^ 1 was last read before the previous barrier
      ce0 = le0;
      cnumel = sg.numel;
      advance();
    }
    __syncthreads();
    have = more;
  }

  // the wave's 32 x 32 tile as [16][16] slabs of the 2 nt 16-client tiles; a diagonal tile has no lower slab
  if (!cact) return;
  const int nt16 = 2 * nt;
  double* out = partial + (int64_t)blockIdx.x * (nt16 * (nt16 + 1) / 2) * 256;
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int i = li + 8 * r, j = lj + 8 * c;
      const int ta = 2 * pti + (i >> 4), tb = 2 * ptj + (j >> 4);
      if (ta <= tb) out[pair_index(ta, tb, nt16) * 256 + (i & 15) * 16 + (j & 15)] = dacc[r][c];
    }
}

}  // namespace

extern "C" {

size_t fa_pairwise_gram_q1_scratch_bytes(int32_t num_segments, const int64_t* seg_numel, int32_t k) {
  if (k < 1 || k > FA_Q1_GRAM_MAX_K || num_segments <= 0 || !seg_numel) return 0;
  for (int s = 0; s < num_segments; ++s)
    if (seg_numel[s] < 0) return 0;
  const int64_t nwg = gram_workgroups(gram_units(num_segments, seg_numel, kUnit), FA_Q1_GRAM_MIN_UNITS,
                                      FA_Q1_GRAM_MAX_WORKGROUPS);
  return sizeof(double) * ((size_t)nwg * gram_plan(k).np16 * 256 + (size_t)k * k);
}

int fa_pairwise_gram_q1(fa_ctx* ctx, int32_t num_segments, const int64_t* seg_numel, int32_t k, int32_t block,
                        const void* const* d_bits, const void* const* d_scale, void* d_gram, void* d_dist,
                        void* d_scratch, size_t scratch_bytes, void* hip_stream) {
  const char* fn = "fa_pairwise_gram_q1";
  if (!ctx) return fail(FA_ERR_INVALID, "%s: ctx is NULL", fn);
  const int shift = block_shift(kQ1Gram, block);
  if (shift < 0) return block_fail(fn, kQ1Gram, block);
  if (k <= 0 || k > FA_Q1_GRAM_MAX_K || num_segments <= 0)
    return fail(FA_ERR_INVALID, "%s: k (1 .. %d) and num_segments must be positive", fn, FA_Q1_GRAM_MAX_K);
  if (!seg_numel || !d_bits || !d_scale || !d_dist) return fail(FA_ERR_INVALID, "%s: a table is NULL", fn);
  int nseg = 0;
  for (int s = 0; s < num_segments; ++s) {
    if (seg_numel[s] < 0) return fail(FA_ERR_INVALID, "%s: segment %d has negative numel", fn, s);
    if (seg_numel[s] == 0) continue;
    for (int i = 0; i < k; ++i) {
      const int64_t t = (int64_t)s * k + i;
      if (!data_ok(kQ1Gram, d_bits[t]))
        return fail(FA_ERR_INVALID, "%s: segment %d client %d: bits NULL or not 4-byte aligned", fn, s, i);
      if (!scale_ok(kQ1Gram, d_scale[t]))
        return fail(FA_ERR_INVALID, "%s: segment %d client %d: scale NULL or not 4-byte aligned", fn, s, i);
    }
    ++nseg;
  }
  const size_t need = fa_pairwise_gram_q1_scratch_bytes(num_segments, seg_numel, k);
  if (!d_scratch || ((uintptr_t)d_scratch & 7u) || scratch_bytes < need)
    return fail(FA_ERR_INVALID, "%s: scratch must hold %zu bytes, 8-byte aligned", fn, need);

  const GramPlan pl = gram_plan(k);
  const int64_t nunits = gram_units(num_segments, seg_numel, kUnit);
  const int nwg = (int)gram_workgroups(nunits, FA_Q1_GRAM_MIN_UNITS, FA_Q1_GRAM_MAX_WORKGROUPS);
  double* slabs = (double*)d_scratch;
  double* gram = d_gram ? (double*)d_gram : slabs + (size_t)nwg * pl.np16 * 256;
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(FA_ERR_HIP, "hipSetDevice(%d) failed", ctx->device);
  hipStream_t st = (hipStream_t)hip_stream;
  GramTables tb;
  if (nseg) {
    const int rc = gram_stage_tables(ctx, num_segments, seg_numel, k, nseg, kUnit, d_bits, d_scale, st, &tb);
    if (rc) return rc;
    const int wpb = shift >= 9 ? kSW : 1 << (shift - 5);
    const dim3 grid((unsigned)nwg), blk((unsigned)pl.threads);
    const size_t lds = gram_lds(pl.nt, wpb);
#define FA_GRAM(WPB)                                                                                         \
  hipLaunchKernelGGL((k_gram_q1<WPB>), grid, blk, lds, st, tb.segs, nseg, tb.data, tb.scale, (int)k, pl.nt, \
                     shift, nunits, slabs)
    switch (wpb) {
      case 1: FA_GRAM(1); break;
      case 2: FA_GRAM(2); break;
      case 4: FA_GRAM(4); break;
      case 8: FA_GRAM(8); break;
      default: FA_GRAM(kSW); break;
    }
#undef FA_GRAM
  }
  gram_reduce_dist(st, slabs, nwg, (int)k, pl.nt16, gram, (double*)d_dist);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    if (tb.slot) (void)release(tb.slot, st);
    return fail(FA_ERR_HIP, "%s: %s", fn, hipGetErrorString(e));
  }
  return tb.slot ? release(tb.slot, st) : FA_OK;
}

}  // extern "C"
