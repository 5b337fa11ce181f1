// signvote.hip -- MI355X (gfx950) kernel + C ABI of the sign-vote weighted sum (include/fedagg_robust.h:
// fa_sign_vote_sum, fa_sign_vote_sum_tiled): the robust learning rate of Ozdayi, Kantarcioglu and Gel
// (AAAI 2021) fused into the FedAvg sum.
//
// Per element e: u_i = op(x_i - center) (or x_i itself without a center), the vote s_i = sign(u_i)
// (+-0 and NaN vote 0), net = sum_i s_i, the ordered sum acc of t_i = op(u_i c_i) with the arithmetic
// of wsum_dist.hip's kCenter / kPlain modes, acc negated where |net| < threshold, and
// out = op(center + acc) (or acc).  The vote is taken from the registers the sum reads, so the
// clients are read from HBM once, in one walk in client order.
//
// k_sign_vote: a workgroup owns ONE 4-KiB slot per client (a slot = one arena tile, so the tiled and
// the flat layout differ only in the slot's address) -- the weighted-sum kernel's default shape
// (fedagg.hip, U = 8, S = 1): 16 bytes per lane and client, non-temporal, kU clients' loads issued
// before any is consumed.  Unaligned segments and a segment's ragged last slot take the same code
// with coalesced element loads.  Every vote counter is a 32-bit integer per element (|net| <= k for
// any k).  The count of flipped elements goes lane -> workgroup through one LDS integer, workgroup ->
// its own int in the staging slot's scratch (a plain vector store), and k_sign_vote_count adds those
// into *d_flipped: integer adds, so the value does not depend on their order.  (One global integer
// atomic per workgroup on the one word instead -- 16,384 of them at P = 2^24 -- doubled the K = 8 time
// and cost 17 % at K = 128.)  Numbers and what is not built: DESIGN.md.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "elem.h"
#include "fa_internal.h"
#include "fedagg_robust.h"
#include "median_common.h"
#include "median_host.h"

using namespace fa_detail;

namespace {

constexpr int kU = 8;   // clients whose loads are in flight together (whole aligned slots)
constexpr int kUE = 4;  // the same on the element path

// One client into the lane's V sums and votes.  (The slot's loads: SlotLoad, median_common.h.)
template <int DT, bool CEN>
__device__ __forceinline__ void sv_consume(const typename El<DT>::A (&x)[El<DT>::V],
                                           const typename El<DT>::A (&cen)[El<DT>::V], typename El<DT>::A c,
                                           typename El<DT>::A (&acc)[El<DT>::V], int (&net)[El<DT>::V]) {
  using T = El<DT>;
  using A = typename T::A;
#pragma unroll
  for (int v = 0; v < T::V; ++v) {
    const A u = CEN ? T::rnd(op_sub(x[v], cen[v])) : x[v];
    net[v] += (int)(u > (A)0) - (int)(u < (A)0);  // NaN and +-0: neither comparison holds
    acc[v] = T::rnd(op_add(acc[v], T::rnd(op_mul(u, c))));
  }
}

// The slot tl of segment sg; returns the number of this lane's elements (inside the segment) whose
// sum was negated.  `center`: the segment's flat center (CEN).
template <int DT, bool CEN, bool VEC>
__device__ __forceinline__ int sv_slot(const MSeg& sg, int64_t tl, const void* const* __restrict__ in,
                                       const void* __restrict__ center, const double* __restrict__ coef, int k,
                                       int threshold) {
  using L = SlotLoad<DT, VEC>;
  using T = El<DT>;
  using A = typename T::A;
  constexpr int V = T::V, NR = L::NR;
  constexpr int64_t E = FA_TILE_BYTES / T::SZ;
  constexpr int U = VEC ? kU : kUE;
  const int tid = (int)threadIdx.x;
  const int64_t e0 = tl * E;  // a multiple of E: the slot is one whole tile
  const int64_t ts = sg.tstride;

  L ld;
  unsigned live = 0;  // bit j: the lane's element j lies inside the segment
  if constexpr (VEC) {
    ld.off[0] = (ts ? tl * ts : e0 * T::SZ) + (int64_t)tid * 16;
    live = ~0u;
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const int64_t e = e0 + (int64_t)j * kBlock + tid;
      if (e < sg.numel) live |= 1u << j;
      const int64_t ec = e < sg.numel ? e : sg.numel - 1;  // clamped: every load unconditional
      ld.off[j] = ts ? (ec / E) * (ts / T::SZ) + ec % E : ec;
    }
  }

  // the lane's elements of the center (flat, like out; the lane that owns an element reads it here
  // and only then stores it, so out may be the center itself)
  A cen[V] = {};
  if constexpr (CEN) {
    if constexpr (VEC) {
      T::unpack(*(const __attribute__((address_space(1))) u32x4*)((const char*)center + e0 * T::SZ + (int64_t)tid * 16),
                cen);
    } else {
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const int64_t e = e0 + (int64_t)j * kBlock + tid;
        cen[j] = T::from_bits(gld<typename T::S>(center, e < sg.numel ? e : sg.numel - 1));
      }
    }
  }

  A acc[V];
  int net[V];
#pragma unroll
  for (int v = 0; v < V; ++v) {
    acc[v] = (A)-0.0;  // -0 + t == t bitwise for every t
    net[v] = 0;
  }
  // whole groups unguarded, so every load of a group is issued before the first client's arithmetic
  int i0 = 0;
  for (; i0 + U <= k; i0 += U) {
    typename L::Raw r[U][NR];
#pragma unroll
    for (int u = 0; u < U; ++u) ld.load(r[u], in[i0 + u]);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      A x[V];
      L::get(r[u], x);
      sv_consume<DT, CEN>(x, cen, (A)coef[i0 + u], acc, net);
    }
  }
  if (i0 < k) {
    typename L::Raw r[U][NR];
#pragma unroll
    for (int u = 0; u < U; ++u) ld.load(r[u], in[min(i0 + u, k - 1)]);  // clamped: every load unconditional
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (i0 + u < k) {  // wave-uniform
        A x[V];
        L::get(r[u], x);
        sv_consume<DT, CEN>(x, cen, (A)coef[i0 + u], acc, net);
      }
    }
  }

  int flips = 0;
#pragma unroll
  for (int v = 0; v < V; ++v) {
    const bool flip = (net[v] < 0 ? -net[v] : net[v]) < threshold;
    acc[v] = flip ? -acc[v] : acc[v];  // the sign bit alone: exact, and after it no rounding is due
    if constexpr (CEN) acc[v] = T::rnd(op_add(cen[v], acc[v]));
    flips += (flip && (live >> v & 1u)) ? 1 : 0;
  }
  if constexpr (VEC) {
    __builtin_nontemporal_store(T::pack(acc), (__attribute__((address_space(1))) u32x4*)((char*)sg.out + e0 * T::SZ +
                                                                                         (int64_t)tid * 16));
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j)
      if (live >> j & 1u) ((typename T::S*)sg.out)[e0 + (int64_t)j * kBlock + tid] = T::bits(acc[j]);
  }
  return flips;
}

// cens[j]: the center of the table's segment j (CEN; not read otherwise).  counts: NULL, or one
// int per workgroup, which the workgroup writes.
template <int DT, bool CEN>
__global__ void __launch_bounds__(kBlock)
k_sign_vote(const MSeg* __restrict__ segs, int nseg, const void* const* __restrict__ ptrs,
            const void* const* __restrict__ cens, const double* __restrict__ coef, int k, int threshold,
            int* __restrict__ counts) {
  __shared__ int wg_flips;
  constexpr int64_t E = FA_TILE_BYTES / El<DT>::SZ;
  const int64_t tile = blockIdx.x;
  const int si = nseg > 1 ? find_seg(segs, nseg, tile) : 0;
  const MSeg sg = segs[si];
  const int64_t tl = tile - sg.tile_start;
  const void* const* in = ptrs + sg.ptr_base;
  const void* center = CEN ? cens[si] : nullptr;
  if (counts) {  // uniform
    if (threadIdx.x == 0) wg_flips = 0;
    __syncthreads();
  }
  const int flips = sg.aligned && (tl + 1) * E <= sg.numel
                        ? sv_slot<DT, CEN, true>(sg, tl, in, center, coef, k, threshold)
                        : sv_slot<DT, CEN, false>(sg, tl, in, center, coef, k, threshold);
  if (counts) {
    if (flips) atomicAdd(&wg_flips, flips);  // LDS
    __syncthreads();
    if (threadIdx.x == 0) counts[tile] = wg_flips;
  }
}

// *flipped = the sum of the workgroups' counts: one workgroup, each lane its share, the lanes through
// one LDS integer (integer adds: the value does not depend on their order).
constexpr int kSumBlock = 1024;
__global__ void __launch_bounds__(kSumBlock)
k_sign_vote_count(const int* __restrict__ counts, int64_t n, long long* __restrict__ flipped) {
  __shared__ unsigned long long total;
  if (threadIdx.x == 0) total = 0;
  __syncthreads();
  unsigned long long s = 0;
  for (int64_t i = threadIdx.x; i < n; i += kSumBlock) s += (unsigned long long)counts[i];
  if (s) atomicAdd(&total, s);  // LDS
  __syncthreads();
  if (threadIdx.x == 0) *flipped = (long long)total;
}

template <bool CEN>
void sv_launch(int dtype, dim3 grid, hipStream_t st, const MSeg* ds, int n, const void* const* dp,
               const void* const* dcen, const double* dc, int k, int threshold, int* counts) {
  const dim3 block(kBlock);
  switch (dtype) {
#define FA_SV(DT) \
  case DT: hipLaunchKernelGGL((k_sign_vote<DT, CEN>), grid, block, 0, st, ds, n, dp, dcen, dc, k, threshold, counts); break;
    FA_SV(FA_DTYPE_F32) FA_SV(FA_DTYPE_BF16) FA_SV(FA_DTYPE_F16)
    default: hipLaunchKernelGGL((k_sign_vote<FA_DTYPE_F64, CEN>), grid, block, 0, st, ds, n, dp, dcen, dc, k, threshold, counts); break;
#undef FA_SV
  }
}

int64_t slot_elems(int dtype) { return FA_TILE_BYTES / (dtype == FA_DTYPE_F64 ? 8 : dtype == FA_DTYPE_F32 ? 4 : 2); }

int sv_impl(const ColArgs& a, const double* coef, int32_t threshold, void* d_flipped) {
  if (const int rc = col_check_args(a)) return rc;
  const int k = a.k;
  if (!coef) return fail(FA_ERR_INVALID, "%s: coef is NULL", a.fn);
  if (threshold < 0 || threshold > k)
    return fail(FA_ERR_INVALID, "%s: threshold must satisfy 0 <= threshold <= k (threshold %d, k %d)", a.fn,
                (int)threshold, k);
  const int64_t cols = slot_elems(a.dtype);
  int nseg;
  int64_t tiles;
  if (const int rc = col_count(a, cols, &nseg, &tiles)) return rc;
  const bool centered = a.d_center != nullptr;
  hipStream_t stream = (hipStream_t)a.hip_stream;
  if (nseg == 0) {  // nothing to read: nothing flipped
    if (!d_flipped) return FA_OK;
    DeviceGuard g(a.ctx->device);
    if (!g.ok) return fail(FA_ERR_HIP, "hipSetDevice(%d) failed", a.ctx->device);
    FA_HIP(hipMemsetAsync(d_flipped, 0, sizeof(int64_t), stream));
    return FA_OK;
  }
  // the payload: the k coefficients, then (centered) the non-empty segments' center pointers; behind
  // it the slot's scratch for the workgroups' counts
  const size_t coef_bytes = sizeof(double) * (size_t)k;
  const size_t extra = coef_bytes + (centered ? sizeof(void*) * (size_t)nseg : 0);
  return col_stage_launch(
      a, cols, nseg, tiles, extra,
      [&](void* h) {
        for (int i = 0; i < k; ++i) ((double*)h)[i] = coef[i];
        if (centered) {
          const void** hc = (const void**)((char*)h + coef_bytes);
          for (int s = 0, j = 0; s < a.num_segments; ++s)
            if (a.seg_numel[s]) hc[j++] = a.d_center[s];
        }
      },
      [&](dim3 grid, hipStream_t st, const MSeg* ds, int n, const void* const* dp, const void* payload) {
        const double* dc = (const double*)payload;
        const void* const* dcen = (const void* const*)((const char*)payload + coef_bytes);
        int* counts = d_flipped ? (int*)((char*)const_cast<void*>(payload) + extra) : nullptr;
        if (centered) sv_launch<true>(a.dtype, grid, st, ds, n, dp, dcen, dc, k, threshold, counts);
        else sv_launch<false>(a.dtype, grid, st, ds, n, dp, nullptr, dc, k, threshold, counts);
        if (counts)
          hipLaunchKernelGGL(k_sign_vote_count, dim3(1), dim3(kSumBlock), 0, st, (const int*)counts, tiles,
                             (long long*)d_flipped);
      },
      d_flipped ? sizeof(int) * (size_t)tiles : 0);
}

}  // namespace

extern "C" {

int fa_sign_vote_sum(fa_ctx* ctx, int dtype, int32_t num_segments, const int64_t* seg_numel, int32_t k,
                     const void* const* d_in, const void* const* d_center, const double* coef, int32_t threshold,
                     void* const* d_out, void* d_flipped, void* hip_stream) {
  return sv_impl({"fa_sign_vote_sum", ctx, dtype, num_segments, seg_numel, k, d_in, 0, d_out, hip_stream, d_center},
                 coef, threshold, d_flipped);
}

int fa_sign_vote_sum_tiled(fa_ctx* ctx, int dtype, int32_t num_segments, const int64_t* seg_numel, int32_t k,
                           const void* const* d_in, int64_t tile_stride, const void* const* d_center,
                           const double* coef, int32_t threshold, void* const* d_out, void* d_flipped,
                           void* hip_stream) {
  if (ctx && tile_stride <= 0) return fail(FA_ERR_INVALID, "fa_sign_vote_sum_tiled: tile_stride must be > 0");
  return sv_impl({"fa_sign_vote_sum_tiled", ctx, dtype, num_segments, seg_numel, k, d_in, tile_stride, d_out,
                  hip_stream, d_center},
                 coef, threshold, d_flipped);
}

}  // extern "C"
