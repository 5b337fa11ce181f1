// noise.hip -- MI355X (gfx950) kernels + C ABI of the differential-privacy entries (include/fedagg_dp.h):
// the counter-based noise generator (Philox4x32-10 words -> float32 Gaussian or Laplace deviates), its
// add to a tensor (fa_add_noise) and the clipped centered sum with the noise added in the same read
// (fa_centered_sum_noise, fa_centered_sum_noise_tiled).
//
// k_sum_noise has signvote.hip's shape: a workgroup owns ONE 4-KiB slot per client (one arena tile,
// so the tiled and the flat layout differ only in the slot's address), 16 bytes per lane and client,
// non-temporal, kU clients' loads issued before any is consumed; unaligned segments and a segment's
// ragged last slot take the same code with coalesced element loads.  The sum is sv_slot's at
// threshold 0 (no vote is taken), so y is fa_sign_vote_sum's out bit for bit.  The lane's noise is
// generated after the first group's loads are issued and before they are consumed: its VALU work
// (10 Philox rounds, one logf + sqrtf + sincospif per two Gaussian deviates) runs under the loads'
// latency.  On the vector path a lane's 16 bytes are one Philox block (F32), two (16-bit types) or
// half of one (F64: the two lanes that share a block each take one Box-Muller pair); on the element
// path every element computes its own block and picks its word.  Both go through noise_block /
// noise_pair, so they give the same bits.  Numbers: DESIGN.md.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <type_traits>

#include "elem.h"
#include "fa_internal.h"
#include "fedagg_dp.h"
#include "median_common.h"
#include "median_host.h"

using namespace fa_detail;

namespace {

constexpr int kU = 8;   // clients whose loads are in flight together (whole aligned slots)
constexpr int kUE = 4;  // the same on the element path

enum { kSum = 0, kCentered = 1, kAdd = 2 };  // y: the MUL_W sum, the centered sum, the one input (or +0)

struct NoiseP {
  uint32_t k0, k1, round;
  int mech;
  double scale;
};

// Philox4x32-10 of counter (lo32(b), hi32(b), seg, round) under key (k0, k1).
__device__ __forceinline__ u32x4 noise_block(uint32_t k0, uint32_t k1, uint64_t b, uint32_t seg, uint32_t round) {
  constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
  uint32_t c0 = (uint32_t)b, c1 = (uint32_t)(b >> 32), c2 = seg, c3 = round;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(M0, c0), lo0 = M0 * c0;
    const uint32_t hi1 = __umulhi(M1, c2), lo1 = M1 * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += W0;
    k1 += W1;
  }
  return u32x4{c0, c1, c2, c3};
}

// u = ((w >> 9) + 0.5) 2^-23: exact, in (0, 1)
__device__ __forceinline__ float noise_uniform(uint32_t w) {
  return op_mul(op_add((float)(w >> 9), 0.5f), 0x1p-23f);
}

// The two deviates of the words (wa, wb): Box-Muller's pair, or Laplace's one per word.
__device__ __forceinline__ void noise_pair(int mech, uint32_t wa, uint32_t wb, float& z0, float& z1) {
  const float ua = noise_uniform(wa), ub = noise_uniform(wb);
  if (mech == FA_NOISE_GAUSSIAN) {  // uniform
    const float r = sqrtf(op_mul(-2.0f, logf(ua)));
    float s, c;
    sincospif(op_mul(2.0f, ub), &s, &c);  // the argument is exact
    z0 = op_mul(r, c);
    z1 = op_mul(r, s);
  } else {
    const float va = op_sub(ua, 0.5f), vb = op_sub(ub, 0.5f);           // exact, never 0
    const float la = logf(op_sub(1.0f, op_mul(2.0f, fabsf(va))));        // the argument: exact, >= 2^-23
    const float lb = logf(op_sub(1.0f, op_mul(2.0f, fabsf(vb))));
    z0 = va > 0.0f ? -la : la;
    z1 = vb > 0.0f ? -lb : lb;
  }
}

// t = rnd((A)scale * (A)z)
template <int DT>
__device__ __forceinline__ typename El<DT>::A noise_term(const NoiseP& np, float z) {
  using A = typename El<DT>::A;
  return El<DT>::rnd(op_mul((A)np.scale, (A)z));
}

// The terms of the lane's V consecutive elements from e (a multiple of V) of segment id `seg`.
template <int DT>
__device__ __forceinline__ void noise_vec(const NoiseP& np, uint32_t seg, int64_t e, typename El<DT>::A (&t)[El<DT>::V]) {
  constexpr int V = El<DT>::V;
  if constexpr (V == 2) {  // half a block: the pair (2p, 2p + 1)
    const u32x4 w = noise_block(np.k0, np.k1, (uint64_t)e >> 2, seg, np.round);
    const bool hi = (e & 2) != 0;
    float z0, z1;
    noise_pair(np.mech, hi ? w[2] : w[0], hi ? w[3] : w[1], z0, z1);
    t[0] = noise_term<DT>(np, z0);
    t[1] = noise_term<DT>(np, z1);
  } else {
#pragma unroll
    for (int q = 0; q < V / 4; ++q) {
      const u32x4 w = noise_block(np.k0, np.k1, ((uint64_t)e >> 2) + q, seg, np.round);
      float z[4];
      noise_pair(np.mech, w[0], w[1], z[0], z[1]);
      noise_pair(np.mech, w[2], w[3], z[2], z[3]);
#pragma unroll
      for (int j = 0; j < 4; ++j) t[4 * q + j] = noise_term<DT>(np, z[j]);
    }
  }
}

// The term of element e alone: its own block, its word's pair, its deviate of the two.
template <int DT>
__device__ __forceinline__ typename El<DT>::A noise_one(const NoiseP& np, uint32_t seg, int64_t e) {
  const u32x4 w = noise_block(np.k0, np.k1, (uint64_t)e >> 2, seg, np.round);
  const bool hi = (e & 2) != 0;
  float z0, z1;
  noise_pair(np.mech, hi ? w[2] : w[0], hi ? w[3] : w[1], z0, z1);
  return noise_term<DT>(np, (e & 1) ? z1 : z0);
}

// One client into the lane's V sums: sv_consume (signvote.hip) without the vote.
template <int DT, bool CEN>
__device__ __forceinline__ void dn_consume(const typename El<DT>::A (&x)[El<DT>::V],
                                           const typename El<DT>::A (&cen)[El<DT>::V], typename El<DT>::A c,
                                           typename El<DT>::A (&acc)[El<DT>::V]) {
  using T = El<DT>;
  using A = typename T::A;
#pragma unroll
  for (int v = 0; v < T::V; ++v) {
    const A u = CEN ? T::rnd(op_sub(x[v], cen[v])) : x[v];
    acc[v] = T::rnd(op_add(acc[v], T::rnd(op_mul(u, c))));
  }
}

// The slot tl of segment sg.  kSum / kCentered: sv_slot's walk over the k clients.  kAdd: k is 1 (y =
// the input's element, untouched) or 0 (y = +0).  NZ: the noise is generated and added.
template <int DT, int MODE, bool NZ, bool VEC>
__device__ __forceinline__ void dn_slot(const MSeg& sg, int64_t tl, const void* const* __restrict__ in,
                                        const void* __restrict__ center, const double* __restrict__ coef, int k,
                                        const NoiseP& np, uint32_t seg_id) {
  using L = SlotLoad<DT, VEC>;
  using T = El<DT>;
  using A = typename T::A;
  constexpr bool CEN = MODE == kCentered;
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

  A t[V] = {};
  auto make_noise = [&]() {
    if constexpr (NZ) {
      if constexpr (VEC) {
        noise_vec<DT>(np, seg_id, e0 + (int64_t)tid * V, t);
      } else {
#pragma unroll
        for (int j = 0; j < V; ++j) t[j] = noise_one<DT>(np, seg_id, e0 + (int64_t)j * kBlock + tid);
      }
    }
  };

  A acc[V];
  if constexpr (MODE == kAdd) {
#pragma unroll
    for (int v = 0; v < V; ++v) acc[v] = (A)0.0;
    typename L::Raw r[NR];
    if (k) ld.load(r, in[0]);  // uniform
    make_noise();
    if (k) L::get(r, acc);
  } else {
#pragma unroll
    for (int v = 0; v < V; ++v) acc[v] = (A)-0.0;  // -0 + t == t bitwise for every t
    // whole groups unguarded, so every load of a group is issued before the first client's arithmetic;
    // the noise after the first group's loads
    int i0 = 0;
    for (; i0 + U <= k; i0 += U) {
      typename L::Raw r[U][NR];
#pragma unroll
      for (int u = 0; u < U; ++u) ld.load(r[u], in[i0 + u]);
      if (i0 == 0) make_noise();  // uniform
#pragma unroll
      for (int u = 0; u < U; ++u) {
        A x[V];
        L::get(r[u], x);
        dn_consume<DT, CEN>(x, cen, (A)coef[i0 + u], acc);
      }
    }
    if (i0 < k) {
      typename L::Raw r[U][NR];
#pragma unroll
      for (int u = 0; u < U; ++u) ld.load(r[u], in[min(i0 + u, k - 1)]);  // clamped: every load unconditional
      if (i0 == 0) make_noise();  // uniform
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (i0 + u < k) {  // wave-uniform
          A x[V];
          L::get(r[u], x);
          dn_consume<DT, CEN>(x, cen, (A)coef[i0 + u], acc);
        }
      }
    }
  }

#pragma unroll
  for (int v = 0; v < V; ++v) {
    if constexpr (CEN) acc[v] = T::rnd(op_add(cen[v], acc[v]));
    if constexpr (NZ) acc[v] = T::rnd(op_add(acc[v], t[v]));
  }
  if constexpr (VEC) {
    __builtin_nontemporal_store(T::pack(acc), (__attribute__((address_space(1))) u32x4*)((char*)sg.out + e0 * T::SZ +
                                                                                         (int64_t)tid * 16));
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j)
      if (live >> j & 1u) ((typename T::S*)sg.out)[e0 + (int64_t)j * kBlock + tid] = T::bits(acc[j]);
  }
}

// cens[j]: the center of the table's segment j (kCentered); ids[j]: its segment id (NZ).
template <int DT, int MODE, bool NZ>
__global__ void __launch_bounds__(kBlock)
k_sum_noise(const MSeg* __restrict__ segs, int nseg, const void* const* __restrict__ ptrs,
            const void* const* __restrict__ cens, const double* __restrict__ coef, int k,
            const uint32_t* __restrict__ ids, NoiseP np) {
  constexpr int64_t E = FA_TILE_BYTES / El<DT>::SZ;
  const int64_t tile = blockIdx.x;
  const int si = nseg > 1 ? find_seg(segs, nseg, tile) : 0;
  const MSeg sg = segs[si];
  const int64_t tl = tile - sg.tile_start;
  const void* const* in = ptrs + sg.ptr_base;
  const void* center = MODE == kCentered ? cens[si] : nullptr;
  const uint32_t seg_id = NZ ? ids[si] : 0u;
  if (sg.aligned && (tl + 1) * E <= sg.numel) dn_slot<DT, MODE, NZ, true>(sg, tl, in, center, coef, k, np, seg_id);
  else dn_slot<DT, MODE, NZ, false>(sg, tl, in, center, coef, k, np, seg_id);
}

__global__ void __launch_bounds__(kBlock)
k_noise_words(uint32_t k0, uint32_t k1, uint32_t round, uint32_t seg, uint64_t first, int64_t nblocks,
              u32x4* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < nblocks) out[i] = noise_block(k0, k1, first + (uint64_t)i, seg, round);
}

template <int MODE, bool NZ>
void dn_launch(int dtype, dim3 grid, hipStream_t st, const MSeg* ds, int n, const void* const* dp,
               const void* const* dcen, const double* dc, int k, const uint32_t* ids, const NoiseP& np) {
  const dim3 block(kBlock);
  switch (dtype) {
#define FA_DN(DT) \
  case DT: hipLaunchKernelGGL((k_sum_noise<DT, MODE, NZ>), grid, block, 0, st, ds, n, dp, dcen, dc, k, ids, np); break;
    FA_DN(FA_DTYPE_F32) FA_DN(FA_DTYPE_BF16) FA_DN(FA_DTYPE_F16)
    default: hipLaunchKernelGGL((k_sum_noise<FA_DTYPE_F64, MODE, NZ>), grid, block, 0, st, ds, n, dp, dcen, dc, k, ids, np); break;
#undef FA_DN
  }
}

int64_t slot_elems(int dtype) { return FA_TILE_BYTES / (dtype == FA_DTYPE_F64 ? 8 : dtype == FA_DTYPE_F32 ? 4 : 2); }

int check_noise(const char* fn, int mech, double scale, const uint32_t* seg_id) {
  if (mech != FA_NOISE_GAUSSIAN && mech != FA_NOISE_LAPLACE)
    return fail(FA_ERR_INVALID, "%s: mech must be FA_NOISE_GAUSSIAN or FA_NOISE_LAPLACE (got %d)", fn, mech);
  if (!(scale >= 0.0) || !std::isfinite(scale))
    return fail(FA_ERR_INVALID, "%s: scale must be finite and >= 0 (got %g)", fn, scale);
  if (!seg_id) return fail(FA_ERR_INVALID, "%s: seg_id is NULL", fn);
  return FA_OK;
}

// The table, then the payload: the k coefficients (sums), the non-empty segments' center pointers
// (centered), their segment ids.  has_in: kAdd only.
int dn_impl(const ColArgs& a, int mode, bool has_in, const double* coef, int mech, double scale, uint64_t seed,
            uint32_t round, const uint32_t* seg_id) {
  const int64_t cols = slot_elems(a.dtype);
  int nseg;
  int64_t tiles;
  if (const int rc = col_count(a, cols, &nseg, &tiles)) return rc;
  if (nseg == 0) return FA_OK;
  const int k = a.k;
  const bool centered = mode == kCentered;
  const size_t coef_bytes = mode == kAdd ? 0 : sizeof(double) * (size_t)k;
  const size_t cen_bytes = centered ? sizeof(void*) * (size_t)nseg : 0;
  const size_t extra = coef_bytes + cen_bytes + sizeof(uint32_t) * (size_t)nseg;
  const NoiseP np{(uint32_t)seed, (uint32_t)(seed >> 32), round, mech, scale};
  const bool nz = scale != 0.0;
  return col_stage_launch(
      a, cols, nseg, tiles, extra,
      [&](void* h) {
        for (size_t i = 0; i < coef_bytes / sizeof(double); ++i) ((double*)h)[i] = coef[i];
        const void** hc = (const void**)((char*)h + coef_bytes);
        uint32_t* hi = (uint32_t*)((char*)h + coef_bytes + cen_bytes);
        for (int s = 0, j = 0; s < a.num_segments; ++s) {
          if (!a.seg_numel[s]) continue;
          if (centered) hc[j] = a.d_center[s];
          hi[j++] = seg_id[s];
        }
      },
      [&](dim3 grid, hipStream_t st, const MSeg* ds, int n, const void* const* dp, const void* payload) {
        const double* dc = (const double*)payload;
        const void* const* dcen = (const void* const*)((const char*)payload + coef_bytes);
        const uint32_t* ids = (const uint32_t*)((const char*)payload + coef_bytes + cen_bytes);
        if (mode == kAdd) dn_launch<kAdd, true>(a.dtype, grid, st, ds, n, dp, nullptr, nullptr, has_in ? 1 : 0, ids, np);
        else if (centered && nz) dn_launch<kCentered, true>(a.dtype, grid, st, ds, n, dp, dcen, dc, k, ids, np);
        else if (centered) dn_launch<kCentered, false>(a.dtype, grid, st, ds, n, dp, dcen, dc, k, ids, np);
        else if (nz) dn_launch<kSum, true>(a.dtype, grid, st, ds, n, dp, nullptr, dc, k, ids, np);
        else dn_launch<kSum, false>(a.dtype, grid, st, ds, n, dp, nullptr, dc, k, ids, np);
      });
}

int sum_noise_impl(const ColArgs& a, const double* coef, int mech, double scale, uint64_t seed, uint32_t round,
                   const uint32_t* seg_id) {
  if (const int rc = col_check_args(a)) return rc;
  if (!coef) return fail(FA_ERR_INVALID, "%s: coef is NULL", a.fn);
  if (const int rc = check_noise(a.fn, mech, scale, seg_id)) return rc;
  return dn_impl(a, a.d_center ? kCentered : kSum, false, coef, mech, scale, seed, round, seg_id);
}

}  // namespace

extern "C" {

int fa_noise_words(fa_ctx* ctx, uint64_t seed, uint32_t round, uint32_t seg_id, uint64_t first_block,
                   int64_t nblocks, void* d_out_u32, void* hip_stream) {
  const char* fn = "fa_noise_words";
  if (!ctx) return fail(FA_ERR_INVALID, "%s: ctx is NULL", fn);
  if (nblocks < 0 || (nblocks > 0 && (uint64_t)(nblocks - 1) > ~0ull - first_block))
    return fail(FA_ERR_INVALID, "%s: need nblocks >= 0 and first_block + nblocks <= 2^64", fn);
  if (nblocks == 0) return FA_OK;
  if (!d_out_u32 || !al16(d_out_u32)) return fail(FA_ERR_INVALID, "%s: d_out_u32 must be non-NULL and 16-byte aligned", fn);
  const int64_t grid = (nblocks + kBlock - 1) / kBlock;
  if (grid > 0x7FFFFFFFll) return fail(FA_ERR_INVALID, "%s: too many blocks for one call", fn);
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(FA_ERR_HIP, "hipSetDevice(%d) failed", ctx->device);
  hipLaunchKernelGGL(k_noise_words, dim3((unsigned)grid), dim3(kBlock), 0, (hipStream_t)hip_stream, (uint32_t)seed,
                     (uint32_t)(seed >> 32), round, seg_id, first_block, nblocks, (u32x4*)d_out_u32);
  FA_HIP(hipGetLastError());
  return FA_OK;
}

int fa_add_noise(fa_ctx* ctx, int dtype, int mech, double scale, uint64_t seed, uint32_t round, int32_t num_segments,
                 const int64_t* seg_numel, const uint32_t* seg_id, const void* const* d_in, void* const* d_out,
                 void* hip_stream) {
  const char* fn = "fa_add_noise";
  if (!ctx) return fail(FA_ERR_INVALID, "%s: ctx is NULL", fn);
  if (num_segments <= 0 || !seg_numel || !d_out) return fail(FA_ERR_INVALID, "%s: invalid arguments", fn);
  if (const int rc = check_noise(fn, mech, scale, seg_id)) return rc;
  // without an input the outputs stand in for it in the table (checked and aligned alike, never read)
  const ColArgs a{fn, ctx, dtype, num_segments, seg_numel, 1, d_in ? d_in : (const void* const*)d_out, 0, d_out, hip_stream};
  if (scale != 0.0) return dn_impl(a, kAdd, d_in != nullptr, nullptr, mech, scale, seed, round, seg_id);
  // scale 0: out = x bit for bit
  int nseg;
  int64_t tiles;
  if (const int rc = col_count(a, slot_elems(dtype), &nseg, &tiles)) return rc;
  if (nseg == 0) return FA_OK;
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(FA_ERR_HIP, "hipSetDevice(%d) failed", ctx->device);
  const size_t sz = (size_t)(FA_TILE_BYTES / slot_elems(dtype));
  for (int s = 0; s < num_segments; ++s) {
    const size_t bytes = (size_t)seg_numel[s] * sz;
    if (!bytes) continue;
    if (!d_in) FA_HIP(hipMemsetAsync(d_out[s], 0, bytes, (hipStream_t)hip_stream));
    else if (d_in[s] != d_out[s])
      FA_HIP(hipMemcpyAsync(d_out[s], d_in[s], bytes, hipMemcpyDeviceToDevice, (hipStream_t)hip_stream));
  }
  return FA_OK;
}

int fa_centered_sum_noise(fa_ctx* ctx, int dtype, int32_t num_segments, const int64_t* seg_numel, int32_t k,
                          const void* const* d_in, const void* const* d_center, const double* coef, int mech,
                          double scale, uint64_t seed, uint32_t round, const uint32_t* seg_id, void* const* d_out,
                          void* hip_stream) {
  return sum_noise_impl({"fa_centered_sum_noise", ctx, dtype, num_segments, seg_numel, k, d_in, 0, d_out, hip_stream,
                         d_center},
                        coef, mech, scale, seed, round, seg_id);
}

int fa_centered_sum_noise_tiled(fa_ctx* ctx, int dtype, int32_t num_segments, const int64_t* seg_numel, int32_t k,
                                const void* const* d_in, int64_t tile_stride, const void* const* d_center,
                                const double* coef, int mech, double scale, uint64_t seed, uint32_t round,
                                const uint32_t* seg_id, void* const* d_out, void* hip_stream) {
  if (ctx && tile_stride <= 0) return fail(FA_ERR_INVALID, "fa_centered_sum_noise_tiled: tile_stride must be > 0");
  return sum_noise_impl({"fa_centered_sum_noise_tiled", ctx, dtype, num_segments, seg_numel, k, d_in, tile_stride,
                         d_out, hip_stream, d_center},
                        coef, mech, scale, seed, round, seg_id);
}

}  // extern "C"
