// wsum_dist.hip -- MI355X (gfx950) kernels + C ABI of the fused weighted sum and squared distances
// (include/fedagg_robust.h: fa_weighted_sum_sqdist, fa_weighted_sum_sqdist_tiled): one pass of the
// smoothed Weiszfeld iteration for the geometric median (Pillutla, Kakade, Harchaoui: RFA).
//
// Per element e: out[e] = the FA_MODE_MUL_W ordered sum of fedagg.hip (t_i = op(x_i c_i), out = t_0,
// out = op(out + t_i), op rounds once to the storage type, nothing fused), and per client i the two
// sums d2_i = sum_e (x_i[e] - out[e])^2 (against the STORED out) and ss_i = sum_e x_i[e]^2.
//
// k_wsd: a workgroup owns a chunk of kS 4-KiB slots per client (a slot = one arena tile, so the
// tiled and the flat layout differ only in the slot's address).  Phase 1 walks the clients in order
// with the weighted-sum kernel's structure (16 bytes per lane and slot, U clients' loads issued
// before any is consumed) and keeps out in registers, already rounded to the storage type, so it IS
// the stored value.  Phase 2 walks the clients again and forms each lane's two float64 sums over its
// kS x V elements (differences in float32 from exactly widened inputs, float64 for float64 inputs;
// squares and sums in float64 FMAs), one DPP row reduction per client and chunk, the sixteen rows
// added in row order through LDS, and writes the chunk's 2K sums to its row of the caller's
// scratch.  The second walk misses the caches (K x 16 KiB per workgroup, times the resident
// workgroups), so this kernel reads the input twice from HBM: correct for every K, dtype and layout,
// the fallback and the A/B baseline.  Unaligned segments and a segment's ragged last chunk take the
// same code with coalesced element loads.  k_wsd_reg (float32, K <= 32) holds a tile's K values in
// registers between the phases and reads the input once.  k_wsd_reduce then adds the rows in a fixed
// order (k_gram_reduce's split, robust.hip): no floating-point atomics anywhere, so the same call
// gives the same bits.  Kept and lost forms, with their numbers: DESIGN.md.
//
// fa_centered_sum_sqdist[_tiled] (one pass of centered clipping) are the same kernels in two more
// modes of the template parameter CM: kCenter forms out = op(center + the ordered sum of
// t_i = op(op(x_i - center) c_i)) around a flat center the caller supplies and measures against that
// out; kDist (coef NULL) measures against the center itself in one walk and stores nothing.  The
// center pointers travel in the entry's payload behind the coefficients.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <type_traits>

#include "elem.h"
#include "fa_internal.h"
#include "fedagg_robust.h"
#include "median_common.h"
#include "median_host.h"

using namespace fa_detail;

namespace {

// The weighted sum's arithmetic and conversions are elem.h's, the ones fedagg.hip's FA_MODE_MUL_W
// uses; only the element accessors are this file's: global address space, plain stores.
template <int DT>
__device__ __forceinline__ typename El<DT>::A ld1(const void* p, int64_t e) {
  return El<DT>::from_bits(gld<typename El<DT>::S>(p, e));
}
template <int DT>
__device__ __forceinline__ void st1(void* p, int64_t e, typename El<DT>::A v) {
  ((typename El<DT>::S*)p)[e] = El<DT>::bits(v);
}

constexpr int kS = 4;     // 4-KiB slots per client and workgroup
constexpr int kKB = 128;  // clients per pass of phase 2 (the LDS block of wave sums)
constexpr int kRows = kBlock / 16;  // 16-lane DPP rows per workgroup
enum { kPlain = 0, kCenter = 1, kDist = 2 };  // what a pass forms (wsd_chunk)

// Sum over the lane's 16-lane row, left in every lane of the row: four DPP exchanges (xor 1, xor 2 by
// quad_perm, then row_half_mirror and row_mirror), plain VALU, in a fixed order.  The rows of a wave
// are NOT combined here (that would take cross-row permutes through the LDS crossbar, and a wait
// each): the row leaders store to LDS and the workgroup's 16 row sums are added in row order.
template <int CTRL>
__device__ __forceinline__ double dpp_add(double v) {
  const u32x2 b = __builtin_bit_cast(u32x2, v);
  const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)b[0], CTRL, 0xF, 0xF, true);
  const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)b[1], CTRL, 0xF, 0xF, true);
  return v + __builtin_bit_cast(double, u32x2{lo, hi});
}
__device__ __forceinline__ double row_sum(double v) {
  v = dpp_add<0xB1>(v);   // quad_perm [1, 0, 3, 2]
  v = dpp_add<0x4E>(v);   // quad_perm [2, 3, 0, 1]
  v = dpp_add<0x141>(v);  // row_half_mirror
  v = dpp_add<0x140>(v);  // row_mirror
  return v;
}

// the workgroup's row sums of clients [b0, b0 + bn) -> its row of partials, rows added in row order
__device__ __forceinline__ void flush_rows(double (&red)[kRows][2 * kKB], int b0, int bn, int k,
                                           double* __restrict__ part) {
  __syncthreads();
  for (int t = (int)threadIdx.x; t < 2 * kKB; t += kBlock) {
    const int i = b0 + (t < kKB ? t : t - kKB);
    if (i < b0 + bn) {
      double s = red[0][t];
#pragma unroll
      for (int w = 1; w < kRows; ++w) s += red[w][t];
      part[t < kKB ? i : k + i] = s;
    }
  }
  __syncthreads();
}

// One client's kS x V elements of this lane.  VEC: kS 16-byte loads (slot s at byte offset off[s]);
// else element loads at the clamped element indices off[j] (coalesced across the wave: element j of
// lane l is the chunk's element j * kBlock + l).
template <int DT, bool VEC>
struct Chunk {
  using T = El<DT>;
  using A = typename T::A;
  static constexpr int V = T::V, NE = kS * V;
  static constexpr int64_t E = FA_TILE_BYTES / T::SZ;
  static constexpr int NR = VEC ? kS : NE;
  using Raw = typename std::conditional<VEC, u32x4, A>::type;

  int64_t off[NR];  // VEC: byte offsets of the lane's 16 bytes in each slot; else element indices

  __device__ void load(Raw (&r)[NR], const void* p) const {
    if constexpr (VEC) {
#pragma unroll
      for (int s = 0; s < kS; ++s) r[s] = *(const __attribute__((address_space(1))) u32x4*)((const char*)p + off[s]);
    } else {
#pragma unroll
      for (int j = 0; j < NE; ++j) r[j] = ld1<DT>(p, off[j]);
    }
  }
  __device__ static void get(const Raw (&r)[NR], A (&x)[NE]) {
    if constexpr (VEC) {
#pragma unroll
      for (int s = 0; s < kS; ++s) T::unpack(r[s], &x[s * V]);
    } else {
#pragma unroll
      for (int j = 0; j < NE; ++j) x[j] = r[j];
    }
  }
};

// The element's term of client i.  CM == kPlain: t_i = op(x_i c_i); kCenter: u_i = op(x_i - center),
// t_i = op(u_i c_i).
template <int DT, int CM>
__device__ __forceinline__ typename El<DT>::A wsd_term(typename El<DT>::A x, typename El<DT>::A cen,
                                                       typename El<DT>::A c) {
  using T = El<DT>;
  if constexpr (CM == kCenter) return T::rnd(op_mul(T::rnd(op_sub(x, cen)), c));
  else return T::rnd(op_mul(x, c));
}

// CM: kPlain, the weighted sum; kCenter, out = op(center + the ordered sum of the clipped differences);
// kDist, out IS the center: no first walk and no store.  `center`: the segment's flat center (CM != kPlain).
template <int DT, bool VEC, int CM>
__device__ __forceinline__ void wsd_chunk(const MSeg& sg, int64_t tl, const void* const* __restrict__ in,
                                          const void* __restrict__ center, const double* __restrict__ coef, int k,
                                          double* __restrict__ part, double (&red)[kRows][2 * kKB]) {
  using C = Chunk<DT, VEC>;
  using T = El<DT>;
  using A = typename T::A;
  constexpr int V = T::V, NE = C::NE, NR = C::NR;
  constexpr int64_t E = C::E;
  constexpr int U = VEC ? 4 : 2;  // clients whose loads are in flight together
  const int tid = (int)threadIdx.x;
  const int64_t e0 = tl * (kS * E);
  const int64_t ts = sg.tstride;

  C ck;
  unsigned live = 0;  // bit j: the lane's element j lies inside the segment
  if constexpr (VEC) {
#pragma unroll
    for (int s = 0; s < kS; ++s) {
      const int64_t es = e0 + s * E;  // a multiple of E: the slot is one whole tile
      ck.off[s] = (ts ? (es / E) * ts : es * T::SZ) + (int64_t)tid * 16;
    }
    live = ~0u;
  } else {
#pragma unroll
    for (int j = 0; j < NE; ++j) {
      const int64_t e = e0 + (int64_t)j * kBlock + tid;
      if (e < sg.numel) live |= 1u << j;
      const int64_t ec = e < sg.numel ? e : sg.numel - 1;  // clamped: every load unconditional
      ck.off[j] = ts ? (ec / E) * (ts / T::SZ) + ec % E : ec;
    }
  }

  // the lane's elements of the center (flat, like out; the lane that owns an element reads it here
  // and only then stores it, so out may be the center itself)
  A cen[CM == kPlain ? 1 : NE] = {};
  if constexpr (CM != kPlain) {
    if constexpr (VEC) {
#pragma unroll
      for (int s = 0; s < kS; ++s)
        T::unpack(*(const __attribute__((address_space(1))) u32x4*)((const char*)center + (e0 + s * E) * T::SZ +
                                                                     (int64_t)tid * 16),
                  &cen[s * V]);
    } else {
#pragma unroll
      for (int j = 0; j < NE; ++j) {
        const int64_t e = e0 + (int64_t)j * kBlock + tid;
        cen[j] = ld1<DT>(center, e < sg.numel ? e : sg.numel - 1);
      }
    }
  }

  // phase 1: out, clients in order
  A acc[NE];
#pragma unroll
  for (int j = 0; j < NE; ++j)
    acc[j] = CM == kDist ? cen[CM == kPlain ? 0 : j] : (A)-0.0;  // -0 + t == t bitwise for every t
  if constexpr (CM != kDist) {
    int i0 = 0;
    for (; i0 + U <= k; i0 += U) {
      typename C::Raw r[U][NR];
#pragma unroll
      for (int u = 0; u < U; ++u) ck.load(r[u], in[i0 + u]);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const A c = (A)coef[i0 + u];
        A x[NE];
        C::get(r[u], x);
#pragma unroll
        for (int j = 0; j < NE; ++j)
          acc[j] = T::rnd(op_add(acc[j], wsd_term<DT, CM>(x[j], cen[CM == kPlain ? 0 : j], c)));
      }
    }
    if (i0 < k) {
      typename C::Raw r[U][NR];
#pragma unroll
      for (int u = 0; u < U; ++u) ck.load(r[u], in[min(i0 + u, k - 1)]);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (i0 + u < k) {  // wave-uniform
          const A c = (A)coef[i0 + u];
          A x[NE];
          C::get(r[u], x);
#pragma unroll
          for (int j = 0; j < NE; ++j)
            acc[j] = T::rnd(op_add(acc[j], wsd_term<DT, CM>(x[j], cen[CM == kPlain ? 0 : j], c)));
        }
      }
    }
    if constexpr (CM == kCenter) {
#pragma unroll
      for (int j = 0; j < NE; ++j) acc[j] = T::rnd(op_add(cen[j], acc[j]));
    }
    if constexpr (VEC) {
#pragma unroll
      for (int s = 0; s < kS; ++s)
        *(u32x4*)((char*)sg.out + (e0 + s * E) * T::SZ + (int64_t)tid * 16) = T::pack(&acc[s * V]);
    } else {
#pragma unroll
      for (int j = 0; j < NE; ++j)
        if (live >> j & 1u) st1<DT>(sg.out, e0 + (int64_t)j * kBlock + tid, acc[j]);
    }
  }

  // phase 2: the two sums of every client against the registers' out, kKB clients per LDS block
  const int row = tid >> 4;
  for (int b0 = 0; b0 < k; b0 += kKB) {
    const int bn = min(kKB, k - b0);
    for (int i0 = b0; i0 < b0 + bn; i0 += U) {
      typename C::Raw r[U][NR];
#pragma unroll
      for (int u = 0; u < U; ++u) ck.load(r[u], in[min(i0 + u, b0 + bn - 1)]);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (i0 + u < b0 + bn) {  // wave-uniform
          A x[NE];
          C::get(r[u], x);
          double d2 = 0.0, ss = 0.0;
#pragma unroll
          for (int j = 0; j < NE; ++j) {
            const double dd = (double)op_sub(x[j], acc[j]), xd = (double)x[j];
            if (VEC || (live >> j & 1u)) {
              d2 = __builtin_fma(dd, dd, d2);
              ss = __builtin_fma(xd, xd, ss);
            }
          }
          d2 = row_sum(d2);
          ss = row_sum(ss);
          if ((tid & 15) == 0) {
            red[row][i0 + u - b0] = d2;
            red[row][kKB + i0 + u - b0] = ss;
          }
        }
      }
    }
    flush_rows(red, b0, bn, k, part);
  }
}

// cens[j]: the center of the table's segment j (CM != kPlain; not read otherwise)
template <int DT, int CM>
__global__ void __launch_bounds__(kBlock)
k_wsd(const MSeg* __restrict__ segs, int nseg, const void* const* __restrict__ ptrs,
      const void* const* __restrict__ cens, const double* __restrict__ coef, int k, double* __restrict__ partial) {
  __shared__ double red[kRows][2 * kKB];
  constexpr int64_t CH = kS * (FA_TILE_BYTES / El<DT>::SZ);  // elements per chunk
  const int64_t tile = blockIdx.x;
  const int si = nseg > 1 ? find_seg(segs, nseg, tile) : 0;
  const MSeg sg = segs[si];
  const int64_t tl = tile - sg.tile_start;
  const void* const* in = ptrs + sg.ptr_base;
  const void* center = CM == kPlain ? nullptr : cens[si];
  double* part = partial + tile * (2 * (int64_t)k);
  if (sg.aligned && (tl + 1) * CH <= sg.numel)
    wsd_chunk<DT, true, CM>(sg, tl, in, center, coef, k, part, red);
  else
    wsd_chunk<DT, false, CM>(sg, tl, in, center, coef, k, part, red);
}

// Single-read form, K <= KM <= 32: the same chunk, one 4-KiB slot at a time with the slot's K x 16
// bytes of every lane held in registers between the two phases, so each input byte is read from HBM
// once (non-temporal) and never again -- the generic kernel's second walk over K x 16 KiB per
// workgroup misses L2, and across the resident workgroups the Infinity Cache as well.  No branch
// depends on the client index (clients past k repeat client k - 1 and are masked by selects), so
// every load of a slot is issued before the first is consumed.  The row leaders keep their running
// sums over the four slots in LDS; the sums' order differs from the generic kernel's, the bound does
// not.  Chunks that are ragged or unaligned take the generic element-load path.
// The centered forms hold the slot's 16 bytes of the center beside the K rows.
template <int DT, int KM, int CM>
__global__ void __launch_bounds__(kBlock)
k_wsd_reg(const MSeg* __restrict__ segs, int nseg, const void* const* __restrict__ ptrs,
          const void* const* __restrict__ cens, const double* __restrict__ coef, int k,
          double* __restrict__ partial) {
  using T = El<DT>;
  using A = typename T::A;
  constexpr int V = T::V;
  constexpr int64_t E = FA_TILE_BYTES / T::SZ, CH = kS * E;
  __shared__ double red[kRows][2 * kKB];
  const int64_t tile = blockIdx.x;
  const int si = nseg > 1 ? find_seg(segs, nseg, tile) : 0;
  const MSeg sg = segs[si];
  const int64_t tl = tile - sg.tile_start;
  const void* const* in = ptrs + sg.ptr_base;
  const void* center = CM == kPlain ? nullptr : cens[si];
  double* part = partial + tile * (2 * (int64_t)k);
  if (!(sg.aligned && (tl + 1) * CH <= sg.numel)) {
    wsd_chunk<DT, false, CM>(sg, tl, in, center, coef, k, part, red);
    return;
  }
  const int tid = (int)threadIdx.x, row = tid >> 4;
  const bool lead = (tid & 15) == 0;
#pragma unroll 1
  for (int s = 0; s < kS; ++s) {
    const int64_t es = tl * CH + s * E;  // a multiple of E: the slot is one whole tile
    const int64_t off = (sg.tstride ? (es / E) * sg.tstride : es * T::SZ) + (int64_t)tid * 16;
    u32x4 r[KM];
#pragma unroll
    for (int i = 0; i < KM; ++i)
      r[i] = __builtin_nontemporal_load(
          (const __attribute__((address_space(1))) u32x4*)((const char*)in[min(i, k - 1)] + off));
    A cen[V] = {};  // read by the lane that stores these 16 bytes of out below: out may be the center
    if constexpr (CM != kPlain)
      T::unpack(*(const __attribute__((address_space(1))) u32x4*)((const char*)center + es * T::SZ + (int64_t)tid * 16),
                cen);
    A acc[V];
#pragma unroll
    for (int v = 0; v < V; ++v) acc[v] = CM == kDist ? cen[v] : (A)-0.0;
    if constexpr (CM != kDist) {
#pragma unroll
      for (int i = 0; i < KM; ++i) {
        const A c = (A)coef[min(i, k - 1)];
        A x[V];
        T::unpack(r[i], x);
#pragma unroll
        for (int v = 0; v < V; ++v) {
          const A nxt = T::rnd(op_add(acc[v], wsd_term<DT, CM>(x[v], cen[v], c)));
          acc[v] = i < k ? nxt : acc[v];
        }
      }
      if constexpr (CM == kCenter) {
#pragma unroll
        for (int v = 0; v < V; ++v) acc[v] = T::rnd(op_add(cen[v], acc[v]));
      }
      *(u32x4*)((char*)sg.out + es * T::SZ + (int64_t)tid * 16) = T::pack(acc);
    }
#pragma unroll
    for (int i = 0; i < KM; ++i) {
      A x[V];
      T::unpack(r[i], x);
      double d2 = 0.0, ss = 0.0;
#pragma unroll
      for (int v = 0; v < V; ++v) {
        const double dd = (double)op_sub(x[v], acc[v]), xd = (double)x[v];
        d2 = __builtin_fma(dd, dd, d2);
        ss = __builtin_fma(xd, xd, ss);
      }
      d2 = row_sum(d2);
      ss = row_sum(ss);
      if (lead && i < k) {
        red[row][i] = s ? red[row][i] + d2 : d2;
        red[row][kKB + i] = s ? red[row][kKB + i] + ss : ss;
      }
    }
  }
  flush_rows(red, 0, k, k, part);
}

constexpr int kRegMaxK = 32;  // clients the single-read form holds in registers (KM = 48 lost)

bool wsd_reg_enabled() {  // FA_WSD_REG=0: the generic kernel for every K (A/B); read per call
  const char* e = getenv("FA_WSD_REG");
  return !(e && e[0] == '0');
}

// stats[e] = the sum over the chunks' rows of partial[row][e] in a fixed order (k_gram_reduce's
// split, robust.hip): a workgroup of 16 waves takes 16 consecutive entries and splits the rows 64
// ways (128-byte row reads, each lane its rows in row order), then one lane per entry adds the 64
// split sums in split order through LDS.
constexpr int kRW = 16, kRE = 16, kRS = kRW * 64 / kRE;
__global__ void __launch_bounds__(64 * kRW)
k_wsd_reduce(const double* __restrict__ partial, int64_t nparts, int n2k, double* __restrict__ stats) {
  __shared__ double red[kRW * 64];
  const int el = threadIdx.x % kRE, rs = threadIdx.x / kRE;
  const int e = blockIdx.x * kRE + el;
  const bool on = e < n2k;
  const int ec = on ? e : n2k - 1;
  double s = 0.0;
  int64_t b = rs;
  for (; b + 7 * kRS < nparts; b += 8 * kRS) {  // 8 loads in flight, added in row order
    double x[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) x[u] = partial[(b + u * kRS) * n2k + ec];
#pragma unroll
    for (int u = 0; u < 8; ++u) s += x[u];
  }
  for (; b < nparts; b += kRS) s += partial[b * n2k + ec];
  red[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x < kRE && on) {
    double t = 0.0;
    for (int u = 0; u < kRS; ++u) t += red[u * kRE + threadIdx.x];
    stats[e] = t;
  }
}

int64_t chunk_elems(int dtype) {
  return (int64_t)kS * (FA_TILE_BYTES / (dtype == FA_DTYPE_F64 ? 8 : dtype == FA_DTYPE_F32 ? 4 : 2));
}

// The launch of one pass in mode CM (the kernels' template parameter).
template <int CM>
void wsd_launch(int dtype, int k, dim3 grid, hipStream_t st, const MSeg* ds, int n, const void* const* dp,
                const void* const* dcen, const double* dc, double* part) {
  const dim3 block(kBlock);
  if (dtype == FA_DTYPE_F32 && k <= kRegMaxK && wsd_reg_enabled()) {
    switch ((k + 7) / 8) {  // KM = K rounded up to 8
#define FA_WR(Q) \
  case Q: hipLaunchKernelGGL((k_wsd_reg<FA_DTYPE_F32, 8 * Q, CM>), grid, block, 0, st, ds, n, dp, dcen, dc, k, part); break;
      FA_WR(1) FA_WR(2) FA_WR(3) FA_WR(4)
#undef FA_WR
    }
    return;
  }
  switch (dtype) {
#define FA_WG(DT) \
  case DT: hipLaunchKernelGGL((k_wsd<DT, CM>), grid, block, 0, st, ds, n, dp, dcen, dc, k, part); break;
    FA_WG(FA_DTYPE_F32) FA_WG(FA_DTYPE_BF16) FA_WG(FA_DTYPE_F16)
    default: hipLaunchKernelGGL((k_wsd<FA_DTYPE_F64, CM>), grid, block, 0, st, ds, n, dp, dcen, dc, k, part); break;
#undef FA_WG
  }
}

// centered: the fa_centered_* entries (a.d_center is theirs; coef NULL: distance-only, d_out unused).
int wsd_impl(ColArgs a, bool centered, const double* coef, void* d_stats, void* d_scratch, size_t scratch_bytes) {
  const void* const* d_center = a.d_center;
  const int mode = !centered ? kPlain : coef ? kCenter : kDist;
  if (mode == kDist) a.d_out = (void* const*)d_center;  // nothing is stored: the table's out is the center
  if (const int rc = col_check_args(a)) return rc;
  const int k = a.k;
  if (centered && !d_center) return fail(FA_ERR_INVALID, "%s: d_center is NULL", a.fn);
  if (!centered && !coef) return fail(FA_ERR_INVALID, "%s: coef is NULL", a.fn);
  if (!d_stats) return fail(FA_ERR_INVALID, "%s: d_stats is NULL", a.fn);
  const int64_t ch = chunk_elems(a.dtype);
  int nseg;
  int64_t tiles;
  if (const int rc = col_count(a, ch, &nseg, &tiles)) return rc;
  const size_t need = (size_t)tiles * 2 * (size_t)k * sizeof(double);
  if (need > scratch_bytes || (need && !d_scratch))
    return fail(FA_ERR_INVALID, "%s: scratch too small (%zu bytes, need %zu)", a.fn, d_scratch ? scratch_bytes : (size_t)0,
                need);
  if (nseg == 0) {  // nothing to read: every sum is 0
    DeviceGuard g(a.ctx->device);
    if (!g.ok) return fail(FA_ERR_HIP, "hipSetDevice(%d) failed", a.ctx->device);
    FA_HIP(hipMemsetAsync(d_stats, 0, sizeof(double) * 2 * (size_t)k, (hipStream_t)a.hip_stream));
    return FA_OK;
  }
  double* part = (double*)d_scratch;
  // the payload: the k coefficients, then (centered) the non-empty segments' center pointers
  const size_t coef_bytes = sizeof(double) * (size_t)k;
  return col_stage_launch(
      a, ch, nseg, tiles, coef_bytes + (centered ? sizeof(void*) * (size_t)nseg : 0),
      [&](void* h) {
        for (int i = 0; i < k; ++i) ((double*)h)[i] = coef ? coef[i] : 0.0;
        if (centered) {
          const void** hc = (const void**)((char*)h + coef_bytes);
          for (int s = 0, j = 0; s < a.num_segments; ++s)
            if (a.seg_numel[s]) hc[j++] = d_center[s];
        }
      },
      [&](dim3 grid, hipStream_t st, const MSeg* ds, int n, const void* const* dp, const void* payload) {
        const double* dc = (const double*)payload;
        const void* const* dcen = (const void* const*)((const char*)payload + coef_bytes);
        switch (mode) {
          case kPlain: wsd_launch<kPlain>(a.dtype, k, grid, st, ds, n, dp, nullptr, dc, part); break;
          case kCenter: wsd_launch<kCenter>(a.dtype, k, grid, st, ds, n, dp, dcen, dc, part); break;
          default: wsd_launch<kDist>(a.dtype, k, grid, st, ds, n, dp, dcen, dc, part); break;
        }
        hipLaunchKernelGGL(k_wsd_reduce, dim3((unsigned)((2 * k + kRE - 1) / kRE)), dim3(64 * kRW), 0, st,
                           (const double*)part, tiles, 2 * k, (double*)d_stats);
      });
}

}  // namespace

extern "C" {

int fa_weighted_sum_sqdist(fa_ctx* ctx, int dtype, int32_t num_segments, const int64_t* seg_numel, int32_t k,
                           const void* const* d_in, const double* coef, void* const* d_out, void* d_stats,
                           void* d_scratch, size_t scratch_bytes, void* hip_stream) {
  return wsd_impl({"fa_weighted_sum_sqdist", ctx, dtype, num_segments, seg_numel, k, d_in, 0, d_out, hip_stream}, false,
                  coef, d_stats, d_scratch, scratch_bytes);
}

int fa_weighted_sum_sqdist_tiled(fa_ctx* ctx, int dtype, int32_t num_segments, const int64_t* seg_numel, int32_t k,
                                 const void* const* d_in, int64_t tile_stride, const double* coef, void* const* d_out,
                                 void* d_stats, void* d_scratch, size_t scratch_bytes, void* hip_stream) {
  if (ctx && tile_stride <= 0) return fail(FA_ERR_INVALID, "fa_weighted_sum_sqdist_tiled: tile_stride must be > 0");
  return wsd_impl({"fa_weighted_sum_sqdist_tiled", ctx, dtype, num_segments, seg_numel, k, d_in, tile_stride, d_out,
                   hip_stream},
                  false, coef, d_stats, d_scratch, scratch_bytes);
}

int fa_centered_sum_sqdist(fa_ctx* ctx, int dtype, int32_t num_segments, const int64_t* seg_numel, int32_t k,
                           const void* const* d_in, const void* const* d_center, const double* coef,
                           void* const* d_out, void* d_stats, void* d_scratch, size_t scratch_bytes, void* hip_stream) {
  return wsd_impl({"fa_centered_sum_sqdist", ctx, dtype, num_segments, seg_numel, k, d_in, 0, d_out, hip_stream,
                   d_center},
                  true, coef, d_stats, d_scratch, scratch_bytes);
}

int fa_centered_sum_sqdist_tiled(fa_ctx* ctx, int dtype, int32_t num_segments, const int64_t* seg_numel, int32_t k,
                                 const void* const* d_in, int64_t tile_stride, const void* const* d_center,
                                 const double* coef, void* const* d_out, void* d_stats, void* d_scratch,
                                 size_t scratch_bytes, void* hip_stream) {
  if (ctx && tile_stride <= 0) return fail(FA_ERR_INVALID, "fa_centered_sum_sqdist_tiled: tile_stride must be > 0");
  return wsd_impl({"fa_centered_sum_sqdist_tiled", ctx, dtype, num_segments, seg_numel, k, d_in, tile_stride, d_out,
                   hip_stream, d_center},
                  true, coef, d_stats, d_scratch, scratch_bytes);
}

// The per-chunk rows of the smallest chunk any dtype uses (float64's), so one size serves every dtype.
size_t fa_weighted_sum_sqdist_scratch_bytes(int32_t num_segments, const int64_t* seg_numel, int32_t k) {
  if (k <= 0 || num_segments <= 0 || !seg_numel) return 0;
  const int64_t ch = chunk_elems(FA_DTYPE_F64);
  int64_t tiles = 0;
  for (int s = 0; s < num_segments; ++s) {
    if (seg_numel[s] < 0) return 0;
    tiles += (seg_numel[s] + ch - 1) / ch;
  }
  if (tiles > 0x7FFFFFFFll) return 0;
  return (size_t)tiles * 2 * (size_t)k * sizeof(double);
}

}  // extern "C"
