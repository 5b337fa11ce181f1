// pairdot.hip -- MI355X (gfx950) kernel + C ABI of the fused history update and Gram matrix
// (include/fedagg_robust.h: fa_pairwise_dot, fa_pairwise_dot_tiled): the device work of FoolsGold
// (Fung, Yoon, Beschastnikh 2018), which needs every pairwise inner product of the clients' running
// update sums.
//
// Per element e: u_i = rnd(x_i - center) (or x_i itself without a center); with a history
// h_i = rnd(h_i + u_i), stored in place, and y_i = the stored h_i; otherwise y_i = u_i.
// G[i][j] = sum_e y_i y_j for all i, j, the diagonal included.
//
// k_pairdot has the structure of robust.hip's k_pairdist: a workgroup owns a contiguous run of chunks
// (pe coordinates of one segment, all k clients); a chunk is staged in LDS transposed, [e][client], so
// the 4 clients of a block are one 16-byte read; each thread owns one 4x4 client-pair tile over a slice
// of the chunk's coordinates; two LDS buffers, one barrier per chunk; float32 runs of <= kPE
// coordinates summed in float64; per-workgroup float64 partials to scratch and a second kernel that
// adds them in block order.  What differs from k_pairdist:
//   - the staging thread OWNS its elements: 16 bytes of one client (an "item") are loaded from the
//     input, the center and the history, u and h are formed in registers, h is stored back by the same
//     lane (16-byte store where everything is aligned, element stores otherwise), and y goes to LDS.
//     The loads of chunk i + 1 are issued before the pair loop of chunk i and consumed after it.
//   - the tiles cover the upper triangle of 4-client blocks WITH its diagonal (bi <= bj): a diagonal
//     tile gives the block's 4 norms and 6 inner pairs (its 6 mirrored slots are computed and dropped)
//   - the tile operator is one FMA per pair and coordinate, a_x * b_y + acc
// Items: consecutive lanes take 4 consecutive 16-byte items of one client (64 contiguous bytes), then
// the next client: a wave's loads cover 16 clients, its LDS stores of one element index go to 16
// different columns, and a client's 128-byte line is consumed within one chunk.
// Numbers (the fused history update is slower than an add followed by the plain form) and what is not
// built: DESIGN.md.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <type_traits>

#include "elem.h"
#include "fa_internal.h"
#include "fedagg_robust.h"
#include "median_common.h"

using namespace fa_detail;

namespace {

constexpr int kPE = 64;          // longest float32 run (coordinates)
constexpr int kMaxDotK = 128;
constexpr int kMaxDotThreads = 576;  // k = 128: 528 tiles, 9 waves (3 per SIMD: a budget of 168 VGPRs)
constexpr int kNI = 2;           // 16-byte items of each stream (input, center, history) per thread and chunk
constexpr int kMaxChunk = 256;   // coordinates per chunk at most: divides every dtype's tile
constexpr int kDotBlocks = 1024; // workgroups at most (each writes every partial once)
constexpr size_t kDotLds = 64 * 1024;

struct DSeg {
  int64_t numel;
  int64_t tile_start;  // first chunk of this segment (find_seg keys on it)
  int64_t tstride;     // 0: flat inputs; > 0: tile-interleaved inputs, bytes between a client's tiles
  int32_t ptr_base;
  int32_t aligned;     // every input, history and the center are 16-byte aligned
};
static_assert(sizeof(DSeg) == 32, "DSeg layout");

int elem_size(int dtype) { return dtype == FA_DTYPE_F64 ? 8 : dtype == FA_DTYPE_F32 ? 4 : 2; }

// Work split: ntiles 4x4 tiles (upper triangle of 4-client blocks, diagonal included), one per thread,
// times `esplit` coordinate slices of a chunk (slice s: coordinates [s pe / esplit, (s + 1) pe / esplit));
// at least 256 threads, so that every item of a chunk has a staging thread.  pe: a power of two (it
// divides a tile's element count, so no chunk straddles a tile), at most kNI items per thread, the
// two LDS buffers within kDotLds, and a slice never longer than one float32 run.
struct DotPlan { int kp, nb, ntiles, esplit, nthreads, pe, cemax; size_t lds; };
DotPlan dot_plan(int k, int dtype) {
  DotPlan q;
  const int sz = elem_size(dtype), v = 16 / sz, asz = sz == 8 ? 8 : 4;
  q.kp = (k + 3) & ~3;
  q.nb = q.kp / 4;
  q.ntiles = q.nb * (q.nb + 1) / 2;
  const int cap = q.ntiles <= 64 ? 256 : 512;  // more than 256 tiles (k > 88): one slice, <= 576 threads
  q.esplit = std::max(1, std::min(kPE, cap / q.ntiles));
  q.nthreads = std::max(256, (q.ntiles * q.esplit + 63) / 64 * 64);
  const size_t row = (size_t)asz * (q.kp + 4);
  int64_t lim = std::min<int64_t>(kMaxChunk, (int64_t)kNI * q.nthreads * v / k);
  lim = std::min<int64_t>(lim, (int64_t)(kDotLds / (2 * row)));
  lim = std::min<int64_t>(lim, (int64_t)kPE * q.esplit);
  q.pe = v;
  while (q.pe * 2 <= lim) q.pe *= 2;
  q.cemax = (q.pe + q.esplit - 1) / q.esplit;
  q.lds = 2 * row * q.pe;
  if (q.esplit > 1) q.lds = std::max(q.lds, sizeof(double) * 16 * (size_t)q.ntiles);
  return q;
}

__device__ __forceinline__ float fma_(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fma_(double a, double b, double c) { return __builtin_fma(a, b, c); }

// tile -> (bi, bj), bi <= bj: row-major over the upper triangle of nb blocks
__device__ __forceinline__ void tile_blocks(int tile, int nb, int& bi, int& bj) {
  int r = 0, rem = tile;
  while (rem >= nb - r) { rem -= nb - r; ++r; }
  bi = r;
  bj = r + rem;
}
__device__ __forceinline__ int64_t tri_index(int i, int j, int k) {  // i <= j
  return (int64_t)i * k - (int64_t)i * (i - 1) / 2 + (j - i);
}

// An item: V consecutive elements of one tensor as 16 raw bytes.  vec: one 16-byte access; else the
// first nlive elements by element accesses (the rest read as zero bits and are not stored).
template <int DT, bool NT>
__device__ __forceinline__ u32x4 item_load(const void* p, int64_t off, int nlive, bool vec) {
  using T = El<DT>;
  using S = typename T::S;
  const char* q = (const char*)p + off;
  if (vec) {
    if constexpr (NT) return __builtin_nontemporal_load((const __attribute__((address_space(1))) u32x4*)q);
    else return *(const __attribute__((address_space(1))) u32x4*)q;
  }
  u32x4 r = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int v = 0; v < T::V; ++v) {
    if (v < nlive) {
      const S s = gld<S>(q, v);
      if constexpr (T::SZ == 4) {
        r[v] = __builtin_bit_cast(unsigned, s);
      } else if constexpr (T::SZ == 2) {
        r[v / 2] |= (unsigned)s << (16 * (v & 1));
      } else {
        const u32x2 w = __builtin_bit_cast(u32x2, s);
        r[2 * v] = w[0];
        r[2 * v + 1] = w[1];
      }
    }
  }
  return r;
}
// The V values y of an item, each rounded once to the storage type: one 16-byte store, or the first
// nlive of them by element stores -- taken from the values, not out of the packed 16 bytes: element
// stores of r[v] under `v < nlive` were compiled to stores of r[0] at every offset.
template <int DT>
__device__ __forceinline__ void item_store(void* p, int64_t off, int nlive, bool vec,
                                           const typename El<DT>::A (&y)[El<DT>::V]) {
  using T = El<DT>;
  using S = typename T::S;
  char* q = (char*)p + off;
  if (vec) {
    *(__attribute__((address_space(1))) u32x4*)q = T::pack(y);
    return;
  }
#pragma unroll
  for (int v = 0; v < T::V; ++v)
    if (v < nlive) ((__attribute__((address_space(1))) S*)q)[v] = T::bits(y[v]);
}

// cens[j] / hists[ptr_base + i]: the center of the table's segment j and client i's history of it;
// NULL tables: no center / no history.  TILED only selects the input addressing (the center and the
// histories are flat in both entries).
template <int DT, bool TILED>
__global__ void __launch_bounds__(kMaxDotThreads)
k_pairdot(const DSeg* __restrict__ segs, int nseg, const void* const* __restrict__ ptrs,
          const void* const* __restrict__ cens, void* const* __restrict__ hists, int k, int kp, int64_t nchunks,
          int ntiles, int esplit, int pe, int cemax, double* __restrict__ partial) {
  using T = El<DT>;
  using A = typename T::A;
  typedef A A4 __attribute__((ext_vector_type(4)));
  constexpr int V = T::V, SZ = T::SZ;
  constexpr bool kF64 = std::is_same<A, double>::value;  // float64: every sum in accd, no float32 run
  constexpr int64_t E = FA_TILE_BYTES / SZ;
  extern __shared__ __attribute__((aligned(32))) unsigned char smem[];
  A* lds = (A*)smem;                             // [2][pe][kp + 4]
  const int S = kp + 4;
  const int nb = kp / 4;
  const int t = threadIdx.x, nt = (int)blockDim.x;
  const bool pact = t < ntiles * esplit;         // the rest only stage
  const int es = pact ? t / ntiles : 0;          // coordinate slice
  const int tile = pact ? t % ntiles : 0;
  int bi = 0, bj = 0;
  if (pact) tile_blocks(tile, nb, bi, bj);
  const int e_lo = (int)((int64_t)es * pe / esplit), e_hi = (int)((int64_t)(es + 1) * pe / esplit);
  const bool cen = cens != nullptr, hist = hists != nullptr;

  double accd[16];
  A acc[16];
  int run = 0;  // coordinates summed in acc since the last flush (uniform)
#pragma unroll
  for (int u = 0; u < 16; ++u) {
    accd[u] = 0.0;
    acc[u] = (A)0;
  }
  auto flush = [&]() {
    if constexpr (!kF64) {
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        accd[u] += (double)acc[u];
        acc[u] = (A)0;
      }
    }
    run = 0;
  };

  // staging role (the same in every chunk): item n of this thread is client si[n]'s elements
  // sj[n] * V .. + V - 1 of the chunk
  const int ipc = pe / V;                        // items per client and chunk
  const int g = ipc < 4 ? ipc : 4;               // consecutive lanes on one client
  int si[kNI], sj[kNI];
  bool sact[kNI];
#pragma unroll
  for (int n = 0; n < kNI; ++n) {
    const int idx = t + n * nt;
    sact[n] = idx < k * ipc;
    const int c = sact[n] ? idx : 0;
    si[n] = (c / g) % k;
    sj[n] = (c / (g * k)) * g + c % g;
  }
  u32x4 rx[kNI], rc[kNI], rh[kNI];
  int nlive[kNI];
  bool vec[kNI];
  int64_t hoff[kNI];                             // byte offset of the item in a flat tensor
  int cseg = -1;
  DSeg sg;
  const void* src[kNI];
  void* hp[kNI];
  const void* cp = nullptr;
  auto load = [&](int64_t ch) {
    const int sidx = nseg > 1 ? find_seg(segs, nseg, ch) : 0;
    if (sidx != cseg) {  // one set of pointer loads per segment, not per chunk
      cseg = sidx;
      sg = segs[sidx];
      cp = cen ? cens[sidx] : nullptr;
#pragma unroll
      for (int n = 0; n < kNI; ++n) {
        src[n] = ptrs[sg.ptr_base + si[n]];
        hp[n] = hist ? hists[sg.ptr_base + si[n]] : nullptr;
      }
    }
    const int64_t b0 = (ch - sg.tile_start) * pe;
#pragma unroll
    for (int n = 0; n < kNI; ++n) {
      const int64_t e = b0 + (int64_t)sj[n] * V;
      const int64_t left = sg.numel - e;
      nlive[n] = !sact[n] || left <= 0 ? 0 : left < V ? (int)left : V;
      vec[n] = sg.aligned && nlive[n] == V;
      hoff[n] = e * SZ;
      rx[n] = rc[n] = rh[n] = u32x4{0u, 0u, 0u, 0u};
      if (nlive[n]) {
        // a chunk never straddles a tile: pe divides E and a segment's chunks start at multiples of pe
        const int64_t xoff = TILED ? (e / E) * sg.tstride + (e % E) * SZ : hoff[n];
        rx[n] = item_load<DT, true>(src[n], xoff, nlive[n], vec[n]);
        if (cen) rc[n] = item_load<DT, false>(cp, hoff[n], nlive[n], vec[n]);
        if (hist) rh[n] = item_load<DT, false>(hp[n], hoff[n], nlive[n], vec[n]);
      }
    }
  };
  // forms u, updates the history in place and writes y to LDS buffer `buf`, transposed
  const int bufsz = pe * S;
  auto put = [&](int buf) {
#pragma unroll
    for (int n = 0; n < kNI; ++n) {
      if (!sact[n]) continue;
      A y[V];
      T::unpack(rx[n], y);
      if (cen) {
        A c[V];
        T::unpack(rc[n], c);
#pragma unroll
        for (int v = 0; v < V; ++v) y[v] = T::rnd(op_sub(y[v], c[v]));
      }
      if (hist) {
        A h[V];
        T::unpack(rh[n], h);
#pragma unroll
        for (int v = 0; v < V; ++v) y[v] = T::rnd(op_add(h[v], y[v]));
        if (nlive[n]) item_store<DT>(hp[n], hoff[n], nlive[n], vec[n], y);
      }
      A* l = lds + buf * bufsz + sj[n] * V * S + si[n];
#pragma unroll
      for (int v = 0; v < V; ++v) l[v * S] = v < nlive[n] ? y[v] : (A)0;  // past the segment's end: 0 to every sum
    }
  };

  // clients k .. kp - 1 are zero columns of both buffers, written once
  for (int idx = t; idx < 2 * pe * (kp - k); idx += nt) lds[(idx / (kp - k)) * S + k + idx % (kp - k)] = (A)0;

  // each workgroup takes a contiguous run of chunks (a 128-byte line split between two chunks is then
  // fetched by one workgroup)
  const int64_t c0 = nchunks * blockIdx.x / gridDim.x, c1 = nchunks * (blockIdx.x + 1) / gridDim.x;
  if (c0 < c1) {
    load(c0);
    put(0);
  }
  __syncthreads();
  int cur = 0;
  for (int64_t ch = c0; ch < c1; ++ch, cur ^= 1) {
    if (ch + 1 < c1) load(ch + 1);  // in flight during the pair loop
    if (pact) {
      const A* pa = lds + cur * bufsz + 4 * bi;
      const A* pb = lds + cur * bufsz + 4 * bj;
#pragma unroll 4
      for (int e = e_lo; e < e_hi; ++e) {
        const A4 a = *(const A4*)(pa + e * S);
        const A4 b = *(const A4*)(pb + e * S);
#pragma unroll
        for (int x = 0; x < 4; ++x) {
#pragma unroll
          for (int y = 0; y < 4; ++y) {
            if constexpr (kF64) accd[4 * x + y] = fma_(a[x], b[y], accd[4 * x + y]);
            else acc[4 * x + y] = fma_(a[x], b[y], acc[4 * x + y]);
          }
        }
      }
    }
    run += cemax;
    if (run + cemax > kPE) flush();  // float32 runs of <= kPE coordinates, then float64
    if (ch + 1 < c1) put(cur ^ 1);   // buffer cur ^ 1 was last read before the previous barrier
    __syncthreads();
  }
  flush();

  // the block's partials of every (i <= j < k): the tiles' slices added in slice order through LDS
  double* out = partial + (int64_t)blockIdx.x * ((int64_t)k * (k + 1) / 2);
  if (esplit == 1) {
    if (pact) {
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int i = 4 * bi + u / 4, j = 4 * bj + u % 4;
        if (i <= j && j < k) out[tri_index(i, j, k)] = accd[u];
      }
    }
  } else {
    double* red = (double*)smem;
    for (int s = 0; s < esplit; ++s) {
      if (pact && es == s) {
#pragma unroll
        for (int u = 0; u < 16; ++u) red[tile * 16 + u] = (s == 0 ? 0.0 : red[tile * 16 + u]) + accd[u];
      }
      __syncthreads();
    }
    for (int idx = t; idx < ntiles * 16; idx += nt) {
      const int u = idx % 16;
      int r, c;
      tile_blocks(idx / 16, nb, r, c);
      const int i = 4 * r + u / 4, j = 4 * c + u % 4;
      if (i <= j && j < k) out[tri_index(i, j, k)] = red[idx];
    }
  }
}

// G = the workgroups' partials added in block order: kRP entries per workgroup, kBlock / kRP lanes
// per entry (lane l adds blocks l, l + L, ...; then the L lane sums in lane order) -- a fixed order.
// Both triangles get the one value.
__global__ void __launch_bounds__(kBlock)
k_pairdot_reduce(const double* __restrict__ partial, int nblocks, int k, double* __restrict__ gram) {
  constexpr int kRP = 8, L = kBlock / kRP;
  __shared__ double red[L][kRP + 1];
  const int64_t ntri = (int64_t)k * (k + 1) / 2;
  const int pl = threadIdx.x % kRP, lane = threadIdx.x / kRP;
  const int64_t p = (int64_t)blockIdx.x * kRP + pl;
  double s = 0.0;
  if (p < ntri)
    for (int b = lane; b < nblocks; b += L) s += partial[(int64_t)b * ntri + p];
  red[lane][pl] = s;
  __syncthreads();
  if (lane == 0 && p < ntri) {
    double tsum = 0.0;
    for (int l = 0; l < L; ++l) tsum += red[l][pl];
    int i = 0;  // p -> (i, j), i <= j
    int64_t rem = p;
    while (rem >= k - i) { rem -= k - i; ++i; }
    const int j = i + (int)rem;
    gram[(int64_t)i * k + j] = tsum;
    gram[(int64_t)j * k + i] = tsum;
  }
}

int64_t dot_chunks(int32_t num_segments, const int64_t* seg_numel, int pe) {
  int64_t n = 0;
  for (int s = 0; s < num_segments; ++s)
    if (seg_numel[s] > 0) n += (seg_numel[s] + pe - 1) / pe;
  return n;
}

int dot_impl(const char* fn, fa_ctx* ctx, int dtype, int32_t num_segments, const int64_t* seg_numel, int32_t k,
             const void* const* d_in, int64_t tstride, const void* const* d_center, void* const* d_hist,
             void* d_gram, void* d_scratch, size_t scratch_bytes, void* hip_stream) {
  if (!ctx) return fail(FA_ERR_INVALID, "%s: ctx is NULL", fn);
  if (k < 1 || k > kMaxDotK || num_segments <= 0 || !seg_numel || !d_in)
    return fail(FA_ERR_INVALID, "%s: invalid arguments (1 <= k <= %d)", fn, kMaxDotK);
  if (!d_gram) return fail(FA_ERR_INVALID, "%s: d_gram is NULL", fn);
  if (dtype != FA_DTYPE_F32 && dtype != FA_DTYPE_BF16 && dtype != FA_DTYPE_F16 && dtype != FA_DTYPE_F64)
    return fail(FA_ERR_DTYPE, "%s: dtype %d not supported (F32, BF16, F16, F64)", fn, dtype);
  if (tstride < 0 || tstride % FA_TILE_BYTES)
    return fail(FA_ERR_INVALID, "%s: tile_stride must be a positive multiple of %d (got %lld)", fn, FA_TILE_BYTES,
                (long long)tstride);
  const DotPlan q = dot_plan(k, dtype);
  int nseg = 0;
  for (int s = 0; s < num_segments; ++s) {
    if (seg_numel[s] < 0) return fail(FA_ERR_INVALID, "%s: segment %d has negative numel", fn, s);
    if (seg_numel[s] == 0) continue;
    if (d_center && !d_center[s]) return fail(FA_ERR_INVALID, "%s: segment %d: center NULL", fn, s);
    if (d_hist)
      for (int i = 0; i < k; ++i)
        if (!d_hist[(int64_t)s * k + i])
          return fail(FA_ERR_INVALID, "%s: segment %d client %d: history NULL", fn, s, i);
    for (int i = 0; i < k; ++i)
      if (!d_in[(int64_t)s * k + i]) return fail(FA_ERR_INVALID, "%s: segment %d client %d: input NULL", fn, s, i);
    ++nseg;
  }
  const int64_t nchunks = dot_chunks(num_segments, seg_numel, q.pe);
  const int64_t ntri = (int64_t)k * (k + 1) / 2;
  const int nblocks = (int)std::max<int64_t>(1, std::min<int64_t>(nchunks, kDotBlocks));
  const size_t need = fa_pairwise_dot_scratch_bytes(num_segments, seg_numel, k);
  if (nseg && (!d_scratch || scratch_bytes < need))
    return fail(FA_ERR_INVALID, "%s: scratch must hold %zu bytes", fn, need);
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(FA_ERR_HIP, "hipSetDevice(%d) failed", ctx->device);
  hipStream_t st = (hipStream_t)hip_stream;
  if (nseg == 0) {
    FA_HIP(hipMemsetAsync(d_gram, 0, sizeof(double) * (size_t)k * k, st));
    return FA_OK;
  }
  // the tables: segments, input pointers, then (given) history pointers and center pointers
  const size_t seg_bytes = align16(sizeof(DSeg) * nseg);
  const size_t ptr_bytes = sizeof(void*) * (size_t)nseg * k;
  const size_t hist_bytes = d_hist ? ptr_bytes : 0;
  const size_t cen_bytes = d_center ? sizeof(void*) * (size_t)nseg : 0;
  fa_ctx::Slot* slot = nullptr;
  int rc = acquire_slot(ctx, seg_bytes + ptr_bytes + hist_bytes + cen_bytes, &slot);
  if (rc) return rc;
  char* h = (char*)slot->host;
  DSeg* hs = (DSeg*)h;
  const void** hp = (const void**)(h + seg_bytes);
  void** hh = (void**)(h + seg_bytes + ptr_bytes);
  const void** hc = (const void**)(h + seg_bytes + ptr_bytes + hist_bytes);
  int j = 0;
  int64_t c0 = 0;
  for (int s = 0; s < num_segments; ++s) {
    const int64_t n = seg_numel[s];
    if (n == 0) continue;
    bool aligned = !d_center || al16(d_center[s]);
    for (int i = 0; i < k; ++i) {
      hp[(int64_t)j * k + i] = d_in[(int64_t)s * k + i];
      aligned = aligned && al16(d_in[(int64_t)s * k + i]);
      if (d_hist) {
        hh[(int64_t)j * k + i] = d_hist[(int64_t)s * k + i];
        aligned = aligned && al16(d_hist[(int64_t)s * k + i]);
      }
    }
    if (d_center) hc[j] = d_center[s];
    hs[j] = DSeg{n, c0, tstride, j * k, aligned ? 1 : 0};
    c0 += (n + q.pe - 1) / q.pe;
    ++j;
  }
  rc = stage(slot, seg_bytes + ptr_bytes + hist_bytes + cen_bytes, st, true);
  if (rc) return rc;
  const char* dv = (const char*)slot->dev;
  const DSeg* ds = (const DSeg*)dv;
  const void* const* dp = (const void* const*)(dv + seg_bytes);
  void* const* dh = d_hist ? (void* const*)(dv + seg_bytes + ptr_bytes) : nullptr;
  const void* const* dc = d_center ? (const void* const*)(dv + seg_bytes + ptr_bytes + hist_bytes) : nullptr;
  const dim3 grid((unsigned)nblocks), block((unsigned)q.nthreads);
#define FA_PDOT(DT, TL)                                                                                        \
  hipLaunchKernelGGL((k_pairdot<DT, TL>), grid, block, q.lds, st, ds, nseg, dp, dc, dh, (int)k, q.kp, nchunks, \
                     q.ntiles, q.esplit, q.pe, q.cemax, (double*)d_scratch)
#define FA_PDOT_T(DT) \
  if (tstride) FA_PDOT(DT, true); else FA_PDOT(DT, false)
  switch (dtype) {
    case FA_DTYPE_F32: FA_PDOT_T(FA_DTYPE_F32); break;
    case FA_DTYPE_BF16: FA_PDOT_T(FA_DTYPE_BF16); break;
    case FA_DTYPE_F16: FA_PDOT_T(FA_DTYPE_F16); break;
    default: FA_PDOT_T(FA_DTYPE_F64); break;
  }
#undef FA_PDOT_T
#undef FA_PDOT
  hipLaunchKernelGGL(k_pairdot_reduce, dim3((unsigned)((ntri + 7) / 8)), dim3(kBlock), 0, st,
                     (const double*)d_scratch, nblocks, (int)k, (double*)d_gram);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    (void)release(slot, st);
    return fail(FA_ERR_HIP, "%s: %s", fn, hipGetErrorString(e));
  }
  return release(slot, st);
}

}  // namespace

extern "C" {

int fa_pairwise_dot(fa_ctx* ctx, int dtype, int32_t num_segments, const int64_t* seg_numel, int32_t k,
                    const void* const* d_in, const void* const* d_center, void* const* d_hist, void* d_gram,
                    void* d_scratch, size_t scratch_bytes, void* hip_stream) {
  return dot_impl("fa_pairwise_dot", ctx, dtype, num_segments, seg_numel, k, d_in, 0, d_center, d_hist, d_gram,
                  d_scratch, scratch_bytes, hip_stream);
}

int fa_pairwise_dot_tiled(fa_ctx* ctx, int dtype, int32_t num_segments, const int64_t* seg_numel, int32_t k,
                          const void* const* d_in, int64_t tile_stride, const void* const* d_center,
                          void* const* d_hist, void* d_gram, void* d_scratch, size_t scratch_bytes,
                          void* hip_stream) {
  if (ctx && tile_stride <= 0) return fail(FA_ERR_INVALID, "fa_pairwise_dot_tiled: tile_stride must be > 0");
  return dot_impl("fa_pairwise_dot_tiled", ctx, dtype, num_segments, seg_numel, k, d_in, tile_stride, d_center,
                  d_hist, d_gram, d_scratch, scratch_bytes, hip_stream);
}

// The partials of the dtype with the most chunks (the smallest chunk), so one buffer serves every dtype.
size_t fa_pairwise_dot_scratch_bytes(int32_t num_segments, const int64_t* seg_numel, int32_t k) {
  if (k < 1 || k > kMaxDotK || num_segments <= 0 || !seg_numel) return 0;
  int64_t nchunks = 0;
  for (int dt : {FA_DTYPE_F32, FA_DTYPE_BF16, FA_DTYPE_F16, FA_DTYPE_F64})
    nchunks = std::max(nchunks, dot_chunks(num_segments, seg_numel, dot_plan(k, dt).pe));
  const int64_t nblocks = std::max<int64_t>(1, std::min<int64_t>(nchunks, kDotBlocks));
  return sizeof(double) * (size_t)((int64_t)k * (k + 1) / 2) * (size_t)nblocks;
}

}  // extern "C"
