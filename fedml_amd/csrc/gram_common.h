// gram_common.h -- what the Gram-matrix entries of the block-compressed families share (quant_gram.hip:
// q8 on the int8 matrix cores; signgram.hip: q1 on XOR and population counts): the work split of
// fedagg_quant_gram.h / fedagg_sign_gram.h, the staged segment and pointer tables, the per-workgroup
// float64 slab layout [pair of 16-client tiles][16][16], the fixed-order reduction of the slabs into both
// triangles of G and the distances from G's bits.  Not part of the ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "fa_internal.h"

namespace fa_detail {

struct GSeg {
  int64_t numel;
  int64_t tile_start;  // first unit of this segment (find_seg keys on it)
  int32_t ptr_base;
  int32_t aligned;     // every data pointer of the segment is 16-byte aligned
};
static_assert(sizeof(GSeg) == 24, "GSeg layout");

// The split: units of `unit` elements over the non-empty segments, dealt in consecutive runs to
// min(max_wg, ceil(units / min_units)) workgroups.
inline int64_t gram_units(int32_t num_segments, const int64_t* seg_numel, int64_t unit) {
  int64_t n = 0;
  for (int s = 0; s < num_segments; ++s)
    if (seg_numel[s] > 0) n += (seg_numel[s] + unit - 1) / unit;
  return n;
}
inline int64_t gram_workgroups(int64_t units, int64_t min_units, int64_t max_wg) {
  return std::min<int64_t>(max_wg, (units + min_units - 1) / min_units);
}

// upper-triangular pairs of nt tiles, row-major: pair -> (ti, tj), ti <= tj, and back
__host__ __device__ __forceinline__ void pair_tiles(int p, int nt, int& ti, int& tj) {
  int r = 0, rem = p;
  while (rem >= nt - r) { rem -= nt - r; ++r; }
  ti = r;
  tj = r + rem;
}
__host__ __device__ __forceinline__ int pair_index(int ti, int tj, int nt) {
  return ti * nt - ti * (ti - 1) / 2 + (tj - ti);
}

// The device tables of one call: the non-empty segments, then their data and their scale pointers,
// [segment][client].  Filled on the host, staged through one slot of the context (acquire_slot .. stage);
// the caller releases the slot after its launches.
struct GramTables {
  fa_ctx::Slot* slot = nullptr;
  const GSeg* segs = nullptr;
  const void* const* data = nullptr;
  const void* const* scale = nullptr;
};
inline int gram_stage_tables(fa_ctx* ctx, int32_t num_segments, const int64_t* seg_numel, int32_t k, int nseg,
                             int64_t unit, const void* const* d_data, const void* const* d_scale, hipStream_t st,
                             GramTables* t) {
  const size_t seg_bytes = align16(sizeof(GSeg) * nseg);
  const size_t ptr_bytes = sizeof(void*) * (size_t)nseg * k;
  int rc = acquire_slot(ctx, seg_bytes + 2 * ptr_bytes, &t->slot);
  if (rc) return rc;
  char* h = (char*)t->slot->host;
  GSeg* hs = (GSeg*)h;
  const void** hq = (const void**)(h + seg_bytes);
  const void** hsc = (const void**)(h + seg_bytes + ptr_bytes);
  int j = 0;
  int64_t t0 = 0;
  for (int s = 0; s < num_segments; ++s) {
    const int64_t n = seg_numel[s];
    if (n == 0) continue;
    bool aligned = true;
    for (int i = 0; i < k; ++i) {
      hq[(int64_t)j * k + i] = d_data[(int64_t)s * k + i];
      hsc[(int64_t)j * k + i] = d_scale[(int64_t)s * k + i];
      aligned = aligned && al16(d_data[(int64_t)s * k + i]);
    }
    hs[j] = GSeg{n, t0, j * k, aligned ? 1 : 0};
    t0 += (n + unit - 1) / unit;
    ++j;
  }
  rc = stage(t->slot, seg_bytes + 2 * ptr_bytes, st, true);
  if (rc) return rc;
  const char* dv = (const char*)t->slot->dev;
  t->segs = (const GSeg*)dv;
  t->data = (const void* const*)(dv + seg_bytes);
  t->scale = (const void* const*)(dv + seg_bytes + ptr_bytes);
  return FA_OK;
}

// G = the workgroups' slabs added in a fixed order: kRP entries per workgroup here, kBlock / kRP lanes per
// entry (lane l adds slabs l, l + L, ...; then the L lane sums in lane order).  The entries i <= j of a
// pair's tile go to both triangles; a diagonal tile's i > j entries and the rows past k are dropped.
static __global__ void __launch_bounds__(kBlock)
k_gram_reduce(const double* __restrict__ partial, int nslabs, int k, int nt, double* __restrict__ gram) {
  constexpr int kRP = 8, L = kBlock / kRP;
  __shared__ double red[L][kRP + 1];
  const int64_t nent = (int64_t)nt * (nt + 1) / 2 * 256;
  const int pl = threadIdx.x % kRP, lane = threadIdx.x / kRP;
  const int64_t p = (int64_t)blockIdx.x * kRP + pl;
  double s = 0.0;
  if (p < nent)
    for (int b = lane; b < nslabs; b += L) s += partial[(int64_t)b * nent + p];
  red[lane][pl] = s;
  __syncthreads();
  if (lane == 0 && p < nent) {
    double tsum = 0.0;
    for (int l = 0; l < L; ++l) tsum += red[l][pl];
    int ti, tj;
    pair_tiles((int)(p / 256), nt, ti, tj);
    const int i = 16 * ti + (int)(p % 256) / 16, j = 16 * tj + (int)(p % 16);
    if (i <= j && j < k) {
      gram[(int64_t)i * k + j] = tsum;
      gram[(int64_t)j * k + i] = tsum;
    }
  }
}

// D_ij = max(+0, (G_ii + G_jj) - 2 G_ij), every op rounded once; a NaN passes; D_ii = +0
static __global__ void __launch_bounds__(kBlock)
k_gram_dist(const double* __restrict__ gram, int k, double* __restrict__ dist) {
  const int idx = (int)(blockIdx.x * kBlock + threadIdx.x);
  if (idx >= k * k) return;
  const int i = idx / k, j = idx % k;
  double d = 0.0;
  if (i != j) {
    const double a = gram[(int64_t)i * k + i] + gram[(int64_t)j * k + j];
    d = a - 2.0 * gram[idx];
    d = d != d ? d : d > 0.0 ? d : 0.0;
  }
  dist[idx] = d;
}

// The two launches after the partial sums: nwg slabs of nt (nt + 1) / 2 tile pairs -> G -> D.  With no
// slab (all segments empty) the reduction writes +0 everywhere.
inline void gram_reduce_dist(hipStream_t st, const double* slabs, int nwg, int k, int nt, double* gram, double* dist) {
  hipLaunchKernelGGL(k_gram_reduce, dim3((unsigned)(nt * (nt + 1) / 2 * 256 / 8)), dim3(kBlock), 0, st, slabs, nwg, k,
                     nt, gram);
  hipLaunchKernelGGL(k_gram_dist, dim3((unsigned)((k * k + kBlock - 1) / kBlock)), dim3(kBlock), 0, st,
                     (const double*)gram, k, dist);
}

}  // namespace fa_detail
