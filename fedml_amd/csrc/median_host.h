// median_host.h -- the host path shared by the C entries that launch over an MSeg table (median.hip,
// trimmed.hip, wsum_dist.hip, signvote.hip, fedopt_adaptive.hip): argument checks, the grid for a given element count per
// workgroup, the MSeg + pointer table (and an entry's own payload) in a staging slot, and the launch.
// An entry checks in this order: col_check_args (NULL context, then the other arguments), its own
// arguments (the trim; d_center, coef and d_stats; coef and the threshold), col_count (dtype,
// tile_stride, then the segments), its scratch.
// Not part of the ABI.
#pragma once

#include "fa_internal.h"
#include "median_common.h"

namespace fa_detail {

// The arguments every per-column entry takes; fn is the entry's name for the messages.
struct ColArgs {
  const char* fn;
  fa_ctx* ctx;
  int dtype;
  int32_t num_segments;
  const int64_t* seg_numel;
  int32_t k;
  const void* const* d_in;  // [num_segments][k]
  int64_t tstride;          // 0: flat segments; > 0: tile-interleaved inputs
  void* const* d_out;
  void* hip_stream;
  // wsum_dist.hip's and signvote.hip's centered entries: [num_segments] flat tensors, checked with the segments and
  // part of a segment's `aligned`; the entry stages the pointers in its own payload, so the
  // tables staged here do not depend on them.  NULL: no center.
  const void* const* d_center = nullptr;
};

inline int col_check_args(const ColArgs& a) {
  if (!a.ctx) return fail(FA_ERR_INVALID, "%s: ctx is NULL", a.fn);
  if (a.k <= 0 || a.num_segments <= 0 || !a.seg_numel || !a.d_in || !a.d_out)
    return fail(FA_ERR_INVALID, "%s: invalid arguments", a.fn);
  return FA_OK;
}

// Checks the dtype, the tile stride and every non-empty segment's pointers; counts the non-empty
// segments and their workgroups at `cols` elements each -- a count that divides a tile's element
// count (512 float64 at the least), so no workgroup straddles a tile.  (static: the library exports
// nothing of this header)
static inline int col_count(const ColArgs& a, int64_t cols, int* nseg, int64_t* tiles) {
  if (a.dtype != FA_DTYPE_F32 && a.dtype != FA_DTYPE_BF16 && a.dtype != FA_DTYPE_F16 && a.dtype != FA_DTYPE_F64)
    return fail(FA_ERR_DTYPE, "%s: dtype %d not supported (F32, BF16, F16, F64)", a.fn, a.dtype);
  if (a.tstride < 0 || a.tstride % FA_TILE_BYTES)
    return fail(FA_ERR_INVALID, "%s: tile_stride must be a positive multiple of %d (got %lld)", a.fn, FA_TILE_BYTES,
                (long long)a.tstride);
  *nseg = 0;
  *tiles = 0;
  for (int s = 0; s < a.num_segments; ++s) {
    if (a.seg_numel[s] < 0) return fail(FA_ERR_INVALID, "%s: segment %d has negative numel", a.fn, s);
    if (a.seg_numel[s] == 0) continue;
    if (a.d_center && !a.d_center[s]) return fail(FA_ERR_INVALID, "%s: segment %d: center NULL", a.fn, s);
    if (!a.d_out[s]) return fail(FA_ERR_INVALID, "%s: segment %d: output NULL", a.fn, s);
    for (int i = 0; i < a.k; ++i)
      if (!a.d_in[(int64_t)s * a.k + i])
        return fail(FA_ERR_INVALID, "%s: segment %d client %d: input NULL", a.fn, s, i);
    ++*nseg;
    *tiles += (a.seg_numel[s] + cols - 1) / cols;
  }
  if (*tiles > 0x7FFFFFFFll) return fail(FA_ERR_INVALID, "%s: too many tiles", a.fn);
  return FA_OK;
}

// After col_count found nseg > 0 segments and `tiles` workgroups: stages the segment and pointer
// tables of the non-empty segments, followed by `extra` bytes (8-byte aligned) that fill(host
// address) writes (the copy is skipped when the slot already holds all of it), and calls
// launch(grid, stream, segs, nseg, ptrs, the payload's device address).  `scratch` more bytes of the
// slot's device buffer follow the payload (at its address + extra): never copied, theirs to write for
// the kernels launched here (signvote.hip: the per-workgroup counts).
template <class Fill, class Launch>
int col_stage_launch(const ColArgs& a, int64_t cols, int nseg, int64_t tiles, size_t extra, Fill fill,
                     Launch launch, size_t scratch = 0) {
  const int k = a.k;
  const size_t seg_bytes = align16(sizeof(MSeg) * nseg);
  const size_t ptr_bytes = sizeof(void*) * (size_t)nseg * k;
  DeviceGuard g(a.ctx->device);
  if (!g.ok) return fail(FA_ERR_HIP, "hipSetDevice(%d) failed", a.ctx->device);
  hipStream_t st = (hipStream_t)a.hip_stream;
  fa_ctx::Slot* slot = nullptr;
  int rc = acquire_slot(a.ctx, seg_bytes + ptr_bytes + extra + scratch, &slot);
  if (rc) return rc;
  char* h = (char*)slot->host;
  MSeg* hs = (MSeg*)h;
  const void** hp = (const void**)(h + seg_bytes);
  int j = 0;
  int64_t t0 = 0;
  for (int s = 0; s < a.num_segments; ++s) {
    const int64_t n = a.seg_numel[s];
    if (n == 0) continue;
    bool aligned = al16(a.d_out[s]) && (!a.d_center || al16(a.d_center[s]));
    for (int i = 0; i < k; ++i) {
      hp[(int64_t)j * k + i] = a.d_in[(int64_t)s * k + i];
      aligned = aligned && al16(a.d_in[(int64_t)s * k + i]);
    }
    hs[j] = MSeg{n, t0, a.d_out[s], a.tstride, j * k, aligned ? 1 : 0};
    t0 += (n + cols - 1) / cols;
    ++j;
  }
  fill((void*)(h + seg_bytes + ptr_bytes));
  rc = stage(slot, seg_bytes + ptr_bytes + extra, st, true);
  if (rc) return rc;
  const char* dv = (const char*)slot->dev;
  launch(dim3((unsigned)tiles), st, (const MSeg*)dv, nseg, (const void* const*)(dv + seg_bytes),
         (const void*)(dv + seg_bytes + ptr_bytes));
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    (void)release(slot, st);
    return fail(FA_ERR_HIP, "%s: %s", a.fn, hipGetErrorString(e));
  }
  return release(slot, st);
}

// The two steps for an entry with nothing of its own between them or in the slot (no segment with
// elements: nothing to do).  launch(grid, stream, segs, nseg, ptrs).
template <class Launch>
int col_launch(const ColArgs& a, int64_t cols, Launch launch) {
  int nseg;
  int64_t tiles;
  if (const int rc = col_count(a, cols, &nseg, &tiles)) return rc;
  if (nseg == 0) return FA_OK;
  return col_stage_launch(a, cols, nseg, tiles, 0, [](void*) {},
                          [&](dim3 grid, hipStream_t st, const MSeg* ds, int n, const void* const* dp, const void*) {
                            launch(grid, st, ds, n, dp);
                          });
}

}  // namespace fa_detail
