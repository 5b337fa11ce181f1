// blockq_host.h -- the host path shared by the block-compressed client formats: q8 (quant.hip, one
// int8 per element) and q1 (signbits.hip, one sign bit per element), both with one float32 scale per
// block of B elements, and mx (mx.hip, one FP8 or FP4 code per element with one E8M0 scale byte per
// block of 32).  The two entries of a format differ only in the names in their messages, the block
// range, the alignment their data and scales need and the kernel they launch; the argument checks (in the
// order the headers state), the staged tables and the payload are the same and live here once.
// Not part of the ABI.
#pragma once

#include "median_host.h"

namespace fa_detail {

enum { kDataAligned = 1, kOutAligned = 2 };  // per-segment flags of a format's sum kernel

inline bool al4(const void* p) { return ((uintptr_t)p & 3u) == 0; }

// What tells one format from the other on the host.
struct BlockFmt {
  const char* data;      // the data table's name in the messages ("q", "bits", "data")
  int block_min, block_max;
  uintptr_t data_mask;   // alignment the data pointers need, as a mask (0: any)
  uintptr_t scale_mask = 3;  // the same for the scale pointers: float32 scales 3, mx's scale bytes 0
};

// log2 of a valid block size, or -1
inline int block_shift(const BlockFmt& f, int32_t block) {
  if (block < f.block_min || block > f.block_max || (block & (block - 1))) return -1;
  int s = 0;
  while ((1 << s) < block) ++s;
  return s;
}

inline int block_fail(const char* fn, const BlockFmt& f, int32_t block) {
  return fail(FA_ERR_INVALID, "%s: block %d is not a power of two in [%d, %d]", fn, block, f.block_min, f.block_max);
}

inline bool data_ok(const BlockFmt& f, const void* p) { return p && !((uintptr_t)p & f.data_mask); }
inline const char* data_what(const BlockFmt& f) { return f.data_mask ? " or not 4-byte aligned" : ""; }
inline bool scale_ok(const BlockFmt& f, const void* p) { return p && !((uintptr_t)p & f.scale_mask); }
inline const char* scale_what(const BlockFmt& f) { return f.scale_mask ? " or not 4-byte aligned" : ""; }

// Every non-empty segment's output (d_out NULL: the entry has none) and its k data and scale pointers, in
// that order; counts the non-empty segments and their workgroups of `slot` elements.
inline int block_check_segments(const char* fn, const BlockFmt& f, int64_t slot, int32_t num_segments,
                                const int64_t* seg_numel, int32_t k, const void* const* d_data,
                                const void* const* d_scale, void* const* d_out, int* nseg, int64_t* tiles) {
  *nseg = 0;
  *tiles = 0;
  for (int s = 0; s < num_segments; ++s) {
    if (seg_numel[s] < 0) return fail(FA_ERR_INVALID, "%s: segment %d has negative numel", fn, s);
    if (seg_numel[s] == 0) continue;
    if (d_out && (!d_out[s] || !al4(d_out[s])))
      return fail(FA_ERR_INVALID, "%s: segment %d: output NULL or not 4-byte aligned", fn, s);
    for (int i = 0; i < k; ++i) {
      const int64_t t = (int64_t)s * k + i;
      if (!data_ok(f, d_data[t]))
        return fail(FA_ERR_INVALID, "%s: segment %d client %d: %s NULL%s", fn, s, i, f.data, data_what(f));
      if (!scale_ok(f, d_scale[t]))
        return fail(FA_ERR_INVALID, "%s: segment %d client %d: scale NULL%s", fn, s, i, scale_what(f));
    }
    ++*nseg;
    *tiles += (seg_numel[s] + slot - 1) / slot;
  }
  if (*tiles > 0x7FFFFFFFll) return fail(FA_ERR_INVALID, "%s: too many tiles", fn);
  return FA_OK;
}

// The fused decompress-and-sum of k clients: d_data[s * k + i], d_scale[s * k + i], d_out[s]; a
// workgroup owns `slot` elements.  Checks in the order of fedagg_quant.h / fedagg_sign.h, then stages
// the MSeg and data-pointer tables and, as the payload, the k coefficients, the non-empty segments'
// scale pointers ([segment][client], as the data table) and one flag word per segment, and calls
// launch(grid, stream, segs, nseg, data ptrs, scale ptrs, flags, coef, shift).  kDataAligned is staged for
// every format; q8 and mx read it (k_wsum_q1 loads one dword per lane, the same at any 4-byte alignment).
template <class Launch>
int block_sum_entry(const char* fn, const BlockFmt& f, int64_t slot, fa_ctx* ctx, int mode, int32_t num_segments,
                    const int64_t* seg_numel, int32_t k, int32_t block, const void* const* d_data,
                    const void* const* d_scale, const double* coef, void* const* d_out, void* hip_stream,
                    Launch launch) {
  if (!ctx) return fail(FA_ERR_INVALID, "%s: ctx is NULL", fn);
  const int shift = block_shift(f, block);
  if (shift < 0) return block_fail(fn, f, block);
  if (k <= 0 || num_segments <= 0) return fail(FA_ERR_INVALID, "%s: k and num_segments must be positive", fn);
  if (!seg_numel || !d_data || !d_scale || !d_out) return fail(FA_ERR_INVALID, "%s: a table is NULL", fn);
  if (!coef && mode != FA_MODE_SUM) return fail(FA_ERR_INVALID, "%s: coef is NULL (allowed for FA_MODE_SUM only)", fn);
  if (mode != FA_MODE_MUL_W && mode != FA_MODE_SUM)
    return fail(FA_ERR_DTYPE, "%s: mode %d not supported (FA_MODE_MUL_W, FA_MODE_SUM)", fn, mode);
  int nseg = 0;
  int64_t tiles = 0;
  if (const int rc = block_check_segments(fn, f, slot, num_segments, seg_numel, k, d_data, d_scale, d_out, &nseg, &tiles))
    return rc;
  if (nseg == 0) return FA_OK;

  const ColArgs a{fn, ctx, FA_DTYPE_F32, num_segments, seg_numel, k, d_data, 0, d_out, hip_stream};
  const size_t coef_bytes = sizeof(double) * (size_t)k;
  const size_t ptr_bytes = sizeof(void*) * (size_t)nseg * k;
  const size_t fl_off = coef_bytes + ptr_bytes;
  const size_t extra = fl_off + ((sizeof(int) * (size_t)nseg + 7) & ~size_t(7));
  return col_stage_launch(
      a, slot, nseg, tiles, extra,
      [&](void* h) {
        for (int i = 0; i < k; ++i) ((double*)h)[i] = coef ? coef[i] : 0.0;
        const void** hs = (const void**)((char*)h + coef_bytes);
        int* hfl = (int*)((char*)h + fl_off);
        int j = 0;
        for (int s = 0; s < num_segments; ++s) {
          if (!seg_numel[s]) continue;
          bool dal = true;
          for (int i = 0; i < k; ++i) {
            hs[(int64_t)j * k + i] = d_scale[(int64_t)s * k + i];
            dal = dal && al16(d_data[(int64_t)s * k + i]);
          }
          hfl[j] = (dal ? kDataAligned : 0) | (al16(d_out[s]) ? kOutAligned : 0);
          ++j;
        }
        if (nseg & 1) hfl[nseg] = 0;  // the padding is staged too
      },
      [&](dim3 grid, hipStream_t st, const MSeg* ds, int n, const void* const* dp, const void* payload) {
        const char* pl = (const char*)payload;
        launch(grid, st, ds, n, dp, (const void* const*)(pl + coef_bytes), (const int*)(pl + fl_off),
               (const double*)pl, shift);
      });
}

// A per-coordinate operator over k <= max_k clients (fedagg_quant_col.h): d_data[s * k + i], d_scale[s * k + i],
// d_out[s]; a workgroup owns `slot` columns.  Checks in that header's order -- check_arg(), the operator's own
// argument (the trim, the keep), after the tables and before the segments -- then stages the MSeg and
// data-pointer tables and, as the payload, the scale pointers and one flag word per segment: kDataAligned here
// says that the segment's data pointers are all 4-byte aligned (dword loads), kOutAligned that its output is
// 16-byte aligned.  Calls launch(grid, stream, segs, nseg, data ptrs, scale ptrs, flags, shift).
template <class ArgCheck, class Launch>
int block_col_entry(const char* fn, const BlockFmt& f, int64_t slot, int32_t max_k, fa_ctx* ctx, int32_t num_segments,
                    const int64_t* seg_numel, int32_t k, int32_t block, const void* const* d_data,
                    const void* const* d_scale, void* const* d_out, void* hip_stream, ArgCheck check_arg,
                    Launch launch) {
  if (!ctx) return fail(FA_ERR_INVALID, "%s: ctx is NULL", fn);
  const int shift = block_shift(f, block);
  if (shift < 0) return block_fail(fn, f, block);
  if (k <= 0 || num_segments <= 0) return fail(FA_ERR_INVALID, "%s: k and num_segments must be positive", fn);
  if (k > max_k)
    return fail(FA_ERR_INVALID, "%s: k %d exceeds %d: dequantize the clients and use the float entry", fn, k, max_k);
  if (!seg_numel || !d_data || !d_scale || !d_out) return fail(FA_ERR_INVALID, "%s: a table is NULL", fn);
  if (const int rc = check_arg()) return rc;
  int nseg = 0;
  int64_t tiles = 0;
  if (const int rc = block_check_segments(fn, f, slot, num_segments, seg_numel, k, d_data, d_scale, d_out, &nseg, &tiles))
    return rc;
  if (nseg == 0) return FA_OK;

  const ColArgs a{fn, ctx, FA_DTYPE_F32, num_segments, seg_numel, k, d_data, 0, d_out, hip_stream};
  const size_t ptr_bytes = sizeof(void*) * (size_t)nseg * k;
  return col_stage_launch(
      a, slot, nseg, tiles, ptr_bytes + ((sizeof(int) * (size_t)nseg + 7) & ~size_t(7)),
      [&](void* h) {
        const void** hs = (const void**)h;
        int* hfl = (int*)((char*)h + ptr_bytes);
        int j = 0;
        for (int s = 0; s < num_segments; ++s) {
          if (!seg_numel[s]) continue;
          bool dal = true;
          for (int i = 0; i < k; ++i) {
            hs[(int64_t)j * k + i] = d_scale[(int64_t)s * k + i];
            dal = dal && al4(d_data[(int64_t)s * k + i]);
          }
          hfl[j] = (dal ? kDataAligned : 0) | (al16(d_out[s]) ? kOutAligned : 0);
          ++j;
        }
        if (nseg & 1) hfl[nseg] = 0;  // the padding is staged too
      },
      [&](dim3 grid, hipStream_t st, const MSeg* ds, int n, const void* const* dp, const void* payload) {
        const char* pl = (const char*)payload;
        launch(grid, st, ds, n, dp, (const void* const*)pl, (const int*)(pl + ptr_bytes), shift);
      });
}

// The quantizer of num_segments tensors of one dtype: d_in[s], d_data[s], d_scale[s].  The table holds
// one "client" per segment (the input), MSeg.out is the segment's data, MSeg.aligned says that input and
// data are 16-byte aligned, the payload is the scale pointers.  Calls
// launch(grid, stream, segs, nseg, input ptrs, scale ptrs, shift).
template <class Launch>
int block_quant_entry(const char* fn, const BlockFmt& f, int64_t slot, fa_ctx* ctx, int dtype, int32_t num_segments,
                      const int64_t* seg_numel, int32_t block, const void* const* d_in, void* const* d_data,
                      void* const* d_scale, void* hip_stream, Launch launch) {
  if (!ctx) return fail(FA_ERR_INVALID, "%s: ctx is NULL", fn);
  const int shift = block_shift(f, block);
  if (shift < 0) return block_fail(fn, f, block);
  if (num_segments <= 0) return fail(FA_ERR_INVALID, "%s: num_segments must be positive", fn);
  if (!seg_numel || !d_in || !d_data || !d_scale) return fail(FA_ERR_INVALID, "%s: a table is NULL", fn);
  if (dtype != FA_DTYPE_F32 && dtype != FA_DTYPE_BF16 && dtype != FA_DTYPE_F16)
    return fail(FA_ERR_DTYPE, "%s: dtype %d not supported (F32, BF16, F16)", fn, dtype);
  const uintptr_t in_mask = dtype == FA_DTYPE_F32 ? 3u : 1u;
  int nseg = 0;
  int64_t tiles = 0;
  for (int s = 0; s < num_segments; ++s) {
    if (seg_numel[s] < 0) return fail(FA_ERR_INVALID, "%s: segment %d has negative numel", fn, s);
    if (seg_numel[s] == 0) continue;
    if (!d_in[s] || ((uintptr_t)d_in[s] & in_mask))
      return fail(FA_ERR_INVALID, "%s: segment %d: input NULL or not aligned to its element", fn, s);
    if (!data_ok(f, d_data[s])) return fail(FA_ERR_INVALID, "%s: segment %d: %s NULL%s", fn, s, f.data, data_what(f));
    if (!scale_ok(f, d_scale[s])) return fail(FA_ERR_INVALID, "%s: segment %d: scale NULL%s", fn, s, scale_what(f));
    ++nseg;
    tiles += (seg_numel[s] + slot - 1) / slot;
  }
  if (tiles > 0x7FFFFFFFll) return fail(FA_ERR_INVALID, "%s: too many tiles", fn);
  if (nseg == 0) return FA_OK;

  const ColArgs a{fn, ctx, dtype, num_segments, seg_numel, 1, d_in, 0, d_data, hip_stream};
  return col_stage_launch(
      a, slot, nseg, tiles, sizeof(void*) * (size_t)nseg,
      [&](void* h) {
        for (int s = 0, j = 0; s < num_segments; ++s)
          if (seg_numel[s]) ((void**)h)[j++] = d_scale[s];
      },
      [&](dim3 grid, hipStream_t st, const MSeg* ds, int n, const void* const* dp, const void* payload) {
        launch(grid, st, ds, n, dp, (void* const*)payload, shift);
      });
}

// The fused sum and squared distances of k clients (fedagg_quant_dist.h): block_sum_entry's tables, with a
// flat float32 center per segment (centered), 2k float64 sums in d_stats and the workgroups' rows of them
// in d_scratch.  centered with coef NULL measures against the center and has no output: d_out is not
// looked at and MSeg.out is the center, which is not written.  Checks in the header's order: ctx; block;
// the tables as block_sum_entry orders them; the center; d_stats; the scratch.  The payload is the k
// coefficients, the scale pointers, one flag word per segment -- kDataAligned here says that the segment's
// q pointers, its output and its center are ALL 16-byte aligned -- and the center pointers.  Calls
// launch(grid, stream, segs, nseg, data ptrs, scale ptrs, flags, center ptrs, coef, shift, tiles).
template <class Launch>
int block_dist_entry(const char* fn, const BlockFmt& f, int64_t slot, fa_ctx* ctx, bool centered, int32_t num_segments,
                     const int64_t* seg_numel, int32_t k, int32_t block, const void* const* d_data,
                     const void* const* d_scale, const void* const* d_center, const double* coef, void* const* d_out,
                     void* d_stats, void* d_scratch, size_t scratch_bytes, void* hip_stream, Launch launch) {
  if (!ctx) return fail(FA_ERR_INVALID, "%s: ctx is NULL", fn);
  const int shift = block_shift(f, block);
  if (shift < 0) return block_fail(fn, f, block);
  const bool dist = centered && !coef;
  if (dist) d_out = nullptr;
  if (k <= 0 || num_segments <= 0) return fail(FA_ERR_INVALID, "%s: k and num_segments must be positive", fn);
  if (!seg_numel || !d_data || !d_scale || (!dist && !d_out)) return fail(FA_ERR_INVALID, "%s: a table is NULL", fn);
  if (!coef && !centered) return fail(FA_ERR_INVALID, "%s: coef is NULL", fn);
  int nseg = 0;
  int64_t tiles = 0;
  if (const int rc = block_check_segments(fn, f, slot, num_segments, seg_numel, k, d_data, d_scale, d_out, &nseg, &tiles))
    return rc;
  if (centered) {
    if (!d_center) return fail(FA_ERR_INVALID, "%s: d_center is NULL", fn);
    for (int s = 0; s < num_segments; ++s)
      if (seg_numel[s] && (!d_center[s] || !al4(d_center[s])))
        return fail(FA_ERR_INVALID, "%s: segment %d: center NULL or not 4-byte aligned", fn, s);
  }
  if (!d_stats) return fail(FA_ERR_INVALID, "%s: d_stats is NULL", fn);
  const size_t need = (size_t)tiles * 2 * (size_t)k * sizeof(double);
  if (need > scratch_bytes || (need && !d_scratch))
    return fail(FA_ERR_INVALID, "%s: scratch too small (%zu bytes, need %zu)", fn, d_scratch ? scratch_bytes : (size_t)0,
                need);
  if (nseg == 0) {  // nothing to read: every sum is 0
    DeviceGuard g(ctx->device);
    if (!g.ok) return fail(FA_ERR_HIP, "hipSetDevice(%d) failed", ctx->device);
    FA_HIP(hipMemsetAsync(d_stats, 0, sizeof(double) * 2 * (size_t)k, (hipStream_t)hip_stream));
    return FA_OK;
  }

  void* const* outs = dist ? (void* const*)d_center : d_out;
  const ColArgs a{fn, ctx, FA_DTYPE_F32, num_segments, seg_numel, k, d_data, 0, outs, hip_stream};
  const size_t coef_bytes = sizeof(double) * (size_t)k;
  const size_t ptr_bytes = sizeof(void*) * (size_t)nseg * k;
  const size_t fl_off = coef_bytes + ptr_bytes;
  const size_t cen_off = fl_off + ((sizeof(int) * (size_t)nseg + 7) & ~size_t(7));
  return col_stage_launch(
      a, slot, nseg, tiles, cen_off + sizeof(void*) * (size_t)nseg,
      [&](void* h) {
        for (int i = 0; i < k; ++i) ((double*)h)[i] = coef ? coef[i] : 0.0;
        const void** hs = (const void**)((char*)h + coef_bytes);
        int* hfl = (int*)((char*)h + fl_off);
        const void** hc = (const void**)((char*)h + cen_off);
        int j = 0;
        for (int s = 0; s < num_segments; ++s) {
          if (!seg_numel[s]) continue;
          bool al = al16(outs[s]) && (!centered || al16(d_center[s]));
          for (int i = 0; i < k; ++i) {
            hs[(int64_t)j * k + i] = d_scale[(int64_t)s * k + i];
            al = al && al16(d_data[(int64_t)s * k + i]);
          }
          hfl[j] = al ? kDataAligned : 0;
          hc[j] = centered ? d_center[s] : nullptr;
          ++j;
        }
        if (nseg & 1) hfl[nseg] = 0;  // the padding is staged too
      },
      [&](dim3 grid, hipStream_t st, const MSeg* ds, int n, const void* const* dp, const void* payload) {
        const char* pl = (const char*)payload;
        launch(grid, st, ds, n, dp, (const void* const*)(pl + coef_bytes), (const int*)(pl + fl_off),
               (const void* const*)(pl + cen_off), (const double*)pl, shift, tiles);
      });
}

}  // namespace fa_detail
