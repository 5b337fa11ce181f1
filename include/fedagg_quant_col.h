/*
 * fedagg_quant_col.h -- the coordinate-wise defenses (median, trimmed mean, Bulyan's mean around the median)
 * over k clients' q8 uploads, straight from the uploaded bytes (fedml_amd/csrc/quant_col.hip).  Included by
 * fedagg_quant.h, whose format, memory, asynchrony and error rules hold here.  This header is the
 * specification.
 *
 * Why: fa_coord_median, fa_coord_trimmed_mean and fa_coord_mean_around_median (fedagg_robust.h) read float
 * tensors, so a caller with q8 uploads dequantizes every client first: k * P * 4 bytes of device memory and
 * k * P * (1 + 4 + 4) bytes of extra traffic.  These entries read 1 + 4/B bytes per client element, in one
 * launch for a whole state_dict, and hold no float32 copy of a client.
 *
 * Tables as fa_weighted_sum_q8: d_q[s * k + i], d_scale[s * k + i] client i's data and scales of segment s;
 * d_out[s] seg_numel[s] float32, must not alias an input; block a power of two in [FA_Q8_BLOCK_MIN,
 * FA_Q8_BLOCK_MAX]; 1 <= k <= FA_Q8_COL_MAX_K.  q pointers may have any alignment (a segment whose q
 * pointers are all 4-byte aligned takes dword loads on its whole slots of FA_Q8_COL_SLOT columns, any other
 * segment and a ragged last slot take byte loads: the same bits); scale pointers and outputs are 4-byte
 * aligned; 16-byte aligned outputs take vector stores.
 *
 * Contract.  x_i[e] = rnd((float)q_i[e] * scale_i[e / B]): one float32 multiply, q8's dequantization
 * (fa_weighted_sum_q8 with k = 1 and FA_MODE_SUM).  Per element e the column is x_0[e] .. x_{k-1}[e], ordered
 * ascending with -0.0 below +0.0 and NaN (any sign or payload) above +inf.
 *   fa_coord_trimmed_mean_q8        out is fa_coord_trimmed_mean's FA_DTYPE_F32 result over the x_i, bit for
 *                                   bit: the float64 sum runs in rank order FROM the first kept value, one
 *                                   division, one rounding.  NaN where a NaN is kept, or +inf and -inf are
 *                                   both kept (the NaN's bits are unspecified).
 *   fa_coord_mean_around_median_q8  out is fa_coord_mean_around_median's FA_DTYPE_F32 result over the x_i, bit
 *                                   for bit: steps 2 to 5 of that contract, the [lomin, lomax) restriction
 *                                   included.
 *   fa_coord_median_q8              out is the x value of rank (k - 1) / 2 under the order above; a column
 *                                   that holds a NaN gives NaN (payload unspecified).  This equals
 *                                   fa_coord_median over the x_i bit for bit on every column that does not
 *                                   hold zeros of BOTH signs.  fa_quantize_q8 never produces -0.0: where a
 *                                   scale is 0 every q is 0, scales are >= 0, and a nonzero integer times a
 *                                   nonzero float32 never rounds to zero.  ATen's tie by client index among
 *                                   zeros is dropped on purpose: the float kernel resolves it by a rescan of
 *                                   the column whenever a zero is selected, and on q8 data, where q = 0 is
 *                                   common, that rescan would run on a large share of the columns.
 * A NaN arises from a NaN scale (the quantizer's mark of a non-finite block) or from q = 0 under an infinite
 * scale; such columns are served by the same launch.
 *
 * Checked before any HIP call, in this order: ctx; block; k and num_segments (k > FA_Q8_COL_MAX_K is
 * FA_ERR_INVALID with a message: dequantize and use the float entry); seg_numel, d_q, d_scale, d_out; trim
 * (0 <= trim, 2 * trim < k) or keep (1 <= keep <= k); per non-empty segment its output, then its clients' q
 * and scale pointers and their alignment.  All return FA_ERR_INVALID.  All segments empty is FA_OK with
 * nothing launched.  Never aborts.
 */
#ifndef FEDAGG_QUANT_COL_H
#define FEDAGG_QUANT_COL_H

#include "fedagg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FA_Q8_COL_MAX_K 128
#define FA_Q8_COL_SLOT 1024 /* columns one workgroup owns for k <= 64; half of it for k in (64, 128] */

int fa_coord_median_q8(fa_ctx *ctx, int32_t num_segments, const int64_t *seg_numel, int32_t k, int32_t block,
                       const void *const *d_q, const void *const *d_scale, void *const *d_out, void *hip_stream);

int fa_coord_trimmed_mean_q8(fa_ctx *ctx, int32_t num_segments, const int64_t *seg_numel, int32_t k, int32_t block,
                             int32_t trim, const void *const *d_q, const void *const *d_scale, void *const *d_out,
                             void *hip_stream);

int fa_coord_mean_around_median_q8(fa_ctx *ctx, int32_t num_segments, const int64_t *seg_numel, int32_t k,
                                   int32_t block, int32_t keep, const void *const *d_q, const void *const *d_scale,
                                   void *const *d_out, void *hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* FEDAGG_QUANT_COL_H */
