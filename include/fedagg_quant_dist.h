/*
 * fedagg_quant_dist.h -- one pass of the geometric median (smoothed Weiszfeld) and of centered clipping over
 * k clients' q8 uploads, straight from the uploaded bytes (fedml_amd/csrc/quant_dist.hip).  Included by
 * fedagg_quant.h, whose format, memory, asynchrony and error rules hold here.  This header is the
 * specification.
 *
 * Why: both defenses are iterative -- iters + 1 passes over all k clients, each pass the weighted sum (or
 * the clipped update around a center) AND every client's squared distance to it.  Without these entries a
 * caller dequantizes every client to float32 (4 * k * P bytes written) and fa_weighted_sum_sqdist /
 * fa_centered_sum_sqdist read them iters + 1 times; these entries read 1 + 4/B bytes per client element
 * per pass and hold no float32 copy of the clients.
 *
 * Tables as fa_weighted_sum_q8: d_q[s * k + i], d_scale[s * k + i] client i's data and scales of segment s;
 * block a power of two in [FA_Q8_BLOCK_MIN, FA_Q8_BLOCK_MAX]; any k >= 1.
 *   d_out[s], d_center[s]   seg_numel[s] float32, flat, 4-byte aligned;
 *   d_stats                 2k float64 on the device: d_stats[i] = d2_i, d_stats[k + i] = ss_i;
 *   d_scratch, scratch_bytes   at least fa_weighted_sum_sqdist_q8_scratch_bytes(num_segments, seg_numel, k)
 *                           bytes of device memory, 8-byte aligned, the call's to write.
 * Alignment: a segment whose q pointers, output and center are all 16-byte aligned takes 16-byte loads and
 * stores on its whole slots of FA_Q8_DIST_SLOT elements; any other segment, and a ragged last slot, takes
 * byte loads with the same arithmetic per element.  out carries the same bits either way.
 *
 * Contract.  x_i[e] = rnd((float)q_i[e] * scale_i[e / B]) is q8's dequantization.  float32, clients IN
 * ORDER, every op rounded once (rnd), nothing fused.
 *   plain       fa_weighted_sum_sqdist_q8: out is fa_weighted_sum_q8's FA_MODE_MUL_W result bit for bit:
 *               c = rnd(scale_i[b] * (float)coef[i]) once per block, t_i = rnd((float)q_i[e] * c),
 *               out = t_0, out = rnd(out + t_i).
 *   centered    fa_centered_sum_sqdist_q8 with coef: u_i = rnd(x_i - center), t_i = rnd(u_i * (float)coef[i]),
 *               acc = t_0, acc = rnd(acc + t_i), out = rnd(center + acc): fa_centered_sum_sqdist's
 *               FA_DTYPE_F32 out over the dequantized tensors, bit for bit.  d_out[s] may be d_center[s] (the
 *               lane that owns an element reads it, then writes it).
 *   distance    fa_centered_sum_sqdist_q8 with coef NULL: d2 against the center; d_out is ignored and
 *               nothing but d_stats (and the scratch) is written.
 *   stats       d2_i = sum_e (x_i[e] - ref[e])^2 with ref the STORED out (plain, centered) or the center
 *               (distance); ss_i = sum_e x_i[e]^2.  The differences are formed in float32, squared and
 *               summed in float64.  On whole aligned slots ss_i is formed per 16 elements as the exact
 *               integer sum of q^2 times (double)scale * (double)scale (q * scale against rnd(q * scale)
 *               is 2^-23 relative on a square); elsewhere from x_i in float64.  The order of every sum is
 *               a function of k and the segment sizes and alignments alone and no floating-point atomic
 *               is used: the same call gives the same bits.  With all inputs finite each sum is within
 *               1e-6 relative of its exact value over the x_i defined above (fa_weighted_sum_sqdist's
 *               bound); an exact 0 gives exactly 0.
 *   poisoned    a block whose scale is NaN or +-Inf (the quantizer's mark of a non-finite block, q = 0)
 *   clients     makes that client's ss_i non-finite, and no other client's; in the distance form its d2_i
 *               as well, and no other client's.  The drivers drop such a client.
 *
 * Checked before any HIP call, in this order: ctx; block; k and num_segments; seg_numel, d_q, d_scale and
 * (unless coef is NULL in the centered entry) d_out; coef (NULL only in the centered entry); per non-empty
 * segment its output, then its clients' q and scale pointers and their alignment; d_center and per
 * non-empty segment its center; d_stats; the scratch.  All return FA_ERR_INVALID.  With all segments
 * empty d_stats is zeroed and nothing is launched.  Never aborts.
 */
#ifndef FEDAGG_QUANT_DIST_H
#define FEDAGG_QUANT_DIST_H

#include "fedagg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FA_Q8_DIST_SLOT 4096 /* elements of every client one workgroup owns: one row of the scratch */

int fa_weighted_sum_sqdist_q8(fa_ctx *ctx, int32_t num_segments, const int64_t *seg_numel, int32_t k, int32_t block,
                              const void *const *d_q, const void *const *d_scale, const double *coef,
                              void *const *d_out, void *d_stats, void *d_scratch, size_t scratch_bytes,
                              void *hip_stream);

int fa_centered_sum_sqdist_q8(fa_ctx *ctx, int32_t num_segments, const int64_t *seg_numel, int32_t k, int32_t block,
                              const void *const *d_q, const void *const *d_scale, const void *const *d_center,
                              const double *coef, void *const *d_out, void *d_stats, void *d_scratch,
                              size_t scratch_bytes, void *hip_stream);

/* 2k float64 per slot of FA_Q8_DIST_SLOT elements of every segment.  0 for arguments the entries would
 * reject. */
size_t fa_weighted_sum_sqdist_q8_scratch_bytes(int32_t num_segments, const int64_t *seg_numel, int32_t k);

#ifdef __cplusplus
}
#endif

#endif /* FEDAGG_QUANT_DIST_H */
