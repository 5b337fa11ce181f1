/*
 * fedagg_quant_gram.h -- the Gram matrix and the pairwise squared distances of k clients' q8 uploads,
 * straight from the uploaded bytes (fedml_amd/csrc/quant_gram.hip).  Included by fedagg_quant.h, whose
 * format, memory, asynchrony and error rules hold here.  This header is the specification.
 *
 * Why: Krum and multi-Krum need only the k x k Gram matrix of the clients.  For q8 the Gram matrix of one
 * block is an integer matrix product times two scales,
 *     G_ij = sum_b s_i[b] * s_j[b] * I_ij[b],    I_ij[b] = sum_{e in b} q_i[e] * q_j[e],
 * and |I| <= 128^2 * 1024 = 2^24 is exact in int32 (v_mfma_i32_16x16x64_i8).  Without this entry a caller
 * dequantizes all k clients to float32 (4 * k * P bytes written and read back) before fa_pairwise_sqdist
 * accepts them; this entry reads 1 + 4/B bytes per client element, once, and holds no float32 copy.
 */
#ifndef FEDAGG_QUANT_GRAM_H
#define FEDAGG_QUANT_GRAM_H

#include "fedagg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FA_Q8_GRAM_MAX_K 128
#define FA_Q8_GRAM_BLOCK_MIN 64    /* one v_mfma_i32_16x16x64_i8 spans 64 elements */
/* The work split, a function of the segment sizes alone: a segment is cut into units of FA_Q8_GRAM_UNIT
 * elements (the last may be ragged); the units of all non-empty segments, in order, are dealt in
 * consecutive runs to W = min(FA_Q8_GRAM_MAX_WORKGROUPS, ceil(units / FA_Q8_GRAM_MIN_UNITS)) workgroups,
 * workgroup g taking units [units * g / W, units * (g + 1) / W).  A workgroup stages
 * FA_Q8_GRAM_STAGE_MIN .. FA_Q8_GRAM_UNIT elements of every client at a time (by k: 1024 for k <= 32,
 * 512 for k <= 64, 256 above). */
#define FA_Q8_GRAM_UNIT 1024
#define FA_Q8_GRAM_MIN_UNITS 4
#define FA_Q8_GRAM_MAX_WORKGROUPS 512
#define FA_Q8_GRAM_STAGE_MIN 256

/*
 * G and D of k clients' q8 tensors over num_segments segments, three launches (partial sums, their
 * reduction, the distances):
 *   d_q[s * k + i], d_scale[s * k + i]   client i's data and scales of segment s (fa_weighted_sum_q8's tables);
 *   d_gram   k x k float64, row-major; may be NULL (G is then kept in the scratch only);
 *   d_dist   k x k float64, row-major;
 *   d_scratch, scratch_bytes   at least fa_pairwise_gram_q8_scratch_bytes(num_segments, seg_numel, k)
 *                              bytes of device memory, 8-byte aligned, the call's to write.
 * Ranges: 1 <= k <= FA_Q8_GRAM_MAX_K; block a power of two in [FA_Q8_GRAM_BLOCK_MIN, FA_Q8_BLOCK_MAX]
 * (the format's blocks of 16 and 32 return FA_ERR_INVALID: dequantize those).
 * Alignment: q pointers may have any alignment; a segment whose q pointers are all 16-byte aligned takes
 * 16-byte loads, any other takes byte loads, and both give the same bits.  scale pointers are 4-byte
 * aligned (else FA_ERR_INVALID).
 *
 * Contract.
 *   integer part  I_ij[b] is the exact integer; elements past seg_numel in a ragged last block count as 0.
 *   float part    p_ij[b] = (double)s_i[b] * (double)s_j[b], exact in float64 (two 24-bit significands);
 *                 acc = fma(p_ij[b], (double)I_ij[b], acc): ONE fused multiply-add per term, rounded once.
 *                 Sums are float64 and use no floating-point atomics.  A workgroup adds the blocks of its
 *                 run in block order starting from +0; G is the workgroups' sums added in a fixed order
 *                 that depends on the workgroup count alone (lane l of 32 adds workgroups l, l + 32, ...
 *                 from +0, then the 32 lane sums are added in lane order from +0).  So the order in which
 *                 blocks are summed is a function of the block index and the segment sizes, the same for
 *                 every pair (i, j) and for every k; the same call gives the same bits every time; G is
 *                 symmetric bit for bit (one value is written to both triangles).
 *   error bound   with M the number of blocks over all segments and t_ij[b] = s_i[b] s_j[b] I_ij[b],
 *                     |G_ij - exact| <= (M + 2) * 2^-53 * sum_b |t_ij[b]|
 *                 (each term is rounded once, inside an addition; a sum of M numbers in any order of
 *                 additions stays within (M - 1) u of the sum of magnitudes, to first order).
 *   exact case    where every term and every partial sum is representable in float64 (scales that are
 *                 powers of two in a narrow range, for one), G is exact.
 *   distances     D_ij = max(+0, rnd(rnd(G_ii + G_jj) - 2 * G_ij)) from G's bits, nothing fused; a NaN
 *                 passes through; D_ii = +0.0 whatever G_ii is; D_ij and D_ji carry the same bits.
 *   identical     two clients with identical q and scale have G_ii = G_jj = G_ij bit for bit (the order
 *   clients       rule), so D_ij = +0.0 exactly: the sybil case Krum must see.
 *   poisoned      a block with the quantizer's NaN scale (q = 0, so I = 0 and every term NaN * 0 = NaN)
 *   clients       makes that client's row and column of G NaN, G_ii included, and its row and column of
 *                 D NaN except D_ii = +0.0.  No other entry changes: the other entries are the ones the
 *                 call gives with that block's scale set to 0.
 *
 * Checked before any HIP call, in this order: ctx; block; k and num_segments; seg_numel, d_q, d_scale,
 * d_dist; per non-empty segment its pointers and alignment; the scratch.  All return FA_ERR_INVALID.
 * With all segments empty G and D are written as +0.0.  Never aborts.
 */
int fa_pairwise_gram_q8(fa_ctx *ctx, int32_t num_segments, const int64_t *seg_numel, int32_t k, int32_t block,
                        const void *const *d_q, const void *const *d_scale, void *d_gram, void *d_dist,
                        void *d_scratch, size_t scratch_bytes, void *hip_stream);

/* One float64 slab of 256 entries per upper-triangular pair of 16-client tiles and workgroup, plus
 * k x k float64 for G.  0 for arguments the entry would reject. */
size_t fa_pairwise_gram_q8_scratch_bytes(int32_t num_segments, const int64_t *seg_numel, int32_t k);

#ifdef __cplusplus
}
#endif

#endif /* FEDAGG_QUANT_GRAM_H */
