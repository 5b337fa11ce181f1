/*
 * fedagg_sign_gram.h -- the Gram matrix and the pairwise squared distances of k clients' q1 (1-bit sign)
 * uploads, straight from the uploaded bits (fedml_amd/csrc/signgram.hip).  Includes fedagg_sign.h, whose
 * format, memory, asynchrony and error rules hold here.  This header is the specification.
 *
 * Why: Krum and multi-Krum need only the k x k Gram matrix of the clients.  For two sign vectors the
 * product over a block is a population count,
 *     G_ij = sum_b s_i[b] * s_j[b] * I_ij[b],
 *     I_ij[b] = n_b - 2 * popcount((w_i ^ w_j) over the real elements of block b),
 * n_b the block's real element count, |I| <= 1024.  Without this entry a caller decompresses all k clients
 * to float32 (32 times the upload, written and read back) before fa_pairwise_sqdist accepts them; this
 * entry reads 1/8 + 4/B bytes per client element, once, and holds no float32 copy.
 */
#ifndef FEDAGG_SIGN_GRAM_H
#define FEDAGG_SIGN_GRAM_H

#include "fedagg_sign.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FA_Q1_GRAM_MAX_K 128
/* The work split, a function of the segment sizes alone: a segment is cut into units of FA_Q1_GRAM_UNIT
 * elements (the last may be ragged); the units of all non-empty segments, in order, are dealt in
 * consecutive runs to W = min(FA_Q1_GRAM_MAX_WORKGROUPS, ceil(units / FA_Q1_GRAM_MIN_UNITS)) workgroups,
 * workgroup g taking units [units * g / W, units * (g + 1) / W).  A workgroup stages FA_Q1_GRAM_STAGE
 * elements (16 words) of every client at a time, so a unit is 2 stages and so is a block of 1024. */
#define FA_Q1_GRAM_UNIT 1024
#define FA_Q1_GRAM_MIN_UNITS 4
#define FA_Q1_GRAM_MAX_WORKGROUPS 512
#define FA_Q1_GRAM_STAGE 512

/*
 * G and D of k clients' q1 tensors over num_segments segments, three launches (partial sums, their
 * reduction, the distances):
 *   d_bits[s * k + i], d_scale[s * k + i]   client i's bits and scales of segment s (fa_weighted_sum_q1's tables);
 *   d_gram   k x k float64, row-major; may be NULL (G is then kept in the scratch only);
 *   d_dist   k x k float64, row-major;
 *   d_scratch, scratch_bytes   at least fa_pairwise_gram_q1_scratch_bytes(num_segments, seg_numel, k)
 *                              bytes of device memory, 8-byte aligned, the call's to write.
 * Ranges: 1 <= k <= FA_Q1_GRAM_MAX_K; block every power of two of the format, FA_Q1_BLOCK_MIN (32) to
 * FA_Q1_BLOCK_MAX (1024).
 * Alignment: bits and scale pointers are 4-byte aligned (else FA_ERR_INVALID).  A segment whose bits
 * pointers are all 16-byte aligned takes 16-byte loads, any other takes dword loads, and both give the
 * same bits.
 *
 * Contract.
 *   integer part  I_ij[b] is the exact integer.  Bits past seg_numel in the last word are ignored: they
 *                 are masked, not trusted to be 0.
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
 *   identical     two clients with identical bits and scale have G_ii = G_jj = G_ij bit for bit: the
 *   clients       diagonal goes through the same XOR, count and fma as every other pair (a count of 0), and
 *                 the order rule does the rest.  So D_ij = +0.0 exactly: the sybil case Krum must see.
 *   poisoned      a block with the quantizer's NaN scale makes that client's row and column of G NaN, G_ii
 *   clients       included (I may be 0: NaN * 0 = NaN), and its row and column of D NaN except
 *                 D_ii = +0.0.  No other entry changes: the other entries are the ones the call gives
 *                 with that block's scale set to 0.
 *
 * Checked before any HIP call, in this order: ctx; block; k and num_segments; seg_numel, d_bits, d_scale,
 * d_dist; per non-empty segment its pointers and their 4-byte alignment; the scratch.  All return
 * FA_ERR_INVALID.  With all segments empty G and D are written as +0.0.  Never aborts.
 */
int fa_pairwise_gram_q1(fa_ctx *ctx, int32_t num_segments, const int64_t *seg_numel, int32_t k, int32_t block,
                        const void *const *d_bits, const void *const *d_scale, void *d_gram, void *d_dist,
                        void *d_scratch, size_t scratch_bytes, void *hip_stream);

/* One float64 slab of 256 entries per workgroup and upper-triangular pair of the 2 * ceil(k / 32)
 * 16-client tiles (a wave's 32 x 32 tile is four of them), plus k x k float64 for G.  0 for arguments the
 * entry would reject. */
size_t fa_pairwise_gram_q1_scratch_bytes(int32_t num_segments, const int64_t *seg_numel, int32_t k);

#ifdef __cplusplus
}
#endif

#endif /* FEDAGG_SIGN_GRAM_H */
