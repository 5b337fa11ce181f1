/*
 * fedagg_sign.h -- 1-bit sign-compressed ("q1") client updates: a device quantizer, the fused
 * decompress-and-sum, and the majority vote of libfedagg.so (fedml_amd/csrc/signbits.hip).  This header
 * is the specification.
 *
 * Why: after 8-bit block quantization (fedagg_quant.h) the next step of the compression literature is
 * one sign bit per element.  Two forms matter.  Scaled sign (EF-signSGD, Karimireddy et al. 2019; 1-bit
 * SGD / Adam): one bit per element and one float32 magnitude per block; the server takes the ordinary
 * weighted sum of the decompressed updates and reads 1/8 + 4/B bytes per client element, against q8's
 * 1 + 4/B and float32's 4.  Majority vote (signSGD with majority vote, Bernstein et al. 2019): the
 * server outputs only the sign of the sum of signs, a compressor and a Byzantine-robust aggregator at
 * once; it reads the bits alone and touches no float before its last store.  Without these entries a
 * caller unpacks every client to float32 (32 times the upload, written and read back) before
 * fa_weighted_sum_multi or fa_sign_vote_sum accepts it.
 *
 * Format "q1", per segment (one tensor flattened to n elements):
 *   block size B   a power of two, 32 <= B <= 1024, shared by every segment and client of a call;
 *   blocks         start at the segment's first element; the last block may be ragged;
 *   bits           ceil(n / 32) 32-bit words, 4-byte aligned; element e is bit (e & 31) of word
 *                  (e >> 5); 1 means negative.  Bits past n in the last word are written as 0 by the
 *                  quantizer and ignored by the consumers;
 *   scale          ceil(n / B) float32 values, 4-byte aligned;
 *   meaning        element e has the value  bit ? -scale[e / B] : +scale[e / B].
 *
 * Memory, asynchrony and errors: the rules of fedagg.h (device pointers owned by the caller, host
 * tables staged by the library, asynchronous on hip_stream, a negative fa_status and fa_last_error on
 * failure, never an abort).
 *
 * Out of scope: error feedback and stochastic signs (the client's business: it applies either before
 * this format), tile-interleaved arena storage, a collective (RCCL) path, the robust defenses on q1
 * inputs other than Krum (its Gram matrix straight from the bits is fedagg_sign_gram.h's), and per-client
 * vote weights (every client has one vote).
 */
#ifndef FEDAGG_SIGN_H
#define FEDAGG_SIGN_H

#include "fedagg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FA_Q1_BLOCK_MIN 32
#define FA_Q1_BLOCK_MAX 1024
#define FA_Q1_VOTE_MAX_K 4095

/* How the kernels split the work (what a test needs to reach every path; no argument depends on them):
 * elements per workgroup of the quantizer and the sum, elements per workgroup of the vote, and the
 * number of clients whose loads the sum and the vote keep in flight together. */
#define FA_Q1_SUM_SLOT 8192
#define FA_Q1_VOTE_SLOT 32768
#define FA_Q1_GROUP 8

/*
 * Compress num_segments tensors of one dtype (F32, BF16 or F16) in ONE launch:
 *   d_in[s]     seg_numel[s] elements of `dtype`;
 *   d_bits[s]   ceil(seg_numel[s] / 32) 32-bit words (4-byte aligned);
 *   d_scale[s]  ceil(seg_numel[s] / block) float32 (4-byte aligned).
 * Outputs must not alias inputs.
 *
 * Contract (bit-exact): every element is widened exactly to float32; every op is rounded once (rnd),
 * nothing is fused.  Per block:
 *   non-finite  if any element is NaN or +-Inf: scale = the quiet NaN 0x7fc00000 and every bit of the
 *               block is 0, so the whole block decompresses to NaN (q8's rule, for q8's reason: a
 *               poisoned block stays visible);
 *   finite      bit = the sign bit of the element (so -0.0 sets it);
 *               scale = rnd(S / (float)count), count = the block's real elements (B, or fewer in a
 *               ragged last block), the division correctly rounded, and S the sum of |x| taken as THE
 *               BALANCED BINARY TREE OVER B LEAVES: the leaves are |x_j| in element order, +0 for the
 *               missing leaves of a ragged block; each level adds adjacent pairs; every add is rounded
 *               once.  (A sum of finite elements that overflows gives scale = +Inf; that is not the
 *               non-finite rule.)
 *
 * Checked before any HIP call, in this order: ctx; block; num_segments; seg_numel, d_in, d_bits,
 * d_scale; dtype (FA_ERR_DTYPE); per non-empty segment its pointers and alignment (d_in to its element
 * size, d_bits and d_scale to 4 bytes).  The others return FA_ERR_INVALID.  All segments empty is FA_OK
 * with nothing launched.
 */
int fa_quantize_q1(fa_ctx *ctx, int dtype, int32_t num_segments, const int64_t *seg_numel, int32_t block,
                   const void *const *d_in, void *const *d_bits, void *const *d_scale, void *hip_stream);

/*
 * Fused decompress-and-sum of k clients' q1 tensors, num_segments tensors in ONE launch:
 *   d_bits[s * k + i], d_scale[s * k + i]   client i's bits and scales for segment s (the table layout
 *                                           of fa_weighted_sum_q8);
 *   d_out[s]                                seg_numel[s] float32; must not alias an input.
 * mode is FA_MODE_MUL_W (coef[i] = w_i) or FA_MODE_SUM (coef ignored, may be NULL); any other mode
 * returns FA_ERR_DTYPE.  Any k >= 1.
 *
 * Contract (bit-exact): float32, clients IN ORDER, every op rounded once, nothing fused.
 *   per client i and block b:   MUL_W: c = rnd(scale_i[b] * (float)coef[i]);   SUM: c = scale_i[b]
 *   per element e:              t_i = bit_i[e] ? -c : c;  out = t_0;  out = rnd(out + t_i), i >= 1
 * A NaN scale gives a NaN element; which NaN is not specified.  Decompression is this entry with k = 1
 * and FA_MODE_SUM.
 *
 * Alignment: bits, scale and output pointers must be 4-byte aligned (else FA_ERR_INVALID).  Bits at
 * any 4-byte alignment give the same output bits; 16-byte aligned outputs take vector stores.
 *
 * Checked before any HIP call, in this order: ctx; block; k and num_segments; seg_numel, d_bits,
 * d_scale, d_out; coef (NULL only for FA_MODE_SUM); mode (FA_ERR_DTYPE); per non-empty segment its
 * pointers and alignment.  The others return FA_ERR_INVALID.  All segments empty is FA_OK with nothing
 * launched.
 */
int fa_weighted_sum_q1(fa_ctx *ctx, int mode, int32_t num_segments, const int64_t *seg_numel, int32_t k,
                       int32_t block, const void *const *d_bits, const void *const *d_scale,
                       const double *coef, void *const *d_out, void *hip_stream);

/*
 * Majority vote over k clients' sign bits, num_segments tensors in ONE launch.  It reads bits only:
 *   d_bits[s * k + i]   client i's bits for segment s (4-byte aligned);
 *   d_out[s]            seg_numel[s] float32 (4-byte aligned); must not alias an input.
 *
 * Contract (exact): neg[e] = the number of clients whose bit e is set, net = k - 2 * neg[e];
 *   out[e] = +(float)step  where net >=  threshold,
 *            -(float)step  where net <= -threshold,
 *            +0.0f         otherwise.
 * threshold = 1 is the paper's majority vote, with ties giving 0.
 *
 * Checked before any HIP call, in this order: ctx; k (1 .. FA_Q1_VOTE_MAX_K) and num_segments;
 * seg_numel, d_bits, d_out; threshold (1 .. k); per non-empty segment its pointers and alignment.
 * All return FA_ERR_INVALID.  All segments empty is FA_OK with nothing launched.
 */
int fa_sign_vote_q1(fa_ctx *ctx, int32_t num_segments, const int64_t *seg_numel, int32_t k,
                    const void *const *d_bits, int32_t threshold, double step, void *const *d_out,
                    void *hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* FEDAGG_SIGN_H */
