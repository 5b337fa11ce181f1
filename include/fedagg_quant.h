/*
 * fedagg_quant.h -- block-quantized int8 ("q8") client updates: a device quantizer and the fused
 * dequantize-and-sum of libfedagg.so (fedml_amd/csrc/quant.hip).  This header is the specification.
 *
 * Why: the link between client and server is the scarce resource of federated learning, and the usual
 * answer is 8-bit block quantization (symmetric int8, one scale per block).  The reference
 * (liuliuliu0605/FedML) has no such path; without these entries a caller dequantizes every client to
 * float32 on the device (K * P * 4 bytes written and read back) before fa_weighted_sum_multi accepts
 * it.  The fused sum reads 1 + 4/B bytes per client element instead of 4.  fa_finite_quantize
 * (fedagg_finite.h) is SecAgg's embedding into a prime field and is a different thing.
 *
 * Format "q8", per segment (one tensor flattened to n elements):
 *   block size B   a power of two, 16 <= B <= 1024, shared by every segment and client of a call;
 *   blocks         start at the segment's first element; the last block may be ragged;
 *   data           q: n int8 values;  scale: ceil(n / B) float32 values;
 *   meaning        element e has the value (float)q[e] * scale[e / B].
 *
 * Memory, asynchrony and errors: the rules of fedagg.h (device pointers owned by the caller, host
 * tables staged by the library, asynchronous on hip_stream, a negative fa_status and fa_last_error on
 * failure, never an abort).
 *
 * Out of scope: stochastic rounding (QSGD proper) and error feedback.  The quantizer rounds to
 * nearest, deterministically; a client that wants either applies it before this format.
 */
#ifndef FEDAGG_QUANT_H
#define FEDAGG_QUANT_H

#include "fedagg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FA_Q8_BLOCK_MIN 16
#define FA_Q8_BLOCK_MAX 1024

/*
 * Quantize num_segments tensors of one dtype (F32, BF16 or F16) in ONE launch:
 *   d_in[s]     seg_numel[s] elements of `dtype`;
 *   d_q[s]      seg_numel[s] int8 (any alignment);
 *   d_scale[s]  ceil(seg_numel[s] / block) float32 (4-byte aligned).
 * Outputs must not alias inputs.
 *
 * Contract (bit-exact): every element is widened exactly to float32; every op is rounded once (rnd),
 * nothing is fused.  Per block:
 *   non-finite  if any element is NaN or +-Inf: scale = the quiet NaN 0x7fc00000 and every q of the
 *               block is 0, so the whole block dequantizes to NaN.  This is deliberate: a poisoned
 *               block stays visible instead of being clamped into a plausible value.
 *   finite      amax = max |x|;  scale = rnd(amax / 127.0f);
 *               scale == 0: every q is 0;
 *               else q = clamp((int)rint(rnd(x / scale)), -127, 127): the division is correctly
 *               rounded, rint rounds ties to even.
 * The clamp is part of the contract: with a subnormal scale the quotient can exceed 127 (amax =
 * 190 * 2^-149 gives scale = 2^-149 and a quotient of 190).  -128 is never produced.
 *
 * Checked before any HIP call, in this order: ctx; block; num_segments; seg_numel, d_in, d_q,
 * d_scale; dtype (FA_ERR_DTYPE); per non-empty segment its pointers and alignment (d_in to its
 * element size, d_scale to 4 bytes).  The others return FA_ERR_INVALID.  All segments empty is FA_OK
 * with nothing launched.
 */
int fa_quantize_q8(fa_ctx *ctx, int dtype, int32_t num_segments, const int64_t *seg_numel, int32_t block,
                   const void *const *d_in, void *const *d_q, void *const *d_scale, void *hip_stream);

/*
 * Fused dequantize-and-sum of k clients' q8 tensors, num_segments tensors in ONE launch:
 *   d_q[s * k + i], d_scale[s * k + i]   client i's data and scales for segment s (the table layout
 *                                        of fa_weighted_sum_multi);
 *   d_out[s]                             seg_numel[s] float32; must not alias an input.
 * mode is FA_MODE_MUL_W (coef[i] = w_i) or FA_MODE_SUM (coef ignored, may be NULL);
 * FA_MODE_MUL_N_DIV_N returns FA_ERR_DTYPE.  Any k >= 1.
 *
 * Contract (bit-exact): float32, clients IN ORDER, every op rounded once, nothing fused.
 *   per client i and block b:   MUL_W: c = rnd(scale_i[b] * (float)coef[i]);   SUM: c = scale_i[b]
 *   per element e:              t_i = rnd((float)q_i[e] * c);  out = t_0;  out = rnd(out + t_i), i >= 1
 * The coefficient is folded into the block's scale ONCE PER BLOCK, not once per element.  That is this
 * engine's contract (no reference exists for it), chosen so that the per-element work is one
 * conversion, one multiply and one add; it differs in the last bit from rnd(rnd(q * scale) * w).
 * Dequantization is this entry with k = 1 and FA_MODE_SUM: out = rnd((float)q * scale).
 *
 * Alignment: q pointers may have any alignment; a segment whose q pointers are all 16-byte aligned
 * takes 16-byte loads, any other takes byte loads, and both give the same bits.  scale pointers and
 * outputs must be 4-byte aligned (else FA_ERR_INVALID); 16-byte aligned outputs take vector stores.
 *
 * Checked before any HIP call, in this order: ctx; block; k and num_segments; seg_numel, d_q, d_scale,
 * d_out; coef (NULL only for FA_MODE_SUM); mode (FA_ERR_DTYPE); per non-empty segment its pointers and
 * alignment.  The others return FA_ERR_INVALID.  All segments empty is FA_OK with nothing launched.
 */
int fa_weighted_sum_q8(fa_ctx *ctx, int mode, int32_t num_segments, const int64_t *seg_numel, int32_t k,
                       int32_t block, const void *const *d_q, const void *const *d_scale,
                       const double *coef, void *const *d_out, void *hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* FEDAGG_QUANT_H */
