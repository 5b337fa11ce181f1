/*
 * fedagg_dp.h -- differential privacy on the device: a counter-based noise generator, the add of its
 * noise to a tensor, and the clipped (centered) weighted sum with the noise added in the same read.
 * Part of libfedagg.so's C ABI (FA_ABI_VERSION is fedagg.h's; these entries only add symbols).
 * Kernels: fedml_amd/csrc/noise.hip.  Host layers: fedml_amd/dp.py, fedml_amd/core/dp/.
 *
 * THE NOISE CONTRACT.  The noise of an element depends only on (seed, round, segment id, element
 * index e within its segment) -- not on k, the dtype, the flat or tiled layout, the alignment, or on
 * how segments are grouped into calls.
 *
 * Words: Philox4x32-10 (Salmon, Moraes, Dror, Shaw, "Parallel Random Numbers: As Easy as 1, 2, 3",
 * SC 2011): multipliers 0xD2511F53, 0xCD9E8D57, Weyl constants 0x9E3779B9, 0xBB67AE85,
 *   key     = (lo32(seed), hi32(seed))
 *   counter = (lo32(b), hi32(b), seg_id, round)  with b = e >> 2, the block of element e,
 * and element e takes word w = block[e & 3].  Exact.
 *
 * Uniform: u = ((w >> 9) + 0.5f) * 2^-23: exact in float32, 0 < u < 1 (23 bits: 2m + 1 fits 24).
 *
 * FA_NOISE_GAUSSIAN (Box-Muller, float32): elements 4b, 4b+1 from (u0, u1) and 4b+2, 4b+3 from
 * (u2, u3):  r = sqrtf(-2 logf(ua));  z = r cospi(2 ub),  r sinpi(2 ub)  (2 ub is exact).
 * |z| <= sqrt(2 ln 2^24) < 5.77.
 * FA_NOISE_LAPLACE: element 4b+j from u_j:  v = u - 0.5 (exact, never 0);
 * z = -sgn(v) logf(1 - 2|v|) (the argument is exact and >= 2^-23).  |z| <= ln 2^23 < 15.95.
 *
 * z is a float32 and is NOT pinned to the bit: it is what the device's logf (<= 1 ulp), sqrtf
 * (correctly rounded) and sincospif (<= 2 ulp) give.  Against a float64 evaluation from the same
 * words, with h = 2^-24 (the unit roundoff: one rounding is <= h relative, 1 ulp <= 2h relative):
 *   Gaussian: L = -2 logf(ua) has relative error <= 2h (the factor 2 is exact); the square root
 *     halves it (h) and rounds once (h): r within 2h relative, r < 5.77; the cosine or sine c has
 *     absolute error <= 2 ulp <= 2h (|c| <= 1, an ulp below 1 is h); the product rounds once (h).  So
 *     |z - z64| <= r (2h |c| + 2h) + h |z| <= 5.77 * 5 * 2^-24 = 1.72e-6 to first order; the stated
 *     bound leaves room for the second-order terms.
 *   Laplace: one logf of an exact argument, |z| < 16, an ulp there is 2^-20 = 9.6e-7.
 * FA_NOISE_Z_ABS_ERR bounds both.  (tests/test_gpu_dp_noise.py; the measured maximum: DESIGN.md.)
 *
 * Applying it.  A and rnd as in fedagg_robust.h (A = float32 for F32, BF16, F16, float64 for F64; rnd
 * rounds once to the storage type); nothing is fused:
 *   t = rnd((A)scale * (A)z);   out = rnd(y + t)
 * scale == 0: no noise is generated and out = y bit for bit (-0 and NaN payloads included).  scale
 * must be finite and >= 0 (else FA_ERR_INVALID).
 *
 * Limits, stated plainly: the tails are truncated (5.77 sigma; 15.95 b); float32 noise carries no
 * protection against floating-point attacks on its low bits (Mironov 2012); in 16-bit storage noise
 * below half an ulp of y vanishes in rnd(y + t); there is no privacy accountant.
 */
#ifndef FEDAGG_DP_H
#define FEDAGG_DP_H

#include "fedagg.h"

#ifdef __cplusplus
extern "C" {
#endif

enum fa_noise_mech { FA_NOISE_GAUSSIAN = 0, FA_NOISE_LAPLACE = 1 };

/* |z - z64| for every element, both mechanisms (derivation above). */
#define FA_NOISE_Z_ABS_ERR 2.4e-6

/*
 * The raw words of blocks first_block .. first_block + nblocks - 1 of (seed, round, seg_id): 4 uint32
 * per block to d_out_u32 (device, 16-byte aligned), through the device function every kernel below
 * calls.  For exact tests of the generator, past 2^32 blocks too.
 * Checked before any HIP call, in this order: ctx; nblocks >= 0 and first_block + nblocks <= 2^64;
 * d_out_u32 non-NULL and 16-byte aligned (when nblocks > 0).  nblocks == 0: nothing is done.
 */
int fa_noise_words(fa_ctx *ctx, uint64_t seed, uint32_t round, uint32_t seg_id, uint64_t first_block,
                   int64_t nblocks, void *d_out_u32, void *hip_stream);

/*
 * out[s][e] = rnd(x + t) with x = d_in[s][e] and t the noise of (seed, round, seg_id[s], e); d_in ==
 * NULL: x = +0, so out = t.  d_out[s] may be d_in[s] (in place); no other overlap.  Flat contiguous
 * segments of `dtype` (F32, BF16, F16, F64; I64: FA_ERR_DTYPE); empty segments are skipped.  One
 * launch, asynchronous on the caller's stream; the host tables are staged by the library.
 * scale == 0: out = x bit for bit (a device copy; nothing when in place).
 * Checked before any HIP call, in this order: ctx; num_segments, seg_numel, d_out; mech; scale;
 * seg_id; dtype; per non-empty segment its output and input pointers.
 */
int fa_add_noise(fa_ctx *ctx, int dtype, int mech, double scale, uint64_t seed, uint32_t round,
                 int32_t num_segments, const int64_t *seg_numel, const uint32_t *seg_id, const void *const *d_in,
                 void *const *d_out, void *hip_stream);

/*
 * The clipped sum of DP-FedAvg (McMahan, Ramage, Talwar, Zhang 2018) with the noise added in the same
 * read: y is exactly fa_sign_vote_sum's out at threshold 0 for the same inputs, center and
 * coefficients (fedagg_robust.h) -- with a center rnd(c + sum_i rnd(rnd(x_i - c) (A)coef_i)) in client
 * order, without one the FA_MODE_MUL_W sum -- and out[s][e] = rnd(y + t), t as in fa_add_noise.  So
 * the result equals fa_add_noise applied to fa_sign_vote_sum's out, bit for bit -- except that where
 * NaNs of different sign or payload meet in one add of the sum, which of them the NaN result carries
 * is the implementation's (IEEE 754 6.2.3); it is a NaN in both.  d_out[s] may be the
 * very pointer d_center[s].  Pointer layout, dtypes, segment rules and the tiled addressing:
 * fa_sign_vote_sum's.  Any k >= 1.  No statistics, no scratch.
 * Checked before any HIP call, in this order: ctx; (tiled) tile_stride > 0; k, num_segments, seg_numel,
 * d_in, d_out; coef; mech; scale; seg_id; dtype (I64: FA_ERR_DTYPE); (tiled) tile_stride a multiple of
 * FA_TILE_BYTES; per non-empty segment its center (when d_center is given), output and input pointers.
 */
int fa_centered_sum_noise(fa_ctx *ctx, int dtype, int32_t num_segments, const int64_t *seg_numel, int32_t k,
                          const void *const *d_in, const void *const *d_center, const double *coef, int mech,
                          double scale, uint64_t seed, uint32_t round, const uint32_t *seg_id, void *const *d_out,
                          void *hip_stream);
int fa_centered_sum_noise_tiled(fa_ctx *ctx, int dtype, int32_t num_segments, const int64_t *seg_numel, int32_t k,
                                const void *const *d_in, int64_t tile_stride, const void *const *d_center,
                                const double *coef, int mech, double scale, uint64_t seed, uint32_t round,
                                const uint32_t *seg_id, void *const *d_out, void *hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* FEDAGG_DP_H */
