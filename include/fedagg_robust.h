/*
 * fedagg_robust.h -- C ABI of the robust-aggregation kernels (libfedagg.so), same context,
 * memory, stream and error conventions as fedagg.h.  Entries and the reference code each replaces
 * (paths relative to liuliuliu0605/FedML python/fedml/):
 *
 *   fa_coord_median     core/security/defense/coordinate_wise_median_defense.py:26-31
 *                       torch.median(torch.cat(client vectors, -1), dim=-1).values
 *   fa_coord_median_tiled  the same over tile-interleaved arena rows
 *   fa_coord_trimmed_mean, fa_coord_trimmed_mean_tiled  no reference code: the per-coordinate trimmed
 *                       mean of Yin et al. 2018 (the reference's "trimmed mean" trims whole clients)
 *   fa_coord_mean_around_median, fa_coord_mean_around_median_tiled  no reference code here: the second
 *                       stage of Bulyan (El Mhamdi et al. 2018), the mean of the values nearest the median
 *   fa_weighted_sum_sqdist, fa_weighted_sum_sqdist_tiled  no reference code here: one smoothed Weiszfeld
 *                       pass of the geometric median (RFA), the weighted sum fused with every
 *                       client's squared distance to it
 *   fa_centered_sum_sqdist, fa_centered_sum_sqdist_tiled  no reference code here: one pass of centered
 *                       clipping (Karimireddy, He, Jaggi 2021) around a center the caller supplies,
 *                       fused with every client's squared distance to the result; or the distances alone
 *   fa_sign_vote_sum, fa_sign_vote_sum_tiled  no reference code here (the reference lists it as
 *                       robust_learning_rate): the robust learning rate of Ozdayi, Kantarcioglu, Gel 2021,
 *                       the weighted sum fused with a per-coordinate vote of the clients' signs that
 *                       negates the sum where too few agree
 *   fa_pairwise_dot, fa_pairwise_dot_tiled  core/security/defense/foolsgold_defense.py (the running sum of
 *                       every client's updates and the pairwise cosine similarity of those sums): the
 *                       update added into its history in place, fused with the Gram matrix of the
 *                       stored histories; served as "fools_gold", defined by the contract below
 *   fa_pairwise_sqdist  core/security/defense/krum_defense.py:52-66 (_compute_krum_score's
 *                       compute_euclidean_distance(v_i, v_j) ** 2 for every pair)
 *   fa_pairwise_sqdist_rt  the same for bfloat16 / float16 models (differences in the model dtype)
 *   fa_pairwise_sqdist_gram  the same for float32 models in the Gram form (matrix cores, kappa-guarded)
 *   fa_pairwise_sqdist_gram_limit  the kappa limit that guard applies to an input (its error model)
 *
 * Contract (bit-exact; pinned by tests/golden/g16_*): for every element e, out[e] is the input
 * element (bit pattern) that ATen's median selects: the first NaN in client order if any client
 * holds a NaN there; otherwise the element of rank (k-1)/2 when the k values are ordered by
 * (value, client index), -0.0 == +0.0.  dtype: F32, BF16, F16, F64.
 *
 * fa_pairwise_sqdist is floating-point work whose summation order differs from the reference's
 * float32 `norm()` (itself order-dependent): D[i][j] = sum_e (x_i[e] - x_j[e])^2 with float32
 * differences, float32 sums over <= 64 coordinates, float64 above; relative error <= 1e-6 vs the
 * exact sum (tests/test_gpu_robust.py).  The Krum selection built on it is checked bit-for-bit
 * against the reference (tests/golden/g18_*).
 */
#ifndef FEDAGG_ROBUST_H
#define FEDAGG_ROBUST_H

#include <stddef.h>

#include "fedagg.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * A whole (vectorized) state_dict in one launch: d_in[s * k + i] = client i's tensor of segment s
 * (seg_numel[s] elements of `dtype`), d_out[s] the median tensor of segment s.
 */
int fa_coord_median(fa_ctx *ctx, int dtype, int32_t num_segments, const int64_t *seg_numel, int32_t k,
                    const void *const *d_in, void *const *d_out, void *hip_stream);
/*
 * The same over TILE-INTERLEAVED client rows (fedml_amd/arena.py ClientArena(tiled=True), the
 * layout fa_weighted_sum_tiled reads): element e of client i's segment s is at
 * d_in[s * k + i] + (e / E) * tile_stride + (e % E) * sizeof(dtype), E = FA_TILE_BYTES / sizeof(dtype);
 * every d_in pointer is the start of a tile; tile_stride a positive multiple of FA_TILE_BYTES.
 * Same results, bit for bit, as fa_coord_median over the logical rows.
 */
int fa_coord_median_tiled(fa_ctx *ctx, int dtype, int32_t num_segments, const int64_t *seg_numel, int32_t k,
                          const void *const *d_in, int64_t tile_stride, void *const *d_out, void *hip_stream);

/*
 * Coordinate-wise trimmed mean (Yin et al. 2018) with trim count `trim` = b, 0 <= b and 2 * b < k
 * (else FA_ERR_INVALID).  Everything else -- pointer layout d_in[s * k + i], dtypes (F32, BF16, F16,
 * F64), segment rules, asynchrony on the caller's stream, validation before any HIP call, error
 * codes -- is fa_coord_median's.  Contract (bit-exact; tests/test_gpu_trimmed_mean.py), for every
 * element e:
 *   1. the k values of the column are ordered ascending: -0.0 below +0.0, and NaN (any sign or
 *      payload) above +inf, as torch.sort / numpy.sort place it; the order of equal values is
 *      immaterial;
 *   2. acc = (double)s[b]; acc += (double)s[r] for r = b+1 .. k-1-b, in that order (the sum starts
 *      FROM the first kept value, not from +0.0: a column of -0.0 yields -0.0);
 *   3. q = acc / (double)(k - 2 * b);
 *   4. out[e] = q (F64), (float)q (F32), (dtype)(float)q (BF16, F16: float64 -> float32 -> 16 bits),
 *      every conversion round-to-nearest-even.
 * So up to b NaNs per column are trimmed away, a NaN inside the kept window gives NaN (bits
 * unspecified), as does a kept window holding both +inf and -inf; b = 0 is the unweighted mean in
 * sorted order, and odd k with b = (k-1)/2 the median's value.  The order of the sum is part of the
 * contract because a float64 sum of float32 values is not always exact.  Sample counts play no part.
 */
int fa_coord_trimmed_mean(fa_ctx *ctx, int dtype, int32_t num_segments, const int64_t *seg_numel, int32_t k,
                          int32_t trim, const void *const *d_in, void *const *d_out, void *hip_stream);
/* The same over tile-interleaved client rows (addressing and tile rules of fa_coord_median_tiled). */
int fa_coord_trimmed_mean_tiled(fa_ctx *ctx, int dtype, int32_t num_segments, const int64_t *seg_numel,
                                int32_t k, int32_t trim, const void *const *d_in, int64_t tile_stride,
                                void *const *d_out, void *hip_stream);

/*
 * Coordinate-wise mean around the median: per coordinate the mean of the `keep` values nearest to the
 * column's median, 1 <= keep <= k (else FA_ERR_INVALID) -- the second stage of Bulyan (El Mhamdi,
 * Guerraoui, Rouault 2018, "The Hidden Vulnerability of Distributed Learning in Byzantium") over the
 * clients its first stage selected (fedml_amd/bulyan.py), keep = theta - 2f.  Pointer layout
 * d_in[s * k + i], dtypes (F32, BF16, F16, F64), segment rules, asynchrony on the caller's stream,
 * validation before any HIP call (the context first), error codes: fa_coord_trimmed_mean's.  Contract
 * (bit-exact; tests/test_gpu_mean_around_median.py), for every element e:
 *   1. s = the k values of the column ordered ascending as in fa_coord_trimmed_mean: -0.0 below +0.0,
 *      NaN (any sign or payload) above +inf, the order of equal values immaterial;
 *   2. h = (k - 1) / 2 (integer division), m = s[h], the lower median; m NaN: the result is NaN;
 *   3. dist(v) = 0 if v == m (an IEEE comparison: equal infinities and -0.0 / +0.0 are at distance 0),
 *      +inf if v is NaN, otherwise |(double)v - (double)m|, one float64 subtraction (F64: it may
 *      overflow to +inf);
 *   4. lomin = max(0, h - keep + 1), lomax = min(h, k - keep),
 *      lo = lomin + #{ r in [lomin, lomax) : dist(s[r]) > dist(s[r + keep]) }:
 *      the window of `keep` consecutive ranks that greedy growth from rank h reaches when it takes the
 *      nearer outside neighbour and the lower one on a tie.  The restriction of r to [lomin, lomax) is
 *      part of the contract: every finite distance to an infinite median saturates to +inf, and
 *      [1, 2, 3, 4, inf, inf, inf, inf, inf] with keep = 2 must give {inf, inf}, not {3, 4};
 *   5. acc = (double)s[lo]; acc += (double)s[r] for r = lo+1 .. lo+keep-1, in that order;
 *      q = acc / (double)keep; out[e] = q stored as fa_coord_trimmed_mean stores it (F64 as is, F32 one
 *      rounding, BF16 / F16 float64 -> float32 -> 16 bits, round-to-nearest-even).
 * A NaN inside the window gives NaN (bits unspecified), as does a window holding both +inf and -inf.
 * keep = k is fa_coord_trimmed_mean with trim 0, bit for bit, and keep = 1 on odd k is
 * fa_coord_trimmed_mean with trim (k - 1) / 2.  Sample counts play no part.
 */
int fa_coord_mean_around_median(fa_ctx *ctx, int dtype, int32_t num_segments, const int64_t *seg_numel,
                                int32_t k, int32_t keep, const void *const *d_in, void *const *d_out,
                                void *hip_stream);
/* The same over tile-interleaved client rows (addressing and tile rules of fa_coord_median_tiled). */
int fa_coord_mean_around_median_tiled(fa_ctx *ctx, int dtype, int32_t num_segments, const int64_t *seg_numel,
                                      int32_t k, int32_t keep, const void *const *d_in, int64_t tile_stride,
                                      void *const *d_out, void *hip_stream);

/*
 * One pass of the smoothed Weiszfeld iteration for the geometric median (Pillutla, Kakade, Harchaoui,
 * "Robust Aggregation for Federated Learning"): the weighted sum of the k clients AND every client's
 * squared distance to it, in one read of the inputs from HBM.  Pointer layout d_in[s * k + i], dtypes
 * (F32, BF16, F16, F64; I64: FA_ERR_DTYPE), segment rules, host tables staged by the library,
 * validation before any HIP call (the context first), asynchrony on the caller's stream: fa_coord_median's.
 * Any k >= 1.  coef: k host doubles (required).  Contract, for every element e of every segment:
 *   out[e] = fa_weighted_sum's FA_MODE_MUL_W result for the same inputs and coef, bit for bit (NaNs
 *            included): clients in order, t_i = op(x_i * c_i), out = t_0, out = op(out + t_i), op
 *            rounding once to the storage type, nothing fused, coef cast to the op type;
 *   d_stats = 2 k float64 on the device, all written by the call:
 *     d_stats[i]     = d2_i = sum_e (x_i[e] - out[e])^2 over all segments, against the STORED
 *                      (rounded) out[e];
 *     d_stats[k + i] = ss_i = sum_e x_i[e]^2.
 * The differences are formed in float32 from exactly widened inputs (float64 for F64), squared and
 * summed in float64; the order of the sums is the implementation's, and fixed: the same call gives
 * the same 2 k bit patterns every time (no floating-point atomics).  All inputs finite: each sum is
 * within 1e-6 relative of its exact value (tests/test_gpu_geometric_median.py; one float32 rounding
 * of a difference costs at most 2^-23 on its square, the terms are non-negative), and an exact value
 * of 0 gives exactly 0 (k = 1, coef 1: out = x, d2 = 0).  ss_i is non-finite exactly when client i
 * holds a NaN or +-Inf (F64: also when a square overflows); d2_i is non-finite when any of its terms is.
 * d_scratch: device buffer of at least fa_weighted_sum_sqdist_scratch_bytes(...) bytes (per-workgroup
 * partial sums; caller-owned, reusable; the size serves every dtype; 0 for invalid arguments).
 */
int fa_weighted_sum_sqdist(fa_ctx *ctx, int dtype, int32_t num_segments, const int64_t *seg_numel, int32_t k,
                           const void *const *d_in, const double *coef, void *const *d_out, void *d_stats,
                           void *d_scratch, size_t scratch_bytes, void *hip_stream);
/* The same over tile-interleaved client rows (addressing and tile rules of fa_coord_median_tiled):
 * out bit for bit fa_weighted_sum_sqdist's over the logical rows, the sums within the same bound. */
int fa_weighted_sum_sqdist_tiled(fa_ctx *ctx, int dtype, int32_t num_segments, const int64_t *seg_numel, int32_t k,
                                 const void *const *d_in, int64_t tile_stride, const double *coef,
                                 void *const *d_out, void *d_stats, void *d_scratch, size_t scratch_bytes,
                                 void *hip_stream);
size_t fa_weighted_sum_sqdist_scratch_bytes(int32_t num_segments, const int64_t *seg_numel, int32_t k);

/*
 * One pass of centered clipping (Karimireddy, He, Jaggi 2021, "Learning from History for Byzantine
 * Robust Optimization"): the update v' = v + sum_i s_i (x_i - v) of a center v the caller supplies AND
 * every client's squared distance to v', in one read of the inputs from HBM; with coef NULL, only the
 * distances to v.  d_center[s]: the center of segment s, a flat contiguous tensor of seg_numel[s]
 * elements of `dtype` (flat in the tiled entry too, like d_out[s]).  Everything else -- pointer layout,
 * dtypes, segment rules, staging, asynchrony, error codes, d_scratch and its size
 * (fa_weighted_sum_sqdist_scratch_bytes) -- is fa_weighted_sum_sqdist's.
 *
 * coef non-NULL (k host doubles, the scales s_i): bit-exact contract.  A = float32 for F32, BF16, F16,
 * float64 for F64; rnd rounds once to the storage type; nothing is fused; coef is cast to A.  For
 * every element e, with c = center[e]:
 *   u_i = rnd(x_i[e] - c);  t_i = rnd(u_i * (A)coef_i)
 *   acc = t_0;  acc = rnd(acc + t_i) for i = 1 .. k-1 in client order
 *   out[e] = rnd(c + acc)
 *   d_stats[i] = sum_e (x_i[e] - out[e])^2 against the STORED out;  d_stats[k + i] = sum_e x_i[e]^2
 * with fa_weighted_sum_sqdist's arithmetic, fixed order and 1e-6 bound for the sums (an exact 0 gives
 * 0; tests/test_gpu_centered_clipping.py).  d_out[s] may be the very pointer d_center[s] (an in-place
 * update: each element is read and then written by the one lane that owns it); no other overlap of
 * d_out with d_center or d_in is allowed.
 *
 * coef NULL (distance-only): d_out is ignored and may be NULL; nothing but d_stats is written:
 *   d_stats[i] = sum_e (x_i[e] - center[e])^2;  d_stats[k + i] = sum_e x_i[e]^2.
 *
 * All segments empty: d_stats is zeroed.  Checked before any HIP call, in this order: ctx; (tiled)
 * tile_stride > 0; k, num_segments, seg_numel, d_in (and d_out when coef is given); d_center; d_stats;
 * dtype (I64: FA_ERR_DTYPE); (tiled) tile_stride a multiple of FA_TILE_BYTES; per non-empty segment
 * its center, output and input pointers; the scratch.
 */
int fa_centered_sum_sqdist(fa_ctx *ctx, int dtype, int32_t num_segments, const int64_t *seg_numel, int32_t k,
                           const void *const *d_in, const void *const *d_center, const double *coef,
                           void *const *d_out, void *d_stats, void *d_scratch, size_t scratch_bytes,
                           void *hip_stream);
/* The same over tile-interleaved client rows (addressing and tile rules of fa_coord_median_tiled):
 * out bit for bit fa_centered_sum_sqdist's over the logical rows, the sums within the same bound. */
int fa_centered_sum_sqdist_tiled(fa_ctx *ctx, int dtype, int32_t num_segments, const int64_t *seg_numel, int32_t k,
                                 const void *const *d_in, int64_t tile_stride, const void *const *d_center,
                                 const double *coef, void *const *d_out, void *d_stats, void *d_scratch,
                                 size_t scratch_bytes, void *hip_stream);

/*
 * The robust learning rate (Ozdayi, Kantarcioglu, Gel 2021, "Defending against Backdoors in Federated
 * Learning with Robust Learning Rate"): the weighted sum of the k clients' updates with, per
 * coordinate, a vote of the updates' signs -- where fewer than `threshold` net votes agree, the
 * server's learning rate is negated for that coordinate -- in one read of the inputs from HBM.
 * d_center non-NULL: the updates are x_i - center (d_center[s]: the center of segment s, a flat
 * contiguous tensor of seg_numel[s] elements of `dtype`, flat in the tiled entry too, like d_out[s]) and
 * the result is center + the signed sum; d_center NULL: the inputs are the updates themselves.
 * Pointer layout d_in[s * k + i], dtypes (F32, BF16, F16, F64; I64: FA_ERR_DTYPE), segment rules, host
 * tables staged by the library, asynchrony on the caller's stream, the tiled addressing:
 * fa_centered_sum_sqdist's.  Any k >= 1.  coef: k host doubles (required).  0 <= threshold <= k (else
 * FA_ERR_INVALID).
 *
 * Contract, bit-exact (tests/test_gpu_robust_lr.py).  A = float32 for F32, BF16, F16, float64 for
 * F64; rnd rounds once to the storage type; nothing is fused; coef is cast to A.  For every element e
 * of every segment:
 *   u_i = rnd(x_i[e] - c) with c = center[e];  without a center u_i = x_i[e]
 *   s_i = +1 if u_i > 0, -1 if u_i < 0, else 0 (+-0 and NaN vote 0, +-Inf vote +-1)
 *   net = sum_i s_i, an exact integer (every client has one vote; coef plays no part in it)
 *   t_i = rnd(u_i * (A)coef_i);  acc = t_0;  acc = rnd(acc + t_i) for i = 1 .. k-1 in client order
 *   if |net| < threshold: acc = -acc (the sign bit alone: exact)
 *   out[e] = rnd(c + acc);  without a center out[e] = acc
 * So with threshold 0 and a center, out is fa_centered_sum_sqdist's out for the same inputs and
 * coefficients, and with threshold 0 and no center it is fa_weighted_sum's FA_MODE_MUL_W result, both
 * bit for bit, NaNs included.  d_out[s] may be the very pointer d_center[s] (in place: each element is
 * read and then written by the one lane that owns it); no other overlap of d_out with d_center or d_in
 * is allowed.
 *
 * d_flipped: NULL, or one int64 on the device, to which the call writes the number of elements, over
 * all segments, with |net| < threshold (an integer: one value, whatever the order of the adds; 0 when
 * all segments are empty).
 *
 * Checked before any HIP call, in this order: ctx; (tiled) tile_stride > 0; k, num_segments, seg_numel,
 * d_in, d_out; coef; threshold; dtype (I64: FA_ERR_DTYPE); (tiled) tile_stride a multiple of
 * FA_TILE_BYTES; per non-empty segment its center (when d_center is given), output and input pointers.
 */
int fa_sign_vote_sum(fa_ctx *ctx, int dtype, int32_t num_segments, const int64_t *seg_numel, int32_t k,
                     const void *const *d_in, const void *const *d_center, const double *coef, int32_t threshold,
                     void *const *d_out, void *d_flipped, void *hip_stream);
/* The same over tile-interleaved client rows (addressing and tile rules of fa_coord_median_tiled):
 * out and the count bit for bit fa_sign_vote_sum's over the logical rows. */
int fa_sign_vote_sum_tiled(fa_ctx *ctx, int dtype, int32_t num_segments, const int64_t *seg_numel, int32_t k,
                           const void *const *d_in, int64_t tile_stride, const void *const *d_center,
                           const double *coef, int32_t threshold, void *const *d_out, void *d_flipped,
                           void *hip_stream);

/*
 * FoolsGold's device work (Fung, Yoon, Beschastnikh 2018, "Mitigating Sybils in Federated Learning
 * Poisoning"): every client's update is added into its running history, in place, and the Gram matrix
 * of the stored histories is formed in the same read.  d_in[s * k + i]: client i's tensor of segment s.
 * d_center: NULL, or d_center[s] the center of segment s, a flat contiguous tensor of seg_numel[s]
 * elements of `dtype` (flat in the tiled entry too).  d_hist: NULL, or d_hist[s * k + i] client i's
 * history of segment s, flat and contiguous, of the same dtype (flat in the tiled entry too), updated in
 * place.  d_gram: k x k float64 on the device.  d_scratch: a device buffer of at least
 * fa_pairwise_dot_scratch_bytes(...) bytes (per-workgroup partial sums; caller-owned, reusable; one
 * size serves every dtype).  Dtypes (F32, BF16, F16, F64; I64: FA_ERR_DTYPE), segment rules, host
 * tables staged by the library, asynchrony on the caller's stream, the tiled addressing:
 * fa_sign_vote_sum's.  1 <= k <= 128 (else FA_ERR_INVALID).
 *
 * Contract (tests/test_gpu_pairwise_dot.py).  A = float32 for F32, BF16, F16, float64 for F64; rnd
 * rounds once to the storage type; nothing is fused in the bit-exact part.  For every element e of
 * every segment:
 *   u_i = x_i[e] without a center, otherwise u_i = rnd(x_i[e] - center[e])
 *   with a history: h_i[e] = rnd(h_i[e] + u_i), stored -- bit-exact, NaNs included (each element is read
 *     and then written by the one lane that owns it; a NaN that the rounding to BF16 / F16 produces is
 *     the device's quiet NaN (0x7fc0 for BF16), where a host conversion may write another payload)
 *     -- and y_i = the STORED h_i[e]
 *   without a history: y_i = u_i, and nothing but d_gram is written
 *   G[i][j] = sum_e y_i y_j over all segments, for all i, j: the diagonal and both triangles are
 *     written, G[i][j] and G[j][i] with the same bit pattern
 * Arithmetic of G: products and runs of at most 64 coordinates in float32 from exactly widened values
 * (one fused multiply-add per product inside a run), float64 sums across runs (float64 throughout for
 * F64) -- the scheme of fa_pairwise_sqdist.  The order is the implementation's and is fixed: no
 * floating-point atomics, the same call gives the same k^2 bit patterns every time.
 * Bound: with all y finite and no product below float32's normal range,
 *   |G[i][j] - exact| <= 65 * 2^-24 * sum_e |y_i y_j| <= 3.9e-6 * sqrt(exact_ii * exact_jj)
 * (one rounding per product plus at most 64 per run, then Cauchy-Schwarz), stated as
 * 4e-6 * sqrt(exact_ii * exact_jj): on the diagonal a relative bound.  F64: 1e-12 on the same scale.
 * A client whose y is all zeros gives an exactly-zero row and column.  G[i][i] is non-finite exactly
 * when y_i holds a NaN or +-Inf, or when a float32 product or run overflows; a non-finite client taints
 * only its own row and column.  All segments empty: d_gram is zeroed.  d_hist must not overlap d_in,
 * d_center or itself across clients.
 *
 * Checked before any HIP call, in this order: ctx; (tiled) tile_stride > 0; k, num_segments, seg_numel,
 * d_in; d_gram; dtype (I64: FA_ERR_DTYPE); (tiled) tile_stride a multiple of FA_TILE_BYTES; per
 * non-empty segment its center (when d_center is given), history (when d_hist is given) and input
 * pointers; the scratch.
 */
int fa_pairwise_dot(fa_ctx *ctx, int dtype, int32_t num_segments, const int64_t *seg_numel, int32_t k,
                    const void *const *d_in, const void *const *d_center, void *const *d_hist,
                    void *d_gram, void *d_scratch, size_t scratch_bytes, void *hip_stream);
/* The same over tile-interleaved client rows (addressing and tile rules of fa_coord_median_tiled): the
 * histories bit for bit fa_pairwise_dot's over the logical rows, G within the same bound. */
int fa_pairwise_dot_tiled(fa_ctx *ctx, int dtype, int32_t num_segments, const int64_t *seg_numel, int32_t k,
                          const void *const *d_in, int64_t tile_stride, const void *const *d_center,
                          void *const *d_hist, void *d_gram, void *d_scratch, size_t scratch_bytes,
                          void *hip_stream);
size_t fa_pairwise_dot_scratch_bytes(int32_t num_segments, const int64_t *seg_numel, int32_t k);

/*
 * Pairwise squared Euclidean distances of k float32 client vectors (2 <= k <= 128), each given
 * as num_segments pieces (d_in[s * k + i], seg_numel[s] elements): d_dist = k x k float64 device
 * matrix (symmetric, zero diagonal).  d_scratch: device buffer of at least
 * fa_pairwise_sqdist_scratch_bytes(...) bytes (per-block partial sums; caller-owned, reusable).
 *
 * Contract of fa_pairwise_sqdist and fa_pairwise_sqdist_rt (tests/test_gpu_krum_exact.py, on inputs of
 * four or five chunks per workgroup, one segment and many, 16-byte aligned and not).  For every pair,
 *   D[i][j] = sum_e rnd(x_i[e] - x_j[e])^2 over all segments,
 * rnd the rounding to diff_dtype (none for F32).  Arithmetic: the difference, its rounding and the
 * square in float32, float32 sums over runs of at most 64 coordinates (one fused multiply-add per
 * coordinate inside a run), float64 sums across runs; float64 throughout for F64.  The order is the
 * implementation's and is fixed: no floating-point atomics, the same call gives the same k^2 bit
 * patterns every time; D[i][j] and D[j][i] carry the same bits and the diagonal is +0.0.
 * Exactness: where every difference (after rnd), every square and every run sum is representable in
 * float32 and the total in float64, D is the exact value, bit for bit -- e.g. integer inputs of
 * magnitude <= 15 at any length below 2^53 / 900, or the same times a power of two while the squares
 * stay inside float32's normal range.  Otherwise relative error <= 1e-6 against the exact sum.
 * Non-finite inputs: a client that holds a NaN or +-Inf taints only its own row and column; every
 * entry between two finite clients has the bits the same call gives with that value replaced by 0
 * (no other client's sums read it).  The tainted entries have
 * the class float64 arithmetic gives: an Inf against a finite value +Inf, an Inf against an equal Inf
 * at the same coordinate (Inf - Inf), and anything against a NaN, NaN.  The Gram form's guard hands
 * such inputs to these kernels (kappa_max = +inf).
 * Range: a square below float32's normal range may be lost (flushed or rounded as a subnormal), and a
 * float32 square or run sum that overflows gives +Inf in that entry -- stated, not tested.
 */
int fa_pairwise_sqdist(fa_ctx *ctx, int32_t num_segments, const int64_t *seg_numel, int32_t k,
                       const void *const *d_in, void *d_dist, void *d_scratch, size_t scratch_bytes,
                       void *hip_stream);
/*
 * As fa_pairwise_sqdist, with every difference x_i[e] - x_j[e] rounded to `diff_dtype` before it is
 * squared: FA_DTYPE_F32 (no rounding; = fa_pairwise_sqdist), FA_DTYPE_BF16 or FA_DTYPE_F16 (round
 * to nearest even, overflow to inf).  Replaces the same loop for bfloat16 / float16 models, where
 * the reference's vectorize_weight (core/security/common/utils.py:8-13) keeps the model's dtype and
 * `(v1 - v2)` (utils.py:24-27) rounds each difference to it; the inputs stay float32 (the clients'
 * values widened exactly).  The caller rounds sqrt(D) to the same dtype to reproduce the
 * reference's `.norm()` result (the norm of a bf16/f16 tensor is returned in that dtype).
 * FA_DTYPE_F64: float64 models -- the inputs are FLOAT64 vectors and every difference, square and
 * sum is computed in float64 (the reference's vectorize_weight keeps float64 and `(v1 - v2).norm()`
 * runs in it; krum_defense.py:50-66).
 */
int fa_pairwise_sqdist_rt(fa_ctx *ctx, int diff_dtype, int32_t num_segments, const int64_t *seg_numel, int32_t k,
                          const void *const *d_in, void *d_dist, void *d_scratch, size_t scratch_bytes,
                          void *hip_stream);
size_t fa_pairwise_sqdist_scratch_bytes(int32_t num_segments, const int64_t *seg_numel, int32_t k);
/*
 * fa_pairwise_sqdist for float32 vectors in the Gram form on the matrix cores (r05):
 * D_ij = A_i + A_j - 2 G_ij over y_i = x_i - c (c: the per-coordinate median of clients 0..4), G = Y Y^T
 * on the f32-input MFMA (k <= 32 with 16-byte aligned clients: v_mfma_f32_16x16x4_f32 over the three
 * upper 16x16 tiles, chunks streamed by LDS-DMA; otherwise v_mfma_f32_32x32x2_f32 over the upper
 * 32x32 tiles; k in (32, 128] with 16-byte aligned clients (FA_GRAM3=0: off): y split exactly into three bf16 parts on the
 * bf16 MFMA), float32 runs of n = 64-256 products summed in float64.
 * Same d_dist layout (k x k float64, symmetric, zero diagonal).  The form cancels: its relative error
 * is ~ 0.30 kappa_ij u n / sqrt(P) (one sigma, u = 2^-24, P = total coordinates), kappa_ij =
 * (A_i + A_j) / D_ij -- so it also writes kappa_max = max over pairs (one float64 at d_kappa_max; +inf
 * when some D_ij <= 0 or an input is not finite).  kappa_limit > 0: the direct kernels of
 * fa_pairwise_sqdist are queued behind it, guarded on the device -- they return at once when
 * kappa_max <= fa_pairwise_sqdist_gram_limit(..., kappa_limit) and otherwise recompute d_dist, so the
 * call stays asynchronous and every distance it returns is within 1e-6 relative of the exact value
 * (fedml_amd/engine.py passes 16); kappa_limit <= 0: the Gram result only, no guard.
 * d_scratch: fa_pairwise_sqdist_gram_scratch_bytes(...) bytes.
 */
int fa_pairwise_sqdist_gram(fa_ctx *ctx, int32_t num_segments, const int64_t *seg_numel, int32_t k,
                            const void *const *d_in, void *d_dist, void *d_kappa_max, double kappa_limit,
                            void *d_scratch, size_t scratch_bytes, void *hip_stream);
size_t fa_pairwise_sqdist_gram_scratch_bytes(int32_t num_segments, const int64_t *seg_numel, int32_t k);
/*
 * The kappa limit fa_pairwise_sqdist_gram's guard applies to this input: min(kappa_limit,
 * 1e-6 / (6 x 0.30 u n / sqrt(P) + b)) -- the largest kappa at which 6 sigma of the error model above
 * (plus, for the bf16x3 forms, a measured size-independent part b) stays <= 1e-6 relative (n, b of the
 * kernel the call would run; d_in only for its 16-byte alignment).  0 for
 * invalid arguments or kappa_limit <= 0.  Host only, no device work.
 */
double fa_pairwise_sqdist_gram_limit(int32_t num_segments, const int64_t *seg_numel, int32_t k,
                                     const void *const *d_in, double kappa_limit);

#ifdef __cplusplus
}
#endif

#endif /* FEDAGG_ROBUST_H */
