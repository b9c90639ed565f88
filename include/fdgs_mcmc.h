/* fdgs_mcmc.h -- densification as Markov chain Monte Carlo (Kheradmand et al., "3D Gaussian Splatting as Markov Chain Monte Carlo",
 * NeurIPS 2024): opacity-proportional sampling, relocation, the noise step and the two regularisers (csrc/mcmc.hip, libfdgs.so).
 *
 * A companion of fdgs.h with the same conventions: every function returns FDGS_OK or an error code whose text fdgs_last_error()
 * holds, device pointers are borrowed, `stream` is a hipStream_t, nothing synchronises the host.  FDGS_VERSION does not count the
 * entry points of this header.  Every result is a pure function of its inputs, bit for bit: integer weights, an integer scan,
 * integer atomics, counter-based random numbers, float64 sums in a fixed order, no float atomics.
 *
 * All parameters are RAW (as GaussianParams stores them): opacity is sigmoid(opacity_raw), a scale exp(scaling_raw).
 */
#ifndef FDGS_MCMC_H
#define FDGS_MCMC_H

#include "fdgs.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FDGS_MCMC_WEIGHT_BITS 24      /* a weight is the opacity in units of 2^-24 */
#define FDGS_MCMC_MAX_MULTIPLICITY 51 /* N = min(draws + 1, 51) */

/* ---- sampling weights ---------------------------------------------------------------------------------------------------------------
 * o = 1 / (1 + expf(-opacity_raw)) in float32.  A Gaussian is alive when o > min_opacity.  alive[i] (uint8) = 1 / 0,
 * wq[i] (uint32) = alive ? (uint32) rintf(o * 2^24) : 0, prefix[i] (uint64) = wq[0] + ... + wq[i]: exact.  The total is prefix[P - 1].
 * Three launches.  scratch: fdgs_mcmc_weights_scratch_bytes(P) bytes.
 * FDGS_ERR_INVALID_ARG: P < 1, a NULL pointer. */
size_t fdgs_mcmc_weights_scratch_bytes(int32_t P);
int fdgs_mcmc_weights(int32_t P, const float* opacity_raw, float min_opacity, uint8_t* alive, uint32_t* wq, uint64_t* prefix, void* scratch,
                      void* stream);

/* ---- draws --------------------------------------------------------------------------------------------------------------------------
 * Draw j: w = Philox4x32-10(counter = (j, stream_id, call & 0xffffffff, call >> 32), key = (seed & 0xffffffff, seed >> 32)),
 * r64 = (w0 << 32) | w1, u = (r64 * total) >> 64 with total = prefix[P - 1], so 0 <= u < total; source[j] (int32) = the smallest i with
 * prefix[i] > u, found by binary search (a row of weight 0 is never selected).  counts (int32 [P]) is cleared and then receives how
 * often each row was selected (integer atomics).  words (uint32 [n_draws, 4], optional) receives w.  total == 0: every source is -1.
 * FDGS_ERR_INVALID_ARG: P < 1, n_draws < 0, a NULL prefix / counts, n_draws > 0 with a NULL source. */
int fdgs_mcmc_draw(int32_t P, int32_t n_draws, const uint64_t* prefix, uint64_t seed, uint32_t stream_id, uint64_t call, int32_t* source,
                   int32_t* counts, uint32_t* words, void* stream);

/* ---- rows of a flat bucket ----------------------------------------------------------------------------------------------------------
 * `flat`: a bucket of P rows in num_segments segments laid back to back, segment k holding row_floats[k] floats per row
 * (GaussianParams.flat and both Adam moments).
 * fdgs_mcmc_copy_rows: row dst[j] of every segment := row src[j], j < n, in place.  No dst row may be a src row or appear twice.
 * fdgs_mcmc_zero_rows: rows[j] of every segment := 0 in a and (optional) b.  One launch per segment, float4 accesses where the
 * segment's start and row length allow.
 * FDGS_ERR_INVALID_ARG: num_segments outside 1 .. 16, a NULL or non-positive row_floats, P < 1, n < 0, n > 0 with a NULL pointer. */
int fdgs_mcmc_copy_rows(int32_t num_segments, const int32_t* row_floats /* host */, int64_t P, int32_t n, const int32_t* dst,
                        const int32_t* src, float* flat, void* stream);
int fdgs_mcmc_zero_rows(int32_t num_segments, const int32_t* row_floats /* host */, int64_t P, int32_t n, const int32_t* rows, float* a,
                        float* b, void* stream);

/* ---- opacity and scale of a Gaussian that stands for N copies of itself ---------------------------------------------------------------
 * For j < n: row i = rows[j], N = min(counts[count_of[j]] + 1, 51).  With o = sigmoid(opacity_raw[i]):
 *   o' = 1 - (1 - o)^(1 / N)
 *   D  = sum_{i = 1 .. N} sum_{k = 0 .. i - 1} C(i - 1, k) (-1)^k o'^(k + 1) / sqrt(k + 1)
 *      = sum_{k = 0 .. N - 1} C(N, k + 1) (-1)^k o'^(k + 1) / sqrt(k + 1)           (the inner sums over i fold into one binomial)
 *   every scale *= o / D;  opacity = clamp(o', 0.005, 1 - 2^-23)
 * all of it in float64 (the alternating sum cancels), written back raw (logit, log) with one rounding to float32 each.  scaling_t_raw
 * is updated with gaussian_dim == 4 only.  An opacity clamped from below is written as the smallest float32 logit at or above the
 * nearest one whose float32 opacity exceeds 0.005 (the nearest activates to 0.0049999994: dead again at the default min_opacity).  A row is read and written by its own thread alone: rows must not repeat.  N == 1 (a count
 * of 0) writes nothing.
 * FDGS_ERR_INVALID_ARG: n < 0, gaussian_dim outside {3, 4}, n > 0 with a NULL pointer (scaling_t_raw only with gaussian_dim == 4). */
int fdgs_mcmc_update(int32_t n, int32_t gaussian_dim, const int32_t* rows, const int32_t* count_of, const int32_t* counts,
                     float* opacity_raw, float* scaling_raw, float* scaling_t_raw, void* stream);

/* ---- the noise step -----------------------------------------------------------------------------------------------------------------
 * For every Gaussian: Sigma from the raw parameters (3 x 3 with gaussian_dim == 3; diag(Sigma3, exp(scaling_t_raw)^2) with
 * gaussian_dim == 4 and no rot_4d; the full 4 x 4 with rot_4d), xi ~ N(0, I),
 *   delta = Sigma xi * g(o) * scale,  g(o) = 1 / (1 + exp(-100 ((1 - o) - 0.995))),  xyz += delta_xyz, t += delta_t (gaussian_dim == 4).
 * Sigma xi and the gate are evaluated in float64 from the float32 parameters and rounded once, with the sum into xyz / t.
 * scale: the caller's noise_lr * lr_xyz.  xi_in (float [P, 4], optional): the normals to use (column 3 is ignored with gaussian_dim == 3).
 * Without it: w = Philox4x32-10(counter = (i, stream_id, call & 0xffffffff, call >> 32), key = the seed's halves),
 * u_k = ((w_k >> 8) + 1) * 2^-24 in (0, 1], xi_0 = sqrt(-2 ln u_0) cos(2 pi u_1), xi_1 = sqrt(-2 ln u_0) sin(2 pi u_1), xi_2 and xi_3
 * likewise from (u_2, u_3).  xi_out (float [P, 4]) and words (uint32 [P, 4]), both optional, receive what was used.  One launch.
 * FDGS_ERR_INVALID_ARG: P < 0, gaussian_dim outside {3, 4}, rot_4d without gaussian_dim == 4, P > 0 with a NULL required pointer
 * (t_raw / scaling_t_raw with gaussian_dim == 4, rotation_r_raw with rot_4d). */
int fdgs_mcmc_noise(int32_t P, int32_t gaussian_dim, int32_t rot_4d, float* xyz, float* t, const float* opacity_raw,
                    const float* scaling_raw, const float* scaling_t_raw, const float* rotation_raw, const float* rotation_r_raw,
                    float scale, const float* xi_in, uint64_t seed, uint32_t stream_id, uint64_t call, float* xi_out, uint32_t* words,
                    void* stream);

/* ---- the regularisers ---------------------------------------------------------------------------------------------------------------
 * L_o = lambda_o / P sum_i o_i, L_s = lambda_s / (3 P) sum_i sum_k exp(scaling_raw[i][k]), L_st = lambda_st / P sum_i exp(scaling_t_raw[i]).
 * Their gradients are ADDED into the sinks: dL_dopacity [P] += lambda_o / P o (1 - o), dL_dscales [P, 3] += lambda_s / (3 P) exp(.),
 * dL_dscales_t [P] += lambda_st / P exp(.) (only with lambda_st > 0; scaling_t_raw / dL_dscales_t may then not be NULL).  Each
 * gradient is evaluated in float64 and rounded once before the float32 addition.  terms (double [3], optional) receives
 * (L_o, L_s, L_st) from float64 sums in a fixed order: per-workgroup partials, then one workgroup over them.
 * partials: fdgs_mcmc_regularize_num_partials(P) doubles.  Two launches.
 * FDGS_ERR_INVALID_ARG: P < 1, a NULL opacity_raw / scaling_raw / dL_dopacity / dL_dscales / partials. */
int32_t fdgs_mcmc_regularize_num_partials(int32_t P);
int fdgs_mcmc_regularize(int32_t P, const float* opacity_raw, const float* scaling_raw, const float* scaling_t_raw, float lambda_o,
                         float lambda_s, float lambda_st, float* dL_dopacity, float* dL_dscales, float* dL_dscales_t, double* partials,
                         double* terms, void* stream);

#ifdef __cplusplus
}
#endif
#endif
