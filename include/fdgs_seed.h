/* fdgs_seed.h -- starting a run from a point cloud: thinning, random clouds and the initial model (csrc/seed.hip, libfdgs.so).
 *
 * A companion of fdgs.h with the same conventions: every function returns FDGS_OK or an error code whose text fdgs_last_error()
 * holds, device pointers are borrowed, `stream` is a hipStream_t, nothing synchronises the host.  FDGS_VERSION does not count the
 * entry points of this header.  Every result is a pure function of its inputs, bit for bit, from run to run: integer scans, a stable
 * sort, sequential float sums in a fixed order, no float atomics.
 */
#ifndef FDGS_SEED_H
#define FDGS_SEED_H

#include "fdgs.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- voxel-grid thinning in (x, y, z, t) --------------------------------------------------------------------------------------------
 * The cell index of a coordinate v is floor((v - origin) * inv_cell), every operation in float32 and rounded on its own (no fused
 * multiply-add); the index is then clamped to [0, FDGS_SEED_AXIS_CELLS - 1] (a NaN counts as 0).  origin = (x, y, z, t) and
 * inv_cell = (1 / cell, 1 / cell, 1 / cell, 1 / cell_t) as float32 values the CALLER computed; without `t` the time index is 0.
 * The four indices pack into one 64-bit key, (ix << 48) | (iy << 32) | (iz << 16) | it: 16 bits per axis, so a cloud may span at most
 * FDGS_SEED_AXIS_CELLS cells along an axis (the Python layer raises ValueError beyond that instead of clamping).
 * The points are sorted by key with the library's stable radix sort; every occupied cell gives one output row, in ascending key
 * order: out_key, out_count (members), out_first (the smallest point index of the cell), and the float32 means of position, colour
 * and time, each the cell's values summed one after the other in ascending point index -- a compensated (Kahan) float32 sum that
 * starts from the first member's value with compensation 0 -- and divided by float(count).
 * n_cells (device int32) always receives the number of occupied cells; rows at or beyond `capacity` are not written.  count_only
 * != 0: nothing but n_cells is written and the out_ pointers may be NULL.  rgb may be NULL (out_rgb is then not written), t and
 * out_t likewise.  N == 0 writes n_cells = 0.  scratch: fdgs_seed_thin_scratch_bytes(N) bytes of device memory.
 * FDGS_ERR_INVALID_ARG before any launch: N < 0 or N >= 2^28, capacity < 0, a NULL origin / inv_cell / n_cells, N > 0 with a NULL
 * xyz / scratch, a NULL required output when count_only == 0, a non-finite origin, an inv_cell that is not positive and finite. */
#define FDGS_SEED_AXIS_BITS 16
#define FDGS_SEED_AXIS_CELLS 65536
size_t fdgs_seed_thin_scratch_bytes(int32_t N);
int fdgs_seed_thin(int32_t N, const float* xyz, const float* rgb, const float* t, const float* origin /* host [4] */,
                   const float* inv_cell /* host [4] */, int32_t count_only, int32_t capacity, uint64_t* out_key, float* out_xyz,
                   float* out_rgb, float* out_t, int32_t* out_count, int32_t* out_first, int32_t* n_cells, void* scratch, void* stream);

/* ---- counter-based random clouds ----------------------------------------------------------------------------------------------------
 * Philox4x32-10 with key = (seed & 0xffffffff, seed >> 32) and counter = (point index, stream_id, 0, 0): four 32-bit words w0 .. w3
 * per point, uniforms u_k = (w_k >> 8) * 2^-24 in [0, 1).  What is made of them (params: host floats):
 *   FDGS_SEED_BOX     out [N, 3] = u_k * params[3 + k] + params[k], k = 0 .. 2 (multiply, then add: two roundings)
 *   FDGS_SEED_SPHERE  out [N, 3] on the sphere of radius params[0]: phi = 2 pi u_0, c = 2 u_1 - 1 (the cosine of the polar angle),
 *                     s = sqrt(1 - c c); (r s cos phi, r s sin phi, r c)
 *   FDGS_SEED_TIME    out [N]    = (u_0 * 1.2 - 0.1) * params[1] + params[0]   (params = t0, t1 - t0)
 * words (uint32 [N, 4]) and uniforms (float [N, 4]) optionally receive w and u.  One launch; N == 0 launches nothing.
 * FDGS_ERR_INVALID_ARG: N < 0, an unknown shape, NULL params, N > 0 with a NULL out. */
#define FDGS_SEED_BOX 0
#define FDGS_SEED_SPHERE 1
#define FDGS_SEED_TIME 2
int fdgs_seed_random(int32_t N, uint64_t seed, uint32_t stream_id, int32_t shape, const float* params /* host [6] */, float* out,
                     uint32_t* words, float* uniforms, void* stream);

/* ---- the model a run starts from (scene/gaussian_model.py create_from_pcd) ----------------------------------------------------------
 * Writes all eight segments of a flat parameter bucket of P Gaussians with M SH coefficients (P * (17 + 3 M) floats, segments back
 * to back in the order xyz | opacity | scaling | rotation | t | scaling_t | rotation_r | features) in one launch:
 *   xyz = xyz;  opacity = opacity_raw;  scaling = log(sqrt(max(dist2, 1e-7))) on all three axes, evaluated as half the float64
 *   logarithm of the float32 maximum and rounded once;  rotation = (1, 0, 0, 0);
 *   t = t and scaling_t = scaling_t_raw with gaussian_dim == 4, both 0 otherwise;  rotation_r = (1, 0, 0, 0);
 *   features: coefficient 0 = (rgb - 0.5) / 0.28209479177387814, the rest 0.
 * opacity_raw = inverse_sigmoid(0.1) and scaling_t_raw = log(sqrt((t1 - t0) / 5)) are computed by the caller in float32.
 * FDGS_ERR_INVALID_ARG: P < 0, M < 1, P * (17 + 3 M) >= 2^31, gaussian_dim outside {3, 4}, P > 0 with a NULL xyz / rgb / dist2 / flat,
 * or a NULL t with gaussian_dim == 4. */
int fdgs_seed_init(int32_t P, int32_t M, int32_t gaussian_dim, const float* xyz, const float* rgb, const float* t, const float* dist2,
                   float opacity_raw, float scaling_t_raw, float* flat, void* stream);

#ifdef __cplusplus
}
#endif
#endif
