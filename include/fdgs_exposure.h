/* fdgs_exposure.h -- per-camera colour correction: a learned affine transform of the render before the loss, its own Adam, and the
 * moments of the closed-form colour alignment of held-out views (csrc/exposure.hip, libfdgs.so).
 *
 * A companion of fdgs.h with the same conventions: every function returns FDGS_OK or an error code whose text fdgs_last_error()
 * holds, device pointers are borrowed, `stream` is a hipStream_t, nothing synchronises the host.  FDGS_VERSION does not count the
 * entry points of this header.  Every result is a pure function of its inputs, bit for bit: float64 sums in a fixed order, no atomics.
 *
 * Images are planar float32 [3, H, W].  A camera's transform is a row of 12 floats A = [M | o] (3 x 4, row-major: A[4 i + j] = M[i][j],
 * A[4 i + 3] = o[i]) of a device table [num_cameras, 12]; it is read on the device through the table pointer and the camera index.
 */
#ifndef FDGS_EXPOSURE_H
#define FDGS_EXPOSURE_H

#include "fdgs.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FDGS_EXPOSURE_BLOCK_PIXELS 1024 /* pixels of one workgroup's pass: 256 threads x 4 */
#define FDGS_EXPOSURE_MAX_BLOCKS 4096   /* larger images: the workgroups stride over them */
#define FDGS_EXPOSURE_MAX_VIEWS 64      /* views of one fdgs_exposure_adam launch */

/* ---- the transform ------------------------------------------------------------------------------------------------------------------
 * out[i] = ((M[i][0] r + M[i][1] g) + M[i][2] b) + o[i] per pixel in float32, every operation rounded on its own.  out may be image.
 * float4 accesses where H W is a multiple of 4 and both pointers are 16-byte aligned, one pixel per access otherwise.  One launch.
 * FDGS_ERR_INVALID_ARG: H or W < 1 (or H W >= 2^31), a NULL pointer, camera outside [0, num_cameras). */
int fdgs_exposure_apply(int32_t H, int32_t W, const float* image, const float* table, int32_t num_cameras, int32_t camera, float* out,
                        void* stream);

/* ---- its backward -------------------------------------------------------------------------------------------------------------------
 * One pass over the upstream gradient g' = dL / d out and the UNCORRECTED image:
 *   g_image[j] = ((M[0][j] g'[0] + M[1][j] g'[1]) + M[2][j] g'[2])        float32; g_image may be g_out, NULL: not wanted
 *   dA[4 i + j] = sum over the pixels of g'[i] * (r, g, b, 1)[j]          products and sums in float64, rounded once
 * Every thread sums its pixels in index order, a wave its lanes by halving, a workgroup its waves in wave order into one row of 12
 * doubles of `partials`; one workgroup then adds the rows (thread t: rows t, t + 256, ... in order; the threads as before) and writes
 * (accumulate == 0) or adds (!= 0) the 12 float32 results to dA.  partials: fdgs_exposure_num_partials(H, W) doubles.  Two launches.
 * FDGS_ERR_INVALID_ARG: as fdgs_exposure_apply. */
int32_t fdgs_exposure_num_partials(int32_t H, int32_t W);
int fdgs_exposure_backward(int32_t H, int32_t W, const float* g_out, const float* image, const float* table, int32_t num_cameras,
                           int32_t camera, float* g_image, double* partials, float* dA, int32_t accumulate, void* stream);

/* ---- the table's Adam ---------------------------------------------------------------------------------------------------------------
 * cameras (HOST, read before the call returns): the B camera indices of a step's views; slots [B, 12]: the views' dA.  A row named by
 * at least one view gets g = the float64 sum of its views' slots in view order, steps[row] += 1 (t: the new count) and
 *   m = b1 m + (1 - b1) g,  v = b2 v + (1 - b2) g g,  p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
 * (torch.optim.Adam without weight decay or amsgrad) evaluated in float64 from the float32 state, m and v rounded to float32 before p
 * reads them.  Every other row of table, exp_avg, exp_avg_sq and steps is not touched.  One launch.
 * FDGS_ERR_INVALID_ARG: num_cameras < 1, B < 1, B > FDGS_EXPOSURE_MAX_VIEWS, a NULL pointer, a camera outside [0, num_cameras). */
int fdgs_exposure_adam(int32_t num_cameras, float* table, float* exp_avg, float* exp_avg_sq, int32_t* steps, int32_t B, const float* slots,
                       const int32_t* cameras /* host */, double lr, double beta1, double beta2, double eps, void* stream);

/* ---- moments of the colour alignment of a held-out view -----------------------------------------------------------------------------
 * With c = (r, g, b, 1) of `image` (clamp != 0: r, g, b clamped to [0, 1] first) and t = (r, g, b) of `gt`, summed over the pixels in
 * float64 in the fixed order of fdgs_exposure_backward:
 *   moments[0 .. 9]   = sum c[j] c[k], j <= k: (rr, rg, rb, r, gg, gb, g, bb, b, 1)
 *   moments[10 .. 21] = sum t[i] c[j] at 10 + 4 i + j
 * partials: fdgs_colour_fit_num_partials(H, W) doubles.  Two launches.
 * FDGS_ERR_INVALID_ARG: H or W < 1 (or H W >= 2^31), a NULL pointer. */
int32_t fdgs_colour_fit_num_partials(int32_t H, int32_t W);
int fdgs_colour_fit_moments(int32_t H, int32_t W, const float* image, const float* gt, int32_t clamp, double* partials, double* moments,
                            void* stream);

#ifdef __cplusplus
}
#endif
#endif
