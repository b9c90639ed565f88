// exposure.hip -- per-camera colour correction (include/fdgs_exposure.h) for gfx950: the affine transform of a render and its backward,
// the transform table's Adam, and the moments of the closed-form colour alignment of held-out views.
//
// All four are memory-bound passes over planar [3, H, W] images: float4 accesses where the planes allow them (H W a multiple of 4 and
// 16-byte aligned pointers: every plane then starts on a 16-byte boundary), one pixel per access otherwise.  The sums are float64 per
// thread (an fp32 x fp32 product is exact in a double), reduced over the wave by halving and over the workgroup in wave order into one
// row of doubles per workgroup, and one workgroup adds the rows: no atomics, the same bits on every run.  Built with FP contraction
// off: the float32 results are the header's operations, each rounded on its own.
#include "fdgs_common.h"
#include "../../include/fdgs_exposure.h"
#include <cmath>

namespace fdgs
{
	constexpr int EXP_THREADS = 256;
	constexpr int EXP_WAVES = EXP_THREADS / WAVE;
	static_assert(EXP_THREADS * 4 == FDGS_EXPOSURE_BLOCK_PIXELS, "fdgs_exposure.h states the workgroup's pixels");

	template <int V> __device__ __forceinline__ void ldv(const float* p, float (&x)[V])
	{
		if constexpr (V == 4)
		{
			const float4 t = *reinterpret_cast<const float4*>(p);
			x[0] = t.x; x[1] = t.y; x[2] = t.z; x[3] = t.w;
		}
		else x[0] = *p;
	}
	template <int V> __device__ __forceinline__ void stv(float* p, const float (&x)[V])
	{
		if constexpr (V == 4) *reinterpret_cast<float4*>(p) = make_float4(x[0], x[1], x[2], x[3]);
		else *p = x[0];
	}
	// the three planes of V consecutive pixels starting at pixel p
	template <int V> __device__ __forceinline__ void ld3v(const float* img, size_t HW, size_t p, float (&x)[3][V])
	{
#pragma unroll
		for (int i = 0; i < 3; i++) ldv<V>(img + i * HW + p, x[i]);
	}
	template <int V> __device__ __forceinline__ void st3v(float* img, size_t HW, size_t p, const float (&x)[3][V])
	{
#pragma unroll
		for (int i = 0; i < 3; i++) stv<V>(img + i * HW + p, x[i]);
	}
	// the camera's row A = [M | o]: the same address in every lane
	__device__ __forceinline__ void load_row(const float* table, int cam, float (&a)[12])
	{
#pragma unroll
		for (int k = 0; k < 12; k++) a[k] = table[12 * (size_t)cam + k];
	}

	// Sums of K values over the workgroup: every wave's lanes by halving, then thread k < K adds the waves' totals of value k in wave
	// order and returns it (the other threads return nothing of use).  One use per kernel: no barrier in front.
	template <int K> __device__ __forceinline__ double block_sum_k(double (&v)[K], double* red)
	{
#pragma unroll
		for (int k = 0; k < K; k++)
		{
#pragma unroll
			for (int d = WAVE / 2; d > 0; d >>= 1) v[k] += __shfl_down(v[k], d);
		}
		if ((threadIdx.x & (WAVE - 1)) == 0)
		{
#pragma unroll
			for (int k = 0; k < K; k++) red[(threadIdx.x / WAVE) * K + k] = v[k];
		}
		__syncthreads();
		double s = 0.0;
		if (threadIdx.x < K)
		{
#pragma unroll
			for (int w = 0; w < EXP_WAVES; w++) s += red[w * K + threadIdx.x];
		}
		return s;
	}

	// units: groups of V pixels; the workgroups stride over them
	template <int V>
	__global__ void __launch_bounds__(EXP_THREADS) exposure_apply_kernel(const long long units, const size_t HW, const float* image, const float* table,
	                                                                     const int cam, float* out)
	{
		float a[12];
		load_row(table, cam, a);
		for (long long u = (long long)blockIdx.x * EXP_THREADS + threadIdx.x; u < units; u += (long long)gridDim.x * EXP_THREADS)
		{
			const size_t p = (size_t)u * V;
			float c[3][V], o[3][V];
			ld3v<V>(image, HW, p, c);
#pragma unroll
			for (int i = 0; i < 3; i++)
			{
#pragma unroll
				for (int k = 0; k < V; k++) o[i][k] = ((a[4 * i] * c[0][k] + a[4 * i + 1] * c[1][k]) + a[4 * i + 2] * c[2][k]) + a[4 * i + 3];
			}
			st3v<V>(out, HW, p, o);   // (out may be image: this thread's pixels, all read above)
		}
	}

	// parts[12 * workgroup + 4 i + j] = the workgroup's sum of g'[i] * (r, g, b, 1)[j]
	template <int V>
	__global__ void __launch_bounds__(EXP_THREADS) exposure_backward_kernel(const long long units, const size_t HW, const float* g_out, const float* image,
	                                                                        const float* table, const int cam, float* g_image, double* parts)
	{
		__shared__ double red[EXP_WAVES * 12];
		float a[12];
		load_row(table, cam, a);
		double acc[12];
#pragma unroll
		for (int k = 0; k < 12; k++) acc[k] = 0.0;
		for (long long u = (long long)blockIdx.x * EXP_THREADS + threadIdx.x; u < units; u += (long long)gridDim.x * EXP_THREADS)
		{
			const size_t p = (size_t)u * V;
			float g[3][V], c[3][V];
			ld3v<V>(g_out, HW, p, g);
			ld3v<V>(image, HW, p, c);
#pragma unroll
			for (int k = 0; k < V; k++)
			{
#pragma unroll
				for (int i = 0; i < 3; i++)
				{
					const double gi = (double)g[i][k];
#pragma unroll
					for (int j = 0; j < 3; j++) acc[4 * i + j] += gi * (double)c[j][k];
					acc[4 * i + 3] += gi;
				}
			}
			if (g_image != nullptr)
			{
				float o[3][V];
#pragma unroll
				for (int j = 0; j < 3; j++)
				{
#pragma unroll
					for (int k = 0; k < V; k++) o[j][k] = (a[j] * g[0][k] + a[4 + j] * g[1][k]) + a[8 + j] * g[2][k];
				}
				st3v<V>(g_image, HW, p, o);   // (g_image may be g_out)
			}
		}
		const double s = block_sum_k<12>(acc, red);
		if (threadIdx.x < 12) parts[12 * (size_t)blockIdx.x + threadIdx.x] = s;
	}

	// parts[22 * workgroup + m]: the moments of fdgs_colour_fit_moments
	template <int V>
	__global__ void __launch_bounds__(EXP_THREADS) colour_fit_kernel(const long long units, const size_t HW, const float* image, const float* gt, const int clamp,
	                                                                 double* parts)
	{
		__shared__ double red[EXP_WAVES * 22];
		double acc[22];
#pragma unroll
		for (int k = 0; k < 22; k++) acc[k] = 0.0;
		for (long long u = (long long)blockIdx.x * EXP_THREADS + threadIdx.x; u < units; u += (long long)gridDim.x * EXP_THREADS)
		{
			const size_t p = (size_t)u * V;
			float c[3][V], t[3][V];
			ld3v<V>(image, HW, p, c);
			ld3v<V>(gt, HW, p, t);
#pragma unroll
			for (int k = 0; k < V; k++)
			{
				double x[4];
#pragma unroll
				for (int j = 0; j < 3; j++) x[j] = (double)(clamp ? fminf(fmaxf(c[j][k], 0.f), 1.f) : c[j][k]);
				x[3] = 1.0;
				int m = 0;
#pragma unroll
				for (int j = 0; j < 4; j++)
				{
#pragma unroll
					for (int l = j; l < 4; l++) acc[m++] += x[j] * x[l];
				}
#pragma unroll
				for (int i = 0; i < 3; i++)
				{
#pragma unroll
					for (int j = 0; j < 4; j++) acc[10 + 4 * i + j] += (double)t[i][k] * x[j];
				}
			}
		}
		const double s = block_sum_k<22>(acc, red);
		if (threadIdx.x < 22) parts[22 * (size_t)blockIdx.x + threadIdx.x] = s;
	}

	// one workgroup: thread t adds rows t, t + 256, ... in that order, then the workgroup's fixed-order sum; written, or added to out
	template <int K, typename Out>
	__global__ void __launch_bounds__(EXP_THREADS) exposure_finish_kernel(const int nb, const double* __restrict__ parts, Out* __restrict__ out, const int accumulate)
	{
		__shared__ double red[EXP_WAVES * K];
		double v[K];
#pragma unroll
		for (int k = 0; k < K; k++) v[k] = 0.0;
		for (int b = threadIdx.x; b < nb; b += EXP_THREADS)
		{
#pragma unroll
			for (int k = 0; k < K; k++) v[k] += parts[K * (size_t)b + k];
		}
		const double s = block_sum_k<K>(v, red);
		if (threadIdx.x < K) out[threadIdx.x] = accumulate ? out[threadIdx.x] + (Out)s : (Out)s;
	}

	struct ExposureViews { int n; int cam[FDGS_EXPOSURE_MAX_VIEWS]; };
	// 16 lanes per view, 12 of them at work: the first view that names a row owns it and takes the later views' slots with its own
	__global__ void __launch_bounds__(EXP_THREADS) exposure_adam_kernel(const ExposureViews views, float* table, float* exp_avg, float* exp_avg_sq, int* steps,
	                                                                    const float* __restrict__ slots, const double lr, const double b1, const double b2,
	                                                                    const double eps)
	{
		const int t = blockIdx.x * EXP_THREADS + threadIdx.x;
		const int b = t >> 4, j = t & 15;
		if (b >= views.n || j >= 12) return;
		const int cam = views.cam[b];
		for (int e = 0; e < b; e++)
			if (views.cam[e] == cam) return;
		double g = 0.0;
		for (int e = b; e < views.n; e++)
			if (views.cam[e] == cam) g += (double)slots[12 * e + j];
		// (the row's 12 lanes sit in one wave and the count written below is computed from the one read here: every lane has read
		// before lane 0 writes)
		const int step = steps[cam] + 1;
		const size_t at = 12 * (size_t)cam + j;
		const float m = (float)(b1 * (double)exp_avg[at] + (1.0 - b1) * g);
		const float v = (float)(b2 * (double)exp_avg_sq[at] + (1.0 - b2) * g * g);
		const double bc1 = 1.0 - pow(b1, (double)step), bc2 = 1.0 - pow(b2, (double)step);
		const double denom = sqrt((double)v) / sqrt(bc2) + eps;
		table[at] = (float)((double)table[at] - lr / bc1 * ((double)m / denom));
		exp_avg[at] = m;
		exp_avg_sq[at] = v;
		if (j == 0) steps[cam] = step;
	}

	// what the image entry points share: the size check, the workgroups of a pass and whether float4 accesses fit
	static inline int exposure_blocks(long long HW)
	{
		const long long nb = (HW + FDGS_EXPOSURE_BLOCK_PIXELS - 1) / FDGS_EXPOSURE_BLOCK_PIXELS;
		return (int)(nb < FDGS_EXPOSURE_MAX_BLOCKS ? nb : FDGS_EXPOSURE_MAX_BLOCKS);
	}
	static inline bool bad_size(int H, int W) { return H < 1 || W < 1 || (long long)H * W >= (1ll << 31); }
	static inline bool vec4_ok(long long HW, const void* a, const void* b, const void* c)
	{
		return HW % 4 == 0 && ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c)) & 15) == 0;
	}
}

extern "C" int fdgs_exposure_apply(int32_t H, int32_t W, const float* image, const float* table, int32_t num_cameras, int32_t camera, float* out,
                                   void* stream_v)
{
	using namespace fdgs;
	if (bad_size(H, W)) return fail(FDGS_ERR_INVALID_ARG, "fdgs_exposure_apply: bad image size H=%d W=%d", H, W);
	if (camera < 0 || camera >= num_cameras)
		return fail(FDGS_ERR_INVALID_ARG, "fdgs_exposure_apply: camera=%d is outside the table's %d rows", camera, num_cameras);
	if (!image || !table || !out) return fail(FDGS_ERR_INVALID_ARG, "fdgs_exposure_apply: image / table / out must not be NULL");
	const long long HW = (long long)H * W;
	hipStream_t stream = (hipStream_t)stream_v;
	if (vec4_ok(HW, image, out, nullptr))
		hipLaunchKernelGGL(exposure_apply_kernel<4>, dim3(exposure_blocks(HW)), dim3(EXP_THREADS), 0, stream, HW / 4, (size_t)HW, image, table, camera, out);
	else
		hipLaunchKernelGGL(exposure_apply_kernel<1>, dim3(exposure_blocks(HW)), dim3(EXP_THREADS), 0, stream, HW, (size_t)HW, image, table, camera, out);
	return launched("fdgs_exposure_apply");
}

extern "C" int32_t fdgs_exposure_num_partials(int32_t H, int32_t W) { return fdgs::bad_size(H, W) ? 12 : 12 * fdgs::exposure_blocks((long long)H * W); }

extern "C" int fdgs_exposure_backward(int32_t H, int32_t W, const float* g_out, const float* image, const float* table, int32_t num_cameras,
                                      int32_t camera, float* g_image, double* partials, float* dA, int32_t accumulate, void* stream_v)
{
	using namespace fdgs;
	if (bad_size(H, W)) return fail(FDGS_ERR_INVALID_ARG, "fdgs_exposure_backward: bad image size H=%d W=%d", H, W);
	if (camera < 0 || camera >= num_cameras)
		return fail(FDGS_ERR_INVALID_ARG, "fdgs_exposure_backward: camera=%d is outside the table's %d rows", camera, num_cameras);
	if (!g_out || !image || !table || !partials || !dA)
		return fail(FDGS_ERR_INVALID_ARG, "fdgs_exposure_backward: g_out / image / table / partials / dA must not be NULL");
	const long long HW = (long long)H * W;
	const int nb = exposure_blocks(HW);
	hipStream_t stream = (hipStream_t)stream_v;
	if (vec4_ok(HW, g_out, image, g_image))
		hipLaunchKernelGGL(exposure_backward_kernel<4>, dim3(nb), dim3(EXP_THREADS), 0, stream, HW / 4, (size_t)HW, g_out, image, table, camera, g_image, partials);
	else
		hipLaunchKernelGGL(exposure_backward_kernel<1>, dim3(nb), dim3(EXP_THREADS), 0, stream, HW, (size_t)HW, g_out, image, table, camera, g_image, partials);
	hipLaunchKernelGGL((exposure_finish_kernel<12, float>), dim3(1), dim3(EXP_THREADS), 0, stream, nb, partials, dA, accumulate);
	return launched("fdgs_exposure_backward");
}

extern "C" int fdgs_exposure_adam(int32_t num_cameras, float* table, float* exp_avg, float* exp_avg_sq, int32_t* steps, int32_t B, const float* slots,
                                  const int32_t* cameras, double lr, double beta1, double beta2, double eps, void* stream_v)
{
	using namespace fdgs;
	if (num_cameras < 1) return fail(FDGS_ERR_INVALID_ARG, "fdgs_exposure_adam: num_cameras=%d is below 1", num_cameras);
	if (B < 1) return fail(FDGS_ERR_INVALID_ARG, "fdgs_exposure_adam: B=%d views is below 1", B);
	if (B > FDGS_EXPOSURE_MAX_VIEWS) return fail(FDGS_ERR_INVALID_ARG, "fdgs_exposure_adam: B=%d views is above %d", B, FDGS_EXPOSURE_MAX_VIEWS);
	if (!cameras) return fail(FDGS_ERR_INVALID_ARG, "fdgs_exposure_adam: the host array cameras must not be NULL");
	ExposureViews views;
	views.n = B;
	for (int b = 0; b < FDGS_EXPOSURE_MAX_VIEWS; b++) views.cam[b] = 0;
	for (int b = 0; b < B; b++)
	{
		if (cameras[b] < 0 || cameras[b] >= num_cameras)
			return fail(FDGS_ERR_INVALID_ARG, "fdgs_exposure_adam: cameras[%d]=%d is outside the table's %d rows", b, cameras[b], num_cameras);
		views.cam[b] = cameras[b];
	}
	if (!table || !exp_avg || !exp_avg_sq || !steps || !slots)
		return fail(FDGS_ERR_INVALID_ARG, "fdgs_exposure_adam: table / exp_avg / exp_avg_sq / steps / slots must not be NULL");
	hipLaunchKernelGGL(exposure_adam_kernel, dim3(div_up(16 * B, EXP_THREADS)), dim3(EXP_THREADS), 0, (hipStream_t)stream_v, views, table, exp_avg, exp_avg_sq,
	                   steps, slots, lr, beta1, beta2, eps);
	return launched("fdgs_exposure_adam");
}

extern "C" int32_t fdgs_colour_fit_num_partials(int32_t H, int32_t W) { return fdgs::bad_size(H, W) ? 22 : 22 * fdgs::exposure_blocks((long long)H * W); }

extern "C" int fdgs_colour_fit_moments(int32_t H, int32_t W, const float* image, const float* gt, int32_t clamp, double* partials, double* moments,
                                       void* stream_v)
{
	using namespace fdgs;
	if (bad_size(H, W)) return fail(FDGS_ERR_INVALID_ARG, "fdgs_colour_fit_moments: bad image size H=%d W=%d", H, W);
	if (!image || !gt || !partials || !moments) return fail(FDGS_ERR_INVALID_ARG, "fdgs_colour_fit_moments: image / gt / partials / moments must not be NULL");
	const long long HW = (long long)H * W;
	const int nb = exposure_blocks(HW);
	hipStream_t stream = (hipStream_t)stream_v;
	if (vec4_ok(HW, image, gt, nullptr))
		hipLaunchKernelGGL(colour_fit_kernel<4>, dim3(nb), dim3(EXP_THREADS), 0, stream, HW / 4, (size_t)HW, image, gt, clamp, partials);
	else
		hipLaunchKernelGGL(colour_fit_kernel<1>, dim3(nb), dim3(EXP_THREADS), 0, stream, HW, (size_t)HW, image, gt, clamp, partials);
	hipLaunchKernelGGL((exposure_finish_kernel<22, double>), dim3(1), dim3(EXP_THREADS), 0, stream, nb, partials, moments, 0);
	return launched("fdgs_colour_fit_moments");
}
