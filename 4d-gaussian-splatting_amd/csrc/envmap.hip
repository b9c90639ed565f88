// envmap.hip -- the environment map behind the Gaussians (gaussian_renderer/__init__.py:165-177 of the reference), forward and
// backward (gfx950).
//
//   ray      d = normalize((inv(viewmatrix^T) (px, py, 1, 1))[:3] - campos),  px = (i + .5 - cx) / fl_x,  py = (j + .5 - cy) / fl_y
//            (scene/cameras.py:75-82; the 4x4 inverse is taken here, once per workgroup: no host round trip)
//   sphere   t = -(o.d) + sqrt(delta) / (d.d),  delta = (o.d)^2 - (d.d)(o.o - R^2)   (the reference's operator precedence)
//   lookup   u = atan2(y, x) / 2pi + 0.5,  v = acos(z / R) / pi,  bilinear grid_sample (align_corners = False, zero padding: the
//            seam at u = 0 / 1 does not wrap).  Ray and coordinates in float64 (env_tap), v as atan2(sqrt(x^2 + y^2), z): equal to
//            the clamped acos(clamp(z / R, -1, 1)) on the sphere, never NaN (the reference's fp32 acos is NaN at the pole, where
//            z / R rounds to 1.0000001).
//   out      colour_out = colour_in + T * env(ray)
//
// Backward.  d / d alpha (alpha = 1 - T) = -sum_c g_c env_c: per pixel, no atomics.  d / d env: every pixel scatters g_c T w_k into
// the four texels of its tap.  One float atomic per (pixel, corner, channel) would be 66 MB of atomic adds per view at 1352 x 1014
// (~50 us at the chip's ~1.3 TB/s); a texel of a 500^2 map covers ~15 x 8 pixels at the equator.  So each 16 x 16 pixel tile
// reduces its contributions in an LDS window over the texels the tile touches and flushes the window with one global atomic per
// touched (texel, channel), row segment by row segment.  Near a pole a tile can span hundreds of longitude texels: a window larger
// than ENV_WIN texels falls back to direct global atomics.  Float-atomic sums: reproducible to the order of arrival only.
#include <climits>
#include <cstdio>
#include "fdgs_common.h"

namespace fdgs
{
	constexpr int ENV_TILE = 16;
	constexpr int ENV_THREADS = ENV_TILE * ENV_TILE;
	constexpr int ENV_WIN = 3072;   // texels of a tile's LDS window (x 3 channels: 36 KB, four workgroups per CU)

	struct EnvView { float fx, fy, cx, cy, R; int H, W, eh, ew; };

	// s[0..11]: rows r < 3 of c2w = inv(V^T) = inv(V)^T as (m_r0, m_r1, m_r2 + m_r3); s[12..14]: campos.  Thread 0 only.
	__device__ void env_setup(const float* __restrict__ vm, const float* __restrict__ campos, double* s)
	{
		double a[16], inv[16];
		for (int k = 0; k < 16; k++) a[k] = vm[k];
		inv[0] = a[5] * a[10] * a[15] - a[5] * a[11] * a[14] - a[9] * a[6] * a[15] + a[9] * a[7] * a[14] + a[13] * a[6] * a[11] - a[13] * a[7] * a[10];
		inv[4] = -a[4] * a[10] * a[15] + a[4] * a[11] * a[14] + a[8] * a[6] * a[15] - a[8] * a[7] * a[14] - a[12] * a[6] * a[11] + a[12] * a[7] * a[10];
		inv[8] = a[4] * a[9] * a[15] - a[4] * a[11] * a[13] - a[8] * a[5] * a[15] + a[8] * a[7] * a[13] + a[12] * a[5] * a[11] - a[12] * a[7] * a[9];
		inv[12] = -a[4] * a[9] * a[14] + a[4] * a[10] * a[13] + a[8] * a[5] * a[14] - a[8] * a[6] * a[13] - a[12] * a[5] * a[10] + a[12] * a[6] * a[9];
		inv[1] = -a[1] * a[10] * a[15] + a[1] * a[11] * a[14] + a[9] * a[2] * a[15] - a[9] * a[3] * a[14] - a[13] * a[2] * a[11] + a[13] * a[3] * a[10];
		inv[5] = a[0] * a[10] * a[15] - a[0] * a[11] * a[14] - a[8] * a[2] * a[15] + a[8] * a[3] * a[14] + a[12] * a[2] * a[11] - a[12] * a[3] * a[10];
		inv[9] = -a[0] * a[9] * a[15] + a[0] * a[11] * a[13] + a[8] * a[1] * a[15] - a[8] * a[3] * a[13] - a[12] * a[1] * a[11] + a[12] * a[3] * a[9];
		inv[13] = a[0] * a[9] * a[14] - a[0] * a[10] * a[13] - a[8] * a[1] * a[14] + a[8] * a[2] * a[13] + a[12] * a[1] * a[10] - a[12] * a[2] * a[9];
		inv[2] = a[1] * a[6] * a[15] - a[1] * a[7] * a[14] - a[5] * a[2] * a[15] + a[5] * a[3] * a[14] + a[13] * a[2] * a[7] - a[13] * a[3] * a[6];
		inv[6] = -a[0] * a[6] * a[15] + a[0] * a[7] * a[14] + a[4] * a[2] * a[15] - a[4] * a[3] * a[14] - a[12] * a[2] * a[7] + a[12] * a[3] * a[6];
		inv[10] = a[0] * a[5] * a[15] - a[0] * a[7] * a[13] - a[4] * a[1] * a[15] + a[4] * a[3] * a[13] + a[12] * a[1] * a[7] - a[12] * a[3] * a[5];
		inv[14] = -a[0] * a[5] * a[14] + a[0] * a[6] * a[13] + a[4] * a[1] * a[14] - a[4] * a[2] * a[13] - a[12] * a[1] * a[6] + a[12] * a[2] * a[5];
		inv[3] = -a[1] * a[6] * a[11] + a[1] * a[7] * a[10] + a[5] * a[2] * a[11] - a[5] * a[3] * a[10] - a[9] * a[2] * a[7] + a[9] * a[3] * a[6];
		inv[7] = a[0] * a[6] * a[11] - a[0] * a[7] * a[10] - a[4] * a[2] * a[11] + a[4] * a[3] * a[10] + a[8] * a[2] * a[7] - a[8] * a[3] * a[6];
		inv[11] = -a[0] * a[5] * a[11] + a[0] * a[7] * a[9] + a[4] * a[1] * a[11] - a[4] * a[3] * a[9] - a[8] * a[1] * a[7] + a[8] * a[3] * a[5];
		inv[15] = a[0] * a[5] * a[10] - a[0] * a[6] * a[9] - a[4] * a[1] * a[10] + a[4] * a[2] * a[9] + a[8] * a[1] * a[6] - a[8] * a[2] * a[5];
		const double det = a[0] * inv[0] + a[1] * inv[4] + a[2] * inv[8] + a[3] * inv[12];
		const double id = det != 0.0 ? 1.0 / det : 0.0;
		// V is read row-major (the tensor as torch stores it); c2w[r][c] = inv(V)[c][r]
		for (int r = 0; r < 3; r++)
		{
			s[4 * r + 0] = inv[0 * 4 + r] * id;
			s[4 * r + 1] = inv[1 * 4 + r] * id;
			s[4 * r + 2] = (inv[2 * 4 + r] + inv[3 * 4 + r]) * id;
			s[4 * r + 3] = 0.0;
			s[12 + r] = campos[r];
		}
	}

	// the pixel's bilinear tap: corner (x0, y0) and the weights of (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1)
	struct EnvTap { int x0, y0; float w[4]; bool ok; };

	// In float64 from the pixel to the tap.  The coordinates are ill-conditioned in fp32 where it matters: acos(z / R) near the poles
	// (v loses ~sqrt(eps): 1e-4 of a texel row at 40 rows), u near the seam and the intersection point itself (60 world units
	// from a camera a few units from the origin); the tests hold the composite to 1e-5 of a float64 statement.  v = atan2(rho, z) is
	// acos(z / R) on the sphere, accurate everywhere and never NaN (the reference's fp32 acos(z / R) is NaN where z / R rounds above 1).
	__device__ __forceinline__ EnvTap env_tap(const double* s, const EnvView& v, int i, int j)
	{
		const double a = ((double)i + 0.5 - (double)v.cx) / (double)v.fx, b = ((double)j + 0.5 - (double)v.cy) / (double)v.fy;
		double d[3];
#pragma unroll
		for (int r = 0; r < 3; r++) d[r] = (a * s[4 * r] + b * s[4 * r + 1] + s[4 * r + 2]) - s[12 + r];
		const double n = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
		d[0] /= n; d[1] /= n; d[2] /= n;
		const double ox = s[12], oy = s[13], oz = s[14], R = (double)v.R;
		const double od = ox * d[0] + oy * d[1] + oz * d[2];
		const double dd = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
		const double oo = ox * ox + oy * oy + oz * oz;
		const double delta = od * od - dd * (oo - R * R);
		const double t = -od + sqrt(fmax(delta, 0.0)) / dd;
		const double X = ox + d[0] * t, Y = oy + d[1] * t, Z = oz + d[2] * t;
		const double PI = 3.14159265358979323846;
		const double u = atan2(Y, X) / (2.0 * PI) + 0.5;
		const double vv = atan2(sqrt(X * X + Y * Y), Z) / PI;
		// grid_sample's unnormalisation with align_corners = False ((g + 1) size - 1) / 2 with g = 2 u - 1, and its bilinear weights
		const double ix = u * (double)v.ew - 0.5, iy = vv * (double)v.eh - 0.5;
		EnvTap tp;
		tp.ok = isfinite(ix) && isfinite(iy);
		const double fx0 = tp.ok ? floor(ix) : 0.0, fy0 = tp.ok ? floor(iy) : 0.0;
		tp.x0 = (int)fx0; tp.y0 = (int)fy0;
		const double ax = ix - fx0, ay = iy - fy0;
		tp.w[0] = (float)((1.0 - ax) * (1.0 - ay));
		tp.w[1] = (float)(ax * (1.0 - ay));
		tp.w[2] = (float)((1.0 - ax) * ay);
		tp.w[3] = (float)(ax * ay);
		return tp;
	}

	__device__ __forceinline__ bool env_in(const EnvView& v, int x, int y) { return x >= 0 && x < v.ew && y >= 0 && y < v.eh; }

	__device__ __forceinline__ void env_sample(const EnvView& v, const float* __restrict__ env, const EnvTap& tp, float out[3])
	{
		out[0] = out[1] = out[2] = 0.f;
		if (!tp.ok) return;
		const size_t plane = (size_t)v.eh * v.ew;
#pragma unroll
		for (int k = 0; k < 4; k++)
		{
			const int x = tp.x0 + (k & 1), y = tp.y0 + (k >> 1);
			if (!env_in(v, x, y)) continue;
			const size_t o = (size_t)y * v.ew + x;
#pragma unroll
			for (int c = 0; c < 3; c++) out[c] += tp.w[k] * env[c * plane + o];
		}
	}

	__global__ void __launch_bounds__(ENV_THREADS) env_composite_kernel(EnvView v, const float* __restrict__ vm, const float* __restrict__ campos,
	                                                                    const float* __restrict__ env, const float* __restrict__ T,
	                                                                    const float* colour_in, float* colour_out)
	{
		__shared__ double s[16];
		if (threadIdx.x == 0) env_setup(vm, campos, s);
		__syncthreads();
		const int i = blockIdx.x * ENV_TILE + (threadIdx.x % ENV_TILE), j = blockIdx.y * ENV_TILE + (threadIdx.x / ENV_TILE);
		if (i >= v.W || j >= v.H) return;
		const EnvTap tp = env_tap(s, v, i, j);
		float e[3];
		env_sample(v, env, tp, e);
		const size_t HW = (size_t)v.H * v.W, p = (size_t)j * v.W + i;
		const float Tp = T[p];
#pragma unroll
		for (int c = 0; c < 3; c++) colour_out[c * HW + p] = colour_in[c * HW + p] + Tp * e[c];
	}

	template <bool ENV>
	__global__ void __launch_bounds__(ENV_THREADS) env_backward_kernel(EnvView v, const float* __restrict__ vm, const float* __restrict__ campos,
	                                                                   const float* __restrict__ env, const float* __restrict__ T,
	                                                                   const float* __restrict__ g, float* g_alpha, int accumulate_alpha,
	                                                                   float* g_env)
	{
		__shared__ double s[16];
		__shared__ int box[4];                       // the tile's texel window: x min, x max, y min, y max (inclusive, inside the map)
		__shared__ float win[ENV ? 3 * ENV_WIN : 1];
		if (threadIdx.x == 0)
		{
			env_setup(vm, campos, s);
			box[0] = INT_MAX; box[1] = INT_MIN; box[2] = INT_MAX; box[3] = INT_MIN;
		}
		__syncthreads();
		const int i = blockIdx.x * ENV_TILE + (threadIdx.x % ENV_TILE), j = blockIdx.y * ENV_TILE + (threadIdx.x / ENV_TILE);
		const bool valid = i < v.W && j < v.H;
		const size_t HW = (size_t)v.H * v.W, p = valid ? (size_t)j * v.W + i : 0;
		EnvTap tp{};
		float gw[3] = { 0.f, 0.f, 0.f };
		if (valid)
		{
			tp = env_tap(s, v, i, j);
			const float g0 = g[p], g1 = g[HW + p], g2 = g[2 * HW + p];
			if (g_alpha)
			{
				float e[3];
				env_sample(v, env, tp, e);
				const float ga = -(g0 * e[0] + g1 * e[1] + g2 * e[2]);
				g_alpha[p] = accumulate_alpha ? g_alpha[p] + ga : ga;
			}
			const float Tp = T[p];
			gw[0] = g0 * Tp; gw[1] = g1 * Tp; gw[2] = g2 * Tp;
		}
		if constexpr (!ENV) return;
		const bool scatter = valid && tp.ok;
		if (scatter)
		{
			const int xs = max(tp.x0, 0), xe = min(tp.x0 + 1, v.ew - 1), ys = max(tp.y0, 0), ye = min(tp.y0 + 1, v.eh - 1);
			if (xs <= xe && ys <= ye)
			{
				atomicMin(&box[0], xs); atomicMax(&box[1], xe);
				atomicMin(&box[2], ys); atomicMax(&box[3], ye);
			}
		}
		__syncthreads();
		const int bx0 = box[0], by0 = box[2];
		if (bx0 > box[1]) return;                    // the tile touches no texel (uniform)
		const int ww = box[1] - bx0 + 1, wh = box[3] - by0 + 1;
		const size_t plane = (size_t)v.eh * v.ew;
		if ((long long)ww * wh > ENV_WIN)
		{
			// wide window (near a pole, or across the seam with a tall tap): direct global atomics
			if (!scatter) return;
#pragma unroll
			for (int k = 0; k < 4; k++)
			{
				const int x = tp.x0 + (k & 1), y = tp.y0 + (k >> 1);
				if (!env_in(v, x, y)) continue;
				const size_t o = (size_t)y * v.ew + x;
#pragma unroll
				for (int c = 0; c < 3; c++) atomicAdd(&g_env[c * plane + o], gw[c] * tp.w[k]);
			}
			return;
		}
		const int area = ww * wh;
		for (int k = threadIdx.x; k < 3 * area; k += ENV_THREADS) win[k] = 0.f;
		__syncthreads();
		if (scatter)
		{
#pragma unroll
			for (int k = 0; k < 4; k++)
			{
				const int x = tp.x0 + (k & 1), y = tp.y0 + (k >> 1);
				if (!env_in(v, x, y)) continue;
				const int o = (y - by0) * ww + (x - bx0);
#pragma unroll
				for (int c = 0; c < 3; c++) atomicAdd(&win[c * area + o], gw[c] * tp.w[k]);
			}
		}
		__syncthreads();
		// flush: consecutive threads on consecutive texels of a window row (contiguous in the map); untouched texels hold exactly 0
		for (int k = threadIdx.x; k < 3 * area; k += ENV_THREADS)
		{
			const float val = win[k];
			if (val == 0.f) continue;
			const int c = k / area, r = k - c * area, y = r / ww, x = r - y * ww;
			atomicAdd(&g_env[c * plane + (size_t)(by0 + y) * v.ew + (bx0 + x)], val);
		}
	}
}

using namespace fdgs;

static int env_args(const char* fn, int32_t H, int32_t W, const float* viewmatrix, const float* campos, float fl_x, float fl_y,
                    const float* env, int32_t env_h, int32_t env_w, float radius, EnvView* v)
{
	if (H <= 0 || W <= 0 || H >= 16 * 65535 || env_h <= 0 || env_w <= 0 || (int64_t)env_h * env_w >= ((int64_t)1 << 31) ||
	    !(radius > 0.f) || fl_x == 0.f || fl_y == 0.f)
		return fail(FDGS_ERR_INVALID_ARG, "%s: bad image / map size, radius or focal length", fn);
	if (!viewmatrix || !campos || !env) return fail(FDGS_ERR_INVALID_ARG, "%s: missing pointer", fn);
	v->H = H; v->W = W; v->eh = env_h; v->ew = env_w; v->fx = fl_x; v->fy = fl_y; v->R = radius;
	return FDGS_OK;
}

extern "C" int fdgs_env_composite(int32_t H, int32_t W, const float* viewmatrix, const float* campos, float fl_x, float fl_y, float cx,
                                  float cy, const float* env, int32_t env_h, int32_t env_w, float radius, const float* T,
                                  const float* colour_in, float* colour_out, void* stream_v)
{
	EnvView v;
	const int rc = env_args("fdgs_env_composite", H, W, viewmatrix, campos, fl_x, fl_y, env, env_h, env_w, radius, &v);
	if (rc != FDGS_OK) return rc;
	if (!T || !colour_in || !colour_out) return fail(FDGS_ERR_INVALID_ARG, "fdgs_env_composite: missing pointer");
	v.cx = cx; v.cy = cy;
	hipLaunchKernelGGL(env_composite_kernel, dim3(div_up(W, ENV_TILE), div_up(H, ENV_TILE)), dim3(ENV_THREADS), 0, (hipStream_t)stream_v, v,
	                   viewmatrix, campos, env, T, colour_in, colour_out);
	return launched("fdgs_env_composite");
}

extern "C" int fdgs_env_composite_backward(int32_t H, int32_t W, const float* viewmatrix, const float* campos, float fl_x, float fl_y,
                                           float cx, float cy, const float* env, int32_t env_h, int32_t env_w, float radius, const float* T,
                                           const float* g_colour, float* g_alpha, int32_t accumulate_alpha, float* g_env,
                                           int32_t accumulate_env, void* stream_v)
{
	EnvView v;
	const int rc = env_args("fdgs_env_composite_backward", H, W, viewmatrix, campos, fl_x, fl_y, env, env_h, env_w, radius, &v);
	if (rc != FDGS_OK) return rc;
	if (!T || !g_colour) return fail(FDGS_ERR_INVALID_ARG, "fdgs_env_composite_backward: missing pointer");
	v.cx = cx; v.cy = cy;
	hipStream_t stream = (hipStream_t)stream_v;
	if (!g_alpha && !g_env) return FDGS_OK;
	const dim3 grid(div_up(W, ENV_TILE), div_up(H, ENV_TILE));
	if (g_env)
	{
		if (!accumulate_env) HIP_TRY(hipMemsetAsync(g_env, 0, (size_t)3 * env_h * env_w * sizeof(float), stream), "fdgs_env_composite_backward: hipMemsetAsync");
		hipLaunchKernelGGL(env_backward_kernel<true>, grid, dim3(ENV_THREADS), 0, stream, v, viewmatrix, campos, env, T, g_colour, g_alpha,
		                   accumulate_alpha, g_env);
	}
	else
		hipLaunchKernelGGL(env_backward_kernel<false>, grid, dim3(ENV_THREADS), 0, stream, v, viewmatrix, campos, env, T, g_colour, g_alpha,
		                   accumulate_alpha, g_env);
	return launched("fdgs_env_composite_backward");
}
