// depth_loss.hip -- depth supervision on the rendered depth map (gfx950): Pearson and scale-and-shift-invariant L1 against a depth
// prior, and a normal map from the depth, each with its gradient to the renderer's `depth` and `alpha`.
//
//   z      = depth / alpha  where alpha >= alpha_min  (alpha == NULL: z = depth, every pixel passes)
//   valid  = the alpha test, mask == NULL or mask > 0 and -- for the losses -- a finite prior > 0
//   pearson  L = 1 - rho,  rho = cov(z, p) / (sigma_z sigma_p) over the valid pixels (population moments)
//   ssi      L = sum |s z + b - p| / n,  (s, b) = argmin sum (s z + b - p)^2, constants for the gradient (a detached alignment)
//   normals  n = (b x a) / |b x a|,  a = P(u+1,v) - P(u-1,v),  b = P(u,v+1) - P(u,v-1),  P = ((u+.5-cx)/fl_x z, (v+.5-cy)/fl_y z, z)
//
// The losses: one reduction pass writes six float64 moments per workgroup, a one-workgroup finish sums them in a fixed order and
// derives means, variances, rho and (s, b) on the device, one elementwise pass writes the gradient (and, for ssi, the |r| partials
// that a second finish sums).  No atomics anywhere: every result is bitwise reproducible.  The moments and the per-pixel gradient are
// float64: the variances are differences of sums over 1.4 M pixels, the Pearson gradient is a difference of two terms that cancel as
// rho -> 1, and the passes are bound by the float32 images they read either way.
// The normals: a 16 x 16 tile per workgroup with z and its validity in LDS, a one-pixel halo forward; the backward is a GATHER with a
// two-pixel halo -- a pixel sums what the normals of its four neighbours owe it (its own normal does not depend on its own z),
// each recomputed from the tile.  float32, in the operation order of the statement above (built with FP contraction off).
#include "fdgs_common.h"
#include <math.h>

namespace fdgs
{
	constexpr int DL_THREADS = 256;
	constexpr int DL_ITEMS = 4;                          // pixels per thread: a workgroup owns 1024 consecutive pixels
	constexpr int DL_CHUNK = DL_THREADS * DL_ITEMS;
	constexpr int DL_MOMENTS = 6;                        // n, sum z, sum p, sum z^2, sum z p, sum p^2
	constexpr int DL_STATS = 16;                         // doubles at the head of the partials buffer (layout: ST_* below)
	enum { ST_N = 0, ST_ZM, ST_PM, ST_CZ, ST_CP, ST_S, ST_B, ST_INV_N, ST_DEGENERATE, ST_RHO };
	constexpr int DN_TILE = 16;

	struct DepthArgs
	{
		int H, W, HW;
		const float* depth;
		const float* alpha;
		const float* mask;
		float alpha_min;
	};

	struct DepthGradArgs
	{
		float* d_depth;
		float* d_alpha;
		const float* g_upstream;
		float scale;
		int accumulate;
	};

	__device__ __forceinline__ bool depth_valid(const DepthArgs& a, int i)
	{
		if (a.alpha && !(a.alpha[i] >= a.alpha_min)) return false;
		if (a.mask && !(a.mask[i] > 0.f)) return false;
		return true;
	}
	__device__ __forceinline__ bool prior_valid(float p) { return p > 0.f && p < INFINITY; }    // a NaN fails both

	// fixed-order sum over the workgroup's DL_THREADS threads; every thread gets the total
	__device__ __forceinline__ double block_sum_d(double v, double* red)
	{
#pragma unroll
		for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
		__syncthreads();                                  // the previous call's readers are done with red[]
		if ((threadIdx.x & (WAVE - 1)) == 0) red[threadIdx.x / WAVE] = v;
		__syncthreads();
		return (red[0] + red[1]) + (red[2] + red[3]);
	}

	__device__ __forceinline__ void write_grad(float* g, int i, float v, int accumulate)
	{
		if (g) g[i] = accumulate ? g[i] + v : v;
	}

	// ---- pass 1: the six masked moments, one set of partials per workgroup: parts[m * nb + workgroup] ----
	__global__ void __launch_bounds__(DL_THREADS) depth_moments_kernel(DepthArgs a, const float* __restrict__ prior, int nb,
	                                                                   double* __restrict__ parts)
	{
		__shared__ double red[DL_THREADS / WAVE];
		double m[DL_MOMENTS] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
#pragma unroll
		for (int k = 0; k < DL_ITEMS; k++)
		{
			const int i = blockIdx.x * DL_CHUNK + k * DL_THREADS + threadIdx.x;        // HW < 2^30: no overflow
			if (i >= a.HW || !depth_valid(a, i)) continue;
			const float pf = prior[i];
			if (!prior_valid(pf)) continue;
			const double z = a.alpha ? (double)a.depth[i] / (double)a.alpha[i] : (double)a.depth[i];
			const double p = (double)pf;
			m[0] += 1.0; m[1] += z; m[2] += p; m[3] += z * z; m[4] += z * p; m[5] += p * p;
		}
#pragma unroll
		for (int j = 0; j < DL_MOMENTS; j++)
		{
			const double s = block_sum_d(m[j], red);
			if (threadIdx.x == 0) parts[(size_t)j * nb + blockIdx.x] = s;
		}
	}

	// ---- finish, one workgroup.  stage 0: moments -> stats (and the Pearson value); stage 1: the ssi |r| partials -> its value.
	// out: 4 floats { loss, n, rho (pearson) or s (ssi), 0 (pearson) or b (ssi) }
	__global__ void __launch_bounds__(DL_THREADS) depth_finish_kernel(int nb, const double* __restrict__ parts, int mode, int stage,
	                                                                  double* __restrict__ stats, float* __restrict__ out)
	{
		__shared__ double red[DL_THREADS / WAVE];
		if (stage == 1)
		{
			double v = 0.0;
			for (int i = threadIdx.x; i < nb; i += DL_THREADS) v += parts[i];
			const double tot = block_sum_d(v, red);
			if (threadIdx.x == 0) out[0] = (float)(tot * stats[ST_INV_N]);
			return;
		}
		double tot[DL_MOMENTS];
		for (int j = 0; j < DL_MOMENTS; j++)
		{
			double v = 0.0;
			for (int i = threadIdx.x; i < nb; i += DL_THREADS) v += parts[(size_t)j * nb + i];
			tot[j] = block_sum_d(v, red);
		}
		if (threadIdx.x != 0) return;
		const double n = tot[0];
		double zm = 0.0, pm = 0.0, vz = 0.0, vp = 0.0, cov = 0.0;
		bool degenerate = n < 2.0;
		if (!degenerate)
		{
			zm = tot[1] / n; pm = tot[2] / n;
			vz = tot[3] / n - zm * zm; vp = tot[5] / n - pm * pm; cov = tot[4] / n - zm * pm;
			degenerate = !(vz > 1e-12 * fmax(1.0, zm * zm)) || !(vp > 1e-12 * fmax(1.0, pm * pm));
		}
		double rho = 0.0, s = 0.0, b = 0.0, cz = 0.0, cp = 0.0, inv_n = 0.0;
		if (!degenerate)
		{
			const double sz = sqrt(vz), sp = sqrt(vp);
			rho = cov / (sz * sp);
			// d(1 - rho) / dz_i = -((p_i - pm) - rho (sp / sz) (z_i - zm)) / (n sz sp) = cz (z_i - zm) + cp (p_i - pm)
			cp = -1.0 / (n * sz * sp);
			cz = rho * (sp / sz) / (n * sz * sp);
			s = cov / vz;
			b = pm - s * zm;
			inv_n = 1.0 / n;
		}
		stats[ST_N] = n; stats[ST_ZM] = zm; stats[ST_PM] = pm; stats[ST_CZ] = cz; stats[ST_CP] = cp; stats[ST_S] = s; stats[ST_B] = b;
		stats[ST_INV_N] = inv_n; stats[ST_DEGENERATE] = degenerate ? 1.0 : 0.0; stats[ST_RHO] = rho;
		out[1] = (float)n;
		if (mode == FDGS_DEPTH_PEARSON) { out[0] = degenerate ? 1.f : (float)(1.0 - rho); out[2] = (float)rho; out[3] = 0.f; }
		else { out[0] = 0.f; out[2] = (float)s; out[3] = (float)b; }
	}

	// ---- pass 2: the gradient to depth and alpha; for ssi also the |r| partials, rparts[workgroup] ----
	__global__ void __launch_bounds__(DL_THREADS) depth_apply_kernel(DepthArgs a, const float* __restrict__ prior, int mode,
	                                                                 const double* __restrict__ stats, DepthGradArgs g,
	                                                                 double* __restrict__ rparts)
	{
		__shared__ double red[DL_THREADS / WAVE];
		const bool degenerate = stats[ST_DEGENERATE] != 0.0;
		const double zm = stats[ST_ZM], pm = stats[ST_PM], cz = stats[ST_CZ], cp = stats[ST_CP], s = stats[ST_S], b = stats[ST_B];
		const double inv_n = stats[ST_INV_N];
		const double up = (double)g.scale * (g.g_upstream ? (double)g.g_upstream[0] : 1.0);
		double racc = 0.0;
#pragma unroll
		for (int k = 0; k < DL_ITEMS; k++)
		{
			const int i = blockIdx.x * DL_CHUNK + k * DL_THREADS + threadIdx.x;
			if (i >= a.HW) continue;
			float gd = 0.f, ga = 0.f;                          // an invalid pixel gets exactly 0
			const float pf = prior[i];
			if (!degenerate && depth_valid(a, i) && prior_valid(pf))
			{
				const double A = a.alpha ? (double)a.alpha[i] : 1.0;
				const double z = (double)a.depth[i] / A, p = (double)pf;
				double gz;
				if (mode == FDGS_DEPTH_PEARSON) gz = cz * (z - zm) + cp * (p - pm);
				else
				{
					const double r = s * z + b - p;
					racc += fabs(r);
					gz = r > 0.0 ? s * inv_n : (r < 0.0 ? -s * inv_n : 0.0);
				}
				gz *= up;
				gd = (float)(gz / A);                          // dz/dD = 1 / A
				ga = (float)(-gz * z / A);                     // dz/dA = -D / A^2
			}
			write_grad(g.d_depth, i, gd, g.accumulate);
			write_grad(g.d_alpha, i, ga, g.accumulate);
		}
		if (mode == FDGS_DEPTH_SSI)
		{
			const double tot = block_sum_d(racc, red);
			if (threadIdx.x == 0) rparts[blockIdx.x] = tot;
		}
	}

	// ---- normals from depth ----
	struct NormalCam { float fl_x, fl_y, cx, cy; const float* vm; };      // vm: world_view_transform as the rasterizer takes it, or NULL

	// z and its validity for the tile at (x0, y0) with a HALO-pixel ring, outside the image: invalid
	template <int HALO>
	__device__ __forceinline__ void load_depth_tile(const DepthArgs& a, int x0, int y0, float* __restrict__ z, unsigned char* __restrict__ ok)
	{
		constexpr int S = DN_TILE + 2 * HALO;
		for (int t = threadIdx.y * DN_TILE + threadIdx.x; t < S * S; t += DN_TILE * DN_TILE)
		{
			const int gx = x0 + t % S - HALO, gy = y0 + t / S - HALO;
			bool v = gx >= 0 && gx < a.W && gy >= 0 && gy < a.H;
			float zz = 0.f;
			if (v)
			{
				const int i = gy * a.W + gx;
				v = depth_valid(a, i);
				if (v) zz = a.alpha ? a.depth[i] / a.alpha[i] : a.depth[i];
			}
			z[t] = zz;
			ok[t] = v ? 1 : 0;
		}
		__syncthreads();
	}

	struct NormalAt { bool ok; float ax, ay, az, bx, by, bz, nx, ny, nz, len2; };

	// the stencil of the pixel (u, v), which sits at index c of a tile of row stride S: a, b, N = b x a and |N|^2
	template <int S>
	__device__ __forceinline__ NormalAt normal_at(const float* __restrict__ z, const unsigned char* __restrict__ ok, int c, int u, int v,
	                                              const NormalCam& cam)
	{
		NormalAt r;
		r.ok = ok[c] && ok[c - 1] && ok[c + 1] && ok[c - S] && ok[c + S];
		if (!r.ok) return r;
		const float zl = z[c - 1], zr = z[c + 1], zu = z[c - S], zd = z[c + S];
		const float x = ((float)u + 0.5f - cam.cx) / cam.fl_x, xl = ((float)(u - 1) + 0.5f - cam.cx) / cam.fl_x;
		const float xr = ((float)(u + 1) + 0.5f - cam.cx) / cam.fl_x;
		const float y = ((float)v + 0.5f - cam.cy) / cam.fl_y, yu = ((float)(v - 1) + 0.5f - cam.cy) / cam.fl_y;
		const float yd = ((float)(v + 1) + 0.5f - cam.cy) / cam.fl_y;
		r.ax = xr * zr - xl * zl; r.ay = y * zr - y * zl; r.az = zr - zl;
		r.bx = x * zd - x * zu; r.by = yd * zd - yu * zu; r.bz = zd - zu;
		r.nx = r.by * r.az - r.bz * r.ay;
		r.ny = r.bz * r.ax - r.bx * r.az;
		r.nz = r.bx * r.ay - r.by * r.ax;
		r.len2 = (r.nx * r.nx + r.ny * r.ny) + r.nz * r.nz;
		r.ok = r.len2 > 1e-20f;
		return r;
	}

	__global__ void __launch_bounds__(DN_TILE * DN_TILE) depth_normals_kernel(DepthArgs a, NormalCam cam, float* __restrict__ normals,
	                                                                          unsigned char* __restrict__ valid)
	{
		constexpr int S = DN_TILE + 2;
		__shared__ float z[S * S];
		__shared__ unsigned char ok[S * S];
		const int x0 = blockIdx.x * DN_TILE, y0 = blockIdx.y * DN_TILE;
		load_depth_tile<1>(a, x0, y0, z, ok);
		const int u = x0 + threadIdx.x, v = y0 + threadIdx.y;
		if (u >= a.W || v >= a.H) return;
		const NormalAt r = normal_at<S>(z, ok, (threadIdx.y + 1) * S + threadIdx.x + 1, u, v, cam);
		float nx = 0.f, ny = 0.f, nz = 0.f;
		if (r.ok)
		{
			const float len = sqrtf(r.len2);
			nx = r.nx / len; ny = r.ny / len; nz = r.nz / len;
			if (cam.vm)
			{
				// view -> world: the transposed rotation of the world-to-view matrix, which is stored transposed
				const float* m = cam.vm;
				const float wx = (m[0] * nx + m[1] * ny) + m[2] * nz;
				const float wy = (m[4] * nx + m[5] * ny) + m[6] * nz;
				const float wz = (m[8] * nx + m[9] * ny) + m[10] * nz;
				nx = wx; ny = wy; nz = wz;
			}
		}
		const size_t i = (size_t)v * a.W + u;
		normals[i] = nx; normals[(size_t)a.HW + i] = ny; normals[2 * (size_t)a.HW + i] = nz;
		valid[i] = r.ok ? 1 : 0;
	}

	// dL/da and dL/db of the normal centred at (u, v) (index c of the tile), 0 where that normal is invalid
	template <int S>
	__device__ __forceinline__ void centre_grads(const float* __restrict__ z, const unsigned char* __restrict__ ok, int c, int u, int v,
	                                             const DepthArgs& a, const NormalCam& cam, const float* __restrict__ dL_dn, float* da, float* db)
	{
		da[0] = da[1] = da[2] = db[0] = db[1] = db[2] = 0.f;
		if (u < 0 || u >= a.W || v < 0 || v >= a.H) return;
		const NormalAt r = normal_at<S>(z, ok, c, u, v, cam);
		if (!r.ok) return;
		const size_t i = (size_t)v * a.W + u;
		float gx = dL_dn[i], gy = dL_dn[(size_t)a.HW + i], gz = dL_dn[2 * (size_t)a.HW + i];
		if (cam.vm)
		{
			const float* m = cam.vm;       // world -> view: the transpose of the forward's rotation
			const float vx = (m[0] * gx + m[4] * gy) + m[8] * gz;
			const float vy = (m[1] * gx + m[5] * gy) + m[9] * gz;
			const float vz = (m[2] * gx + m[6] * gy) + m[10] * gz;
			gx = vx; gy = vy; gz = vz;
		}
		const float len = sqrtf(r.len2);
		const float nx = r.nx / len, ny = r.ny / len, nz = r.nz / len;
		const float dot = (nx * gx + ny * gy) + nz * gz;
		// d / dN of N / |N|
		const float lx = (gx - nx * dot) / len, ly = (gy - ny * dot) / len, lz = (gz - nz * dot) / len;
		// N = b x a:  dL/da = dL/dN x b,  dL/db = a x dL/dN
		da[0] = ly * r.bz - lz * r.by; da[1] = lz * r.bx - lx * r.bz; da[2] = lx * r.by - ly * r.bx;
		db[0] = r.ay * lz - r.az * ly; db[1] = r.az * lx - r.ax * lz; db[2] = r.ax * ly - r.ay * lx;
	}

	__global__ void __launch_bounds__(DN_TILE * DN_TILE) depth_normals_bwd_kernel(DepthArgs a, NormalCam cam, const float* __restrict__ dL_dn,
	                                                                              DepthGradArgs g)
	{
		constexpr int S = DN_TILE + 4;
		__shared__ float z[S * S];
		__shared__ unsigned char ok[S * S];
		const int x0 = blockIdx.x * DN_TILE, y0 = blockIdx.y * DN_TILE;
		load_depth_tile<2>(a, x0, y0, z, ok);
		const int u = x0 + threadIdx.x, v = y0 + threadIdx.y;
		if (u >= a.W || v >= a.H) return;
		const int c = (threadIdx.y + 2) * S + threadIdx.x + 2;
		const int i = v * a.W + u;
		float gd = 0.f, ga = 0.f;
		if (ok[c])
		{
			// this pixel is the right neighbour of (u-1, v), the left one of (u+1, v), the lower one of (u, v-1), the upper one of (u, v+1):
			// z enters P(u, v) = ray z, and P enters +a, -a, +b, -b of those four normals
			float da[3], db[3], t[3], acc[3];
			centre_grads<S>(z, ok, c - 1, u - 1, v, a, cam, dL_dn, da, db);
			acc[0] = da[0]; acc[1] = da[1]; acc[2] = da[2];
			centre_grads<S>(z, ok, c + 1, u + 1, v, a, cam, dL_dn, da, db);
			acc[0] -= da[0]; acc[1] -= da[1]; acc[2] -= da[2];
			centre_grads<S>(z, ok, c - S, u, v - 1, a, cam, dL_dn, t, db);
			acc[0] += db[0]; acc[1] += db[1]; acc[2] += db[2];
			centre_grads<S>(z, ok, c + S, u, v + 1, a, cam, dL_dn, t, db);
			acc[0] -= db[0]; acc[1] -= db[1]; acc[2] -= db[2];
			const float x = ((float)u + 0.5f - cam.cx) / cam.fl_x, y = ((float)v + 0.5f - cam.cy) / cam.fl_y;
			float gz = (x * acc[0] + y * acc[1]) + acc[2];
			gz *= g.g_upstream ? g.scale * g.g_upstream[0] : g.scale;
			if (a.alpha)
			{
				const float A = a.alpha[i];
				gd = gz / A;
				ga = -gz * z[c] / A;
			}
			else gd = gz;
		}
		write_grad(g.d_depth, i, gd, g.accumulate);
		write_grad(g.d_alpha, i, ga, g.accumulate);
	}

	// FDGS_OK: the arguments are fine and `a` is filled in; otherwise the entry point `fn` fails with what is wrong with them
	static int depth_args(const char* fn, const fdgs_depth_in* in, DepthArgs& a)
	{
		if (!in) return fail(FDGS_ERR_INVALID_ARG, "%s: in must not be NULL", fn);
		CHECK_STRUCT_IN(fn, in, fdgs_depth_in);
		if (in->H <= 0 || in->W <= 0 || (int64_t)in->H * in->W >= ((int64_t)1 << 30)) return fail(FDGS_ERR_INVALID_ARG, "%s: need H, W > 0 and H * W < 2^30", fn);
		if (in->H >= DN_TILE * 65535) return fail(FDGS_ERR_INVALID_ARG, "%s: H must be below 16 * 65535", fn);
		if (!in->depth) return fail(FDGS_ERR_INVALID_ARG, "%s: depth must not be NULL", fn);
		if (in->alpha && !(in->alpha_min > 0.f && in->alpha_min < INFINITY)) return fail(FDGS_ERR_INVALID_ARG, "%s: alpha_min must be positive and finite (z = depth / alpha)", fn);
		a.H = in->H; a.W = in->W; a.HW = in->H * in->W;
		a.depth = in->depth; a.alpha = in->alpha; a.mask = in->mask; a.alpha_min = in->alpha_min;
		return FDGS_OK;
	}

	// `grads` may be NULL (no gradient); g is filled in either way
	static int depth_grad_args(const char* fn, const fdgs_depth_in* in, const fdgs_depth_grads* grads, DepthGradArgs& g)
	{
		g.d_depth = g.d_alpha = nullptr; g.g_upstream = nullptr; g.scale = 1.f; g.accumulate = 0;
		if (!grads) return FDGS_OK;
		CHECK_STRUCT_IN(fn, grads, fdgs_depth_grads);
		if (grads->d_alpha && !in->alpha) return fail(FDGS_ERR_INVALID_ARG, "%s: d_alpha without alpha", fn);
		g.d_depth = grads->d_depth; g.d_alpha = grads->d_alpha; g.g_upstream = grads->g_upstream; g.scale = grads->scale;
		g.accumulate = grads->accumulate != 0;
		return FDGS_OK;
	}
}

using namespace fdgs;

extern "C" int fdgs_depth_loss_num_partials(int32_t H, int32_t W)
{
	if (H <= 0 || W <= 0 || (int64_t)H * W >= ((int64_t)1 << 30)) return 0;
	return DL_STATS + (DL_MOMENTS + 1) * div_up(H * W, DL_CHUNK);
}

extern "C" int fdgs_depth_loss(const fdgs_depth_in* in, const float* prior, int32_t mode, const fdgs_depth_grads* grads, double* partials,
                               float* out, void* stream_v)
{
	DepthArgs a;
	DepthGradArgs g;
	if (const int rc = depth_args("fdgs_depth_loss", in, a)) return rc;
	if (const int rc = depth_grad_args("fdgs_depth_loss", in, grads, g)) return rc;
	if (mode != FDGS_DEPTH_PEARSON && mode != FDGS_DEPTH_SSI) return fail(FDGS_ERR_INVALID_ARG, "fdgs_depth_loss: mode must be FDGS_DEPTH_PEARSON or FDGS_DEPTH_SSI");
	if (!prior || !partials || !out) return fail(FDGS_ERR_INVALID_ARG, "fdgs_depth_loss: prior, partials and out must not be NULL");
	hipStream_t stream = (hipStream_t)stream_v;
	const int nb = div_up(a.HW, DL_CHUNK);
	double* stats = partials;
	double* parts = partials + DL_STATS;
	double* rparts = parts + (size_t)DL_MOMENTS * nb;
	hipLaunchKernelGGL(depth_moments_kernel, dim3(nb), dim3(DL_THREADS), 0, stream, a, prior, nb, parts);
	hipLaunchKernelGGL(depth_finish_kernel, dim3(1), dim3(DL_THREADS), 0, stream, nb, parts, mode, 0, stats, out);
	if (mode == FDGS_DEPTH_SSI || g.d_depth || g.d_alpha)
		hipLaunchKernelGGL(depth_apply_kernel, dim3(nb), dim3(DL_THREADS), 0, stream, a, prior, mode, stats, g, rparts);
	if (mode == FDGS_DEPTH_SSI)
		hipLaunchKernelGGL(depth_finish_kernel, dim3(1), dim3(DL_THREADS), 0, stream, nb, rparts, mode, 1, stats, out);
	return launched("fdgs_depth_loss");
}

static int normal_cam_args(const char* fn, float fl_x, float fl_y, float cx, float cy, const float* viewmatrix, NormalCam& cam)
{
	if (!(fl_x > 0.f && fl_x < INFINITY) || !(fl_y > 0.f && fl_y < INFINITY)) return fail(FDGS_ERR_INVALID_ARG, "%s: fl_x and fl_y must be positive and finite", fn);
	if (!(fabsf(cx) < INFINITY) || !(fabsf(cy) < INFINITY)) return fail(FDGS_ERR_INVALID_ARG, "%s: cx and cy must be finite", fn);
	cam.fl_x = fl_x; cam.fl_y = fl_y; cam.cx = cx; cam.cy = cy; cam.vm = viewmatrix;
	return FDGS_OK;
}

extern "C" int fdgs_depth_normals(const fdgs_depth_in* in, float fl_x, float fl_y, float cx, float cy, const float* viewmatrix,
                                  float* normals, uint8_t* valid, void* stream)
{
	DepthArgs a;
	NormalCam cam;
	if (const int rc = depth_args("fdgs_depth_normals", in, a)) return rc;
	if (const int rc = normal_cam_args("fdgs_depth_normals", fl_x, fl_y, cx, cy, viewmatrix, cam)) return rc;
	if (!normals || !valid) return fail(FDGS_ERR_INVALID_ARG, "fdgs_depth_normals: normals and valid must not be NULL");
	hipLaunchKernelGGL(depth_normals_kernel, dim3(div_up(a.W, DN_TILE), div_up(a.H, DN_TILE)), dim3(DN_TILE, DN_TILE), 0, (hipStream_t)stream,
	                   a, cam, normals, valid);
	return launched("fdgs_depth_normals");
}

extern "C" int fdgs_depth_normals_backward(const fdgs_depth_in* in, float fl_x, float fl_y, float cx, float cy, const float* viewmatrix,
                                           const float* dL_dnormals, const fdgs_depth_grads* grads, void* stream)
{
	DepthArgs a;
	DepthGradArgs g;
	NormalCam cam;
	if (const int rc = depth_args("fdgs_depth_normals_backward", in, a)) return rc;
	if (const int rc = normal_cam_args("fdgs_depth_normals_backward", fl_x, fl_y, cx, cy, viewmatrix, cam)) return rc;
	if (!grads) return fail(FDGS_ERR_INVALID_ARG, "fdgs_depth_normals_backward: grads must not be NULL");
	if (const int rc = depth_grad_args("fdgs_depth_normals_backward", in, grads, g)) return rc;
	if (!dL_dnormals) return fail(FDGS_ERR_INVALID_ARG, "fdgs_depth_normals_backward: dL_dnormals must not be NULL");
	if (!g.d_depth && !g.d_alpha) return FDGS_OK;
	hipLaunchKernelGGL(depth_normals_bwd_kernel, dim3(div_up(a.W, DN_TILE), div_up(a.H, DN_TILE)), dim3(DN_TILE, DN_TILE), 0,
	                   (hipStream_t)stream, a, cam, dL_dnormals, g);
	return launched("fdgs_depth_normals_backward");
}
