// mcmc.hip -- densification as Markov chain Monte Carlo (include/fdgs_mcmc.h) for gfx950: opacity-proportional sampling in fixed
// point, relocation of dead Gaussians, the per-step noise on the means and the opacity / scale regularisers.
//
// Per-Gaussian (or per-draw) streaming kernels, wave64, 256-thread workgroups, no LDS beyond the scans' and the reductions'.
//   weights    o -> 24-bit integer weight; inclusive prefix sums in uint64: local scan, scan of the workgroup sums, add (exact)
//   draw       one Philox4x32-10 block per draw, u = mulhi64(r64, total), binary search in the prefix, integer atomics for the counts
//   copy/zero  whole rows of a segment, as float4 where the segment allows
//   update     o' = 1 - (1 - o)^(1/N), the scale ratio o / D: float64 throughout (the alternating binomial sum cancels in float32);
//              cold, a few thousand rows per refinement
//   noise      the one kernel of this file that runs every step: 13 floats read, 4 written per Gaussian at rot_4d, one launch;
//              Sigma xi in float64, in fdgs_math.h's conventions (see the kernel)
//   regularise gradients added into the bucket, the term values from float64 partials summed in a fixed order
// Built with FP contraction off: the float32 chains (weights, Box-Muller) are one rounding per operation, as a numpy float32
// restatement computes them.
#pragma clang fp contract(off)
#include "fdgs_common.h"
#include "fdgs_math.h"
#include "philox.h"
#include "scan.h"
#include "../../include/fdgs_mcmc.h"
#include <cmath>

namespace fdgs
{
	constexpr int MCMC_THREADS = 256;
	constexpr int MCMC_MAX_SEG = 16;
	static_assert(MCMC_THREADS % WAVE == 0, "whole waves");

	// ---- weights and their prefix sums ----
	__global__ void __launch_bounds__(MCMC_THREADS) mcmc_weights_kernel(const int P, const float* __restrict__ opacity_raw, const float min_opacity,
	                                                                    uint8_t* __restrict__ alive, uint32_t* __restrict__ wq,
	                                                                    uint64_t* __restrict__ prefix, uint64_t* __restrict__ sums)
	{
		__shared__ uint64_t s_wave[MCMC_THREADS / WAVE];
		const int i = blockIdx.x * MCMC_THREADS + threadIdx.x;
		uint32_t w = 0u;
		if (i < P)
		{
			const float o = act_sigmoid(opacity_raw[i]);
			const bool live = o > min_opacity;
			w = live ? (uint32_t)rintf(o * 16777216.f) : 0u;
			alive[i] = live ? 1 : 0;
			wq[i] = w;
		}
		uint64_t total;
		const uint64_t before = block_rank<MCMC_THREADS>((uint64_t)w, s_wave, total);
		if (i < P) prefix[i] = before + w;
		if (threadIdx.x == 0) sums[blockIdx.x] = total;
	}
	// one workgroup: sums[0 .. nb) -> their exclusive scan, in place
	__global__ void __launch_bounds__(MCMC_THREADS) mcmc_scan_sums_kernel(const int nb, uint64_t* __restrict__ sums)
	{
		__shared__ uint64_t s_wave[MCMC_THREADS / WAVE];
		uint64_t carry = 0;
		for (int base = 0; base < nb; base += MCMC_THREADS)
		{
			const int b = base + (int)threadIdx.x;
			const uint64_t v = b < nb ? sums[b] : 0ull;
			uint64_t total;
			const uint64_t before = block_rank<MCMC_THREADS>(v, s_wave, total);
			if (b < nb) sums[b] = carry + before;
			carry += total;
		}
	}
	__global__ void __launch_bounds__(MCMC_THREADS) mcmc_add_sums_kernel(const int P, const uint64_t* __restrict__ sums, uint64_t* __restrict__ prefix)
	{
		const int i = blockIdx.x * MCMC_THREADS + threadIdx.x;
		if (i < P) prefix[i] += sums[blockIdx.x];
	}

	// ---- draws ----
	__global__ void __launch_bounds__(MCMC_THREADS) mcmc_draw_kernel(const int P, const int n, const uint64_t* __restrict__ prefix, const uint2 key,
	                                                                 const uint32_t stream_id, const uint32_t call_lo, const uint32_t call_hi,
	                                                                 int32_t* __restrict__ source, int32_t* __restrict__ counts,
	                                                                 uint32_t* __restrict__ words)
	{
		const int j = blockIdx.x * MCMC_THREADS + threadIdx.x;
		if (j >= n) return;
		const uint4 w = philox4x32_10(make_uint4((uint32_t)j, stream_id, call_lo, call_hi), key);
		if (words != nullptr) reinterpret_cast<uint4*>(words)[j] = w;
		const uint64_t total = prefix[P - 1];
		if (total == 0ull) { source[j] = -1; return; }
		const uint64_t r64 = ((uint64_t)w.x << 32) | (uint64_t)w.y;
		const uint64_t u = __umul64hi(r64, total);
		// the smallest i with prefix[i] > u: prefix[P - 1] = total > u, so there is one
		int lo = 0, hi = P - 1;
		while (lo < hi)
		{
			const int mid = lo + ((hi - lo) >> 1);
			if (prefix[mid] > u) hi = mid;
			else lo = mid + 1;
		}
		source[j] = lo;
		atomicAdd(&counts[lo], 1);
	}

	// ---- whole rows of one segment ----
	template <typename V>
	__global__ void __launch_bounds__(MCMC_THREADS) mcmc_copy_rows_kernel(const long long P, const int n, const int32_t* __restrict__ dst,
	                                                                      const int32_t* __restrict__ src, V* seg, const int row)
	{
		const long long q = (long long)blockIdx.x * MCMC_THREADS + threadIdx.x;
		if (q >= (long long)n * row) return;
		const int j = (int)(q / row), e = (int)(q - (long long)j * row);
		const long long d = dst[j], s = src[j];
		if (d < 0 || d >= P || s < 0 || s >= P) return;
		seg[d * row + e] = seg[s * row + e];
	}
	template <typename V>
	__global__ void __launch_bounds__(MCMC_THREADS) mcmc_zero_rows_kernel(const long long P, const int n, const int32_t* __restrict__ rows,
	                                                                      V* __restrict__ a, V* __restrict__ b, const int row, const V zero)
	{
		const long long q = (long long)blockIdx.x * MCMC_THREADS + threadIdx.x;
		if (q >= (long long)n * row) return;
		const int j = (int)(q / row), e = (int)(q - (long long)j * row);
		const long long d = rows[j];
		if (d < 0 || d >= P) return;
		a[d * row + e] = zero;
		if (b != nullptr) b[d * row + e] = zero;
	}

	// ---- opacity and scales of a Gaussian that stands for N copies ----
	// log(1 - sigmoid(x)) = -softplus(x), without the cancellation of 1 - o
	__device__ __forceinline__ double log_one_minus_sigmoid(const double x) { return x > 0.0 ? -(x + log1p(exp(-x))) : -log1p(exp(x)); }

	__global__ void __launch_bounds__(MCMC_THREADS) mcmc_update_kernel(const int n, const int dim4, const int32_t* __restrict__ rows,
	                                                                   const int32_t* __restrict__ count_of, const int32_t* __restrict__ counts,
	                                                                   float* __restrict__ opacity_raw, float* __restrict__ scaling_raw,
	                                                                   float* __restrict__ scaling_t_raw)
	{
		const int j = blockIdx.x * MCMC_THREADS + threadIdx.x;
		if (j >= n) return;
		const size_t i = (size_t)rows[j];
		const int drawn = counts[count_of[j]];
		if (drawn < 1) return;
		const int N = min(drawn + 1, FDGS_MCMC_MAX_MULTIPLICITY);
		const double x = (double)opacity_raw[i];
		const double o = 1.0 / (1.0 + exp(-x));
		const double op = -expm1(log_one_minus_sigmoid(x) / (double)N);      // 1 - (1 - o)^(1/N)
		// D = sum_k C(N, k + 1) (-1)^k op^(k + 1) / sqrt(k + 1); the binomials stay exact integers in float64 up to N = 51
		double D = 0.0, c = (double)N, p = op;
#pragma unroll 1
		for (int k = 0; k < N; k++)
		{
			const double term = c * p / sqrt((double)(k + 1));
			D += (k & 1) ? -term : term;
			c = c * (double)(N - k - 1) / (double)(k + 2);
			p *= op;
		}
		const double shift = log(o / D);
		for (int k = 0; k < 3; k++) scaling_raw[3 * i + k] = (float)((double)scaling_raw[3 * i + k] + shift);
		if (dim4) scaling_t_raw[i] = (float)((double)scaling_t_raw[i] + shift);
		const double oc = fmin(fmax(op, 0.005), 1.0 - 1.1920928955078125e-07);
		float raw = (float)log(oc / (1.0 - oc));
		// clamped from below: the nearest float32 logit of 0.005 activates to 0.0049999994, which the weights kernel would call dead
		// right after the relocation; the next values up (2^-21 apart: 2e-9 in opacity) until the float32 opacity exceeds 0.005
		if (op <= 0.005)
			for (int it = 0; it < 4 && !(act_sigmoid(raw) > 0.005f); it++) raw = nextafterf(raw, 0.f);
		opacity_raw[i] = raw;
	}

	// ---- the noise step ----
	struct NoiseArgs
	{
		int P;
		float *xyz, *t;
		const float *opacity, *scaling, *scaling_t, *rot, *rot_r;
		float scale;
		const float* xi_in;
		uint2 key;
		uint32_t stream_id, call_lo, call_hi;
		float* xi_out;
		uint32_t* words;
	};
	__device__ __forceinline__ float mcmc_unit(const uint32_t w) { return (float)((w >> 8) + 1u) * 5.9604644775390625e-08f; }   // (0, 1]

	__device__ __forceinline__ void mcmc_normalize(double* q)   // F.normalize, as act_normalize
	{
		const double inv = 1.0 / fmax(sqrt((q[0] * q[0] + q[1] * q[1]) + (q[2] * q[2] + q[3] * q[3])), 1e-12);
		q[0] *= inv; q[1] *= inv; q[2] *= inv; q[3] *= inv;
	}

	// MODE 0: gaussian_dim 3; 1: gaussian_dim 4 with an independent temporal axis; 2: rot_4d
	template <int MODE>
	__global__ void __launch_bounds__(MCMC_THREADS) mcmc_noise_kernel(const NoiseArgs a)
	{
		const int i = blockIdx.x * MCMC_THREADS + threadIdx.x;
		if (i >= a.P) return;
		float4 xi;
		if (a.xi_in != nullptr) xi = reinterpret_cast<const float4*>(a.xi_in)[i];
		else
		{
			const uint4 w = philox4x32_10(make_uint4((uint32_t)i, a.stream_id, a.call_lo, a.call_hi), a.key);
			if (a.words != nullptr) reinterpret_cast<uint4*>(a.words)[i] = w;
			const float r0 = sqrtf(-2.f * logf(mcmc_unit(w.x))), r1 = sqrtf(-2.f * logf(mcmc_unit(w.z)));
			float s0, c0, s1, c1;
			sincospif(2.f * mcmc_unit(w.y), &s0, &c0);
			sincospif(2.f * mcmc_unit(w.w), &s1, &c1);
			xi = make_float4(r0 * c0, r0 * s0, r1 * c1, r1 * s1);
		}
		if (a.xi_out != nullptr) reinterpret_cast<float4*>(a.xi_out)[i] = xi;
		// float64 from here: the float32 covariance helpers of fdgs_math.h carry a rotation that is orthonormal to 2^-24 only, and with
		// scales from e^-6 to e^2 in one Gaussian that leaks 1e-7 of the largest axis into every component of Sigma xi -- more than the
		// step itself where xi is nearly orthogonal to that axis.  Same conventions as quat_to_R / build_Ml_Mr (Sigma = M^T M, M = S R);
		// Sigma is never formed: delta = M^T (M xi).  The gate's argument is a difference of numbers near 1 scaled by 100.
		const double o = 1.0 / (1.0 + exp(-(double)a.opacity[i]));
		const double f = 1.0 / (1.0 + exp(-100.0 * ((1.0 - o) - 0.995))) * (double)a.scale;
		const float3 scf = ld3(a.scaling, i);
		const double s[4] = { exp((double)scf.x), exp((double)scf.y), exp((double)scf.z), MODE != 0 ? exp((double)a.scaling_t[i]) : 0.0 };
		const float4 qf = reinterpret_cast<const float4*>(a.rot)[i];
		double q[4] = { (double)qf.x, (double)qf.y, (double)qf.z, (double)qf.w };
		mcmc_normalize(q);
		const double x[4] = { (double)xi.x, (double)xi.y, (double)xi.z, (double)xi.w };
		double d[4] = { 0.0, 0.0, 0.0, 0.0 };
		if (MODE == 2)
		{
			const float4 qrf = reinterpret_cast<const float4*>(a.rot_r)[i];
			double qr[4] = { (double)qrf.x, (double)qrf.y, (double)qrf.z, (double)qrf.w };
			mcmc_normalize(qr);
			// columns of M_l and M_r (build_Ml_Mr): R = M_r M_l
			const double l[4][4] = { { q[0], q[1], -q[2], q[3] }, { -q[1], q[0], q[3], q[2] }, { q[2], -q[3], q[0], q[1] }, { -q[3], -q[2], -q[1], q[0] } };
			const double m[4][4] = { { qr[0], qr[1], -qr[2], -qr[3] }, { -qr[1], qr[0], qr[3], -qr[2] }, { qr[2], -qr[3], qr[0], -qr[1] }, { qr[3], qr[2], qr[1], qr[0] } };
			double z[4], y[4], v[4];
#pragma unroll
			for (int k = 0; k < 4; k++) z[k] = (l[0][k] * x[0] + l[1][k] * x[1]) + (l[2][k] * x[2] + l[3][k] * x[3]);      // M_l xi
#pragma unroll
			for (int k = 0; k < 4; k++) y[k] = s[k] * s[k] * ((m[0][k] * z[0] + m[1][k] * z[1]) + (m[2][k] * z[2] + m[3][k] * z[3]));   // S^2 R xi
#pragma unroll
			for (int k = 0; k < 4; k++) v[k] = (m[k][0] * y[0] + m[k][1] * y[1]) + (m[k][2] * y[2] + m[k][3] * y[3]);      // M_r^T .
#pragma unroll
			for (int k = 0; k < 4; k++) d[k] = (l[k][0] * v[0] + l[k][1] * v[1]) + (l[k][2] * v[2] + l[k][3] * v[3]);      // M_l^T .
		}
		else
		{
			// rows of the rotation (quat_to_R stores its transpose): Sigma = R S^2 R^T
			const double r = q[0], qx = q[1], qy = q[2], qz = q[3];
			const double R[3][3] = { { 1.0 - 2.0 * (qy * qy + qz * qz), 2.0 * (qx * qy - r * qz), 2.0 * (qx * qz + r * qy) },
			                         { 2.0 * (qx * qy + r * qz), 1.0 - 2.0 * (qx * qx + qz * qz), 2.0 * (qy * qz - r * qx) },
			                         { 2.0 * (qx * qz - r * qy), 2.0 * (qy * qz + r * qx), 1.0 - 2.0 * (qx * qx + qy * qy) } };
			double y[3];
#pragma unroll
			for (int k = 0; k < 3; k++) y[k] = s[k] * s[k] * (R[0][k] * x[0] + R[1][k] * x[1] + R[2][k] * x[2]);
#pragma unroll
			for (int k = 0; k < 3; k++) d[k] = R[k][0] * y[0] + R[k][1] * y[1] + R[k][2] * y[2];
			if (MODE == 1) d[3] = s[3] * s[3] * x[3];
		}
		const float3 p = ld3(a.xyz, i);
		st3(a.xyz, i, make_float3((float)((double)p.x + d[0] * f), (float)((double)p.y + d[1] * f), (float)((double)p.z + d[2] * f)));
		if (MODE != 0) a.t[i] = (float)((double)a.t[i] + d[3] * f);
	}

	// ---- the regularisers ----
	// sum over the workgroup, every wave's total through LDS and added in wave order: the same order on every run
	__device__ __forceinline__ double mcmc_block_sum(double v, double* red)
	{
#pragma unroll
		for (int d = WAVE / 2; d > 0; d >>= 1) v += __shfl_down(v, d);
		__syncthreads();
		if ((threadIdx.x & (WAVE - 1)) == 0) red[threadIdx.x / WAVE] = v;
		__syncthreads();
		double s = 0.0;
#pragma unroll
		for (int w = 0; w < MCMC_THREADS / WAVE; w++) s += red[w];
		return s;
	}

	struct RegArgs
	{
		int P;
		const float *opacity, *scaling, *scaling_t;
		double co, cs, cst;             // lambda_o / P, lambda_s / (3 P), lambda_st / P
		float *g_opacity, *g_scaling, *g_scaling_t;
	};
	// parts[m * nb + workgroup], m = 0 .. 2: sum o, sum exp(scaling), sum exp(scaling_t) of the workgroup's Gaussians
	__global__ void __launch_bounds__(MCMC_THREADS) mcmc_regularize_kernel(const RegArgs a, double* __restrict__ parts)
	{
		__shared__ double red[MCMC_THREADS / WAVE];
		const int i = blockIdx.x * MCMC_THREADS + threadIdx.x;
		double m[3] = { 0.0, 0.0, 0.0 };
		if (i < a.P)
		{
			// o (1 - o) = e / (1 + e)^2 with e = exp(-|x|): no 1 - o
			const double x = (double)a.opacity[i], e = exp(-fabs(x));
			m[0] = x >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e);
			a.g_opacity[i] += (float)(a.co * (e / ((1.0 + e) * (1.0 + e))));
#pragma unroll
			for (int k = 0; k < 3; k++)
			{
				const double s = exp((double)a.scaling[3 * (size_t)i + k]);
				m[1] += s;
				a.g_scaling[3 * (size_t)i + k] += (float)(a.cs * s);
			}
			if (a.cst > 0.0)
			{
				m[2] = exp((double)a.scaling_t[i]);
				a.g_scaling_t[i] += (float)(a.cst * m[2]);
			}
		}
#pragma unroll
		for (int k = 0; k < 3; k++)
		{
			const double s = mcmc_block_sum(m[k], red);
			if (threadIdx.x == 0) parts[(size_t)k * gridDim.x + blockIdx.x] = s;
		}
	}
	// one workgroup: thread t sums partials t, t + 256, ... in that order, then the workgroup's fixed-order sum
	__global__ void __launch_bounds__(MCMC_THREADS) mcmc_regularize_finish_kernel(const int nb, const double* __restrict__ parts, const double co,
	                                                                              const double cs, const double cst, double* __restrict__ terms)
	{
		__shared__ double red[MCMC_THREADS / WAVE];
		const double coef[3] = { co, cs, cst };
#pragma unroll
		for (int k = 0; k < 3; k++)
		{
			double v = 0.0;
			for (int b = threadIdx.x; b < nb; b += MCMC_THREADS) v += parts[(size_t)k * nb + b];
			const double s = mcmc_block_sum(v, red);
			if (threadIdx.x == 0) terms[k] = coef[k] * s;
		}
	}

	// the segments of a bucket of P rows: where each starts (in floats) and whether float4 accesses fit
	struct McmcSegs { int n; long long start[MCMC_MAX_SEG]; int row[MCMC_MAX_SEG]; };
	static inline bool vec4_fits(const void* base, const long long start, const int row)
	{
		return row % 4 == 0 && start % 4 == 0 && (reinterpret_cast<uintptr_t>(base) & 15) == 0;
	}
}

extern "C" size_t fdgs_mcmc_weights_scratch_bytes(int32_t P)
{
	return fdgs::align_up((size_t)fdgs::div_up(P > 0 ? P : 1, fdgs::MCMC_THREADS) * sizeof(uint64_t));
}

extern "C" int fdgs_mcmc_weights(int32_t P, const float* opacity_raw, float min_opacity, uint8_t* alive, uint32_t* wq, uint64_t* prefix,
                                 void* scratch, void* stream_v)
{
	using namespace fdgs;
	if (P < 1) return fail(FDGS_ERR_INVALID_ARG, "fdgs_mcmc_weights: P=%d is below 1", P);
	if (!opacity_raw || !alive || !wq || !prefix || !scratch)
		return fail(FDGS_ERR_INVALID_ARG, "fdgs_mcmc_weights: opacity_raw / alive / wq / prefix / scratch must not be NULL");
	hipStream_t stream = (hipStream_t)stream_v;
	const int nb = div_up(P, MCMC_THREADS);
	uint64_t* sums = (uint64_t*)scratch;
	hipLaunchKernelGGL(mcmc_weights_kernel, dim3(nb), dim3(MCMC_THREADS), 0, stream, P, opacity_raw, min_opacity, alive, wq, prefix, sums);
	if (nb > 1)
	{
		hipLaunchKernelGGL(mcmc_scan_sums_kernel, dim3(1), dim3(MCMC_THREADS), 0, stream, nb, sums);
		hipLaunchKernelGGL(mcmc_add_sums_kernel, dim3(nb), dim3(MCMC_THREADS), 0, stream, P, sums, prefix);
	}
	return launched("fdgs_mcmc_weights");
}

extern "C" int fdgs_mcmc_draw(int32_t P, int32_t n_draws, const uint64_t* prefix, uint64_t seed, uint32_t stream_id, uint64_t call,
                              int32_t* source, int32_t* counts, uint32_t* words, void* stream_v)
{
	using namespace fdgs;
	if (P < 1 || n_draws < 0) return fail(FDGS_ERR_INVALID_ARG, "fdgs_mcmc_draw: P=%d is below 1 or n_draws=%d is negative", P, n_draws);
	if (!prefix || !counts || (n_draws > 0 && !source)) return fail(FDGS_ERR_INVALID_ARG, "fdgs_mcmc_draw: prefix / counts / source must not be NULL");
	hipStream_t stream = (hipStream_t)stream_v;
	HIP_TRY(hipMemsetAsync(counts, 0, (size_t)P * sizeof(int32_t), stream), "fdgs_mcmc_draw: hipMemsetAsync");
	if (n_draws == 0) return FDGS_OK;
	hipLaunchKernelGGL(mcmc_draw_kernel, dim3(div_up(n_draws, MCMC_THREADS)), dim3(MCMC_THREADS), 0, stream, P, n_draws, prefix, philox_key(seed),
	                   stream_id, (uint32_t)(call & 0xffffffffull), (uint32_t)(call >> 32), source, counts, words);
	return launched("fdgs_mcmc_draw");
}

namespace fdgs
{
	// the argument checks and the segment table of the two row functions; 0 or the error code
	static int mcmc_segments(const char* fn, int num_segments, const int32_t* row_floats, long long P, int n, bool pointers, McmcSegs& s)
	{
		if (num_segments < 1 || num_segments > MCMC_MAX_SEG || !row_floats)
			return fail(FDGS_ERR_INVALID_ARG, "%s: num_segments=%d is outside 1..%d or row_floats is NULL", fn, num_segments, MCMC_MAX_SEG);
		if (P < 1 || P >= (1ll << 31) || n < 0) return fail(FDGS_ERR_INVALID_ARG, "%s: P=%lld is outside [1, 2^31) or n=%d is negative", fn, P, n);
		if (n > 0 && !pointers) return fail(FDGS_ERR_INVALID_ARG, "%s: the row lists and the bucket must not be NULL", fn);
		s.n = num_segments;
		long long at = 0;
		for (int k = 0; k < num_segments; k++)
		{
			if (row_floats[k] <= 0) return fail(FDGS_ERR_INVALID_ARG, "%s: row_floats[%d]=%d is not positive", fn, k, row_floats[k]);
			s.start[k] = at; s.row[k] = row_floats[k];
			at += P * row_floats[k];
		}
		return FDGS_OK;
	}
	static inline unsigned row_blocks(int n, int row) { return (unsigned)(((long long)n * row + MCMC_THREADS - 1) / MCMC_THREADS); }
}

extern "C" int fdgs_mcmc_copy_rows(int32_t num_segments, const int32_t* row_floats, int64_t P, int32_t n, const int32_t* dst, const int32_t* src,
                                   float* flat, void* stream_v)
{
	using namespace fdgs;
	McmcSegs s;
	if (const int rc = mcmc_segments("fdgs_mcmc_copy_rows", num_segments, row_floats, (long long)P, n, dst && src && flat, s)) return rc;
	if (n == 0) return FDGS_OK;
	hipStream_t stream = (hipStream_t)stream_v;
	for (int k = 0; k < s.n; k++)
	{
		float* seg = flat + s.start[k];
		if (vec4_fits(flat, s.start[k], s.row[k]))
			hipLaunchKernelGGL(mcmc_copy_rows_kernel<float4>, dim3(row_blocks(n, s.row[k] / 4)), dim3(MCMC_THREADS), 0, stream, (long long)P, n, dst, src,
			                   reinterpret_cast<float4*>(seg), s.row[k] / 4);
		else
			hipLaunchKernelGGL(mcmc_copy_rows_kernel<float>, dim3(row_blocks(n, s.row[k])), dim3(MCMC_THREADS), 0, stream, (long long)P, n, dst, src, seg,
			                   s.row[k]);
	}
	return launched("fdgs_mcmc_copy_rows");
}

extern "C" int fdgs_mcmc_zero_rows(int32_t num_segments, const int32_t* row_floats, int64_t P, int32_t n, const int32_t* rows, float* a, float* b,
                                   void* stream_v)
{
	using namespace fdgs;
	McmcSegs s;
	if (const int rc = mcmc_segments("fdgs_mcmc_zero_rows", num_segments, row_floats, (long long)P, n, rows && a, s)) return rc;
	if (n == 0) return FDGS_OK;
	hipStream_t stream = (hipStream_t)stream_v;
	for (int k = 0; k < s.n; k++)
	{
		float* sa = a + s.start[k];
		float* sb = b ? b + s.start[k] : nullptr;
		if (vec4_fits(a, s.start[k], s.row[k]) && vec4_fits(b, s.start[k], s.row[k]))
			hipLaunchKernelGGL(mcmc_zero_rows_kernel<float4>, dim3(row_blocks(n, s.row[k] / 4)), dim3(MCMC_THREADS), 0, stream, (long long)P, n, rows,
			                   reinterpret_cast<float4*>(sa), reinterpret_cast<float4*>(sb), s.row[k] / 4, make_float4(0.f, 0.f, 0.f, 0.f));
		else
			hipLaunchKernelGGL(mcmc_zero_rows_kernel<float>, dim3(row_blocks(n, s.row[k])), dim3(MCMC_THREADS), 0, stream, (long long)P, n, rows, sa, sb,
			                   s.row[k], 0.f);
	}
	return launched("fdgs_mcmc_zero_rows");
}

extern "C" int fdgs_mcmc_update(int32_t n, int32_t gaussian_dim, const int32_t* rows, const int32_t* count_of, const int32_t* counts,
                                float* opacity_raw, float* scaling_raw, float* scaling_t_raw, void* stream_v)
{
	using namespace fdgs;
	if (n < 0) return fail(FDGS_ERR_INVALID_ARG, "fdgs_mcmc_update: n=%d is negative", n);
	if (gaussian_dim != 3 && gaussian_dim != 4) return fail(FDGS_ERR_INVALID_ARG, "fdgs_mcmc_update: gaussian_dim=%d is neither 3 nor 4", gaussian_dim);
	if (n == 0) return FDGS_OK;
	if (!rows || !count_of || !counts || !opacity_raw || !scaling_raw || (gaussian_dim == 4 && !scaling_t_raw))
		return fail(FDGS_ERR_INVALID_ARG, "fdgs_mcmc_update: rows / count_of / counts / opacity_raw / scaling_raw (and scaling_t_raw with gaussian_dim == 4) must not be NULL");
	hipLaunchKernelGGL(mcmc_update_kernel, dim3(div_up(n, MCMC_THREADS)), dim3(MCMC_THREADS), 0, (hipStream_t)stream_v, n, gaussian_dim == 4 ? 1 : 0, rows,
	                   count_of, counts, opacity_raw, scaling_raw, scaling_t_raw);
	return launched("fdgs_mcmc_update");
}

extern "C" int fdgs_mcmc_noise(int32_t P, int32_t gaussian_dim, int32_t rot_4d, float* xyz, float* t, const float* opacity_raw,
                               const float* scaling_raw, const float* scaling_t_raw, const float* rotation_raw, const float* rotation_r_raw,
                               float scale, const float* xi_in, uint64_t seed, uint32_t stream_id, uint64_t call, float* xi_out, uint32_t* words,
                               void* stream_v)
{
	using namespace fdgs;
	if (P < 0) return fail(FDGS_ERR_INVALID_ARG, "fdgs_mcmc_noise: P=%d is negative", P);
	if (gaussian_dim != 3 && gaussian_dim != 4) return fail(FDGS_ERR_INVALID_ARG, "fdgs_mcmc_noise: gaussian_dim=%d is neither 3 nor 4", gaussian_dim);
	if (rot_4d && gaussian_dim != 4) return fail(FDGS_ERR_INVALID_ARG, "fdgs_mcmc_noise: rot_4d needs gaussian_dim == 4, got %d", gaussian_dim);
	if (P == 0) return FDGS_OK;
	if (!xyz || !opacity_raw || !scaling_raw || !rotation_raw) return fail(FDGS_ERR_INVALID_ARG, "fdgs_mcmc_noise: xyz / opacity_raw / scaling_raw / rotation_raw must not be NULL");
	if (gaussian_dim == 4 && (!t || !scaling_t_raw)) return fail(FDGS_ERR_INVALID_ARG, "fdgs_mcmc_noise: gaussian_dim == 4 needs t and scaling_t_raw");
	if (rot_4d && !rotation_r_raw) return fail(FDGS_ERR_INVALID_ARG, "fdgs_mcmc_noise: rot_4d needs rotation_r_raw");
	// (the quaternions are read as float4 from wherever their segment starts, as the rasterizer's kernels read them)
	if ((reinterpret_cast<uintptr_t>(xi_in) | reinterpret_cast<uintptr_t>(xi_out) | reinterpret_cast<uintptr_t>(words)) & 15)
		return fail(FDGS_ERR_INVALID_ARG, "fdgs_mcmc_noise: xi_in / xi_out / words must be 16-byte aligned");
	NoiseArgs a;
	a.P = P; a.xyz = xyz; a.t = t; a.opacity = opacity_raw; a.scaling = scaling_raw; a.scaling_t = scaling_t_raw; a.rot = rotation_raw;
	a.rot_r = rotation_r_raw; a.scale = scale; a.xi_in = xi_in; a.key = philox_key(seed); a.stream_id = stream_id;
	a.call_lo = (uint32_t)(call & 0xffffffffull); a.call_hi = (uint32_t)(call >> 32); a.xi_out = xi_out; a.words = words;
	const dim3 grid(div_up(P, MCMC_THREADS)), block(MCMC_THREADS);
	hipStream_t stream = (hipStream_t)stream_v;
	if (rot_4d) hipLaunchKernelGGL(mcmc_noise_kernel<2>, grid, block, 0, stream, a);
	else if (gaussian_dim == 4) hipLaunchKernelGGL(mcmc_noise_kernel<1>, grid, block, 0, stream, a);
	else hipLaunchKernelGGL(mcmc_noise_kernel<0>, grid, block, 0, stream, a);
	return launched("fdgs_mcmc_noise");
}

extern "C" int32_t fdgs_mcmc_regularize_num_partials(int32_t P) { return 3 * fdgs::div_up(P > 0 ? P : 1, fdgs::MCMC_THREADS); }

extern "C" int fdgs_mcmc_regularize(int32_t P, const float* opacity_raw, const float* scaling_raw, const float* scaling_t_raw, float lambda_o,
                                    float lambda_s, float lambda_st, float* dL_dopacity, float* dL_dscales, float* dL_dscales_t, double* partials,
                                    double* terms, void* stream_v)
{
	using namespace fdgs;
	if (P < 1) return fail(FDGS_ERR_INVALID_ARG, "fdgs_mcmc_regularize: P=%d is below 1", P);
	if (!opacity_raw || !scaling_raw || !dL_dopacity || !dL_dscales || !partials)
		return fail(FDGS_ERR_INVALID_ARG, "fdgs_mcmc_regularize: opacity_raw / scaling_raw / dL_dopacity / dL_dscales / partials must not be NULL");
	if (lambda_st > 0.f && (!scaling_t_raw || !dL_dscales_t))
		return fail(FDGS_ERR_INVALID_ARG, "fdgs_mcmc_regularize: lambda_st > 0 needs scaling_t_raw and dL_dscales_t");
	RegArgs a;
	a.P = P; a.opacity = opacity_raw; a.scaling = scaling_raw; a.scaling_t = scaling_t_raw;
	a.co = (double)lambda_o / (double)P; a.cs = (double)lambda_s / (3.0 * (double)P); a.cst = lambda_st > 0.f ? (double)lambda_st / (double)P : 0.0;
	a.g_opacity = dL_dopacity; a.g_scaling = dL_dscales; a.g_scaling_t = dL_dscales_t;
	const int nb = div_up(P, MCMC_THREADS);
	hipStream_t stream = (hipStream_t)stream_v;
	hipLaunchKernelGGL(mcmc_regularize_kernel, dim3(nb), dim3(MCMC_THREADS), 0, stream, a, partials);
	if (terms != nullptr) hipLaunchKernelGGL(mcmc_regularize_finish_kernel, dim3(1), dim3(MCMC_THREADS), 0, stream, nb, partials, a.co, a.cs, a.cst, terms);
	return launched("fdgs_mcmc_regularize");
}
