// time_slice.hip -- a 4D model at one timestamp as a compact set of 3D Gaussians (fdgs_time_slice) for gfx950.
//
// At time t a 4D Gaussian IS a 3D Gaussian: the conditional mean and covariance (rot_4d; forward.cu:279-352) or the plain ones with
// the 1-D temporal marginal (forward.cu:242-276, 431-437), the opacity times that marginal, and an SH row whose two time blocks are
// folded in with cos(2 pi k dt / T).  preprocess_fwd.hip computes the same per view and keeps it to itself; here it is computed once,
// for the Gaussians that pass the forward's own temporal cull (marginal > 0.05) only, and written out compacted in ascending index.
//
// Three launches, no atomics, the output order is the input order:
//   1 flags    one lane per Gaussian: the 17 geometry floats -> the cull decision; one ballot word per wave, one count per workgroup
//   2 scan     one workgroup: exclusive scan of the workgroup counts (in place), n_live -- compact.h's, shared with the mesh kernels.
//              Launches 1 and 3 are not on compact.h's frame: their ranks come from the saved ballot words, not from a block scan,
//              so the write pass neither derives the cull decision again nor touches a culled Gaussian.
//   3 write    one lane per Gaussian: rank = workgroup start + the earlier waves' counts + the ballot bits below the lane; the
//              geometry is derived again (68 bytes read per Gaussian instead of 44 written and read back) and stored at the rank;
//              then the wave walks its OUTPUT rows linearly -- they are contiguous -- and folds the SH rows of its live Gaussians,
//              16 bytes per lane where the rows allow it.  SH rows of culled Gaussians are never read.
// Rows at or beyond `capacity` are never written; n_live always is.
//
// Bit-exactness: slice_geometry is the forward's gaussian_at_time (fdgs_math.h) for raw parameters, put together from the same shared
// pieces -- activate, cov4_build / cov3_build, temporal_marginal -- in the same order and built with the same flags (no FP contraction,
// no SLP vectorizer): where the forward keeps a Gaussian, mean, covariance and opacity here are the forward's, bit for bit
// (tests/test_gpu_slice.py).  Nothing of a culled Gaussian is stored.
#pragma clang fp contract(off)
#include "fdgs_common.h"
#include "fdgs_math.h"
#include "sh_eval.h"
#include "compact.h"

namespace fdgs
{
	struct SliceArgs
	{
		int P, D, D_t, M, capacity;
		const float *means3D, *shs, *opacities, *ts, *scales, *scales_t, *rotations, *rotations_r;
		float scale_modifier, prefilter_var, timestamp, time_duration;
		int rot_4d, force_sh_3d;
		int32_t* index; float *xyz, *cov3D, *opacity, *out_shs, *out_scales, *out_rotations;
		unsigned long long* masks;   // [SLICE_WAVES * workgroups] the waves' ballots of the flag pass
		uint32_t* counts;            // [workgroups] live Gaussians per workgroup -> (scan) the workgroup's first rank
	};

	// gaussian_at_time (fdgs_math.h) for raw parameters and gaussian_dim == 4, from the same shared pieces in the same order.  Kept as
	// its own function: calling gaussian_at_time here compiles to the same operations per Gaussian, but its per-branch activations and
	// `if (alive)` form cost slice_write_kernel 14 registers (62 -> 76).  A culled Gaussian's fields are computed and never stored.
	__device__ __forceinline__ void slice_geometry(const SliceArgs& a, const int idx, GaussAtTime& o)
	{
		o.mean = ld3(a.means3D, idx);
		o.opacity = act_sigmoid(a.opacities[idx]);
		float unused;
		float3 sc = ld3(a.scales, idx);
		float4 q = reinterpret_cast<const float4*>(a.rotations)[idx];
		activate(sc, q, &unused);
		const float mod = a.scale_modifier;
		float marginal_t;
		if (a.rot_4d)
		{
			float sct = a.scales_t[idx];
			float4 qr = reinterpret_cast<const float4*>(a.rotations_r)[idx];
			activate(sct, qr, &unused);
			const float dt = a.timestamp - a.ts[idx];
			const M4 Sigma = cov4_build(sc, sct, mod, q, qr).Sigma;
			const float cov_t = Sigma.c[3][3];
			marginal_t = temporal_marginal(dt, cov_t, a.prefilter_var);
			const float c12[3] = { Sigma.c[0][3], Sigma.c[1][3], Sigma.c[2][3] };
			o.cov[0] = Sigma.c[0][0] - (c12[0] * c12[0]) / cov_t;
			o.cov[1] = Sigma.c[0][1] - (c12[1] * c12[0]) / cov_t;
			o.cov[2] = Sigma.c[0][2] - (c12[2] * c12[0]) / cov_t;
			o.cov[3] = Sigma.c[1][1] - (c12[1] * c12[1]) / cov_t;
			o.cov[4] = Sigma.c[1][2] - (c12[2] * c12[1]) / cov_t;
			o.cov[5] = Sigma.c[2][2] - (c12[2] * c12[2]) / cov_t;
			o.mean.x += c12[0] / cov_t * dt;
			o.mean.y += c12[1] / cov_t * dt;
			o.mean.z += c12[2] / cov_t * dt;
		}
		else
		{
			const M3 Sigma = cov3_build(sc, mod, q).Sigma;
			o.cov[0] = Sigma.c[0][0]; o.cov[1] = Sigma.c[0][1]; o.cov[2] = Sigma.c[0][2];
			o.cov[3] = Sigma.c[1][1]; o.cov[4] = Sigma.c[1][2]; o.cov[5] = Sigma.c[2][2];
			marginal_t = temporal_marginal(a.ts[idx] - a.timestamp, expf(a.scales_t[idx]) * mod, a.prefilter_var);
		}
		o.alive = marginal_t > 0.05;
		o.opacity *= marginal_t;
	}

	constexpr int SLICE_THREADS = COMPACT_THREADS;       // one count per workgroup, as compact_scan takes them
	constexpr int SLICE_WAVES = SLICE_THREADS / WAVE;
	static_assert(WAVE == 64 && SLICE_THREADS % WAVE == 0, "one 64-bit ballot word per wave");

	__global__ void __launch_bounds__(SLICE_THREADS) slice_flag_kernel(const SliceArgs a)
	{
		__shared__ uint32_t s_cnt[SLICE_WAVES];
		const int tid_g = blockIdx.x * blockDim.x + threadIdx.x;
		const bool valid = tid_g < a.P;
		const int idx = valid ? tid_g : a.P - 1;   // out-of-range lanes shadow the last Gaussian and count for nothing
		const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
		GaussAtTime g;
		slice_geometry(a, idx, g);
		const unsigned long long mask = __ballot(valid && g.alive);
		if (lane == 0)
		{
			a.masks[(size_t)blockIdx.x * SLICE_WAVES + wave] = mask;
			s_cnt[wave] = (uint32_t)__popcll(mask);
		}
		__syncthreads();
		if (threadIdx.x == 0)
		{
			uint32_t total = 0;
#pragma unroll
			for (int w = 0; w < SLICE_WAVES; w++) total += s_cnt[w];
			a.counts[blockIdx.x] = total;
		}
	}

	// ---- cov3D = R diag(s^2) R^T: cyclic Jacobi on the symmetric 3x3 (double: the result is as good as its fp32 rounding) ----
	template <int p, int q, int r>
	__device__ __forceinline__ void jacobi_rotate(double (&A)[3][3], double (&V)[3][3])
	{
		const double apq = A[p][q];
		if (apq == 0.0) return;
		const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
		const double t = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));   // the smaller root: |angle| <= pi / 4
		const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
		const double arp = c * A[r][p] - s * A[r][q], arq = s * A[r][p] + c * A[r][q];
		A[p][p] -= t * apq; A[q][q] += t * apq;
		A[p][q] = 0.0; A[q][p] = 0.0;
		A[r][p] = arp; A[p][r] = arp; A[r][q] = arq; A[q][r] = arq;
#pragma unroll
		for (int k = 0; k < 3; k++)
		{
			const double vp = c * V[k][p] - s * V[k][q], vq = s * V[k][p] + c * V[k][q];
			V[k][p] = vp; V[k][q] = vq;
		}
	}
	// scales (square roots of the eigenvalues, floored at 1e-15: their logarithm is finite) and the unit quaternion (w, x, y, z) of the
	// eigenvector matrix in the convention of quat_to_R / the reference's build_rotation.  A product of plane rotations: det = +1.
	__device__ inline void slice_decompose(const float* cov, float* scales, float4& quat)
	{
		double A[3][3] = { { cov[0], cov[1], cov[2] }, { cov[1], cov[3], cov[4] }, { cov[2], cov[4], cov[5] } };
		double V[3][3] = { { 1.0, 0.0, 0.0 }, { 0.0, 1.0, 0.0 }, { 0.0, 0.0, 1.0 } };
#pragma unroll 1
		for (int sweep = 0; sweep < 8; sweep++)
		{
			const double off = fabs(A[0][1]) + fabs(A[0][2]) + fabs(A[1][2]);
			if (!(off > 1e-20 * (fabs(A[0][0]) + fabs(A[1][1]) + fabs(A[2][2])))) break;   // (also NaN)
			jacobi_rotate<0, 1, 2>(A, V);
			jacobi_rotate<0, 2, 1>(A, V);
			jacobi_rotate<1, 2, 0>(A, V);
		}
#pragma unroll
		for (int k = 0; k < 3; k++) scales[k] = fmaxf((float)sqrt(fmax(A[k][k], 0.0)), 1e-15f);
		const double tr = V[0][0] + V[1][1] + V[2][2];
		double w, x, y, z;
		if (tr >= V[0][0] && tr >= V[1][1] && tr >= V[2][2])
		{
			w = 0.5 * sqrt(fmax(1.0 + tr, 0.0));
			const double f = 0.25 / w;
			x = (V[2][1] - V[1][2]) * f; y = (V[0][2] - V[2][0]) * f; z = (V[1][0] - V[0][1]) * f;
		}
		else if (V[0][0] >= V[1][1] && V[0][0] >= V[2][2])
		{
			x = 0.5 * sqrt(fmax(1.0 + V[0][0] - V[1][1] - V[2][2], 0.0));
			const double f = 0.25 / x;
			w = (V[2][1] - V[1][2]) * f; y = (V[0][1] + V[1][0]) * f; z = (V[0][2] + V[2][0]) * f;
		}
		else if (V[1][1] >= V[2][2])
		{
			y = 0.5 * sqrt(fmax(1.0 - V[0][0] + V[1][1] - V[2][2], 0.0));
			const double f = 0.25 / y;
			w = (V[0][2] - V[2][0]) * f; x = (V[0][1] + V[1][0]) * f; z = (V[1][2] + V[2][1]) * f;
		}
		else
		{
			z = 0.5 * sqrt(fmax(1.0 - V[0][0] - V[1][1] + V[2][2], 0.0));
			const double f = 0.25 / z;
			w = (V[1][0] - V[0][1]) * f; x = (V[0][2] + V[2][0]) * f; y = (V[1][2] + V[2][1]) * f;
		}
		double inv = 1.0 / sqrt((w * w + x * x) + (y * y + z * z));
		if (!(inv < 1e300)) { w = 1.0; x = 0.0; y = 0.0; z = 0.0; inv = 1.0; }   // a covariance with NaN / inf in it
		if (w < 0.0) inv = -inv;
		quat = make_float4((float)(w * inv), (float)(x * inv), (float)(y * inv), (float)(z * inv));
	}

	// VEC = floats per lane and access of the SH fold (4: rows of whole, 16-byte aligned float4s)
	template <int VEC>
	__global__ void __launch_bounds__(SLICE_THREADS) slice_write_kernel(const SliceArgs a)
	{
		// the wave's live Gaussians in rank order: lane of the Gaussian, its two time factors
		__shared__ int s_src[SLICE_WAVES][WAVE];
		__shared__ float s_t1[SLICE_WAVES][WAVE], s_t2[SLICE_WAVES][WAVE];
		const int tid_g = blockIdx.x * blockDim.x + threadIdx.x;
		const int idx = tid_g < a.P ? tid_g : a.P - 1;
		const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
		unsigned long long mask = 0ull;
		uint32_t rank0 = a.counts[blockIdx.x];
#pragma unroll
		for (int w = 0; w < SLICE_WAVES; w++)
		{
			const unsigned long long m = a.masks[(size_t)blockIdx.x * SLICE_WAVES + w];
			if (w < wave) rank0 += (uint32_t)__popcll(m);
			if (w == wave) mask = m;
		}
		const bool live = (mask >> lane) & 1ull;   // (never set for a lane beyond P)
		const int r_in = __popcll(mask & ((1ull << lane) - 1ull));
		const ShPlan plan = sh_plan(a.D, a.D_t, 4, a.force_sh_3d, a.M);
		if (live)
		{
			GaussAtTime g;
			slice_geometry(a, idx, g);
			const size_t r = (size_t)rank0 + (size_t)r_in;
			if (r < (size_t)a.capacity)
			{
				a.index[r] = idx;
				st3(a.xyz, r, g.mean);
#pragma unroll
				for (int k = 0; k < 6; k++) a.cov3D[6 * r + k] = g.cov[k];
				a.opacity[r] = g.opacity;
				if (a.out_scales != nullptr)
				{
					float s[3];
					float4 q;
					slice_decompose(g.cov, s, q);
					a.out_scales[3 * r + 0] = s[0]; a.out_scales[3 * r + 1] = s[1]; a.out_scales[3 * r + 2] = s[2];
					a.out_rotations[4 * r + 0] = q.x; a.out_rotations[4 * r + 1] = q.y;
					a.out_rotations[4 * r + 2] = q.z; a.out_rotations[4 * r + 3] = q.w;
				}
			}
			// the forward's time factors (sh_eval.h; dir_t = ts - timestamp in fp32 as in preprocess_fwd.hip)
			const float dir_t = a.ts[idx] - a.timestamp;
			s_src[wave][r_in] = lane;
			s_t1[wave][r_in] = plan.nblocks > 1 ? sh_time_factor(1, dir_t, a.time_duration) : 0.f;
			s_t2[wave][r_in] = plan.nblocks > 2 ? sh_time_factor(2, dir_t, a.time_duration) : 0.f;
		}
		// wave-private LDS rows, one wave's LDS operations execute in order: only the compiler must keep the order
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

		// ---- the SH fold: the wave's output rows [rank0, rank0 + n) are one contiguous run of n * 48 floats ----
		const int n = __popcll(mask);
		constexpr int RC = 48 / VEC;               // accesses per row
		const int nact = 3 * plan.ncoef0;          // floats of block 0 the active degree reads; the rest of the row is zero
		const int g0 = blockIdx.x * blockDim.x + wave * WAVE;
		const size_t row_floats = (size_t)3 * a.M;
		RowWalk w(lane, RC);                       // access e = lane, lane + 64, ...  ->  (row w.g of the wave, position w.q of the row)
		for (int e = lane; e < n * RC; e += WAVE)
		{
			const size_t r = (size_t)rank0 + (size_t)w.g;
			const int f0 = VEC * w.q;              // first float of this access in the row
			if (r < (size_t)a.capacity)
			{
				const float* src = a.shs + (size_t)(g0 + s_src[wave][w.g]) * row_floats + f0;
				float* dst = a.out_shs + r * 48 + f0;
				const float t1 = s_t1[wave][w.g], t2 = s_t2[wave][w.g];
				if constexpr (VEC == 4)
				{
					float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
					if (f0 < nact)
					{
						v = *reinterpret_cast<const float4*>(src);   // (3 M is a multiple of 4 and f0 < 3 M: within the row)
						if (plan.nblocks > 1)
						{
							const float4 c1 = *reinterpret_cast<const float4*>(src + 48);
							v = make_float4(v.x + t1 * c1.x, v.y + t1 * c1.y, v.z + t1 * c1.z, v.w + t1 * c1.w);
						}
						if (plan.nblocks > 2)
						{
							const float4 c2 = *reinterpret_cast<const float4*>(src + 96);
							v = make_float4(v.x + t2 * c2.x, v.y + t2 * c2.y, v.z + t2 * c2.z, v.w + t2 * c2.w);
						}
						// an access that straddles the end of the active coefficients (degree 0, 2): what lies beyond is not data
						if (f0 + 1 >= nact) v.y = 0.f;
						if (f0 + 2 >= nact) v.z = 0.f;
						if (f0 + 3 >= nact) v.w = 0.f;
					}
					*reinterpret_cast<float4*>(dst) = v;
				}
				else
				{
					float v = 0.f;
					if (f0 < nact)
					{
						v = src[0];
						if (plan.nblocks > 1) v = v + t1 * src[48];
						if (plan.nblocks > 2) v = v + t2 * src[96];
					}
					dst[0] = v;
				}
			}
			w.step();
		}
	}

	size_t time_slice_scratch_bytes(int P)
	{
		const size_t nb = (size_t)div_up(P > 0 ? P : 1, SLICE_THREADS);
		return align_up(nb * SLICE_WAVES * sizeof(unsigned long long)) + align_up(nb * sizeof(uint32_t));
	}

	hipError_t launch_time_slice(const fdgs_slice_in& in, const fdgs_slice_out& out, void* scratch, hipStream_t stream)
	{
		if (in.P <= 0) return hipMemsetAsync(out.n_live, 0, sizeof(int32_t), stream);
		const int nb = div_up(in.P, SLICE_THREADS);
		SliceArgs a;
		a.P = in.P; a.D = in.D; a.D_t = in.D_t; a.M = in.M; a.capacity = out.capacity;
		a.means3D = in.means3D; a.shs = in.shs; a.opacities = in.opacities; a.ts = in.ts; a.scales = in.scales; a.scales_t = in.scales_t;
		a.rotations = in.rotations; a.rotations_r = in.rotations_r;
		a.scale_modifier = in.scale_modifier; a.prefilter_var = in.prefilter_var; a.timestamp = in.timestamp; a.time_duration = in.time_duration;
		a.rot_4d = in.rot_4d != 0; a.force_sh_3d = in.force_sh_3d != 0;
		a.index = out.index; a.xyz = out.xyz; a.cov3D = out.cov3D; a.opacity = out.opacity; a.out_shs = out.shs;
		a.out_scales = out.scales; a.out_rotations = out.rotations;
		a.masks = reinterpret_cast<unsigned long long*>(scratch);
		a.counts = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(scratch) + align_up((size_t)nb * SLICE_WAVES * sizeof(unsigned long long)));
		hipLaunchKernelGGL(slice_flag_kernel, dim3(nb), dim3(SLICE_THREADS), 0, stream, a);
		compact_scan(ScanJob{ a.counts, nb, 1u, out.n_live }, stream);
		const bool vec = (reinterpret_cast<uintptr_t>(in.shs) & 15) == 0 && (reinterpret_cast<uintptr_t>(out.shs) & 15) == 0 && (3 * in.M) % 4 == 0;
		if (vec) hipLaunchKernelGGL(slice_write_kernel<4>, dim3(nb), dim3(SLICE_THREADS), 0, stream, a);
		else hipLaunchKernelGGL(slice_write_kernel<1>, dim3(nb), dim3(SLICE_THREADS), 0, stream, a);
		return hipGetLastError();
	}
}
