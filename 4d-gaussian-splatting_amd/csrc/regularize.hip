// regularize.hip -- the reference trainer's loss terms besides L1 + SSIM (train.py:119-159), forward and backward (gfx950).
//
//   rigid   L_rigid  = sum_ij exp(-100 d2_ij) |v_nbr(i,j) - v_i| / k / P      (the k-NN of the means: knn.hip, fdgs_knn_query)
//   motion  L_motion = mean_i |v_i|
//   mask    L_opa    = mean(-(1 - gt_alpha_mask) log(1 - clamp(alpha, 1e-6, 1 - 1e-6)))
// with the velocity v = Sigma[0:3,3] / Sigma[3,3] * dt, dt = (t + 0.1f) - t: the conditional mean shift of the 4D Gaussian
// (scene/gaussian_model.py:34-47, 247-251), Sigma from fdgs_math.h's cov4_build: the call the preprocess and the time slice make.
// Every sum is a fixed-order reduction of per-workgroup partials (no float atomics), and the rigid term's neighbour-side gradient
// is GATHERED through a reverse-neighbour list -- the (neighbour, pair) table sorted stably by neighbour with the library's radix
// sort -- so the gradients are bitwise reproducible (its cost at C3: profiles/HISTORY.md).
// Built with FP contraction off: dt must be the rounded (t + 0.1f) - t of the reference's float32 tensor code.
#include "fdgs_common.h"
#include "fdgs_math.h"

namespace fdgs
{
	constexpr int REG_THREADS = 256;

	struct RegLayout { size_t parts, keys[2], vals[2], hist, seg_lo, seg_hi, total; };
	static inline RegLayout reg_layout(int P, int k)
	{
		RegLayout L;
		ScratchCursor c;
		const int p = P > 0 ? P : 1;
		const size_t pk = (size_t)p * (size_t)(k > 0 ? k : 1);
		L.parts = c.take((size_t)2 * div_up(p, REG_THREADS) * 4);
		for (int i = 0; i < 2; i++) L.keys[i] = c.take(pk * 4);
		for (int i = 0; i < 2; i++) L.vals[i] = c.take(pk * 4);
		L.hist = c.take((size_t)RADIX * (sort_blocks((int)pk) + 1) * 4);
		L.seg_lo = c.take((size_t)p * 4);
		L.seg_hi = c.take((size_t)p * 4);
		L.total = c.o;
		return L;
	}

	// deterministic sum over a workgroup of REG_THREADS threads; the total is valid in thread 0
	__device__ __forceinline__ float block_sum(float v, float* red)
	{
#pragma unroll
		for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
		if ((threadIdx.x & (WAVE - 1)) == 0) red[threadIdx.x / WAVE] = v;
		__syncthreads();
		return (red[0] + red[1]) + (red[2] + red[3]);
	}

	struct RegGauss { Cov4 c; float4 q, qr; float inv_q, inv_qr; float3 sc; float sct, dt; };

	__device__ __forceinline__ RegGauss reg_gauss(int i, const float* __restrict__ scaling, const float* __restrict__ scaling_t,
	                                              const float* __restrict__ rotation, const float* __restrict__ rotation_r,
	                                              const float* __restrict__ t)
	{
		RegGauss g;
		g.sc = ld3(scaling, i);
		g.sct = scaling_t[i];
		// scalar loads: a slice of a flat parameter bucket need not be 16-byte aligned
		g.q = make_float4(rotation[4 * (size_t)i], rotation[4 * (size_t)i + 1], rotation[4 * (size_t)i + 2], rotation[4 * (size_t)i + 3]);
		g.qr = make_float4(rotation_r[4 * (size_t)i], rotation_r[4 * (size_t)i + 1], rotation_r[4 * (size_t)i + 2], rotation_r[4 * (size_t)i + 3]);
		activate(g.sc, g.q, &g.inv_q);
		activate(g.sct, g.qr, &g.inv_qr);
		g.c = cov4_build(g.sc, g.sct, 1.0f, g.q, g.qr);
		const float ti = t[i];
		g.dt = (ti + 0.1f) - ti;
		return g;
	}

	__device__ __forceinline__ float norm3(float x, float y, float z) { return sqrtf((x * x + y * y) + z * z); }

	__global__ void __launch_bounds__(REG_THREADS) reg_velocity_kernel(int P, const float* __restrict__ scaling, const float* __restrict__ scaling_t,
	                                                                   const float* __restrict__ rotation, const float* __restrict__ rotation_r,
	                                                                   const float* __restrict__ t, float* __restrict__ velocity,
	                                                                   float* __restrict__ part_motion)
	{
		__shared__ float red[REG_THREADS / WAVE];
		const int i = blockIdx.x * REG_THREADS + threadIdx.x;
		float nv = 0.f;
		if (i < P)
		{
			const RegGauss g = reg_gauss(i, scaling, scaling_t, rotation, rotation_r, t);
			const float ct = g.c.Sigma.c[3][3];
			const float vx = g.c.Sigma.c[0][3] / ct * g.dt, vy = g.c.Sigma.c[1][3] / ct * g.dt, vz = g.c.Sigma.c[2][3] / ct * g.dt;
			velocity[3 * (size_t)i] = vx; velocity[3 * (size_t)i + 1] = vy; velocity[3 * (size_t)i + 2] = vz;
			nv = norm3(vx, vy, vz);
		}
		const float s = block_sum(nv, red);
		if (threadIdx.x == 0) part_motion[blockIdx.x] = s;
	}

	__global__ void __launch_bounds__(REG_THREADS) reg_rigid_kernel(int P, int k, const float* __restrict__ velocity, const int64_t* __restrict__ idx,
	                                                                const float* __restrict__ d2, float* __restrict__ part_rigid)
	{
		__shared__ float red[REG_THREADS / WAVE];
		const int i = blockIdx.x * REG_THREADS + threadIdx.x;
		float acc = 0.f;
		if (i < P)
		{
			const float3 vi = ld3(velocity, i);
			for (int j = 0; j < k; j++)
			{
				const int64_t n = idx[(size_t)i * k + j];
				if (n < 0 || n >= P) continue;
				const float3 vn = ld3(velocity, (size_t)n);
				acc += expf(-100.f * d2[(size_t)i * k + j]) * norm3(vn.x - vi.x, vn.y - vi.y, vn.z - vi.z);
			}
		}
		const float s = block_sum(acc, red);
		if (threadIdx.x == 0) part_rigid[blockIdx.x] = s;
	}

	// out[s] = (sum of parts[s][0 .. nparts) / div_a[s]) / div_b[s], s < nsets <= 2, summed in a fixed order by one workgroup
	struct RegDivs { float a[2], b[2]; };
	__global__ void __launch_bounds__(REG_THREADS) reg_reduce_kernel(int nparts, int nsets, const float* __restrict__ parts, RegDivs divs,
	                                                                 float* __restrict__ out)
	{
		__shared__ float red[REG_THREADS / WAVE];
		for (int s = 0; s < nsets; s++)
		{
			float v = 0.f;
			for (int i = threadIdx.x; i < nparts; i += REG_THREADS) v += parts[(size_t)s * nparts + i];
			const float tot = block_sum(v, red);
			if (threadIdx.x == 0) out[s] = tot / divs.a[s] / divs.b[s];
			__syncthreads();
		}
	}

	// the (neighbour, pair) table; an index outside [0, P) goes to the bucket P, which no Gaussian reads
	__global__ void reg_pairs_kernel(int P, int PK, const int64_t* __restrict__ idx, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals)
	{
		const int p = blockIdx.x * blockDim.x + threadIdx.x;
		if (p >= PK) return;
		const int64_t n = idx[p];
		keys[p] = (n >= 0 && n < P) ? (uint32_t)n : (uint32_t)P;
		vals[p] = (uint32_t)p;
	}

	__global__ void reg_segments_kernel(int P, int PK, const uint32_t* __restrict__ keys, int* __restrict__ seg_lo, int* __restrict__ seg_hi)
	{
		const int p = blockIdx.x * blockDim.x + threadIdx.x;
		if (p >= PK) return;
		const uint32_t key = keys[p];
		if (key >= (uint32_t)P) return;
		if (p == 0 || keys[p - 1] != key) seg_lo[key] = p;
		if (p == PK - 1 || keys[p + 1] != key) seg_hi[key] = p + 1;
	}

	// g * (v_i - v_o) / |v_i - v_o|, 0 at a zero difference (torch.norm's gradient there)
	__device__ __forceinline__ void add_unit(float3& acc, float w, const float3 vi, const float3 vo)
	{
		const float dx = vi.x - vo.x, dy = vi.y - vo.y, dz = vi.z - vo.z;
		const float nrm = norm3(dx, dy, dz);
		if (nrm > 0.f)
		{
			const float s = w / nrm;
			acc.x += s * dx; acc.y += s * dy; acc.z += s * dz;
		}
	}

	__global__ void __launch_bounds__(REG_THREADS) reg_backward_kernel(
		int P, int k, const float* __restrict__ scaling, const float* __restrict__ scaling_t, const float* __restrict__ rotation,
		const float* __restrict__ rotation_r, const float* __restrict__ t, const int64_t* __restrict__ idx, const float* __restrict__ d2,
		const float* __restrict__ velocity, const uint32_t* __restrict__ pairs, const int* __restrict__ seg_lo, const int* __restrict__ seg_hi,
		const float* __restrict__ g_losses, float scale, float* __restrict__ d_scaling, float* __restrict__ d_scaling_t,
		float* __restrict__ d_rotation, float* __restrict__ d_rotation_r)
	{
		const int i = blockIdx.x * REG_THREADS + threadIdx.x;
		if (i >= P) return;
		const float g_rigid = g_losses[0], g_motion = g_losses[1];
		const float3 vi = ld3(velocity, i);
		// dL/dv_i: motion (d mean|v| = v / |v| / P), then the rigid pairs in which i is the query, then those in which it is the
		// neighbour (the reverse list, in pair order)
		float3 gv = make_float3(0.f, 0.f, 0.f);
		add_unit(gv, g_motion / (float)P, vi, make_float3(0.f, 0.f, 0.f));
		float3 acc = make_float3(0.f, 0.f, 0.f);
		for (int j = 0; j < k; j++)
		{
			const int64_t n = idx[(size_t)i * k + j];
			if (n < 0 || n >= P) continue;
			add_unit(acc, expf(-100.f * d2[(size_t)i * k + j]), vi, ld3(velocity, (size_t)n));
		}
		for (int p = seg_lo[i]; p < seg_hi[i]; p++)
		{
			const uint32_t pair = pairs[p];
			add_unit(acc, expf(-100.f * d2[pair]), vi, ld3(velocity, pair / (uint32_t)k));
		}
		const float cr = g_rigid / (float)k / (float)P;
		gv.x += cr * acc.x; gv.y += cr * acc.y; gv.z += cr * acc.z;

		// v = c12 / ct * dt  ->  Sigma  ->  scale / rotations (cov4_backward, as the preprocess backward)
		const RegGauss g = reg_gauss(i, scaling, scaling_t, rotation, rotation_r, t);
		const float ct = g.c.Sigma.c[3][3];
		const float c12[3] = { g.c.Sigma.c[0][3], g.c.Sigma.c[1][3], g.c.Sigma.c[2][3] };
		const float d12[3] = { gv.x / ct * g.dt, gv.y / ct * g.dt, gv.z / ct * g.dt };
		const float ddot = gv.x * c12[0] + gv.y * c12[1] + gv.z * c12[2];
		M4 dSig;
#pragma unroll
		for (int j = 0; j < 4; j++)
#pragma unroll
			for (int r = 0; r < 4; r++) dSig.c[j][r] = 0.f;
#pragma unroll
		for (int r = 0; r < 3; r++) { dSig.c[r][3] = 0.5f * d12[r]; dSig.c[3][r] = 0.5f * d12[r]; }
		dSig.c[3][3] = -ddot / (ct * ct) * g.dt;
		float3 dscale;
		float dscale_t;
		float4 drot, drot_r;
		cov4_backward(g.c, dSig, dscale, dscale_t, drot, drot_r);
		// scale multiplies the finished gradient (not the upstream weights): scale = s gives s x the scale = 1 result, one rounding each
		d_scaling[3 * (size_t)i] += scale * (dscale.x * g.sc.x);             // d exp
		d_scaling[3 * (size_t)i + 1] += scale * (dscale.y * g.sc.y);
		d_scaling[3 * (size_t)i + 2] += scale * (dscale.z * g.sc.z);
		d_scaling_t[i] += scale * (dscale_t * g.sct);
		const float4 dq = act_normalize_bwd(g.q, g.inv_q, drot), dqr = act_normalize_bwd(g.qr, g.inv_qr, drot_r);
		float* oq = d_rotation + 4 * (size_t)i;
		float* oqr = d_rotation_r + 4 * (size_t)i;
		oq[0] += scale * dq.x; oq[1] += scale * dq.y; oq[2] += scale * dq.z; oq[3] += scale * dq.w;
		oqr[0] += scale * dqr.x; oqr[1] += scale * dqr.y; oqr[2] += scale * dqr.z; oqr[3] += scale * dqr.w;
	}

	// ---- opacity mask ----
	__global__ void __launch_bounds__(REG_THREADS) opa_mask_kernel(int HW, const float* __restrict__ alpha, int alpha_is_T,
	                                                               const float* __restrict__ mask, float lo, float hi,
	                                                               const float* __restrict__ g_upstream, float scale,
	                                                               float* __restrict__ grad, int accumulate, float* __restrict__ parts)
	{
		__shared__ float red[REG_THREADS / WAVE];
		const int i = blockIdx.x * REG_THREADS + threadIdx.x;
		float val = 0.f;
		if (i < HW)
		{
			const float a = alpha_is_T ? 1.f - alpha[i] : alpha[i];
			const float o = fminf(fmaxf(a, lo), hi);
			const float sky = 1.f - mask[i];
			val = -sky * logf(1.f - o);
			if (grad)
			{
				const float s = g_upstream ? scale * g_upstream[0] : scale;
				const float g = (a >= lo && a <= hi) ? sky / (1.f - o) / (float)HW * s : 0.f;   // torch.clamp passes lo <= a <= hi
				grad[i] = accumulate ? grad[i] + g : g;
			}
		}
		const float s = block_sum(val, red);
		if (threadIdx.x == 0) parts[blockIdx.x] = s;
	}
}

using namespace fdgs;

static bool reg_args_ok(int P, int k)
{
	return P >= 0 && k >= 1 && (int64_t)P * k < ((int64_t)1 << 31);
}

extern "C" size_t fdgs_rigid_motion_scratch_bytes(int32_t P, int32_t k) { return reg_layout(P, k).total; }

extern "C" int fdgs_rigid_motion_forward(int32_t P, int32_t k, const float* scaling, const float* scaling_t, const float* rotation,
                                         const float* rotation_r, const float* t, const int64_t* knn_idx, const float* knn_d2, float* velocity,
                                         float* losses, void* scratch, void* stream_v)
{
	if (!reg_args_ok(P, k)) return fail(FDGS_ERR_INVALID_ARG, "fdgs_rigid_motion_forward: need P >= 0, k >= 1, P * k < 2^31");
	if (P == 0) return fail(FDGS_ERR_INVALID_ARG, "fdgs_rigid_motion_forward: no Gaussians (the reference's mean is undefined)");
	if (!scaling || !scaling_t || !rotation || !rotation_r || !t || !knn_idx || !knn_d2 || !velocity || !losses || !scratch)
		return fail(FDGS_ERR_INVALID_ARG, "fdgs_rigid_motion_forward: missing pointer");
	hipStream_t stream = (hipStream_t)stream_v;
	const RegLayout L = reg_layout(P, k);
	float* parts = (float*)((char*)scratch + L.parts);
	const int nb = div_up(P, REG_THREADS);
	hipLaunchKernelGGL(reg_velocity_kernel, dim3(nb), dim3(REG_THREADS), 0, stream, P, scaling, scaling_t, rotation, rotation_r, t, velocity,
	                   parts + nb);
	hipLaunchKernelGGL(reg_rigid_kernel, dim3(nb), dim3(REG_THREADS), 0, stream, P, k, velocity, knn_idx, knn_d2, parts);
	const RegDivs divs = { { (float)k, 1.f }, { (float)P, (float)P } };   // (sum / k) / N  and  sum / N
	hipLaunchKernelGGL(reg_reduce_kernel, dim3(1), dim3(REG_THREADS), 0, stream, nb, 2, parts, divs, losses);
	return launched("fdgs_rigid_motion_forward");
}

extern "C" int fdgs_rigid_motion_backward(int32_t P, int32_t k, const float* scaling, const float* scaling_t, const float* rotation,
                                          const float* rotation_r, const float* t, const int64_t* knn_idx, const float* knn_d2,
                                          const float* velocity, const float* g_losses, float scale, float* d_scaling, float* d_scaling_t,
                                          float* d_rotation, float* d_rotation_r, void* scratch, void* stream_v)
{
	if (!reg_args_ok(P, k)) return fail(FDGS_ERR_INVALID_ARG, "fdgs_rigid_motion_backward: need P >= 0, k >= 1, P * k < 2^31");
	if (P == 0) return FDGS_OK;
	if (!scaling || !scaling_t || !rotation || !rotation_r || !t || !knn_idx || !knn_d2 || !velocity || !g_losses || !d_scaling ||
	    !d_scaling_t || !d_rotation || !d_rotation_r || !scratch)
		return fail(FDGS_ERR_INVALID_ARG, "fdgs_rigid_motion_backward: missing pointer");
	hipStream_t stream = (hipStream_t)stream_v;
	const RegLayout L = reg_layout(P, k);
	char* s = (char*)scratch;
	const int PK = P * k;
	uint32_t* keys[2] = { (uint32_t*)(s + L.keys[0]), (uint32_t*)(s + L.keys[1]) };
	uint32_t* vals[2] = { (uint32_t*)(s + L.vals[0]), (uint32_t*)(s + L.vals[1]) };
	int* seg_lo = (int*)(s + L.seg_lo);
	int* seg_hi = (int*)(s + L.seg_hi);
	hipLaunchKernelGGL(reg_pairs_kernel, dim3(div_up(PK, 256)), dim3(256), 0, stream, P, PK, knn_idx, keys[0], vals[0]);
	int bits = 0;
	while (bits < 32 && ((uint64_t)1 << bits) <= (uint64_t)P) bits++;      // keys are 0 .. P
	int res = 0;
	HIP_TRY(radix_sort_pairs(keys, vals, PK, 0, bits, (uint32_t*)(s + L.hist), stream, &res), "fdgs_rigid_motion_backward: radix_sort_pairs");
	HIP_TRY(hipMemsetAsync(seg_lo, 0, (size_t)P * 4, stream), "fdgs_rigid_motion_backward: hipMemsetAsync");
	HIP_TRY(hipMemsetAsync(seg_hi, 0, (size_t)P * 4, stream), "fdgs_rigid_motion_backward: hipMemsetAsync");
	hipLaunchKernelGGL(reg_segments_kernel, dim3(div_up(PK, 256)), dim3(256), 0, stream, P, PK, keys[res], seg_lo, seg_hi);
	hipLaunchKernelGGL(reg_backward_kernel, dim3(div_up(P, REG_THREADS)), dim3(REG_THREADS), 0, stream, P, k, scaling, scaling_t, rotation,
	                   rotation_r, t, knn_idx, knn_d2, velocity, vals[res], seg_lo, seg_hi, g_losses, scale, d_scaling, d_scaling_t, d_rotation,
	                   d_rotation_r);
	return launched("fdgs_rigid_motion_backward");
}

extern "C" int fdgs_opa_mask_num_partials(int32_t H, int32_t W)
{
	return (H > 0 && W > 0) ? div_up(H * W, REG_THREADS) : 0;
}

extern "C" int fdgs_opa_mask_loss(int32_t H, int32_t W, const float* alpha, int32_t alpha_is_T, const float* mask, const float* g_upstream,
                                  float scale, float* grad, int32_t accumulate, float* partials, float* loss, void* stream_v)
{
	if (H <= 0 || W <= 0 || (int64_t)H * W >= ((int64_t)1 << 31)) return fail(FDGS_ERR_INVALID_ARG, "fdgs_opa_mask_loss: bad image size");
	if (!alpha || !mask || !partials || !loss) return fail(FDGS_ERR_INVALID_ARG, "fdgs_opa_mask_loss: missing pointer");
	hipStream_t stream = (hipStream_t)stream_v;
	const int HW = H * W, nb = div_up(HW, REG_THREADS);
	// torch.clamp(alpha, 1e-6, 1 - 1e-6) on a float32 tensor: both bounds rounded to float
	hipLaunchKernelGGL(opa_mask_kernel, dim3(nb), dim3(REG_THREADS), 0, stream, HW, alpha, alpha_is_T, mask, 1e-6f, (float)(1.0 - 1e-6),
	                   g_upstream, scale, grad, accumulate, partials);
	const RegDivs divs = { { 1.f, 1.f }, { (float)HW, 1.f } };
	hipLaunchKernelGGL(reg_reduce_kernel, dim3(1), dim3(REG_THREADS), 0, stream, nb, 1, partials, divs, loss);
	return launched("fdgs_opa_mask_loss");
}
