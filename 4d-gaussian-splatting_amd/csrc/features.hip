// features.hip -- per-Gaussian feature channels blended with the weights of a finished forward, and the adjoint (gfx950, wave64).
//
//   forward    out[c, y, x]  = sum over the pixel's contributions of w * F[id, c]        (overwritten; no contributor: exactly 0)
//   backward   dF[id, c]    += sum over the pixels Gaussian id contributes to of w * g[c, y, x]      (accumulated in place)
// w = alpha * T is the blending weight of the rendered image: both kernels walk the buffers a forward leaves behind (blend records,
// tile lists, ranges) with blend_fwd.hip's own decisions and arithmetic (blend_common.h: pixel_block, queue_chunk, blend_weight -- the walk of
// contribution.hip), so the set of (pixel, entry) contributions is the rendered image's own.  GEOMETRY IS HELD CONSTANT: w is a
// number here, no gradient reaches alpha, the positions or the covariances; the backward is the adjoint of the forward as a linear map
// of F, nothing else.  Nothing is composited behind the features.
//
// Work decomposition: blend_fwd's -- one wave64 per 8x8 pixel block in the blend kernels' tile order (grid.x), 64 list entries per
// chunk, culled with block_reaches and compacted into a wave-private LDS queue; grid.y: the group of channels the wave handles, every
// group walks the list again (the walk costs about what 16 channels' arithmetic does).
//
// Forward (NCH = 4, 16 or 32 channels per wave): the lane that queues an entry copies its NCH feature values into an LDS row; per
// queued entry every lane computes its pixel's w and runs acc[j] = fmaf(w, F[id, c0 + j], acc[j]) over the row, read wave-uniformly
// (broadcast).  A channel's value is one fmaf chain over the pixel's entries in list order, whatever the other channels of its group
// or the group width are: bit-identical run to run and for every C.  No atomics.
//
// Backward (NG = 1 or 2 groups of 16 channels per wave): the per-block reduction over the 64 pixels is a matrix product,
//   D[entry e][channel c] = sum over the block's pixels p of w[e][p] * g[c][p]        (16 entries x 64 pixels) . (64 pixels x 16 channels)
// on v_mfma_f32_16x16x4_f32 (exact fp32: a k-ordered fmaf chain), 16 k-steps of 4 pixels.  Every lane stores its pixel's w of an entry
// into a row of an LDS staging area, as contribution_kernel does; every 16 entries the area is drained:
//   A operand, k-step s: lane l holds A[row l & 15][k = l >> 4] = s_w[entry l & 15][pixel 4 s + (l >> 4)]     (one LDS read per step)
//   B operand, k-step s: lane l holds B[k = l >> 4][column l & 15] = g[c0 + (l & 15)][pixel 4 s + (l >> 4)]   (16 registers per group,
//                        loaded once per block: the block's 64 x 16 slice of g lives in the wave's registers for the whole walk)
//   D: lane l holds D[row 4 (l >> 4) + r][column l & 15] in register r = 0..3: entry 4 (l >> 4) + r, channel c0 + (l & 15)
// and the lane adds its four values to dF with float atomics -- at most ONE atomic request per (block, Gaussian, channel), none for an
// entry that contributed to no pixel of the block (a Gaussian is listed once per tile), 16 consecutive floats of a row per request group.
#include "blend_common.h"

namespace fdgs
{
	constexpr int FEAT_GROUP = 16;             // entries staged between two drains = rows of the MFMA tile
	constexpr int FEAT_ROW = WAVE + 4;         // row stride of the staging area in floats: the A-operand reads (4 (l & 15) + (l >> 4) + 4 s) hit 64 different banks
	typedef float feat_f32x4 __attribute__((ext_vector_type(4)));

	template <int NCH>
	__global__ void __launch_bounds__(WAVE) feature_fwd_kernel(
		const uint2* __restrict__ ranges, const uint32_t* __restrict__ point_list, const float4* __restrict__ records,
		const uint32_t* __restrict__ tile_order, int W, int H, int grid_x, int ntiles, const float* __restrict__ features, int C,
		float* __restrict__ out)
	{
		constexpr int PITCH = NCH / 4 + 1;   // float4s per feature row (+ 1: the row writes of neighbouring lanes spread over the banks)
		__shared__ float4 s_qa[WAVE], s_qb[WAVE];
		__shared__ float4 s_f[WAVE * PITCH];   // [queue slot][channel of the group]

		const int lane = threadIdx.x;
		PixelBlock pb;
		if (!pixel_block(blockIdx.x, ntiles, tile_order, grid_x, W, H, lane, pb)) return;
		const int c0 = blockIdx.y * NCH;
		const bool inside = pb.inside;

		const uint2 range = ranges[pb.tile];
		const int n = (int)(range.y - range.x);

		lanemask done = mask_of(!inside);
		float T = 1.0f;
		float acc[NCH];
#pragma unroll
		for (int j = 0; j < NCH; j++) acc[j] = 0.0f;

		for (int base = 0; base < n; base += WAVE)
		{
			if (done == ~0ull) break; // all 64 pixels finished
			bool keep;
			uint32_t id;
			int slot;
			const int cnt = queue_chunk(point_list, records, range, n, base, lane, pb, s_qa, s_qb, keep, id, slot);
			if (keep)
			{
				// the group's slice of the entry's feature row; channels at and beyond C read as 0 (and are never stored)
				const float* const f = features + ((size_t)id * C + c0);
#pragma unroll
				for (int j = 0; j < NCH / 4; j++)
				{
					float4 v;
					v.x = c0 + 4 * j + 0 < C ? f[4 * j + 0] : 0.0f;
					v.y = c0 + 4 * j + 1 < C ? f[4 * j + 1] : 0.0f;
					v.z = c0 + 4 * j + 2 < C ? f[4 * j + 2] : 0.0f;
					v.w = c0 + 4 * j + 3 < C ? f[4 * j + 3] : 0.0f;
					s_f[slot * PITCH + j] = v;
				}
			}
			__syncthreads(); // single-wave workgroup: orders the LDS writes before the cross-lane reads

			for (int i = 0; i < cnt; i++)
			{
				const float4 qa = s_qa[i], qb = s_qb[i];
				lanemask contrib;
				const float w = blend_weight(qa, qb, pb.pixfx, pb.pixfy, T, done, contrib);
				if (contrib != 0ull)   // wave-uniform: an entry no pixel of the block takes costs no arithmetic
				{
#pragma unroll
					for (int j = 0; j < NCH / 4; j++)
					{
						const float4 v = s_f[i * PITCH + j];   // the same address on every lane: a broadcast
						acc[4 * j + 0] = fmaf(w, v.x, acc[4 * j + 0]);
						acc[4 * j + 1] = fmaf(w, v.y, acc[4 * j + 1]);
						acc[4 * j + 2] = fmaf(w, v.z, acc[4 * j + 2]);
						acc[4 * j + 3] = fmaf(w, v.w, acc[4 * j + 3]);
					}
				}
				if (done == ~0ull) break;
			}
			__syncthreads(); // the queue is rewritten by the next chunk
		}

		if (inside)
		{
			const size_t plane = (size_t)W * H;
			float* const o = out + ((size_t)c0 * plane + (size_t)W * pb.py + pb.px);
#pragma unroll
			for (int j = 0; j < NCH; j++)
				if (c0 + j < C) o[(size_t)j * plane] = acc[j];
		}
	}

	template <int NG>
	__global__ void __launch_bounds__(WAVE) feature_bwd_kernel(
		const uint2* __restrict__ ranges, const uint32_t* __restrict__ point_list, const float4* __restrict__ records,
		const uint32_t* __restrict__ tile_order, int W, int H, int grid_x, int ntiles, const float* __restrict__ dL_dout, int C,
		float* __restrict__ dL_dfeatures)
	{
		__shared__ float4 s_qa[WAVE], s_qb[WAVE];
		__shared__ float s_w[FEAT_GROUP * FEAT_ROW];   // [entry of the group][pixel]

		const int lane = threadIdx.x;
		PixelBlock pb;
		if (!pixel_block(blockIdx.x, ntiles, tile_order, grid_x, W, H, lane, pb)) return;
		const int c0 = blockIdx.y * (16 * NG);
		const bool inside = pb.inside;

		const uint2 range = ranges[pb.tile];
		const int n = (int)(range.y - range.x);
		if (n == 0) return;

		// the B operands: this lane's column (channel) and k (pixel 4 s + (lane >> 4) of the block) for the 16 k-steps; 0 outside the
		// image and beyond C
		const int col = lane & 15, kq = lane >> 4;
		float b[NG][16];
#pragma unroll
		for (int gi = 0; gi < NG; gi++)
		{
			const int c = c0 + 16 * gi + col;
			const float* const gc = dL_dout + (size_t)(c < C ? c : 0) * ((size_t)W * H);
#pragma unroll
			for (int s = 0; s < 16; s++)
			{
				const int p = 4 * s + kq;
				const int gx = pb.bx0 + (p & (BLK - 1)), gy = pb.by0 + (p >> 3);
				b[gi][s] = (c < C && gx < W && gy < H) ? gc[(size_t)W * gy + gx] : 0.0f;
			}
		}

		lanemask done = mask_of(!inside);
		float T = 1.0f;
		const float* const arow = s_w + col * FEAT_ROW + kq;

		// gmask: bit e = staged entry e contributed to some pixel of the block; q0: first queue slot of the group.  Rows of the area
		// beyond the group's last entry hold what an earlier drain left there: a row of A only reaches its own row of D, which is not used.
		auto drain = [&](const uint32_t gmask, const int q0) __attribute__((always_inline))
		{
			__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // compiler ordering only: the LDS executes a wave's operations in order
			__builtin_amdgcn_wave_barrier();
			feat_f32x4 d[NG];
#pragma unroll
			for (int gi = 0; gi < NG; gi++) d[gi] = feat_f32x4{ 0.0f, 0.0f, 0.0f, 0.0f };
#pragma unroll
			for (int s = 0; s < 16; s++)
			{
				const float a = arow[4 * s];
#pragma unroll
				for (int gi = 0; gi < NG; gi++) d[gi] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b[gi][s], d[gi], 0, 0, 0);
			}
#pragma unroll
			for (int r = 0; r < 4; r++)
			{
				const int e = 4 * kq + r;
				if ((gmask >> e) & 1u)
				{
					const uint32_t id = __float_as_uint(s_qb[q0 + e].z);
					float* const row = dL_dfeatures + (size_t)id * C;
#pragma unroll
					for (int gi = 0; gi < NG; gi++)
					{
						const int c = c0 + 16 * gi + col;
						if (c < C) atomicAdd(row + c, d[gi][r]);
					}
				}
			}
			__builtin_amdgcn_wave_barrier();
			__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
		};

		for (int base = 0; base < n; base += WAVE)
		{
			if (done == ~0ull) break; // all 64 pixels finished
			bool keep;
			uint32_t id;
			int slot;
			const int cnt = queue_chunk(point_list, records, range, n, base, lane, pb, s_qa, s_qb, keep, id, slot);
			__syncthreads(); // single-wave workgroup: orders the LDS writes before the cross-lane reads

			uint32_t gmask = 0u;
			for (int i = 0; i < cnt; i++)
			{
				const float4 qa = s_qa[i], qb = s_qb[i];
				lanemask contrib;
				const float w = blend_weight(qa, qb, pb.pixfx, pb.pixfy, T, done, contrib);
				const int g = i & (FEAT_GROUP - 1);
				s_w[g * FEAT_ROW + lane] = w;
				gmask |= (contrib != 0ull ? 1u : 0u) << g;
				const bool stop = done == ~0ull;
				if (g == FEAT_GROUP - 1 || i == cnt - 1 || stop)
				{
					if (gmask) drain(gmask, i - g);
					gmask = 0u;
				}
				if (stop) break;
			}
			__syncthreads(); // the queue is rewritten by the next chunk
		}
	}

	static inline dim3 feat_grid(int ntiles, int C, int per_wave) { return dim3(blend_grid(ntiles), div_up(C, per_wave)); }

	// (C is in 1 .. FDGS_FEATURE_MAX_CHANNELS: checked where the call comes in)
	hipError_t launch_feature_blend(const fdgs_feature_in& in, float* out, const FinishedForward& ff, hipStream_t stream)
	{
#define LAUNCH_FEAT_FWD(NCH) hipLaunchKernelGGL(feature_fwd_kernel<NCH>, feat_grid(ff.ntiles, in.C, NCH), dim3(WAVE), 0, stream, \
		                   ff.ranges, ff.point_list, ff.records, ff.tile_order, ff.W, ff.H, ff.gx, ff.ntiles, in.features, in.C, out)
		if (in.C <= 4) LAUNCH_FEAT_FWD(4);
		else if (in.C <= 16) LAUNCH_FEAT_FWD(16);
		else LAUNCH_FEAT_FWD(32);
#undef LAUNCH_FEAT_FWD
		return hipGetLastError();
	}

	hipError_t launch_feature_blend_bwd(const fdgs_feature_in& in, const float* dL_dout, float* dL_dfeatures, const FinishedForward& ff,
	                                    hipStream_t stream)
	{
#define LAUNCH_FEAT_BWD(NG) hipLaunchKernelGGL(feature_bwd_kernel<NG>, feat_grid(ff.ntiles, in.C, 16 * NG), dim3(WAVE), 0, stream, \
		                   ff.ranges, ff.point_list, ff.records, ff.tile_order, ff.W, ff.H, ff.gx, ff.ntiles, dL_dout, in.C, dL_dfeatures)
		if (in.C <= 16) LAUNCH_FEAT_BWD(1);
		else LAUNCH_FEAT_BWD(2);
#undef LAUNCH_FEAT_BWD
		return hipGetLastError();
	}
}
