// contribution.hip -- per-Gaussian contribution statistics and the per-pixel ID map of a finished forward (gfx950).
//
// One pass over the buffers a forward leaves behind (blend records, tile lists, ranges): per pixel the tile's list is walked
// front to back with blend_fwd's own decisions -- skip power > 0 and alpha < 1/255, an entry that would take T below 1e-4 ends
// the pixel and does not contribute -- and the blending weight w = alpha * T of every contribution is summarised per Gaussian:
//   weight_sum += pix_weight * w     weight_max = max(., w)     hits += 1     (over the pixels the Gaussian contributes to)
// and per pixel: dominant_id = the contributor with the largest w (the earliest on a tie), dominant[that Gaussian] += 1.
// power, alpha and T are blend_fwd.hip's expressions (association, FMA, hardware exp2, min(0.99, .)), so the set of
// (pixel, entry) contributions is the rendered image's own.
//
// Work decomposition: blend_fwd's -- one wave64 per 8x8 pixel block in the blend kernels' tile order, 64 list entries per chunk, one
// entry per lane culled against the block (block_reaches, run again: nothing depends on the forward's cull planes) and compacted
// into a wave-private LDS queue (blend_common.h: pixel_block, queue_chunk, blend_weight -- the walk features.hip takes too).  The reduction over the block's 64 pixels stays on chip: every lane stores its pixel's w of an
// entry into a row of an LDS staging area; every GROUP entries the area is transposed -- four lanes per entry read 16 pixels each
// and fold sum / max / count, two DPP quad steps finish them -- and one lane per entry issues the atomics:
//   at most ONE atomic request per (block, Gaussian, output), none for an entry that contributed to no pixel of the block.
// weight_max is an unsigned integer max on the float's bits (w >= 0), hits / dominant are integer adds: reproducible run to run;
// weight_sum is a float atomic sum (its last bits depend on the arrival order).
#include "blend_common.h"

namespace fdgs
{
	constexpr int CONTRIB_GROUP = 16;          // entries staged between two drains
	constexpr int CONTRIB_ROW = WAVE + 1;      // row stride of the staging area in floats: the transposed reads hit 64 different banks

	__device__ __forceinline__ float quad_xor1(float v) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, false)); }   // quad_perm:[1,0,3,2]
	__device__ __forceinline__ float quad_xor2(float v) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, false)); }   // quad_perm:[2,3,0,1]

	// WEIGHTED = false: pix_weight == NULL, every pixel counts with weight 1
	template <bool WEIGHTED>
	__global__ void __launch_bounds__(WAVE) contribution_kernel(
		const uint2* __restrict__ ranges, const uint32_t* __restrict__ point_list, const float4* __restrict__ records,
		const uint32_t* __restrict__ tile_order, int W, int H, int grid_x, int ntiles, const float* __restrict__ pix_weight,
		float* __restrict__ weight_sum, float* __restrict__ weight_max, uint32_t* __restrict__ hits, uint32_t* __restrict__ dominant,
		int32_t* __restrict__ dominant_id)
	{
		// wave-private queue of the surviving entries of the current chunk: (x, y, conic.x, conic.y) and (conic.z, opacity, Gaussian id, -)
		__shared__ float4 s_qa[WAVE], s_qb[WAVE];
		__shared__ float s_w[CONTRIB_GROUP * CONTRIB_ROW];   // [entry of the group][pixel]
		__shared__ float s_pw[WAVE];                         // the block's pixel weights

		const int lane = threadIdx.x;
		PixelBlock pb;
		if (!pixel_block(blockIdx.x, ntiles, tile_order, grid_x, W, H, lane, pb)) return;
		const bool inside = pb.inside;
		const size_t pix_id = (size_t)W * pb.py + pb.px;

		// a pixel with weight <= 0 (and one outside the image) takes no contribution at all: finished before it starts
		float pw = inside ? 1.0f : 0.0f;
		if (WEIGHTED && inside) pw = pix_weight[pix_id];
		const bool live = pw > 0.0f;
		if (WEIGHTED) s_pw[lane] = live ? pw : 0.0f;

		const uint2 range = ranges[pb.tile];
		const int n = (int)(range.y - range.x);

		lanemask done = mask_of(!live);
		float T = 1.0f, best_w = 0.0f;
		int32_t best_id = -1;

		// drain: lane (e, q) = (lane >> 2, lane & 3) folds pixels 16 q .. 16 q + 15 of staged entry e
		const int de = lane >> 2, dq = lane & 3;
		const float* const row = s_w + de * CONTRIB_ROW + dq * 16;
		const float* const pwq = s_pw + dq * 16;
		const bool want_stats = weight_sum != nullptr || weight_max != nullptr || hits != nullptr;
		// gmask: bit e = staged entry e contributed to some pixel of the block; q0: first queue slot of the group
		auto drain = [&](const uint32_t gmask, const int q0) __attribute__((always_inline))
		{
			__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // compiler ordering only: the LDS executes a wave's operations in order
			__builtin_amdgcn_wave_barrier();
			float sum = 0.0f, mx = 0.0f, cnt = 0.0f;
#pragma unroll
			for (int k = 0; k < 16; k++)
			{
				const float w = row[k];
				sum = WEIGHTED ? fmaf(pwq[k], w, sum) : sum + w;
				mx = fmaxf(mx, w);
				cnt += w > 0.0f ? 1.0f : 0.0f;   // a contribution has w >= 1e-4 / 255 > 0
			}
			sum += quad_xor1(sum); mx = fmaxf(mx, quad_xor1(mx)); cnt += quad_xor1(cnt);
			sum += quad_xor2(sum); mx = fmaxf(mx, quad_xor2(mx)); cnt += quad_xor2(cnt);
			if (dq == 0 && ((gmask >> de) & 1u))
			{
				const uint32_t id = __float_as_uint(s_qb[q0 + de].z);
				if (weight_sum) atomicAdd(weight_sum + id, sum);
				if (weight_max) atomicMax(reinterpret_cast<unsigned int*>(weight_max) + id, __float_as_uint(mx));
				if (hits) atomicAdd(hits + id, (uint32_t)cnt);
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
				if (w > best_w) { best_w = w; best_id = (int32_t)__float_as_uint(qb.z); }   // strictly larger: the earliest entry wins a tie
				const int g = i & (CONTRIB_GROUP - 1);
				if (want_stats)
				{
					s_w[g * CONTRIB_ROW + lane] = w;
					gmask |= (contrib != 0ull ? 1u : 0u) << g;
				}
				const bool stop = done == ~0ull;
				if (g == CONTRIB_GROUP - 1 || i == cnt - 1 || stop)
				{
					if (gmask) drain(gmask, i - g);
					gmask = 0u;
				}
				if (stop) break;
			}
			__syncthreads(); // the queue is rewritten by the next chunk
		}

		if (dominant_id != nullptr && inside) dominant_id[pix_id] = best_id;
		if (dominant != nullptr)
		{
			// one add per distinct dominant Gaussian of the block: the lanes that share the first pending lane's id are counted together
			lanemask pending = mask_of(best_id >= 0);
			while (pending != 0ull)
			{
				const int leader = __builtin_ctzll(pending);
				const int32_t lid = __builtin_amdgcn_readlane(best_id, leader);
				const lanemask same = mask_of(best_id == lid) & pending;
				if (lane == leader) atomicAdd(dominant + lid, (uint32_t)__popcll(same));
				pending &= ~same;
			}
		}
	}

	hipError_t launch_contribution(const fdgs_contribution_in& in, const fdgs_contribution_out& out, const FinishedForward& ff, hipStream_t stream)
	{
#define LAUNCH_CONTRIB(WEIGHTED) hipLaunchKernelGGL(contribution_kernel<WEIGHTED>, dim3(blend_grid(ff.ntiles)), dim3(WAVE), 0, stream, \
		                   ff.ranges, ff.point_list, ff.records, ff.tile_order, ff.W, ff.H, ff.gx, ff.ntiles, in.pix_weight, \
		                   out.weight_sum, out.weight_max, out.hits, out.dominant, out.dominant_id)
		if (in.pix_weight != nullptr) LAUNCH_CONTRIB(true);
		else LAUNCH_CONTRIB(false);
#undef LAUNCH_CONTRIB
		return hipGetLastError();
	}
}
