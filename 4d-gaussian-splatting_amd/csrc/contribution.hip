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
// into a wave-private LDS queue.  The reduction over the block's 64 pixels stays on chip: every lane stores its pixel's w of an
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
		const BlockId blk = block_of(blockIdx.x, ntiles, tile_order);
		if (blk.tile >= ntiles) return;
		const int bx0 = (blk.tile % grid_x) * TILE_X + (blk.sub & 1) * BLK;
		const int by0 = (blk.tile / grid_x) * TILE_Y + (blk.sub >> 1) * BLK;
		if (bx0 >= W || by0 >= H) return; // block entirely outside the image
		const int px = bx0 + (lane & (BLK - 1)), py = by0 + (lane >> 3);
		const bool inside = px < W && py < H;
		const size_t pix_id = (size_t)W * py + px;
		const float pixfx = (float)px, pixfy = (float)py;
		const float rx0 = (float)bx0, rx1 = (float)min(bx0 + BLK - 1, W - 1);
		const float ry0 = (float)by0, ry1 = (float)min(by0 + BLK - 1, H - 1);

		// a pixel with weight <= 0 (and one outside the image) takes no contribution at all: finished before it starts
		float pw = inside ? 1.0f : 0.0f;
		if (WEIGHTED && inside) pw = pix_weight[pix_id];
		const bool live = pw > 0.0f;
		if (WEIGHTED) s_pw[lane] = live ? pw : 0.0f;

		const uint2 range = ranges[blk.tile];
		const int n = (int)(range.y - range.x);
		const unsigned long long lt_mask = (1ull << lane) - 1ull;

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
			const int pos = base + lane;
			bool keep = false;
			uint32_t id = 0;
			float4 a, b;
			if (pos < n)
			{
				id = point_list[range.x + pos];
				a = record_word(records, id, 0);
				b = record_word(records, id, 1);
				keep = block_reaches(a, b, rx0, rx1, ry0, ry1);
			}
			const unsigned long long mask = __ballot(keep);
			const int cnt = __popcll(mask);
			if (keep)
			{
				const int slot = __popcll(mask & lt_mask);   // list order is preserved
				s_qa[slot] = a;
				s_qb[slot] = make_float4(b.x, b.y, __uint_as_float(id), 0.0f);
			}
			__syncthreads(); // single-wave workgroup: orders the LDS writes before the cross-lane reads

			uint32_t gmask = 0u;
			for (int i = 0; i < cnt; i++)
			{
				const float4 qa = s_qa[i], qb = s_qb[i];
				// blend_fwd.hip's expressions, element for element (forward.cu:585-597)
				const float dx = qa.x - pixfx, dy = qa.y - pixfy;
				const float s2 = fmaf(qb.x * dy, dy, (qa.z * dx) * dx);
				const float power = fmaf(-0.5f, s2, -((qa.w * dx) * dy));
				const float alpha = fminf(0.99f, qb.y * __builtin_amdgcn_exp2f(power * 1.4426950408889634f));
				const float test_T = T * (1.0f - alpha);
				const lanemask valid = ~done & mask_of(!(power > 0.0f)) & mask_of(!(alpha < 1.0f / 255.0f));
				const lanemask low = mask_of(test_T < 0.0001f);
				const lanemask contrib = valid & ~low;
				const float w = mask_select(contrib, alpha * T, 0.0f);
				T = mask_select(contrib, test_T, T);
				done |= valid & low;
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

	hipError_t launch_contribution(const fdgs_contribution_in& in, const fdgs_contribution_out& out, const float* records,
	                               const uint32_t* point_list, const uint32_t* ranges, const uint32_t* tile_order, hipStream_t stream)
	{
		const int gx = div_up(in.W, TILE_X), gy = div_up(in.H, TILE_Y);
		const int ntiles = gx * gy;
		if (in.P >= (1 << 26)) return hipErrorInvalidValue;   // 32-bit byte offsets into the 48-byte records
#define LAUNCH_CONTRIB(WEIGHTED) hipLaunchKernelGGL(contribution_kernel<WEIGHTED>, dim3(blend_grid(ntiles)), dim3(WAVE), 0, stream, \
		                   reinterpret_cast<const uint2*>(ranges), point_list, reinterpret_cast<const float4*>(records), tile_order, \
		                   in.W, in.H, gx, ntiles, in.pix_weight, out.weight_sum, out.weight_max, out.hits, out.dominant, out.dominant_id)
		if (in.pix_weight != nullptr) LAUNCH_CONTRIB(true);
		else LAUNCH_CONTRIB(false);
#undef LAUNCH_CONTRIB
		return hipGetLastError();
	}
}
