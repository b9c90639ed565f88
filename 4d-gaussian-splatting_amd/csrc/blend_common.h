// blend_common.h -- pieces shared by the forward and backward blend kernels (gfx950, wave64).
//
// Work decomposition: one wave64 (= one 64-thread workgroup) owns one 8x8 pixel
// block, four blocks per 16x16 tile.  The tile list itself (point_list / ranges) is
// the reference's AABB list, bit-identical to the oracle (with fdgs_forward_out.tile_cull: that list
// without the instances that cannot reach alpha >= 1/255 in the tile, preprocess_fwd.hip); what changes is how a wave
// consumes it: each lane fetches ONE list entry, tests whether that Gaussian can
// reach alpha >= 1/255 anywhere inside the wave's pixel block (exact minimum of the
// conic quadratic over the block rectangle, conservative slack), and the survivors
// are ballot-compacted into a wave-private LDS queue.  On the C3 workload only ~43 %
// of (entry, block) pairs survive, and every survivor costs the 64 lanes the full
// per-pixel evaluation, so the test (done once per entry by one lane) removes more
// than half of the blend arithmetic without changing a single pixel: an entry is
// dropped only if the per-pixel test (alpha < 1/255, reference forward.cu:590) would
// have rejected it for every pixel of the block.  List positions are kept so
// n_contrib keeps the reference's meaning (position in the full tile list).
#pragma once
#include "fdgs_common.h"

namespace fdgs
{
	constexpr int BLK = 8;        // pixel block edge per wave
	constexpr int NUM_XCDS = 8;

	__device__ __forceinline__ float fast_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.4426950408889634f); }

	// Lane predicates as wave masks.  A predicate that is the AND of several compares costs the compiler a
	// v_cndmask(0/1) + v_cmp_ne pair whenever a ballot of it is needed; keeping the compares as 64-bit masks (one v_cmp each,
	// combined on the scalar unit) and selecting with the mask directly avoids both.  Uniform control flow only (all 64 lanes active).
	typedef unsigned long long lanemask;
	__device__ __forceinline__ lanemask mask_of(bool pred) { return __builtin_amdgcn_ballot_w64(pred); }
	// mask bit set ? a : b
	__device__ __forceinline__ float mask_select(lanemask m, float a, float b)
	{
		float r;
		asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(b), "v"(a), "s"(m));
		return r;
	}
	__device__ __forceinline__ uint32_t mask_select(lanemask m, uint32_t a, uint32_t b)
	{
		uint32_t r;
		asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(b), "v"(a), "s"(m));
		return r;
	}

	// float4 k of Gaussian id's 48-byte blend record: uniform base + 32-bit byte offset (P < 2^26, checked by the launchers), so
	// that the gather needs one multiply-add per lane instead of 64-bit pointer arithmetic
	__device__ __forceinline__ float4 record_word(const float4* __restrict__ records, uint32_t id, uint32_t k)
	{
		return *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(records) + (id * 48u + 16u * k));
	}

	struct BlockId { int tile, sub; };
	// Workgroup id -> (tile, 8x8 sub-block).  Workgroups are dealt round-robin to the 8 XCDs (id % 8): the 4 sub-blocks of a tile stay on
	// one XCD (the shared list and records in one L2), and position p of the tile order goes to XCD p % 8.  `order` (tilebin.hip,
	// tile_order_block) lists ALL tiles longest-first, so every XCD gets the same share of the long and the short lists and ends its
	// part of the launch on short tiles (the ramp-down of a 21 760-workgroup launch in index order was ~10 % of its duration; with the
	// longest-first order inside a contiguous eighth of the tiles per XCD -- rounds 2-4 -- the XCDs' unequal shares of the scene cost
	// the blend kernels another 16 % on the bench's cameras); NULL: index order, dealt out the same way.
	__device__ __forceinline__ BlockId block_of(int wg, int ntiles, const uint32_t* __restrict__ order)
	{
		const int xcd = wg % NUM_XCDS, k = wg / NUM_XCDS;
		BlockId b;
		b.sub = k & 3;
		const int p = (k >> 2) * NUM_XCDS + xcd;   // may be >= ntiles at the end of the grid: the caller returns
		b.tile = (order != nullptr && p < ntiles) ? (int)order[p] : p;
		return b;
	}
	static inline int blend_grid(int ntiles) { return div_up(ntiles, NUM_XCDS) * NUM_XCDS * 4; }

	// Can the Gaussian (record words a = (x, y, conic.x, conic.y), b = (conic.z, opacity, ..))
	// reach alpha >= 1/255 at some point of the rectangle [rx0,rx1] x [ry0,ry1] (pixel centres)?
	// alpha = opacity * exp(-q), q(d) = 0.5 (A dx^2 + C dy^2) + B dx dy  ==>  need min q <= ln(255 opacity).
	// The minimum of the convex q over the rectangle is 0 if the mean is inside, otherwise it lies
	// on an edge that faces the mean (1-D quadratics, clamped).  Slack 0.05 in q (5 % in alpha) covers
	// every rounding difference to the per-pixel evaluation; degenerate conics are never culled.
	__device__ __forceinline__ bool block_reaches(const float4 a, const float4 b, float rx0, float rx1, float ry0, float ry1)
	{
		const float A = a.z, B = a.w, Cc = b.x, op = b.y;
		if (!(op >= 0.0039f)) return false;                 // alpha <= opacity < 1/255 (1/255 = 0.003922)
		// degenerate conics, and conics that are not positive definite with a margin (a needle of 300 : 1 whose determinant has
		// lost its bits): never culled -- what follows needs q convex
		if (!(A > 0.0f && Cc > 0.0f && A * Cc > 1.00001f * (B * B))) return true;
		const float dx0 = rx0 - a.x, dx1 = rx1 - a.x, dy0 = ry0 - a.y, dy1 = ry1 - a.y;
		const bool xin = dx0 <= 0.0f && dx1 >= 0.0f, yin = dy0 <= 0.0f && dy1 >= 0.0f;
		if (xin && yin) return true;
		// 255 op >= 0.99: normal range; v_log_f32 (log2, 1 ulp) is exact enough by five orders of magnitude for a bound with 0.05 of slack
		const float tau = __builtin_amdgcn_logf(255.0f * op) * 0.69314718056f + 0.05f;
		// A convex q takes its minimum over the rectangle on an edge that FACES the mean (the mean strictly beyond the edge's
		// line: at the minimiser p the direction towards the mean leaves the rectangle, and it can only leave it through a
		// constraint that is active at p).  That is at most one vertical and one horizontal edge.
		const float ex = dx0 > 0.0f ? dx0 : dx1, ey = dy0 > 0.0f ? dy0 : dy1;
		const float invA = __builtin_amdgcn_rcpf(A), invC = __builtin_amdgcn_rcpf(Cc);
		const float dyv = __builtin_amdgcn_fmed3f(-B * ex * invC, dy0, dy1);   // clamp (dy0 <= dy1)
		const float qv = 0.5f * (A * ex * ex + Cc * dyv * dyv) + B * ex * dyv;
		const float dxh = __builtin_amdgcn_fmed3f(-B * ey * invA, dx0, dx1);
		const float qh = 0.5f * (A * dxh * dxh + Cc * ey * ey) + B * dxh * ey;
		const float qmin = fminf(xin ? 3.0e38f : qv, yin ? 3.0e38f : qh);
		return qmin <= tau;
	}

	// ---- the wave's pixel block and the walk of a tile's list: stated once, for every kernel that takes a forward's lists ----
	// blend_fwd.hip, blend_bwd.hip, contribution.hip and features.hip all start from pixel_block; the walk itself is fetch_and_cull
	// (one list entry per lane, culled against the block) -> queue_chunk (the survivors, in list order, into the wave-private queue)
	// -> blend_weight per queued entry (entry_alpha, then blend_step: the decisions of forward.cu:585-597).  A change to the cull or
	// to the transmittance logic is made here, once -- and in the copies the two timed kernels keep, each marked with the name of the
	// function it mirrors, because built on the function they compile to other code: fetch_and_cull and blend_step in blend_fwd.hip
	// (which shares pixel_block and, in its debug kernel, entry_alpha), pixel_block in blend_bwd.hip (which reads the forward's cull
	// planes instead of testing again).

	// The 8x8 pixel block of a workgroup and this lane's pixel in it.
	struct PixelBlock
	{
		int tile, sub;                // tile index, 8x8 sub-block of the tile (0..3)
		int bx0, by0;                 // the block's first pixel
		int px, py;                   // this lane's pixel
		bool inside;                  // ... is inside the image
		float pixfx, pixfy;           // ... as floats
		float rx0, rx1, ry0, ry1;     // pixel-centre bounds of the block, clamped to the image (block_reaches)
		unsigned long long lt_mask;   // the lanes below this one
	};
	// false: nothing to do (beyond the grid's padding, or entirely outside the image)
	__device__ __forceinline__ bool pixel_block(int wg, int ntiles, const uint32_t* __restrict__ tile_order, int grid_x, int W, int H, int lane,
	                                            PixelBlock& pb)
	{
		const BlockId blk = block_of(wg, ntiles, tile_order);
		if (blk.tile >= ntiles) return false;
		pb.tile = blk.tile;
		pb.sub = blk.sub;
		pb.bx0 = (blk.tile % grid_x) * TILE_X + (blk.sub & 1) * BLK;
		pb.by0 = (blk.tile / grid_x) * TILE_Y + (blk.sub >> 1) * BLK;
		if (pb.bx0 >= W || pb.by0 >= H) return false;
		pb.px = pb.bx0 + (lane & (BLK - 1));
		pb.py = pb.by0 + (lane >> 3);
		pb.inside = pb.px < W && pb.py < H;
		pb.pixfx = (float)pb.px;
		pb.pixfy = (float)pb.py;
		pb.rx0 = (float)pb.bx0;
		pb.rx1 = (float)min(pb.bx0 + BLK - 1, W - 1);
		pb.ry0 = (float)pb.by0;
		pb.ry1 = (float)min(pb.by0 + BLK - 1, H - 1);
		pb.lt_mask = (1ull << lane) - 1ull;
		return true;
	}

	// List position `pos` of the n entries the range holds: this lane fetches the entry's Gaussian id and record words a, b (meaningful
	// where `keep`) and tests it against the block.  Returns the wave's mask of survivors.
	__device__ __forceinline__ unsigned long long fetch_and_cull(const uint32_t* __restrict__ point_list, const float4* __restrict__ records,
	                                                             const uint2 range, const int n, const int pos, const PixelBlock& pb, bool& keep,
	                                                             uint32_t& id, float4& a, float4& b)
	{
		keep = false;
		id = 0;
		if (pos < n)
		{
			id = point_list[range.x + pos];
			a = record_word(records, id, 0);
			b = record_word(records, id, 1);
			keep = block_reaches(a, b, pb.rx0, pb.rx1, pb.ry0, pb.ry1);
		}
		return __ballot(keep);
	}

	// One chunk of a tile's list (entries [base, base + 64) of n): the survivors of fetch_and_cull go, in list order, into the
	// wave-private queue as (x, y, conic.x, conic.y) and (conic.z, opacity, Gaussian id, -).  Returns the number queued; `id` / `slot`:
	// this lane's Gaussian and its queue slot (meaningful where `keep`).  The caller puts a __syncthreads() between this and its reads
	// of the queue.
	__device__ __forceinline__ int queue_chunk(const uint32_t* __restrict__ point_list, const float4* __restrict__ records, const uint2 range,
	                                           const int n, const int base, const int lane, const PixelBlock& pb, float4* s_qa, float4* s_qb,
	                                           bool& keep, uint32_t& id, int& slot)
	{
		float4 a, b;
		const unsigned long long mask = fetch_and_cull(point_list, records, range, n, base + lane, pb, keep, id, a, b);
		slot = 0;
		if (keep)
		{
			slot = __popcll(mask & pb.lt_mask);   // list order is preserved
			s_qa[slot] = a;
			s_qb[slot] = make_float4(b.x, b.y, __uint_as_float(id), 0.0f);
		}
		return __popcll(mask);
	}

	// alpha of the entry with record words a = (x, y, conic.x, conic.y), b = (conic.z, opacity, ..) at pixel (pixfx, pixfy), and the
	// exponent `power`: the reference's association per element (forward.cu:585-590), FMA, hardware exp2.  blend_fwd.hip and
	// blend_bwd.hip evaluate the same expressions on two entries at once (packed fp32).
	__device__ __forceinline__ float entry_alpha(const float4 a, const float4 b, const float pixfx, const float pixfy, float& power)
	{
		const float dx = a.x - pixfx, dy = a.y - pixfy;
		const float s2 = fmaf(b.x * dy, dy, (a.z * dx) * dx);
		power = fmaf(-0.5f, s2, -((a.w * dx) * dy));
		return fminf(0.99f, b.y * __builtin_amdgcn_exp2f(power * 1.4426950408889634f));
	}

	// forward.cu:588-597 on lane masks: valid = not finished, power <= 0, alpha >= 1/255; a valid entry that would take T below 1e-4
	// finishes the pixel (and is not counted), any other valid entry contributes.  Returns the blending weight w = alpha * T (0 where
	// the entry does not contribute), steps T and `done`; `contrib`: the lanes it contributes to.
	__device__ __forceinline__ float blend_step(const float alpha, const float power, float& T, lanemask& done, lanemask& contrib)
	{
		const float test_T = T * (1.0f - alpha);
		const lanemask valid = ~done & mask_of(!(power > 0.0f)) & mask_of(!(alpha < 1.0f / 255.0f));
		const lanemask low = mask_of(test_T < 0.0001f);
		contrib = valid & ~low;
		const float w = mask_select(contrib, alpha * T, 0.0f);
		T = mask_select(contrib, test_T, T);
		done |= valid & low;
		return w;
	}

	// One queued entry at this lane's pixel: its blending weight (see blend_step)
	__device__ __forceinline__ float blend_weight(const float4 qa, const float4 qb, const float pixfx, const float pixfy, float& T,
	                                              lanemask& done, lanemask& contrib)
	{
		float power;
		const float alpha = entry_alpha(qa, qb, pixfx, pixfy, power);
		return blend_step(alpha, power, T, done, contrib);
	}
}
