// sh_bwd.hip -- SH / 4D-SH backward with coalesced HBM traffic (gfx950).
//
// The reference evaluates this inside its per-Gaussian backward kernel (computeColorFromSH / _4D,
// backward.cu:20-139, 144-481): every thread reads its own 12*M bytes of coefficients and writes its own
// 12*M bytes of dL_dsh with a 12*M-byte stride between threads.  At M = 48 that is 576 B in and 576 B out per
// Gaussian -- 80 % of all bytes the whole per-Gaussian backward moves -- so it gets its own kernel here:
//   * every output of the kernel is linear in the Gaussian's dL_dRGB, and a Gaussian that is visible but contributed to no
//     pixel (occluded, or too faint everywhere: 58 % of the visible ones on C3) has dL_dRGB == 0 exactly.  A wave walks
//     its range of consecutive Gaussians 64 at a time and ballot-compacts the LIVE ones (those with a colour gradient) into a list;
//     the others only get their zeros (the stage record / the dL_dsh row; their accumulator words 12..15 are zero already);
//   * whenever 64 live Gaussians are waiting (and at the end of the range) they are evaluated, one per lane: their rows are staged block by block (16 coefficients
//     = 192 B per Gaussian) through a wave-private LDS tile with coalesced dwordx4 loads (gathered rows, contiguous runs);
//   * each lane walks ITS Gaussian's row in LDS (row stride 49 floats: conflict free), accumulates the
//     direction / time dot products in registers and overwrites the row with dL_dsh;
//   * the tile is written back with coalesced dwordx4 stores.
//   (One lane per Gaussian of the span instead -- the first version -- left 13 of 64 lanes with work in the evaluation.)
// The four numbers the geometry backward needs from here -- the mean gradient through the view direction
// (3) and the time gradient (1) -- travel in the spare words 12..15 of the Gaussian's packed accumulator record.
//
// One table-driven formulation serves both the 3D and the 4D path: basis values l[k] and their x/y/z
// derivatives for k < 16; blocks 1 and 2 reuse them times cos(2 pi j dt / T).  Bug-compatible with the
// reference: Q1 dL_dsh[1] = l[0] * dRGB in the 4D path, Q2 sign of d cos/dt,
// Q3 the last time block overwrites dRGB/dt, Q4 view direction from the SHIFTED mean.  fdgs_scene.analytic_sh_grad
// (opt-in) switches Q1-Q3 to the analytic gradient of the forward pass.
//
// Where things live: the per-(Gaussian, view) evaluation -- liveness (sh_live), ShBwdEval::begin / block / finish with the tables,
// the time factors and Q1-Q4 -- and the launchers' float4 flag (sh_rows_vec_ok) are in sh_eval.h; dnormvdv is in fdgs_math.h.  This
// file holds what differs between the kernels: how rows travel between memory and LDS (sh_bwd_kernel: block by block, gathered
// rows; sh_bwd_batch_kernel: whole rows once for all views; sh_flush_kernel: whole rows out), the argument structs (ShModelArgs +
// ShViewArgs, one fill function each) and the launchers.
#pragma clang fp contract(off)
#include "fdgs_common.h"
#include "fdgs_math.h"
#include "sh_eval.h"

namespace fdgs
{
	constexpr int SHB_STRIDE = 49;   // LDS row stride in floats (odd: lane-per-row access is conflict free)
	constexpr int SHB_CH = 12;       // float4 chunks per Gaussian and block (16 coefficients x 3 / 4)
	constexpr int SHB_ROWS = WAVE;   // live Gaussians evaluated per round, one per lane (tile: 12.5 KB)

	// what the views of an optimizer step share, and what is a view's own: sh_bwd_kernel takes one view, sh_bwd_batch_kernel SBB_MAX
	struct ShModelArgs
	{
		int P, D, D_t, M;
		const float *shs, *ts;
		float time_duration;
		int gaussian_dim, force_sh_3d, analytic, vec_ok;
	};
	struct ShViewArgs
	{
		const float* campos; float timestamp;
		const int32_t* radii; const float* means; const uint8_t* clamped;
		float* gacc;
		float4* stage;   // deferred mode: [P][2] = (dRGB.xyz, cos factor of time block 1) (dir.xyz, cos factor of block 2) per Gaussian instead of dL_dsh (see sh_flush_kernel)
	};
	struct ShBwdArgs
	{
		ShModelArgs m; ShViewArgs v;
		int accum; float* dL_dsh;   // the dense gradient (not in deferred mode)
	};
	static void fill_sh_model(ShModelArgs& m, const fdgs_scene& s, bool vec_ok)
	{
		m.P = s.P; m.D = s.D; m.D_t = s.D_t; m.M = s.M;
		m.shs = s.shs; m.ts = s.ts; m.time_duration = s.time_duration;
		m.gaussian_dim = s.gaussian_dim; m.force_sh_3d = s.force_sh_3d; m.analytic = s.analytic_sh_grad;
		m.vec_ok = vec_ok ? 1 : 0;
	}
	static void fill_sh_view(ShViewArgs& v, const fdgs_scene& s, const fdgs_backward_in& in, const fdgs_backward_out& out, const char* geom)
	{
		v.campos = s.campos; v.timestamp = s.timestamp;
		v.radii = in.radii; v.means = in.out_means3D;
		v.clamped = reinterpret_cast<const uint8_t*>(geom + geom_layout(s.P).clamped);
		v.gacc = out.grad_accum; v.stage = reinterpret_cast<float4*>(out.sh_stage);
	}
	// the end of one (Gaussian, view) evaluation (sh_eval.h): the stage records (deferred mode) and words 12..15 of the accumulator record
	__device__ __forceinline__ void sh_bwd_finish(const ShBwdEval& e, const ShViewArgs& v, const ShPlan& plan, int idx, bool stage)
	{
		float4 s0, s1;
		const float4 words = e.finish(plan, s0, s1);
		if (stage) { v.stage[2 * (size_t)idx] = s0; v.stage[2 * (size_t)idx + 1] = s1; }
		reinterpret_cast<float4*>(v.gacc + (size_t)idx * GRAD_ACC_WORDS)[3] = words;
	}

	// ---- tile <-> global, coalesced; tile row r belongs to Gaussian g0 + list[r], r < nrows ----
	constexpr int SHB_BATCH = 6;     // float4 per lane in flight while staging (2 batches per block)
	__device__ __forceinline__ void rows_load16(float* __restrict__ tile, const float* __restrict__ src, const uint32_t* list, int nrows,
	                                            int g0, size_t row_floats, int first_float, int lane)
	{
#pragma unroll
		for (int b = 0; b < SHB_CH * SHB_ROWS / WAVE / SHB_BATCH; b++)
		{
			float4 v[SHB_BATCH];
#pragma unroll
			for (int i = 0; i < SHB_BATCH; i++)
			{
				const int c = (b * SHB_BATCH + i) * WAVE + lane, r = c / SHB_CH, q = c - r * SHB_CH;
				v[i] = r < nrows ? *reinterpret_cast<const float4*>(src + (size_t)(g0 + list[r]) * row_floats + first_float + 4 * q)
				                 : make_float4(0.f, 0.f, 0.f, 0.f);
			}
#pragma unroll
			for (int i = 0; i < SHB_BATCH; i++)
			{
				const int c = (b * SHB_BATCH + i) * WAVE + lane, r = c / SHB_CH, q = c - r * SHB_CH;
				float* d = tile + r * SHB_STRIDE + 4 * q;
				d[0] = v[i].x; d[1] = v[i].y; d[2] = v[i].z; d[3] = v[i].w;
			}
		}
	}
	__device__ __forceinline__ void rows_store16(const float* __restrict__ tile, float* __restrict__ dst, const uint32_t* list, int nrows,
	                                             int g0, size_t row_floats, int first_float, int lane, bool accum)
	{
#pragma unroll
		for (int i = 0; i < SHB_CH * SHB_ROWS / WAVE; i++)
		{
			const int c = i * WAVE + lane, r = c / SHB_CH, q = c - r * SHB_CH;
			if (r < nrows)
			{
				const float* t = tile + r * SHB_STRIDE + 4 * q;
				float4* d = reinterpret_cast<float4*>(dst + (size_t)(g0 + list[r]) * row_floats + first_float + 4 * q);
				float4 v = make_float4(t[0], t[1], t[2], t[3]);
				if (accum)
				{
					const float4 o = *d;
					v = make_float4(o.x + v.x, o.y + v.y, o.z + v.z, o.w + v.w);
				}
				*d = v;
			}
		}
	}
	// generic (any float count per row / alignment)
	__device__ __forceinline__ void rows_load_any(float* __restrict__ tile, const float* __restrict__ src, const uint32_t* list, int nrows,
	                                              int g0, size_t row_floats, int first_float, int nf, int lane)
	{
		RowWalk w(lane, nf);
		for (int e = lane; e < nrows * nf; e += WAVE)
		{
			tile[w.g * SHB_STRIDE + w.q] = src[(size_t)(g0 + list[w.g]) * row_floats + first_float + w.q];
			w.step();
		}
	}
	__device__ __forceinline__ void rows_store_any(const float* __restrict__ tile, float* __restrict__ dst, const uint32_t* list, int nrows,
	                                               int g0, size_t row_floats, int first_float, int nf, int lane, bool accum)
	{
		RowWalk w(lane, nf);
		for (int e = lane; e < nrows * nf; e += WAVE)
		{
			float* d = dst + (size_t)(g0 + list[w.g]) * row_floats + first_float + w.q;
			if (accum) *d += tile[w.g * SHB_STRIDE + w.q];
			else *d = tile[w.g * SHB_STRIDE + w.q];
			w.step();
		}
	}

	// One wave per workgroup: the tile is wave-private, so no workgroup barrier is needed anywhere (LDS
	// operations of one wave execute in order) and waves of different phases (load / compute / store) overlap freely.
	// The launch is 1.5 waves per wave slot the device has for this kernel (launcher), wave w takes the CHUNKS of 64 Gaussians
	// w, w + G, w + 2 G, ... (G = waves of the launch): chunks that far apart have nothing to do with each other even when
	// the model is stored in spatial order (where whole neighbourhoods are live or dead), so every wave gets about the same
	// number of live Gaussians.  It collects them and evaluates whenever 64 are waiting (and what is left at the end): the
	// evaluation's latency chain is paid per batch, and most waves need one.  (Fixed spans of 128 Gaussians per wave, the
	// previous version, made 1.14 rounds of two batches each, 64 + 9 rows.)
	// (A ticket counter handing out the chunks was built and measured at 0.19 ms: ~6700 returning atomics on one address.)
	template <bool STAGE>
	__global__ void __launch_bounds__(WAVE) sh_bwd_kernel(const ShBwdArgs a)
	{
		__shared__ float tile[SHB_ROWS * SHB_STRIDE];
		__shared__ uint32_t s_list[2 * WAVE];     // the live Gaussians waiting for evaluation
		const int lane = threadIdx.x;
		const ShModelArgs& m = a.m;
		const ShViewArgs& v = a.v;
		const size_t row_floats = (size_t)3 * m.M;
		const ShPlan plan = sh_plan(m.D, m.D_t, m.gaussian_dim, m.force_sh_3d, m.M);
		const unsigned long long lt_mask = (1ull << lane) - 1ull;
		const int nchunks = (m.P + WAVE - 1) / WAVE;

		int n = 0;      // live Gaussians waiting in s_list
		int next = blockIdx.x;
		bool more = true;
		while (more || n > 0)
		{
			if (more)
			{
				const int base = next * WAVE;
				if (next >= nchunks) { more = false; if (n == 0) break; }
				else
				{
				next += gridDim.x;
				const int g_end = m.P;
				// ---- which of the next 64 Gaussians carry a colour gradient (visible: backward.cu:873) ----
				const int idx = base + lane;
				const bool valid = idx < g_end;
				float3 dRGB;
				const bool live = valid && sh_live(v.radii, v.gacc, v.clamped, idx, dRGB);
				const unsigned long long live_mask = __ballot(live);
				if (live) s_list[n + __popcll(live_mask & lt_mask)] = (uint32_t)idx;
				n += __popcll(live_mask);
				// a Gaussian without a colour gradient: all of its outputs are zero.  Record words 12..15 already are (the record is
				// all zero when the blend backward starts and nobody else writes them); dL_dsh: below; the flush looks at dRGB only
				if (STAGE && valid && !live) v.stage[2 * (size_t)idx] = make_float4(0.f, 0.f, 0.f, 0.f);
				__builtin_amdgcn_wave_barrier();

				if (!STAGE && !a.accum)
				{
					// dL_dsh is fully written by this call: zero rows for the Gaussians without a colour gradient, zeros beyond the
					// active degrees for the others (nothing to add when accumulating)
					const int span = min(WAVE, g_end - base);
					if (m.vec_ok && (plan.act_floats & 3) == 0)
					{
						const int RC = (int)row_floats / 4, total = span * RC;
						RowWalk w(lane, RC);
						for (int c = lane; c < total; c += WAVE)
						{
							const bool lv = (live_mask >> w.g) & 1ull;
							if (!lv || 4 * w.q >= plan.act_floats)
								*reinterpret_cast<float4*>(a.dL_dsh + (size_t)(base + w.g) * row_floats + 4 * w.q) = make_float4(0.f, 0.f, 0.f, 0.f);
							w.step();
						}
					}
					else
					{
						const int rf = (int)row_floats, total = span * rf;
						RowWalk w(lane, rf);
						for (int e = lane; e < total; e += WAVE)
						{
							const bool lv = (live_mask >> w.g) & 1ull;
							if (!lv || w.q >= plan.act_floats) a.dL_dsh[(size_t)(base + w.g) * row_floats + w.q] = 0.f;
							w.step();
						}
					}
				}
				if (n < SHB_ROWS) continue;   // keep collecting
				}
			}

			// ---- up to 64 waiting live Gaussians, one per lane ----
			{
			constexpr int g0 = 0;    // the list holds Gaussian indices
			const int nrows = min(SHB_ROWS, n);
			const uint32_t* list = s_list;
			const bool live = lane < nrows;
			const int idx = g0 + (int)list[live ? lane : 0];
			float* row = tile + lane * SHB_STRIDE;
			// the evaluation (sh_eval.h) of the lane's Gaussian: it is on the list, so sh_live said yes -- its dRGB again
			ShBwdEval e;
			e.begin(plan, m.D, ld3(v.means, idx), v.campos, plan.sh3d ? 0.f : m.ts[idx], v.timestamp, sh_colour_gradient(v.gacc, v.clamped, idx));
			for (int blk = 0; blk < plan.nblocks; blk++)
			{
				const int nk = (blk == 0) ? plan.ncoef0 : 16;
				const int first_float = 48 * blk;
				const bool vec = m.vec_ok && nk == 16;
				if (vec) rows_load16(tile, m.shs, list, nrows, g0, row_floats, first_float, lane);
				else rows_load_any(tile, m.shs, list, nrows, g0, row_floats, first_float, 3 * nk, lane);
				__builtin_amdgcn_wave_barrier();
				if (live) e.block<!STAGE>(plan, m.analytic != 0, m.time_duration, row, nk, blk);
				__builtin_amdgcn_wave_barrier();
				if (!STAGE)
				{
					if (vec) rows_store16(tile, a.dL_dsh, list, nrows, g0, row_floats, first_float, lane, a.accum != 0);
					else rows_store_any(tile, a.dL_dsh, list, nrows, g0, row_floats, first_float, 3 * nk, lane, a.accum != 0);
					__builtin_amdgcn_wave_barrier();
				}
			}
			if (live) sh_bwd_finish(e, v, plan, idx, STAGE);
			// the Gaussians that did not fit into this batch move to the front of the list
			const int left = n - nrows;
			const uint32_t moved = lane < left ? s_list[nrows + lane] : 0u;
			__builtin_amdgcn_wave_barrier();
			if (lane < left) s_list[lane] = moved;
			n = left;
			__builtin_amdgcn_wave_barrier();
			}
		}
	}

	// wave slots of the device for a one-wave kernel (occupancy x CUs), per device
	template <typename K>
	static int resident_waves(K kernel)
	{
		int dev = 0, per_cu = 0, cus = 0;
		if (hipGetDevice(&dev) != hipSuccess) return 2048;
		if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, WAVE, 0) != hipSuccess || per_cu <= 0) per_cu = 8;
		if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
		return per_cu * cus;
	}


	hipError_t launch_sh_bwd(const fdgs_scene& s, const fdgs_backward_in& in, const fdgs_backward_out& out, const char* geom, hipStream_t stream)
	{
		if (s.shs == nullptr || s.M <= 0) return hipSuccess;
		ShBwdArgs a;
		fill_sh_model(a.m, s, sh_rows_vec_ok(s.M, s.shs, out.dL_dsh));
		fill_sh_view(a.v, s, in, out, geom);
		a.dL_dsh = out.dL_dsh; a.accum = out.accumulate;
		// one wave per wave slot the device has for this kernel (cached per device)
		constexpr int MAXDEV = 64;
		static int slots_of[2][MAXDEV] = {};   // same value whoever writes it first
		int dev = 0;
		(void)hipGetDevice(&dev);
		const int k = out.sh_stage ? 1 : 0;
		int& slots = slots_of[k][(unsigned)dev % MAXDEV];
		if (slots == 0) slots = k ? resident_waves(sh_bwd_kernel<true>) : resident_waves(sh_bwd_kernel<false>);
		// 1.5 waves per slot: ~1.5 chunks = ~55 live Gaussians per wave on C3, i.e. ONE evaluation batch for most waves and two
		// rounds of them (C3, random / Morton order: 41 / 42 us; one wave per slot 43 / 50; spans of 128 as before 52 / 43)
		const int grid = min(slots + slots / 2, div_up(s.P, WAVE));
		if (out.sh_stage) hipLaunchKernelGGL(sh_bwd_kernel<true>, dim3(grid), dim3(WAVE), 0, stream, a);
		else hipLaunchKernelGGL(sh_bwd_kernel<false>, dim3(grid), dim3(WAVE), 0, stream, a);
		return hipGetLastError();
	}

	// ------------------------------------------------------------------------------------------------
	// SH backward of SEVERAL views in one pass over the coefficients (fdgs_sh_backward_batch; deferred mode only).
	// What a view's SH backward has to read is the Gaussian's coefficient row (12 M bytes) -- the same row for every view of an
	// optimizer step.  Here a wave scans 64 consecutive Gaussians, ballot-compacts those that carry a colour gradient in ANY
	// view, and takes them 32 at a time: their WHOLE rows (the prefix the active degrees use) are staged once through a
	// wave-private LDS tile with linear float4 loads, and lane = (Gaussian, view parity) evaluates its Gaussian for the views
	// v = parity, parity + 2, ...: per view the 8 staged numbers for the flush (dL_dRGB, direction, the two cosine factors) and
	// the mean / time gradient in words 12..15 of the view's accumulator record.  The per-(Gaussian, view) evaluation is made of the same functions as
	// sh_bwd_kernel<true>'s (sh_eval.h: sh_live, ShBwdEval; sh_bwd_finish above): on the same accumulator records the two are equal
	// bit for bit (test_sh_backward_paths_bitwise).
	// ------------------------------------------------------------------------------------------------
	constexpr int SBB_MAX = 8;        // views per launch
	constexpr int SBB_ROWS = 32;
	constexpr int SBB_SPAN = 64;
	constexpr int SBB_ACT = 144;      // floats of the three coefficient blocks that can be active
	constexpr int SBB_STRIDE = SBB_ACT + 1;
	struct ShBwdBatchArgs
	{
		ShModelArgs m; int nviews;
		ShViewArgs v[SBB_MAX];
	};

	__global__ void __launch_bounds__(WAVE) sh_bwd_batch_kernel(const ShBwdBatchArgs a)
	{
		__shared__ float tile[SBB_ROWS * SBB_STRIDE];
		__shared__ uint32_t s_list[SBB_SPAN];
		const int lane = threadIdx.x;
		const int g0 = blockIdx.x * SBB_SPAN;
		const ShModelArgs& m = a.m;
		const int row_floats = 3 * m.M;
		const ShPlan plan = sh_plan(m.D, m.D_t, m.gaussian_dim, m.force_sh_3d, m.M);
		const unsigned long long lt_mask = (1ull << lane) - 1ull;

		// ---- which Gaussians of the span carry a colour gradient in some view; the others get their zero stage records ----
		int n = 0;
		{
			const int idx = g0 + lane;
			const bool valid = idx < m.P;
			bool any = false;
#pragma unroll 1
			for (int v = 0; v < a.nviews; v++)
			{
				float3 dRGB;
				const bool live = valid && sh_live(a.v[v].radii, a.v[v].gacc, a.v[v].clamped, idx, dRGB);
				if (valid && !live) a.v[v].stage[2 * (size_t)idx] = make_float4(0.f, 0.f, 0.f, 0.f);
				any = any || live;
			}
			const unsigned long long any_mask = __ballot(any);
			if (any) s_list[__popcll(any_mask & lt_mask)] = (uint32_t)lane;
			n = __popcll(any_mask);
		}
		__builtin_amdgcn_wave_barrier();

		const int g = lane & (SBB_ROWS - 1), vpar = lane >> 5;
		for (int r0 = 0; r0 < n; r0 += SBB_ROWS)
		{
			const int nrows = min(SBB_ROWS, n - r0);
			// ---- whole rows into the tile ----
			if (m.vec_ok && (plan.act_floats & 3) == 0)
			{
				const int RC = plan.act_floats / 4, total = nrows * RC;
				RowWalk w(lane, RC);
				for (int c0 = 0; c0 < total; c0 += 6 * WAVE)
				{
					float4 val[6];
					int og[6], oq[6];
#pragma unroll
					for (int i = 0; i < 6; i++)
					{
						og[i] = w.g; oq[i] = w.q;
						w.step();
						if (c0 + i * WAVE + lane >= total) og[i] = -1;
						else val[i] = *reinterpret_cast<const float4*>(m.shs + (size_t)(g0 + (int)s_list[r0 + og[i]]) * row_floats + 4 * oq[i]);
					}
#pragma unroll
					for (int i = 0; i < 6; i++)
					{
						if (og[i] < 0) continue;
						float* d = tile + og[i] * SBB_STRIDE + 4 * oq[i];
						d[0] = val[i].x; d[1] = val[i].y; d[2] = val[i].z; d[3] = val[i].w;
					}
				}
			}
			else
			{
				const int total = nrows * plan.act_floats;
				RowWalk w(lane, plan.act_floats);
				for (int e = lane; e < total; e += WAVE)
				{
					tile[w.g * SBB_STRIDE + w.q] = m.shs[(size_t)(g0 + (int)s_list[r0 + w.g]) * row_floats + w.q];
					w.step();
				}
			}
			__builtin_amdgcn_wave_barrier();

			// ---- lane = (row g, view parity): the views v = vpar, vpar + 2, ... of Gaussian list[r0 + g] ----
			if (g < nrows)
			{
				const int idx = g0 + (int)s_list[r0 + g];
				float* row = tile + g * SBB_STRIDE;
				const float t_in = plan.sh3d ? 0.f : m.ts[idx];
#pragma unroll 1
				for (int v = vpar; v < a.nviews; v += 2)
				{
					float3 dRGB;
					if (!sh_live(a.v[v].radii, a.v[v].gacc, a.v[v].clamped, idx, dRGB)) continue;
					ShBwdEval e;
					e.begin(plan, m.D, ld3(a.v[v].means, idx), a.v[v].campos, t_in, a.v[v].timestamp, dRGB);
					for (int blk = 0; blk < plan.nblocks; blk++)
						e.block<false>(plan, m.analytic != 0, m.time_duration, row + 48 * blk, (blk == 0) ? plan.ncoef0 : 16, blk);
					sh_bwd_finish(e, a.v[v], plan, idx, true);
				}
			}
			__builtin_amdgcn_wave_barrier();
		}
	}

	// views / ins / outs / geoms of the batch: all views share P, M, the degrees and the Gaussian tensors; outs[v]->sh_stage and
	// outs[v]->grad_accum are the view's own
	hipError_t launch_sh_bwd_batch(int nviews, const fdgs_scene* const* views, const fdgs_backward_in* const* ins,
	                               const fdgs_backward_out* const* outs, hipStream_t stream)
	{
		const fdgs_scene& s = *views[0];
		if (s.shs == nullptr || s.M <= 0 || s.P <= 0) return hipSuccess;
		for (int v0 = 0; v0 < nviews; v0 += SBB_MAX)
		{
			ShBwdBatchArgs a;
			fill_sh_model(a.m, s, sh_rows_vec_ok(s.M, s.shs));
			a.nviews = min(SBB_MAX, nviews - v0);
			for (int v = 0; v < SBB_MAX; v++)
			{
				const int w = min(v0 + v, nviews - 1);
				fill_sh_view(a.v[v], *views[w], *ins[w], *outs[w], reinterpret_cast<const char*>(ins[w]->geom_buffer));
			}
			hipLaunchKernelGGL(sh_bwd_batch_kernel, dim3(div_up(s.P, SBB_SPAN)), dim3(WAVE), 0, stream, a);
		}
		return hipGetLastError();
	}

	// ------------------------------------------------------------------------------------------------
	// Deferred SH gradient (gradient accumulation over the views of one optimizer step).
	// dL_dsh of a view is basis(view direction) x time factor (x) dL_dRGB: M x 3 floats written (or read-modified-written,
	// from the second view on) per Gaussian and view, although the view only contributes 8 numbers.  In deferred mode
	// (fdgs_backward_out.sh_stage) sh_bwd_kernel stores those 8 numbers per view and this kernel, once per step, rebuilds
	// the views' contributions in registers and sums them in view order -- the same additions in the same order as the
	// accumulating path.  Two consumers:
	//   MODE 0 (fdgs_sh_flush)      dL_dsh is written once: at C3 / 4 views 1.7 KB of traffic per live Gaussian and view
	//                               become 0.6 KB + 0.6 KB / 4;
	//   MODE 1 (fdgs_adam_step_sh)  the only reader of the summed dL_dsh is the Adam update of the SH coefficients
	//                               (train.py:247-249; 89 % of all parameters at M = 48), so the gradient goes from the LDS
	//                               tile straight into it: read p, m, v, write p, m, v (24 B per coefficient) and dL_dsh
	//                               never travels through memory (it is also written when the caller asks for it).
	// A wave owns 32 consecutive Gaussians; lane = (Gaussian, half of the 16 coefficients of a block), the three possible
	// coefficient blocks accumulate in registers and land in a wave-private LDS tile of whole rows, so that the output phase
	// walks memory strictly linearly (32 x 12 M bytes per array) -- the block-by-block sweeps of sh_bwd_kernel touch every
	// 128-byte line of the 576-byte rows up to three times.
	// ------------------------------------------------------------------------------------------------
	constexpr int SHF_GPW = 32;
	// LDS row stride of the flush tile: the active blocks' floats + 1 (odd: lane-per-row accesses are conflict free)
	__host__ __device__ static inline int shf_tile_stride(const ShPlan& plan) { return 48 * plan.nblocks + 1; }
#ifndef FDGS_SHF_BATCH
#define FDGS_SHF_BATCH 6
#endif
	constexpr int SHF_BATCH = FDGS_SHF_BATCH;   // float4 chunks per lane whose p / m / v loads are in flight together

	struct ShFlushArgs
	{
		int P, D, D_t, M, nviews, gaussian_dim, force_sh_3d, analytic, accum, vec_ok;
		const float4* stages;   // [nviews][P][2]
		float* dL_dsh;
		float *p, *m, *v;       // MODE 1
		AdamScalars k;
	};

	template <int MODE>
	__global__ void __launch_bounds__(WAVE) sh_flush_kernel(const ShFlushArgs a)
	{
		// the tile holds the coefficient blocks that can carry a gradient: 48 floats per active block and Gaussian, + 1 (odd stride); its
		// size is the launch's dynamic LDS (one active block -- 3D SH, M = 16, or the first iterations of the degree ramp -- takes a
		// third of the three-block tile: more waves per CU for the streaming phase)
		extern __shared__ float tile[];
		const int lane = threadIdx.x, g = lane & (SHF_GPW - 1), half = lane >> 5;
		const int g0 = blockIdx.x * SHF_GPW;
		const bool valid = g0 + g < a.P;
		const int idx = valid ? g0 + g : a.P - 1;
		const int row_floats = 3 * a.M;
		const ShPlan plan = sh_plan(a.D, a.D_t, a.gaussian_dim, a.force_sh_3d, a.M);
		const int stride = shf_tile_stride(plan);
		const int tile_floats = min(stride - 1, row_floats);   // row prefix the tile holds: whole blocks (zeros beyond plan.act_floats)

		float3 acc[3][8];
#pragma unroll
		for (int b = 0; b < 3; b++)
#pragma unroll
			for (int j = 0; j < 8; j++) acc[b][j] = make_float3(0.f, 0.f, 0.f);
		bool any = false;
		for (int v = 0; v < a.nviews; v++)
		{
			const float4 s0 = a.stages[2 * ((size_t)v * a.P + idx)];
			const float3 dRGB = make_float3(s0.x, s0.y, s0.z);
			if (!valid || (dRGB.x == 0.f && dRGB.y == 0.f && dRGB.z == 0.f)) continue;   // this view added nothing
			const float4 s1 = a.stages[2 * ((size_t)v * a.P + idx) + 1];
			any = true;
			float l[16];
			sh_values(a.D, s1.x, s1.y, s1.z, !plan.sh3d, l);
#pragma unroll
			for (int j = 0; j < 8; j++)
			{
				const int k = 8 * half + j;
				const float lk = half ? l[8 + j] : l[j];
				const float basis = k < plan.ncoef0 ? sh_grad_basis0(k, lk, l[0], plan, a.analytic != 0) : 0.f;   // Q1: as sh_bwd_kernel<false>
				acc[0][j] = add3(acc[0][j], scl3(basis, dRGB));
				if (plan.nblocks > 1) acc[1][j] = add3(acc[1][j], scl3(s0.w * lk, dRGB));
				if (plan.nblocks > 2) acc[2][j] = add3(acc[2][j], scl3(s1.w * lk, dRGB));
			}
		}
		const unsigned long long vmask = __ballot(any);   // bit g (and g + 32)
		if (any)
		{
			float* row = tile + g * stride + 24 * half;
#pragma unroll
			for (int b = 0; b < 3; b++)
			{
				if (b >= plan.nblocks) break;
#pragma unroll
				for (int j = 0; j < 8; j++)
				{
					row[48 * b + 3 * j] = acc[b][j].x; row[48 * b + 3 * j + 1] = acc[b][j].y; row[48 * b + 3 * j + 2] = acc[b][j].z;
				}
			}
		}
		__builtin_amdgcn_wave_barrier();

		if (MODE == 1 || a.vec_ok)
		{
			// whole rows, float4 by float4, linearly through memory: chunk c of the wave = (Gaussian c / RC, float4 c % RC of its row)
			const int RC = row_floats / 4, total = SHF_GPW * RC;
			RowWalk w(lane, RC);
			for (int c0 = 0; c0 < total; c0 += SHF_BATCH * WAVE)
			{
				float4 pp[SHF_BATCH], mm[SHF_BATCH], vv[SHF_BATCH];
				int og[SHF_BATCH], oq[SHF_BATCH];
#pragma unroll
				for (int i = 0; i < SHF_BATCH; i++)
				{
					og[i] = w.g; oq[i] = w.q;
					w.step();
					const bool in = c0 + i * WAVE + lane < total && g0 + og[i] < a.P;
					if (!in) og[i] = -1;
					if (MODE == 1 && in)
					{
						const size_t o = (size_t)(g0 + og[i]) * row_floats + 4 * oq[i];
						pp[i] = *reinterpret_cast<const float4*>(a.p + o);
						mm[i] = stream_ld(reinterpret_cast<const float4*>(a.m + o));   // the moments: once per step, non-temporal (fdgs_common.h)
						vv[i] = stream_ld(reinterpret_cast<const float4*>(a.v + o));
					}
				}
#pragma unroll
				for (int i = 0; i < SHF_BATCH; i++)
				{
					if (og[i] < 0) continue;
					const int e0 = 4 * oq[i];
					const bool live = ((vmask >> og[i]) & 1ull) && e0 < tile_floats;
					const float* t = tile + og[i] * stride + e0;
					float ge[4] = { 0.f, 0.f, 0.f, 0.f };
					if (live) { ge[0] = t[0]; ge[1] = t[1]; ge[2] = t[2]; ge[3] = t[3]; }
					const size_t o = (size_t)(g0 + og[i]) * row_floats + e0;
					if (MODE == 1)
					{
						float pe[4] = { pp[i].x, pp[i].y, pp[i].z, pp[i].w }, me[4] = { mm[i].x, mm[i].y, mm[i].z, mm[i].w };
						float ve[4] = { vv[i].x, vv[i].y, vv[i].z, vv[i].w };
#pragma unroll
						for (int e = 0; e < 4; e++)
						{
							// the DC coefficient (first 3 floats of the row) has its own learning rate (gaussian_model.py:339-340)
							const float lr = (e0 == 0 && e < 3) ? a.k.lr_head_bc1 : a.k.lr_bc1;
							adam_update(pe[e], me[e], ve[e], ge[e], lr, a.k.b1, a.k.b2, a.k.eps, a.k.inv_sqrt_bc2);
						}
						stream_st(reinterpret_cast<float4*>(a.m + o), make_float4(me[0], me[1], me[2], me[3]));
						stream_st(reinterpret_cast<float4*>(a.v + o), make_float4(ve[0], ve[1], ve[2], ve[3]));
						*reinterpret_cast<float4*>(a.p + o) = make_float4(pe[0], pe[1], pe[2], pe[3]);
						if (a.dL_dsh) *reinterpret_cast<float4*>(a.dL_dsh + o) = make_float4(ge[0], ge[1], ge[2], ge[3]);
					}
					else
					{
						float4* d = reinterpret_cast<float4*>(a.dL_dsh + o);
						if (!a.accum) *d = make_float4(ge[0], ge[1], ge[2], ge[3]);
						else if (live)
						{
							const float4 old = *d;
							*d = make_float4(old.x + ge[0], old.y + ge[1], old.z + ge[2], old.w + ge[3]);
						}
					}
				}
			}
		}
		else
		{
			// any row length / alignment, float by float
			const int total = SHF_GPW * row_floats;
			RowWalk w(lane, row_floats);
			for (int e = lane; e < total; e += WAVE)
			{
				if (g0 + w.g < a.P)
				{
					const bool live = ((vmask >> w.g) & 1ull) && w.q < tile_floats;
					float* d = a.dL_dsh + (size_t)(g0 + w.g) * row_floats + w.q;
					if (!a.accum) *d = live ? tile[w.g * stride + w.q] : 0.f;
					else if (live) *d += tile[w.g * stride + w.q];
				}
				w.step();
			}
		}
	}

	static void fill_flush_args(ShFlushArgs& a, int P, int D, int D_t, int M, int gaussian_dim, int force_sh_3d, int analytic, int nviews,
	                            const float* stages, float* dL_dsh)
	{
		a.P = P; a.D = D; a.D_t = D_t; a.M = M; a.nviews = nviews;
		a.gaussian_dim = gaussian_dim; a.force_sh_3d = force_sh_3d;
		a.analytic = analytic; a.accum = 0;
		a.vec_ok = sh_rows_vec_ok(M, dL_dsh) ? 1 : 0;
		a.stages = reinterpret_cast<const float4*>(stages);
		a.dL_dsh = dL_dsh;
		a.p = a.m = a.v = nullptr;
		a.k = AdamScalars{};
	}

	hipError_t launch_sh_flush(int P, int D, int D_t, int M, int gaussian_dim, int force_sh_3d, int analytic, int nviews,
	                           const float* stages, float* dL_dsh, int accumulate, hipStream_t stream)
	{
		if (P <= 0 || M <= 0 || nviews <= 0) return hipSuccess;
		ShFlushArgs a;
		fill_flush_args(a, P, D, D_t, M, gaussian_dim, force_sh_3d, analytic, nviews, stages, dL_dsh);
		a.accum = accumulate;
		hipLaunchKernelGGL(sh_flush_kernel<0>, dim3(div_up(P, SHF_GPW)), dim3(WAVE), (size_t)SHF_GPW * shf_tile_stride(sh_plan(D, D_t, gaussian_dim, force_sh_3d, M)) * sizeof(float), stream, a);
		return hipGetLastError();
	}

	hipError_t launch_sh_adam(int P, int D, int D_t, int M, int gaussian_dim, int force_sh_3d, int analytic, int nviews,
	                          const float* stages, float* params, float* exp_avg, float* exp_avg_sq, float* dL_dsh,
	                          const AdamScalars& k, hipStream_t stream)
	{
		if (P <= 0 || M <= 0) return hipSuccess;
		// the DC learning rate is applied to the first 3 floats of a row: rows must start on a float4 boundary
		if (nviews <= 0 || !sh_rows_vec_ok(M, params, exp_avg, exp_avg_sq, dL_dsh)) return hipErrorInvalidValue;
		ShFlushArgs a;
		fill_flush_args(a, P, D, D_t, M, gaussian_dim, force_sh_3d, analytic, nviews, stages, dL_dsh);
		a.p = params; a.m = exp_avg; a.v = exp_avg_sq; a.k = k;
		hipLaunchKernelGGL(sh_flush_kernel<1>, dim3(div_up(P, SHF_GPW)), dim3(WAVE), (size_t)SHF_GPW * shf_tile_stride(sh_plan(D, D_t, gaussian_dim, force_sh_3d, M)) * sizeof(float), stream, a);
		return hipGetLastError();
	}
}
