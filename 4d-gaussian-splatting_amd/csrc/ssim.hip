// ssim.hip -- fused photometric loss (1-l) L1 + l (1 - SSIM), forward and backward (gfx950).
//
// The step right after the rasterizer in every training iteration (reference train.py:115-117,
// utils/loss_utils.py:17-64): L1 + SSIM with an 11x11 Gaussian window (sigma 1.5, zero padding,
// C1 = 0.01^2, C2 = 0.03^2, mean over all pixels and channels).  The reference runs it as five
// grouped 11x11 convolutions forward plus their backward through the DL library; on ROCm that
// is ~7.6 ms per 1352x1014 image, four times the whole rasterizer.  Here:
//   forward : one pass.  A 32x32 output tile loads its 42x42 halo of both images into LDS as pairs (u, v) = (x + y, x - y), does
//             the separable window (horizontal, then vertical) for FOUR moments (u, v, u^2, v^2: round 6 -- the window statistics SSIM
//             needs follow from them, see the kernel; rounds 1-5: five, x, y, x^2, y^2, xy), evaluates SSIM and the three partial derivatives
//             d ssim/d mu1, d ssim/d E[x^2], d ssim/d E[xy] per pixel (kept for the backward),
//             and writes per-tile partial sums of |x-y| and ssim (summed by the host: deterministic).
//             The kernel is VALU-issue bound (SQ counters), so it is written for instruction count: the
//             moments travel as pairs (u,v) (u^2,v^2) -> two packed-fp32 FMAs per tap (rounds 2-5: (x,y) (x^2,y^2) + xy: three; before: five);
//             a thread produces 4 adjacent outputs of the horizontal pass (14 b128-loaded inputs instead of
//             44 scalar reads) and 4 adjacent rows of the vertical pass (14 row reads per 4 outputs).  Round 4: 32x32 tile
//             instead of 32x16 (halo 1.72 x instead of 2.13 x the tile, 1.31 instead of 1.63 rows of horizontal pass per
//             output row) with the input tile's LDS bytes reused for the filtered arrays: forward + backward 85.5 -> 76 us
//             per 1352x1014 image.
//   backward: dL/dx(p) = w_l1 sign(x-y) + w_ssim [ (W * dmu1)(p) + 2 x(p) (W * dE11)(p) + y(p) (W * dE12)(p) ]
//             -- three more separable windows over the stored derivative maps (W symmetric).
// fp32, ~200 VALU instructions per pixel-channel forward, ~100 backward; no MFMA (11-tap separable stencil).
// The window machinery itself -- halo load, horizontal and vertical passes, SSIM algebra, tile sums -- is ssim_window.h, shared with metrics.hip.
#include <cstdlib>
#include "ssim_window.h"

namespace fdgs
{
	constexpr int STX = 32, STY = 32;    // output tile
	constexpr int SROWS = STY / 8;       // adjacent output rows a thread finishes in the vertical pass (256 threads = 32 columns x 8 row groups)
	constexpr int SHH = STY + 2 * SR;    // 42: rows of tile + halo (and columns: STX + 2 * SR)
	// LDS row strides (16-byte aligned rows for the b128 accesses), chosen for the banks.  In the horizontal pass 8 threads take a
	// row and a wave 8 rows; a thread's b128 touches 4 of every 8 dwords of a pair-array row, so consecutive rows must be offset by
	// 4 (mod 8) dwords or all 8 rows fall on the same half of the banks (measured with strides 44 / 36: 41 % of the backward's LDS
	// cycles were bank conflicts): 46 and 38 pairs = 92 and 76 dwords.  Scalar arrays read / written 32 dwords per row: 48 (rows 0,
	// 48, 32, 16 mod 64: every bank four times per b128, the minimum).  Effect: 86 -> 85 us for forward + backward: the conflicts were not what holds the
	// kernels at 74 % / 52 % of their VALU issue bound.
	constexpr int SSTR = 46;             // input tile, in (x,y) pairs
	constexpr int SSTR1 = 48;            // input tile of the backward's scalar map
	constexpr int HSTR = 38;             // horizontally filtered moments, pair arrays
	constexpr int HSTR1B = 36;           // ... of the backward (48 would cost its sixth workgroup per CU)

	__global__ void __launch_bounds__(STHREADS) ssim_fwd_kernel(
		const float* __restrict__ img1, const float* __restrict__ img2, int C, int H, int W,
		float* __restrict__ dm_dmu1, float* __restrict__ dm_de11, float* __restrict__ dm_de12,
		float* __restrict__ partial_l1, float* __restrict__ partial_ssim)
	{
		// The input tile shares its bytes with two of the three horizontally filtered arrays: those results wait in registers until
		// every task of the horizontal pass has read its inputs (a barrier in between).  A workgroup then holds 34 KB instead of 49
		// (32-row tile): four workgroups per CU instead of three.  (All three behind the barrier: 16 more VGPRs for nothing -- the
		// results are larger than the inputs.)
		// Round 6: FOUR moment channels instead of five, all of them packed pairs.  With u = x + y, v = x - y the window statistics SSIM
		// needs are E[u], E[v], E[u^2], E[v^2] (ssim_from_uv) -- the scalar fifth channel x y (a plain FMA per tap next to two packed ones,
		// and per pair of outputs four register moves the compiler needed to feed it to a packed multiply) is gone: 3 -> 2 instructions per
		// tap, one LDS array less (28 instead of 34 KB: five workgroups per CU instead of four).
		constexpr int IN_BYTES = SHH * SSTR * 8, HM_BYTES = SHH * HSTR * 8;
		constexpr int SH_BYTES = IN_BYTES > HM_BYTES ? IN_BYTES : HM_BYTES;
		__shared__ __attribute__((aligned(16))) char s_raw[HM_BYTES + SH_BYTES];
		v2f (*h_m)[HSTR] = reinterpret_cast<v2f (*)[HSTR]>(s_raw);                                   // horizontally filtered (u, v)
		v2f (*s_in)[SSTR] = reinterpret_cast<v2f (*)[SSTR]>(s_raw + HM_BYTES);                       // (u, v) = (x + y, x - y)
		v2f (*h_s)[HSTR] = reinterpret_cast<v2f (*)[HSTR]>(s_raw + HM_BYTES);                        // (u^2, v^2): over the input tile
		__shared__ float red[2][STHREADS / WAVE];

		const TileId tile = tile_of((W + STX - 1) / STX, (H + STY - 1) / STY, C);
		if (!tile.valid) return;
		const int x0 = tile.tx * STX, y0 = tile.ty * STY;
		const int tid = threadIdx.x;
		const size_t plane = (size_t)tile.c * H * W;

		float sums[2] = { 0.f, 0.f };   // |x - y| and ssim over the tile's own pixels
		load_halo<STX, STY, SR>(tid, x0, y0, H, W, plane,
			[&](size_t o, bool in) { const float vx = img1[o], vy = img2[o]; return in ? v2f{ vx + vy, vx - vy } : v2f{ 0.0f, 0.0f }; },
			[&](int ly, int hx, v2f p) { s_in[ly][hx] = p; },
			[&](v2f p, bool own) { sums[0] += own ? fabsf(p.y) : 0.0f; });
		__syncthreads();

		v2f as[hpass_rounds(SHH, STX / 4)][4];
		hpass_tasks<SHH, STX / 4, true>(tid, [&](int r, int ly, int cx) {
			v2f am[4];
			hwin4_sq(&s_in[ly][cx], am, as[r]);
			store4(&h_m[ly][cx], am);   // (its own bytes: written at once)
		});
		__syncthreads();   // the input tile has been read: its bytes become the filtered arrays
		hpass_tasks<SHH, STX / 4, false>(tid, [&](int r, int ly, int cx) { store4(&h_s[ly][cx], as[r]); });
		__syncthreads();

		const int lx = tid & (STX - 1), ly0 = (tid >> 5) * SROWS;
		const int gx = x0 + lx;
		vpass2<SROWS>(h_m, h_s, ly0, lx, [&](int j, v2f mu, v2f e2) {
			const int gy = y0 + ly0 + j;
			if (gx < W && gy < H)
			{
				const Ssim s = ssim_from_uv(mu, e2);
				const size_t o = plane + (size_t)gy * W + gx;
				ssim_derivs(s, dm_dmu1[o], dm_de11[o], dm_de12[o]);
				sums[1] += s.m;
			}
		});
		tile_reduce(sums, red, tid);
		if (tid == 0) { partial_l1[tile.index] = sum4<false>(red[0]); partial_ssim[tile.index] = sum4<false>(red[1]); }
	}

	__global__ void __launch_bounds__(STHREADS) ssim_bwd_kernel(
		const float* __restrict__ img1, const float* __restrict__ img2, int C, int H, int W,
		const float* __restrict__ dm_dmu1, const float* __restrict__ dm_de11, const float* __restrict__ dm_de12,
		const float* __restrict__ upstream, float w_l1, float w_ssim, float* __restrict__ dL_dimg1)
	{
		// (inputs and horizontally filtered maps share their bytes, as in the forward kernel)
		constexpr int SP_BYTES = SHH * SSTR * 8, SQ_BYTES = SHH * SSTR1 * 4, HP_BYTES = SHH * HSTR * 8, HQ_BYTES = SHH * HSTR1B * 4;
		constexpr int LDS_BYTES = SP_BYTES + SQ_BYTES > HP_BYTES + HQ_BYTES ? SP_BYTES + SQ_BYTES : HP_BYTES + HQ_BYTES;
		__shared__ __attribute__((aligned(16))) char s_raw[LDS_BYTES];
		v2f (*s_p)[SSTR] = reinterpret_cast<v2f (*)[SSTR]>(s_raw);                       // (dm/dmu1, dm/dE11)
		float (*s_q)[SSTR1] = reinterpret_cast<float (*)[SSTR1]>(s_raw + SP_BYTES);      // dm/dE12
		v2f (*h_p)[HSTR] = reinterpret_cast<v2f (*)[HSTR]>(s_raw);
		float (*h_q)[HSTR1B] = reinterpret_cast<float (*)[HSTR1B]>(s_raw + HP_BYTES);

		const TileId tile = tile_of((W + STX - 1) / STX, (H + STY - 1) / STY, C);
		if (!tile.valid) return;
		const int x0 = tile.tx * STX, y0 = tile.ty * STY;
		const int tid = threadIdx.x;
		const size_t plane = (size_t)tile.c * H * W;

		struct PQ { v2f p; float q; };
		load_halo<STX, STY, SR>(tid, x0, y0, H, W, plane,
			[&](size_t o, bool in) {
				const float va = dm_dmu1[o], vb = dm_de11[o], vc = dm_de12[o];
				return PQ{ in ? v2f{ va, vb } : v2f{ 0.0f, 0.0f }, in ? vc : 0.0f };
			},
			[&](int ly, int hx, PQ v) { s_p[ly][hx] = v.p; s_q[ly][hx] = v.q; },
			[](PQ, bool) {});
		const int lx = tid & (STX - 1), ly0 = (tid >> 5) * SROWS;
		const int gx = x0 + lx;
		float px[SROWS], py[SROWS];
		load_own(img1, img2, gx, y0 + ly0, H, W, plane, px, py);
		__syncthreads();

		constexpr int HR = hpass_rounds(SHH, STX / 4);
		v2f ap[HR][4];
		float aq[HR][4];
		hpass_tasks<SHH, STX / 4, true>(tid, [&](int r, int ly, int cx) { hwin4_pq(&s_p[ly][cx], &s_q[ly][cx], ap[r], aq[r]); });
		__syncthreads();   // the inputs have been read: their bytes become the filtered arrays
		hpass_tasks<SHH, STX / 4, false>(tid, [&](int r, int ly, int cx) { store4(&h_p[ly][cx], ap[r]); store4(&h_q[ly][cx], aq[r]); });
		__syncthreads();
		vgrad_pass<SROWS>(h_p, h_q, ly0, lx, upstream, w_l1, w_ssim, px, py, gx, y0 + ly0, H, W, plane, dL_dimg1);
	}
}

namespace fdgs
{
	// ------------------------------------------------------------------------------------------------------------------------
	// Value AND gradient in ONE kernel (fdgs_l1_ssim_value_and_grad: what a training step needs -- the gradient does not depend
	// on anything but the two images and a scalar).  The two-kernel path writes three fp32 derivative maps (49 MB per 1352x1014
	// image) that the backward reads back with a 1.72 x halo: 367 MB of HBM traffic per image (rocprofv3 FETCH_SIZE / WRITE_SIZE)
	// for ~115 MB of images in and gradient out.  Here a workgroup rebuilds what it needs instead: for a 32x32 output tile the
	// derivative maps on the 42x42 pixels around it (window radius 5), from the moments of the 52x52 input pixels around those --
	// nothing but the two images is read, nothing but the gradient and two partial sums per tile is written.  The price is
	// arithmetic: the forward's windows and SSIM algebra run on 1.72 x the pixels (every derivative pixel is computed by the up to
	// four tiles whose halo it lies in).  Phases 3 and 4 are ssim_bwd_kernel's arithmetic operation by operation.  Phases 1 and 2
	// are NOT ssim_fwd_kernel's: they still filter the five moments x, y, x^2, y^2, xy of rounds 1-5, the forward kernel the four of
	// (u, v) = (x + y, x - y), so the derivative maps -- and with them gradient and ssim sum -- agree with the two-kernel path to
	// rounding, not bit for bit (both are held to the same float64 reference and error bars by the tests); the L1 sums are |x - y|
	// in both and equal.
	//   phase 0  A = 52x52 inputs (x, y) -> LDS (zero padding outside the image); |x - y| over the own 32x32
	//   phase 1  horizontal windows of (x, y), (x^2, y^2), xy on the 52 rows x 44 columns (42 used)
	//   phase 2  vertical windows + SSIM algebra on B = 42x42: ssim (summed over the own 32x32) and d ssim / d mu1, d E[x^2], d E[xy]
	//            (zero outside the image: the maps end there); results wait in registers for the barrier, then take the LDS bytes over
	//   phase 3  horizontal windows of the three derivative maps: 42 rows x 32 columns
	//   phase 4  vertical windows -> dL/dx on the own 32x32
	// LDS: 48.3 KB per workgroup (three per CU).
	// ------------------------------------------------------------------------------------------------------------------------
	constexpr int FT = 32;                  // output tile edge
	constexpr int FB = FT + 2 * SR;         // 42: derivative region edge
	constexpr int FA = FB + 2 * SR;         // 52: input region edge
	constexpr int FBC = 44;                 // columns of the phase-1 results (42 used; whole groups of 4)
	constexpr int FSA = 54;                 // s_in row stride in pairs (>= 44 + 10, 108 dwords = 4 mod 8)
	constexpr int FSH = 46;                 // h_m / h_s row stride in pairs (92 dwords)
	constexpr int FSX = 48;                 // h_x row stride in floats
	constexpr int FSD = 46;                 // d_p row stride in pairs
	constexpr int FSQ = 48;                 // d_q row stride in floats
	constexpr int FRV = 7;                  // rows per thread in phase 2 (42 columns x 6 row groups = 252 threads)

	__device__ __forceinline__ void ssim_fused_body(
		const float* __restrict__ img1, const float* __restrict__ img2, int C, int H, int W,
		const float* __restrict__ upstream, float w_l1, float w_ssim, float* __restrict__ dL_dimg1,
		float* __restrict__ partial_l1, float* __restrict__ partial_ssim)
	{
		constexpr int R0_BYTES = FA * FSH * 8;                                  // h_m; later h_p + h_q
		constexpr int IN_BYTES = FA * FSA * 8, HS_BYTES = FA * FSH * 8, HX_BYTES = FA * FSX * 4;
		constexpr int R1_BYTES = IN_BYTES > HS_BYTES + HX_BYTES ? IN_BYTES : HS_BYTES + HX_BYTES;   // s_in; then h_s + h_x; then d_p + d_q
		static_assert(FB * HSTR * 8 + FB * HSTR1B * 4 <= R0_BYTES, "h_p + h_q must fit where h_m was");
		static_assert(FB * FSD * 8 + FB * FSQ * 4 <= R1_BYTES, "d_p + d_q must fit where h_s + h_x were");
		__shared__ __attribute__((aligned(16))) char s_raw[R0_BYTES + R1_BYTES];
		v2f (*h_m)[FSH] = reinterpret_cast<v2f (*)[FSH]>(s_raw);
		v2f (*s_in)[FSA] = reinterpret_cast<v2f (*)[FSA]>(s_raw + R0_BYTES);
		v2f (*h_s)[FSH] = reinterpret_cast<v2f (*)[FSH]>(s_raw + R0_BYTES);
		float (*h_x)[FSX] = reinterpret_cast<float (*)[FSX]>(s_raw + R0_BYTES + HS_BYTES);
		v2f (*d_p)[FSD] = reinterpret_cast<v2f (*)[FSD]>(s_raw + R0_BYTES);                     // (d ssim/d mu1, d ssim/d E11)
		float (*d_q)[FSQ] = reinterpret_cast<float (*)[FSQ]>(s_raw + R0_BYTES + FB * FSD * 8);  // d ssim/d E12
		v2f (*h_p)[HSTR] = reinterpret_cast<v2f (*)[HSTR]>(s_raw);
		float (*h_q)[HSTR1B] = reinterpret_cast<float (*)[HSTR1B]>(s_raw + FB * HSTR * 8);
		__shared__ float red[2][STHREADS / WAVE];

		const TileId tile = tile_of((W + FT - 1) / FT, (H + FT - 1) / FT, C);
		if (!tile.valid) return;
		const int x0 = tile.tx * FT, y0 = tile.ty * FT;
		const int tid = threadIdx.x;
		const size_t plane = (size_t)tile.c * H * W;

		// ---- phase 0: the 52x52 inputs; thread -> one column and rows tid / 52, + 4, + 8, ... (208 of the 256 threads, 13 trips) ----
		float sums[2] = { 0.f, 0.f };   // |x - y| and ssim over the tile's own pixels
		load_halo<FT, FT, 2 * SR>(tid, x0, y0, H, W, plane,
			[&](size_t o, bool in) { const float vx = img1[o], vy = img2[o]; return in ? v2f{ vx, vy } : v2f{ 0.0f, 0.0f }; },
			[&](int ly, int hx, v2f p) { s_in[ly][hx] = p; },
			[&](v2f p, bool own) { sums[0] += own ? fabsf(p.x - p.y) : 0.0f; });
		// the two pad columns the last group of four of phase 1 reads (its results, columns 42 and 43, are never used)
		if (tid < FA) { s_in[tid][FA] = v2f{ 0.0f, 0.0f }; s_in[tid][FA + 1] = v2f{ 0.0f, 0.0f }; }
		// the own pixels this thread finishes in phase 4
		const int lx = tid & (FT - 1), ly0 = (tid >> 5) * SROWS;
		const int gx = x0 + lx;
		float px[SROWS], py[SROWS];
		load_own(img1, img2, gx, y0 + ly0, H, W, plane, px, py);
		__syncthreads();

		// ---- phase 1: horizontal windows; task -> (row, 4 adjacent columns): 52 x 11 tasks in 3 rounds ----
		{
			constexpr int HR = hpass_rounds(FA, FBC / 4);
			v2f as[HR][4];
			float ax[HR][4];
			hpass_tasks<FA, FBC / 4, true>(tid, [&](int r, int ly, int cx) {
				v2f am[4];
				hwin4_sq<true>(&s_in[ly][cx], am, as[r], ax[r]);
				store4(&h_m[ly][cx], am);
			});
			__syncthreads();   // the input tile has been read: its bytes become h_s / h_x
			hpass_tasks<FA, FBC / 4, false>(tid, [&](int r, int ly, int cx) { store4(&h_s[ly][cx], as[r]); store4(&h_x[ly][cx], ax[r]); });
		}
		__syncthreads();

		// ---- phase 2: vertical windows + SSIM algebra on the 42x42 derivative region; thread -> (column, 7 adjacent rows) ----
		{
			const int bc = tid % FB, rg = tid / FB;          // rg 0..5 (threads 252..255: rg = 6, no work)
			const bool work = rg < FB / FRV;
			const int br0 = work ? rg * FRV : 0;
			v2f dp[FRV];
			float dq[FRV];
			{
				v2f vm[10 + FRV], vs[10 + FRV];
				float vx[10 + FRV];
#pragma unroll
				for (int r = 0; r < 10 + FRV; r++) { vm[r] = h_m[br0 + r][bc]; vs[r] = h_s[br0 + r][bc]; vx[r] = h_x[br0 + r][bc]; }
				const int gxb = x0 + bc - SR;
				const bool col_own = (unsigned)(bc - SR) < (unsigned)FT;
#pragma unroll
				for (int j = 0; j < FRV; j++)
				{
					v2f mu = GW[0] * vm[j], e2 = GW[0] * vs[j];
					float e12 = GW[0] * vx[j];
#pragma unroll
					for (int k = 1; k < 11; k++) { mu += GW[k] * vm[j + k]; e2 += GW[k] * vs[j + k]; e12 += GW[k] * vx[j + k]; }
					const int br = br0 + j, gyb = y0 + br - SR;
					dp[j] = v2f{ 0.0f, 0.0f }; dq[j] = 0.0f;
					if (work && (unsigned)gxb < (unsigned)W && (unsigned)gyb < (unsigned)H)
					{
						const float mu1 = mu.x, mu2 = mu.y;
						const float sg1 = e2.x - mu1 * mu1, sg2 = e2.y - mu2 * mu2, sg12 = e12 - mu1 * mu2;
						const Ssim s = ssim_of(mu1, mu2, sg12, sg1 + sg2);
						float d_mu1, d_e11;
						ssim_derivs(s, d_mu1, d_e11, dq[j]);
						dp[j] = v2f{ d_mu1, d_e11 };
						if (col_own && (unsigned)(br - SR) < (unsigned)FT) sums[1] += s.m;   // the tile's own pixels: each counted by exactly one tile
					}
				}
			}
			__syncthreads();   // every thread has read h_m / h_s / h_x: their bytes become the derivative maps
			if (work)
			{
#pragma unroll
				for (int j = 0; j < FRV; j++) { d_p[br0 + j][bc] = dp[j]; d_q[br0 + j][bc] = dq[j]; }
			}
			// pad columns 42..45 of d_q (the b128 reads of the last group reach column 43) -- d_p needs none (14 pairs from column 28: 41)
			if (tid < FB) { d_q[tid][FB] = 0.0f; d_q[tid][FB + 1] = 0.0f; d_q[tid][FB + 2] = 0.0f; d_q[tid][FB + 3] = 0.0f; }
		}
		__syncthreads();

		// ---- phase 3: horizontal windows of the derivative maps: 42 rows x 8 groups of 4 columns, 2 rounds; results go where h_m was ----
		hpass_tasks<FB, FT / 4, true>(tid, [&](int, int ly, int cx) {
			v2f ap[4];
			float aq[4];
			hwin4_pq(&d_p[ly][cx], &d_q[ly][cx], ap, aq);
			store4(&h_p[ly][cx], ap); store4(&h_q[ly][cx], aq);
		});
		__syncthreads();

		// ---- phase 4: vertical windows -> the gradient of the tile's own pixels ----
		vgrad_pass<SROWS>(h_p, h_q, ly0, lx, upstream, w_l1, w_ssim, px, py, gx, y0 + ly0, H, W, plane, dL_dimg1);
		// per-tile partial sums of |x - y| and ssim (fixed order: deterministic)
		tile_reduce(sums, red, tid);
		if (tid == 0) { partial_l1[tile.index] = sum4<false>(red[0]); partial_ssim[tile.index] = sum4<false>(red[1]); }
	}
}

namespace fdgs
{
	// two register allocations of the same body: held to 3 waves per SIMD (three workgroups per CU, what the LDS allows) or free;
	// FDGS_SSIM_FUSED_WPE=2 in the environment selects the second (A/B).  Hand-written the body took 168 VGPRs and 5 spilled ones when
	// held and 173, two workgroups per CU, when free; with the address arithmetic the compiler makes of the ssim_window.h helpers both
	// take 166 VGPRs without a spill -- today the two kernels are the same code
#define FDGS_SSIM_FUSED_PARAMS const float* __restrict__ img1, const float* __restrict__ img2, int C, int H, int W, const float* __restrict__ upstream, \
		float w_l1, float w_ssim, float* __restrict__ dL_dimg1, float* __restrict__ partial_l1, float* __restrict__ partial_ssim
	__global__ void __launch_bounds__(STHREADS) __attribute__((amdgpu_waves_per_eu(3, 3))) ssim_fused_kernel(FDGS_SSIM_FUSED_PARAMS)
	{
		ssim_fused_body(img1, img2, C, H, W, upstream, w_l1, w_ssim, dL_dimg1, partial_l1, partial_ssim);
	}
	__global__ void __launch_bounds__(STHREADS) ssim_fused_kernel_wpe2(FDGS_SSIM_FUSED_PARAMS)
	{
		ssim_fused_body(img1, img2, C, H, W, upstream, w_l1, w_ssim, dL_dimg1, partial_l1, partial_ssim);
	}
#undef FDGS_SSIM_FUSED_PARAMS
}

extern "C" int fdgs_l1_ssim_value_and_grad(const float* img, const float* gt, int32_t C, int32_t H, int32_t W,
                                           const float* upstream, float lambda_dssim, float* dL_dimg,
                                           float* partial_l1, float* partial_ssim, void* stream)
{
	using namespace fdgs;
	static_assert(FT == STX && FT == STY, "the fused kernel shares the tile's partial-sum layout with the two-kernel path");
	if (!img || !gt || !upstream || !dL_dimg || !partial_l1 || !partial_ssim || C <= 0 || H <= 0 || W <= 0)
		return fail(FDGS_ERR_INVALID_ARG, "fdgs_l1_ssim_value_and_grad: a pointer is NULL, or one of C=%d H=%d W=%d is not positive", C, H, W);
	const float n = (float)C * (float)H * (float)W;
	const float w_l1 = (1.0f - lambda_dssim) / n, w_ssim = -lambda_dssim / n;
	const dim3 grid(grid_of(div_up(W, FT) * div_up(H, FT) * C)), block(STHREADS, 1, 1);
	static const bool wpe2 = []() { const char* e = getenv("FDGS_SSIM_FUSED_WPE"); return e && e[0] == '2'; }();
	if (wpe2) hipLaunchKernelGGL(ssim_fused_kernel_wpe2, grid, block, 0, (hipStream_t)stream, img, gt, C, H, W, upstream, w_l1, w_ssim, dL_dimg, partial_l1, partial_ssim);
	else hipLaunchKernelGGL(ssim_fused_kernel, grid, block, 0, (hipStream_t)stream, img, gt, C, H, W, upstream, w_l1, w_ssim, dL_dimg, partial_l1, partial_ssim);
	return launched("fdgs_l1_ssim_value_and_grad");
}

extern "C" int fdgs_l1_ssim_forward(const float* img, const float* gt, int32_t C, int32_t H, int32_t W,
                                    float* dm_dmu1, float* dm_de11, float* dm_de12,
                                    float* partial_l1, float* partial_ssim, void* stream)
{
	using namespace fdgs;
	if (!img || !gt || !dm_dmu1 || !dm_de11 || !dm_de12 || !partial_l1 || !partial_ssim || C <= 0 || H <= 0 || W <= 0)
		return fail(FDGS_ERR_INVALID_ARG, "fdgs_l1_ssim_forward: a pointer is NULL, or one of C=%d H=%d W=%d is not positive", C, H, W);
	const dim3 grid(grid_of(div_up(W, STX) * div_up(H, STY) * C)), block(STHREADS, 1, 1);
	hipLaunchKernelGGL(ssim_fwd_kernel, grid, block, 0, (hipStream_t)stream, img, gt, C, H, W, dm_dmu1, dm_de11, dm_de12, partial_l1, partial_ssim);
	return launched("fdgs_l1_ssim_forward");
}

extern "C" int fdgs_l1_ssim_backward(const float* img, const float* gt, int32_t C, int32_t H, int32_t W,
                                     const float* dm_dmu1, const float* dm_de11, const float* dm_de12,
                                     const float* upstream, float lambda_dssim, float* dL_dimg, void* stream)
{
	using namespace fdgs;
	if (!img || !gt || !dm_dmu1 || !dm_de11 || !dm_de12 || !upstream || !dL_dimg || C <= 0 || H <= 0 || W <= 0)
		return fail(FDGS_ERR_INVALID_ARG, "fdgs_l1_ssim_backward: a pointer is NULL, or one of C=%d H=%d W=%d is not positive", C, H, W);
	const float n = (float)C * (float)H * (float)W;
	const float w_l1 = (1.0f - lambda_dssim) / n, w_ssim = -lambda_dssim / n;
	const dim3 grid(grid_of(div_up(W, STX) * div_up(H, STY) * C)), block(STHREADS, 1, 1);
	hipLaunchKernelGGL(ssim_bwd_kernel, grid, block, 0, (hipStream_t)stream, img, gt, C, H, W, dm_dmu1, dm_de11, dm_de12, upstream, w_l1, w_ssim, dL_dimg);
	return launched("fdgs_l1_ssim_backward");
}

namespace fdgs
{
	// loss = (1 - lambda) * sum(l1) / n + lambda * (1 - sum(ssim) / n), fixed summation order (deterministic)
	// (blockIdx.x = view: the batch call below reduces every view of an optimizer step in ONE launch; view_stride = floats between the
	// partial arrays of consecutive views, 0 for the single call)
	__global__ void __launch_bounds__(1024) l1_ssim_finish_kernel(const float* __restrict__ partial_l1, const float* __restrict__ partial_ssim,
	                                                              int nparts, float inv_n, float lambda_dssim, float* __restrict__ out, long long view_stride)
	{
		partial_l1 += (size_t)blockIdx.x * view_stride; partial_ssim += (size_t)blockIdx.x * view_stride; out += 3 * (size_t)blockIdx.x;
		// 1024 threads, up to 8 partials per thread and sum in flight at once (the kernel is pure latency), then a fixed
		// shuffle tree per wave and a fixed order over the 16 waves: deterministic
		__shared__ float r0[16], r1[16];
		float a = 0.f, b = 0.f;
		for (int base = 0; base < nparts; base += 8 * 1024)
		{
			float va[8], vb[8];
#pragma unroll
			for (int k = 0; k < 8; k++)
			{
				const int i = base + k * 1024 + (int)threadIdx.x;
				va[k] = i < nparts ? partial_l1[i] : 0.f;
				vb[k] = i < nparts ? partial_ssim[i] : 0.f;
			}
			a += ((va[0] + va[1]) + (va[2] + va[3])) + ((va[4] + va[5]) + (va[6] + va[7]));
			b += ((vb[0] + vb[1]) + (vb[2] + vb[3])) + ((vb[4] + vb[5]) + (vb[6] + vb[7]));
		}
#pragma unroll
		for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o); b += __shfl_xor(b, o); }
		if ((threadIdx.x & 63) == 0) { r0[threadIdx.x >> 6] = a; r1[threadIdx.x >> 6] = b; }
		__syncthreads();
		if (threadIdx.x == 0)
		{
			float s0 = 0.f, s1 = 0.f;
			for (int w = 0; w < 16; w++) { s0 += r0[w]; s1 += r1[w]; }
			const float l1 = s0 * inv_n, ss = s1 * inv_n;
			out[0] = (1.0f - lambda_dssim) * l1 + lambda_dssim * (1.0f - ss);
			out[1] = l1;
			out[2] = ss;
		}
	}
}

extern "C" int fdgs_l1_ssim_loss(const float* partial_l1, const float* partial_ssim, int32_t num_partials, int32_t C, int32_t H, int32_t W,
                                 float lambda_dssim, float* loss_l1_ssim, void* stream)
{
	using namespace fdgs;
	if (!partial_l1 || !partial_ssim || !loss_l1_ssim || num_partials <= 0 || C <= 0 || H <= 0 || W <= 0)
		return fail(FDGS_ERR_INVALID_ARG, "fdgs_l1_ssim_loss: a pointer is NULL, or one of num_partials=%d C=%d H=%d W=%d is not positive", num_partials, C, H, W);
	const float inv_n = 1.0f / ((float)C * (float)H * (float)W);
	hipLaunchKernelGGL(l1_ssim_finish_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, partial_l1, partial_ssim, num_partials, inv_n, lambda_dssim, loss_l1_ssim, 0ll);
	return launched("fdgs_l1_ssim_loss");
}

extern "C" int fdgs_l1_ssim_loss_batch(const float* partials, int32_t num_views, int32_t num_partials, int32_t C, int32_t H, int32_t W,
                                       float lambda_dssim, float* losses, void* stream)
{
	using namespace fdgs;
	if (!partials || !losses || num_views <= 0 || num_partials <= 0 || C <= 0 || H <= 0 || W <= 0)
		return fail(FDGS_ERR_INVALID_ARG, "fdgs_l1_ssim_loss_batch: a pointer is NULL, or one of num_views=%d num_partials=%d C=%d H=%d W=%d is not positive", num_views, num_partials, C, H, W);
	const float inv_n = 1.0f / ((float)C * (float)H * (float)W);
	hipLaunchKernelGGL(l1_ssim_finish_kernel, dim3(num_views), dim3(1024), 0, (hipStream_t)stream, partials, partials + num_partials, num_partials, inv_n,
	                   lambda_dssim, losses, 2ll * num_partials);
	return launched("fdgs_l1_ssim_loss_batch");
}

extern "C" int fdgs_l1_ssim_num_partials(int32_t C, int32_t H, int32_t W)
{
	using namespace fdgs;
	return div_up(W, STX) * div_up(H, STY) * C;
}
