// metrics.hip -- evaluation metrics of a rendered view against its ground truth (gfx950): L1, PSNR, SSIM and MS-SSIM in one pass
// per scale and one reduction, no derivative maps.
//
// The reference's training_report (train.py:276-345) computes for every evaluated view, on clamp(render, 0, 1):
//   l1_loss (utils/loss_utils.py:18), psnr (utils/image_utils.py:17-19, per channel, then the mean), ssim (utils/loss_utils.py:34-66:
//   11x11 Gaussian window, sigma 1.5, zero padding, "same" size) and torchmetrics' MS-SSIM (data_range 1, five scales, the valid
//   window positions of each scale, relu-normalised sim / cs, 2x2 average pooling between scales; MS-SSIM runs on the CPU there).
// Here:
//   scale kernel : one pass over a scale, tiled like ssim_fwd_kernel (ssim.hip): a 32x32 output tile loads its 42x42 halo of both
//                  images into LDS as pairs (u, v) = (x + y, x - y) -- the render clamped to [0, 1] on load, no clamped copy -- does the
//                  separable 11-tap window of (u, v) and (u^2, v^2), and writes per-tile partial sums of
//                    |x - y|, (x - y)^2 (the tile's own pixels; a tile is one channel), the zero-padded SSIM over the own pixels,
//                    and S = SSIM and CS = (2 s_xy + C2) / (s_x^2 + s_y^2 + C2) over the own pixels whose whole window lies inside the
//                    image (the valid region: there zero padding and torchmetrics' reflection both leave the window untouched),
//                  plus the 2x2-pooled pair of the tile's own pixels for the next scale.  Scale 0 and scales 1-4 run the same kernel.
//   finish kernel: one workgroup, fixed summation order (double), writes out4 = [l1, psnr, ssim, msssim]: bitwise reproducible, one
//                  view's row depends on nothing but that view.
#include <math.h>
#include "ssim_window.h"

namespace fdgs
{
namespace metrics
{
	constexpr int TX = 32, TY = 32;     // output tile
	constexpr int ROWS = TY / 8;        // adjacent output rows a thread finishes in the vertical pass (32 columns x 8 row groups)
	constexpr int R = SR;               // window radius
	constexpr int HH = TY + 2 * R;      // 42: rows of tile + halo (and columns: TX + 2 * R)
	constexpr int SSTR = 46;            // LDS row strides in (u, v) pairs (the bank-conflict choice of ssim.hip)
	constexpr int HSTR = 38;
	constexpr int THREADS = STHREADS;
	constexpr int NPART = 5;            // partial sums per tile: |x-y|, (x-y)^2, ssim (all own pixels), S, CS (valid region)
	constexpr int SCALES = 5;
	constexpr int MIN_SIDE = 176;       // torchmetrics: H // 16 > 10 and W // 16 > 10 for five scales and an 11-tap window
	static inline int tiles_of(int C, int H, int W) { return div_up(W, TX) * div_up(H, TY) * C; }

	__device__ __forceinline__ float clamp01(float x) { return fminf(fmaxf(x, 0.0f), 1.0f); }

	// a: render (clamped on load with clamp_a), b: ground truth, [C, H, W].  part: [NPART][ntiles].  pa / pb: the pooled pair
	// [C, H / 2, W / 2] (NULL: not written); the pooled render is already clamped, so the next scale runs with clamp_a = 0.
	__global__ void __launch_bounds__(THREADS) metrics_scale_kernel(
		const float* __restrict__ a, const float* __restrict__ b, int C, int H, int W, int clamp_a,
		float* __restrict__ pa, float* __restrict__ pb, float* __restrict__ part, int ntiles)
	{
		constexpr int IN_BYTES = HH * SSTR * 8, HM_BYTES = HH * HSTR * 8;
		constexpr int SH_BYTES = IN_BYTES > HM_BYTES ? IN_BYTES : HM_BYTES;
		__shared__ __attribute__((aligned(16))) char s_raw[HM_BYTES + SH_BYTES];
		v2f (*h_m)[HSTR] = reinterpret_cast<v2f (*)[HSTR]>(s_raw);                // horizontally filtered (u, v)
		v2f (*s_in)[SSTR] = reinterpret_cast<v2f (*)[SSTR]>(s_raw + HM_BYTES);    // (u, v) = (x + y, x - y)
		v2f (*h_s)[HSTR] = reinterpret_cast<v2f (*)[HSTR]>(s_raw + HM_BYTES);     // (u^2, v^2): over the input tile once it is read
		__shared__ float red[NPART][THREADS / WAVE];

		const TileId tile = tile_of((W + TX - 1) / TX, (H + TY - 1) / TY, C);
		if (!tile.valid) return;
		const int c = tile.c;
		const int x0 = tile.tx * TX, y0 = tile.ty * TY;
		const int tid = threadIdx.x;
		const size_t plane = (size_t)c * H * W;

		// halo; the render clamped on load; |x - y| and (x - y)^2 summed over the own pixels
		float sums[NPART] = { 0.f, 0.f, 0.f, 0.f, 0.f };   // |x-y|, (x-y)^2, ssim, S, CS
		load_halo<TX, TY, R>(tid, x0, y0, H, W, plane,
			[&](size_t o, bool in) {
				const float va = a[o], vb = b[o];
				const float vx = clamp_a ? clamp01(va) : va;
				return in ? v2f{ vx + vb, vx - vb } : v2f{ 0.0f, 0.0f };
			},
			[&](int ly, int hx, v2f p) { s_in[ly][hx] = p; },
			[&](v2f p, bool own) { sums[0] += own ? fabsf(p.y) : 0.0f; sums[1] += own ? p.y * p.y : 0.0f; });
		// the pooled pair of the own 32x32 pixels: thread -> one of the 16x16 outputs (avg_pool2d(2, 2): an odd last row / column is
		// dropped).  Its four source pixels were just loaded by this workgroup: L2 / L1 hits.
		if (pa)
		{
			const int Hp = H >> 1, Wp = W >> 1;
			const int px = (x0 >> 1) + (tid & 15), py = (y0 >> 1) + (tid >> 4);
			if (px < Wp && py < Hp)
			{
				const size_t o = plane + (size_t)(2 * py) * W + 2 * px;
				float a00 = a[o], a01 = a[o + 1], a10 = a[o + W], a11 = a[o + W + 1];
				const float b00 = b[o], b01 = b[o + 1], b10 = b[o + W], b11 = b[o + W + 1];
				if (clamp_a) { a00 = clamp01(a00); a01 = clamp01(a01); a10 = clamp01(a10); a11 = clamp01(a11); }
				const size_t q = (size_t)c * Hp * Wp + (size_t)py * Wp + px;
				pa[q] = ((a00 + a01) + (a10 + a11)) * 0.25f;
				pb[q] = ((b00 + b01) + (b10 + b11)) * 0.25f;
			}
		}
		__syncthreads();

		// horizontal pass: the (u^2, v^2) results wait in registers until every task has read its inputs
		v2f as[hpass_rounds(HH, TX / 4)][4];
		hpass_tasks<HH, TX / 4, true>(tid, [&](int r, int ly, int cx) {
			v2f am[4];
			hwin4_sq(&s_in[ly][cx], am, as[r]);
			store4(&h_m[ly][cx], am);
		});
		__syncthreads();   // the input tile has been read: its bytes become h_s
		hpass_tasks<HH, TX / 4, false>(tid, [&](int r, int ly, int cx) { store4(&h_s[ly][cx], as[r]); });
		__syncthreads();

		// vertical pass: thread -> (column, ROWS adjacent rows); SSIM as ssim_fwd_kernel computes it, plus CS on the valid region
		const int lx = tid & (TX - 1), ly0 = (tid >> 5) * ROWS;
		const int gx = x0 + lx;
		const bool col_valid = gx >= R && gx < W - R;
		vpass2<ROWS>(h_m, h_s, ly0, lx, [&](int j, v2f mu, v2f e2) {
			const int gy = y0 + ly0 + j;
			if (gx < W && gy < H)
			{
				const Ssim s = ssim_from_uv(mu, e2);
				sums[2] += s.m;
				if (col_valid && gy >= R && gy < H - R) { sums[3] += s.m; sums[4] += s.B * s.rD; }
			}
		});
		tile_reduce(sums, red, tid);
		if (tid < NPART) part[(size_t)tid * ntiles + tile.index] = sum4<true>(red[tid]);
	}

	struct Plan
	{
		const float* part[SCALES];
		int ntiles[SCALES];
		int H[SCALES], W[SCALES];
		int C, scales;   // scales: 1 (no MS-SSIM) or 5
	};

	// The finish kernel is a chain of global loads of partials the scale kernels have just written, so it is written for few
	// dependent load rounds: every sum is cut into chunks of 1024 partials, one wave takes a chunk with all 16 loads of a lane in
	// flight at once, and the 16 waves take 16 chunks at a time (at C3: 26 chunks, two rounds; a wave per whole sum took nine).
	constexpr int FT = 1024;                 // threads of the finish kernel
	constexpr int FW = FT / WAVE;            // waves
	constexpr int FCH = 16 * WAVE;           // partials per chunk
	constexpr int FITEMS = 256;              // chunks per round (LDS slots)

	// sums: 0 = |x-y|, 1 = ssim (scale 0), 2..6 = cs_0..cs_3, sim_4 (with MS-SSIM), then (x-y)^2 of channel 0..C-1
	__device__ __forceinline__ void sum_range(const Plan& pl, int j, int nms, const float*& p, int& n)
	{
		const int n0 = pl.ntiles[0];
		if (j == 0) { p = pl.part[0]; n = n0; }
		else if (j == 1) { p = pl.part[0] + 2 * (size_t)n0; n = n0; }
		else if (j < 2 + nms) { const int sc = j - 2; n = pl.ntiles[sc]; p = pl.part[sc] + (size_t)(sc < SCALES - 1 ? 4 : 3) * n; }
		else { n = n0 / pl.C; p = pl.part[0] + n0 + (size_t)(j - 2 - nms) * n; }
	}

	// sum of p[0 .. n), n <= FCH, by one wave: 16 loads per lane issued together, four double accumulators, a fixed shuffle tree
	__device__ __forceinline__ double chunk_sum(const float* __restrict__ p, int n)
	{
		const int lane = threadIdx.x & (WAVE - 1);
		float v[FCH / WAVE];
#pragma unroll
		for (int k = 0; k < FCH / WAVE; k++) { const int i = k * WAVE + lane; v[k] = i < n ? p[i] : 0.0f; }
		double acc[4] = { 0.0, 0.0, 0.0, 0.0 };
#pragma unroll
		for (int k = 0; k < FCH / WAVE; k++) acc[k & 3] += (double)v[k];
		double s = (acc[0] + acc[1]) + (acc[2] + acc[3]);
#pragma unroll
		for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
		return s;
	}

	__global__ void __launch_bounds__(FT) metrics_finish_kernel(Plan pl, float* __restrict__ out4)
	{
		__shared__ double s_item[FITEMS];
		__shared__ double s_tot[2 + SCALES];   // the totals of sums 0 .. 1 + nms
		const int C = pl.C;
		const int nms = pl.scales == SCALES ? SCALES : 0, nsums = 2 + nms + C;
		const int wave = threadIdx.x / WAVE;
		int nitems = 0;
		for (int j = 0; j < nsums; j++) { const float* p; int n; sum_range(pl, j, nms, p, n); nitems += (n + FCH - 1) / FCH; }
		const double hw = (double)pl.H[0] * (double)pl.W[0];
		const double beta[SCALES] = { 0.0448, 0.2856, 0.3001, 0.2363, 0.1333 };
		// thread 0's fold: chunks in index order, i.e. sum by sum and chunk by chunk within a sum: deterministic
		double psnr = 0.0, cur = 0.0;
		int fj = 0, fend = 0;   // the sum being folded and the item index where it ends
		for (int t0 = 0; t0 < nitems; t0 += FITEMS)
		{
			const int t1 = t0 + FITEMS < nitems ? t0 + FITEMS : nitems;
			for (int t = t0 + wave; t < t1; t += FW)
			{
				int j = 0, before = 0, nc = 0;
				const float* p;
				int n;
				for (;; j++)
				{
					sum_range(pl, j, nms, p, n);
					nc = (n + FCH - 1) / FCH;
					if (t < before + nc) break;
					before += nc;
				}
				const int k = t - before, m = n - k * FCH;
				const double v = chunk_sum(p + (size_t)k * FCH, m < FCH ? m : FCH);
				if ((threadIdx.x & (WAVE - 1)) == 0) s_item[t - t0] = v;
			}
			__syncthreads();
			if (threadIdx.x == 0)
			{
				for (int t = t0; t < t1; t++)
				{
					while (t >= fend)   // a new sum starts at item t: finish the previous one
					{
						if (fend > 0)
						{
							if (fj < 2 + nms) s_tot[fj] = cur;
							else psnr += 20.0 * log10(1.0 / sqrt(cur / hw));   // mse = 0: +inf, as the reference
							fj++;
						}
						const float* p;
						int n;
						sum_range(pl, fj, nms, p, n);
						fend += (n + FCH - 1) / FCH;
						cur = 0.0;
					}
					cur += s_item[t - t0];
				}
			}
			__syncthreads();
		}
		if (threadIdx.x == 0)
		{
			psnr += 20.0 * log10(1.0 / sqrt(cur / hw));   // the last sum is channel C-1's (x-y)^2
			const double l1 = s_tot[0] / (hw * C), ssim = s_tot[1] / (hw * C);
			double ms = 1.0;
			for (int sc = 0; sc < nms; sc++)
			{
				const double nv = (double)C * (double)(pl.H[sc] - 2 * R) * (double)(pl.W[sc] - 2 * R);   // valid positions
				ms *= pow(fmax(s_tot[2 + sc] / nv, 0.0), beta[sc]);                                      // normalize="relu"
			}
			out4[0] = (float)l1; out4[1] = (float)(psnr / C); out4[2] = (float)ssim; out4[3] = nms ? (float)ms : (float)NAN;
		}
	}

	// scratch layout: per scale the partials [NPART][ntiles], then per scale 1..4 the pooled pair; 256-byte aligned pieces
	struct Layout { size_t part[SCALES], pa[SCALES], pb[SCALES], total; int H[SCALES], W[SCALES], scales; };
	static inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
	static Layout layout_of(int C, int H, int W, bool ms)
	{
		Layout L = {};
		L.scales = ms ? SCALES : 1;
		size_t off = 0;
		for (int s = 0; s < L.scales; s++)
		{
			L.H[s] = s ? L.H[s - 1] / 2 : H;
			L.W[s] = s ? L.W[s - 1] / 2 : W;
			L.part[s] = off;
			off = align256(off + sizeof(float) * NPART * (size_t)tiles_of(C, L.H[s], L.W[s]));
		}
		for (int s = 1; s < L.scales; s++)
		{
			const size_t bytes = sizeof(float) * (size_t)C * L.H[s] * L.W[s];
			L.pa[s] = off; off = align256(off + bytes);
			L.pb[s] = off; off = align256(off + bytes);
		}
		L.total = off;
		return L;
	}
}
}

extern "C" int fdgs_eval_metrics_scratch_bytes(int32_t C, int32_t H, int32_t W)
{
	using namespace fdgs::metrics;
	if (C <= 0 || H <= 0 || W <= 0) return -1;
	const Layout L = layout_of(C, H, W, H >= MIN_SIDE && W >= MIN_SIDE);
	return L.total > (size_t)INT32_MAX ? -1 : (int)L.total;
}

extern "C" int fdgs_eval_metrics(const float* img, const float* gt, int32_t C, int32_t H, int32_t W, int32_t flags, void* scratch,
                                 float* out4, void* stream)
{
	using namespace fdgs;
	using namespace fdgs::metrics;
	if (!img || !gt || !scratch || !out4) return fail(FDGS_ERR_INVALID_ARG, "fdgs_eval_metrics: missing pointer");
	if (C <= 0 || H <= 0 || W <= 0) return fail(FDGS_ERR_INVALID_ARG, "fdgs_eval_metrics: C, H and W must be positive");
	if ((size_t)C * H * W > (size_t)INT32_MAX) return fail(FDGS_ERR_INVALID_ARG, "fdgs_eval_metrics: image too large");
	const bool ms = !(flags & FDGS_METRICS_NO_MSSSIM);
	if (ms && (H < MIN_SIDE || W < MIN_SIDE))
		return fail(FDGS_ERR_INVALID_ARG, "fdgs_eval_metrics: MS-SSIM with 5 scales and an 11-tap window needs both image sides "
		                                  ">= 176 pixels (H // 16 > 10 and W // 16 > 10)");
	const Layout L = layout_of(C, H, W, ms);
	char* base = static_cast<char*>(scratch);
	const hipStream_t st = (hipStream_t)stream;
	Plan pl = {};
	pl.C = C; pl.scales = L.scales;
	for (int s = 0; s < L.scales; s++)
	{
		const int Hs = L.H[s], Ws = L.W[s], nt = tiles_of(C, Hs, Ws);
		const float* a = s ? reinterpret_cast<const float*>(base + L.pa[s]) : img;
		const float* b = s ? reinterpret_cast<const float*>(base + L.pb[s]) : gt;
		float* pa = s + 1 < L.scales ? reinterpret_cast<float*>(base + L.pa[s + 1]) : nullptr;
		float* pb = s + 1 < L.scales ? reinterpret_cast<float*>(base + L.pb[s + 1]) : nullptr;
		float* part = reinterpret_cast<float*>(base + L.part[s]);
		const int clamp_a = s == 0 && (flags & FDGS_METRICS_CLAMP) ? 1 : 0;
		hipLaunchKernelGGL(metrics_scale_kernel, dim3(grid_of(nt)), dim3(THREADS), 0, st, a, b, C, Hs, Ws, clamp_a, pa, pb, part, nt);
		pl.part[s] = part; pl.ntiles[s] = nt; pl.H[s] = Hs; pl.W[s] = Ws;
	}
	hipLaunchKernelGGL(metrics_finish_kernel, dim3(1), dim3(FT), 0, st, pl, out4);
	return launched("fdgs_eval_metrics");
}
