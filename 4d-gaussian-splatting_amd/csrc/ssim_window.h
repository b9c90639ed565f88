// ssim_window.h -- the 11-tap separable-window machinery of the SSIM kernels (gfx950): ssim_fwd_kernel, ssim_bwd_kernel and the
// one-kernel form of ssim.hip, metrics_scale_kernel of metrics.hip.
//
// A workgroup of 256 threads takes a 32x32 output tile: it loads the tile with a halo into LDS (load_halo), filters it horizontally
// (hpass_tasks + hwin4_*: 4 adjacent outputs from 14 b128-loaded inputs) and vertically (vpass2 / vgrad_pass: a column and N adjacent
// rows per thread), evaluates SSIM per pixel (ssim_from_uv / ssim_of / ssim_derivs) and sums per tile (tile_reduce).  The kernels
// are VALU-issue bound (SQ counters) and tight on registers, so every helper is __forceinline__ and keeps the channels of a
// window interleaved in ONE tap loop: two single-channel loops in sequence cost ssim_fwd_kernel 6 VGPRs (86 -> 92).
#pragma once
#include "fdgs_common.h"

namespace fdgs
{
	constexpr int SR = 5;                // window radius (11 taps)
	constexpr int STHREADS = 256;
	typedef float v2f __attribute__((ext_vector_type(2)));
	typedef float v4f __attribute__((ext_vector_type(4)));

	// gaussian(11, 1.5) normalised, as utils/loss_utils.py:23-25
	__device__ constexpr float GW[11] = {
		0.0010283801f, 0.0075987582f, 0.0360007733f, 0.1093606874f, 0.2130055279f, 0.2660117149f,
		0.2130055279f, 0.1093606874f, 0.0360007733f, 0.0075987582f, 0.0010283801f };

	// Workgroup -> tile.  The hardware deals consecutive workgroup ids round-robin to the 8 XCDs, each with its own L2: with the
	// plain (x, y, channel) grid the tiles that share a halo -- horizontal neighbours -- always sit on DIFFERENT XCDs and every halo
	// byte is fetched from memory once per tile that needs it (FETCH_SIZE: 1.6 x the tile bytes).  Here XCD j takes the j-th eighth of
	// the tiles in row-major order -- a band of tile rows of one channel -- so that neighbours meet in one L2.
	// Tiles are numbered channel by channel, so channel c's tiles are the contiguous range [c * gx * gy, (c + 1) * gx * gy).
	struct TileId { int tx, ty, c, index; bool valid; };
	__device__ __forceinline__ TileId tile_of(int gx, int gy, int C)
	{
		const int total = gx * gy * C, chunk = (total + 7) / 8;
		const int wg = (int)blockIdx.x, xcd = wg & 7, k = wg >> 3;
		TileId t;
		t.index = xcd * chunk + k;
		t.valid = k < chunk && t.index < total;
		const int i = t.valid ? t.index : 0;
		t.c = i / (gx * gy);
		const int r = i - t.c * (gx * gy);
		t.ty = r / gx; t.tx = r - t.ty * gx;
		return t;
	}
	static inline int grid_of(int ntiles) { return ((ntiles + 7) / 8) * 8; }

	// Halo load of the (TH + 2 PAD) x (TW + 2 PAD) pixels around the TW x TH tile at (x0, y0) of one image plane: thread -> one column
	// and rows tid / COLS, + RPT, + 2 RPT, ... (42 columns: every sixth row, 252 of the 256 threads; the column, its bounds test and
	// the address are computed once, a trip only moves down RPT rows).  All loads of the thread are issued before the first one is
	// waited for (a rolled loop paid one global round trip per trip).
	//   make(o, in)       -> the pixel's LDS value from the global offset o; outside the image (in false: o is a valid address all the
	//                        same, branch-free) it returns the zero padding (F.conv2d padding = 5)
	//   store(ly, hx, v)  writes it to row ly, column hx of the region
	//   own(v, is_own)    sees every loaded value; is_own: a pixel of the tile itself (what is summed per tile is summed here: the
	//                     input tile is gone after the horizontal pass)
	template <int TW, int TH, int PAD, typename Make, typename Store, typename Own>
	__device__ __forceinline__ void load_halo(int tid, int x0, int y0, int H, int W, size_t plane, Make make, Store store, Own own)
	{
		constexpr int ROWS = TH + 2 * PAD, COLS = TW + 2 * PAD;
		constexpr int RPT = STHREADS / COLS, TRIPS = (ROWS + RPT - 1) / RPT;
		const int lyb = tid / COLS, hx = tid - lyb * COLS;
		const int gxh = x0 + hx - PAD;
		const bool col_in = tid < RPT * COLS && (unsigned)gxh < (unsigned)W;
		const bool col_own = (unsigned)(hx - PAD) < (unsigned)TW;
		decltype(make((size_t)0, true)) p[TRIPS];
#pragma unroll
		for (int t = 0; t < TRIPS; t++)
		{
			const int ly = lyb + t * RPT, gy = y0 + ly - PAD;
			const bool in = col_in && ly < ROWS && (unsigned)gy < (unsigned)H;
			p[t] = make(in ? plane + (size_t)gy * W + gxh : plane, in);
		}
#pragma unroll
		for (int t = 0; t < TRIPS; t++)
		{
			const int ly = lyb + t * RPT;
			if (tid < RPT * COLS && ly < ROWS) store(ly, hx, p[t]);
			own(p[t], col_own && (unsigned)(ly - PAD) < (unsigned)TH);   // (outside the image: the padding)
		}
	}

	// The image values of the N adjacent pixels of column gx from row gy0 on (the pixels a thread finishes in vgrad_pass): issued
	// early, they travel while the windows are computed
	template <int N>
	__device__ __forceinline__ void load_own(const float* __restrict__ img1, const float* __restrict__ img2, int gx, int gy0, int H, int W,
	                                         size_t plane, float (&px)[N], float (&py)[N])
	{
#pragma unroll
		for (int j = 0; j < N; j++)
		{
			const int gy = gy0 + j;
			const size_t o = (gx < W && gy < H) ? plane + (size_t)gy * W + gx : plane;
			px[j] = img1[o]; py[j] = img2[o];
		}
	}

	// Horizontal pass: task -> (row ly, 4 adjacent columns from cx); ROWS * GPR tasks over the 256 threads in hpass_rounds rounds,
	// f(r, ly, cx) per task of round r.  Where the results overwrite the inputs they stay in registers (indexed by r) until every
	// task has read its inputs: a barrier and a second walk over the tasks (SCHED = false) that stores them.
	// SCHED: a scheduling barrier after every round -- one round's inputs at a time in registers.
	constexpr int hpass_rounds(int rows, int gpr) { return (rows * gpr + STHREADS - 1) / STHREADS; }
	template <int ROWS, int GPR, bool SCHED, typename F>
	__device__ __forceinline__ void hpass_tasks(int tid, F f)
	{
#pragma unroll
		for (int r = 0; r < hpass_rounds(ROWS, GPR); r++)
		{
			const int task = tid + r * STHREADS;
			if (task < ROWS * GPR)
			{
				const int ly = task / GPR;
				f(r, ly, (task - ly * GPR) * 4);
			}
			if (SCHED) __builtin_amdgcn_sched_barrier(0);
		}
	}

	__device__ __forceinline__ void load14(const v2f* row, v2f (&p)[16])
	{
		const v4f* src = reinterpret_cast<const v4f*>(row);
#pragma unroll
		for (int i = 0; i < 7; i++) { const v4f q = src[i]; p[2 * i] = v2f{ q.x, q.y }; p[2 * i + 1] = v2f{ q.z, q.w }; }
	}
	__device__ __forceinline__ void store4(v2f* dst, const v2f (&a)[4])
	{
		v4f* d = reinterpret_cast<v4f*>(dst);
		d[0] = v4f{ a[0].x, a[0].y, a[1].x, a[1].y }; d[1] = v4f{ a[2].x, a[2].y, a[3].x, a[3].y };
	}
	__device__ __forceinline__ void store4(float* dst, const float (&a)[4]) { *reinterpret_cast<v4f*>(dst) = v4f{ a[0], a[1], a[2], a[3] }; }

	// One task of a horizontal pass over pairs p = row[0 .. 13]: the windows of p (am) and of p * p (as) and, with XY, of the scalar
	// p.x * p.y (ax): two packed-fp32 FMAs per tap (+ a plain one)
	template <bool XY>
	__device__ __forceinline__ void hwin4_sq(const v2f* row, v2f (&am)[4], v2f (&as)[4], float (&ax)[4])
	{
		v2f p[16], sq[14];
		float xy[14];
		load14(row, p);
#pragma unroll
		for (int i = 0; i < 14; i++) { sq[i] = p[i] * p[i]; if constexpr (XY) xy[i] = p[i].x * p[i].y; }
#pragma unroll
		for (int j = 0; j < 4; j++)
		{
			am[j] = GW[0] * p[j]; as[j] = GW[0] * sq[j]; if constexpr (XY) ax[j] = GW[0] * xy[j];
#pragma unroll
			for (int k = 1; k < 11; k++) { am[j] += GW[k] * p[j + k]; as[j] += GW[k] * sq[j + k]; if constexpr (XY) ax[j] += GW[k] * xy[j + k]; }
		}
	}
	__device__ __forceinline__ void hwin4_sq(const v2f* row, v2f (&am)[4], v2f (&as)[4])
	{
		float none[4];
		hwin4_sq<false>(row, am, as, none);
	}

	// ... over a pair array and a scalar array: the windows of both
	__device__ __forceinline__ void hwin4_pq(const v2f* prow, const float* qrow, v2f (&ap)[4], float (&aq)[4])
	{
		v2f p[16];
		float q[16];
		load14(prow, p);
		const v4f* sq = reinterpret_cast<const v4f*>(qrow);
#pragma unroll
		for (int i = 0; i < 4; i++) { const v4f t = sq[i]; q[4 * i] = t.x; q[4 * i + 1] = t.y; q[4 * i + 2] = t.z; q[4 * i + 3] = t.w; }
#pragma unroll
		for (int j = 0; j < 4; j++)
		{
			ap[j] = GW[0] * p[j]; aq[j] = GW[0] * q[j];
#pragma unroll
			for (int k = 1; k < 11; k++) { ap[j] += GW[k] * p[j + k]; aq[j] += GW[k] * q[j + k]; }
		}
	}

	// Vertical pass over two pair arrays: thread -> column col, N adjacent output rows from row0 (10 + N row reads per N outputs);
	// body(j, window of h_m, window of h_s) per output row
	template <int N, int SM, int SS, typename Body>
	__device__ __forceinline__ void vpass2(const v2f (*h_m)[SM], const v2f (*h_s)[SS], int row0, int col, Body body)
	{
		v2f vm[10 + N], vs[10 + N];
#pragma unroll
		for (int r = 0; r < 10 + N; r++) { vm[r] = h_m[row0 + r][col]; vs[r] = h_s[row0 + r][col]; }
#pragma unroll
		for (int j = 0; j < N; j++)
		{
			v2f mu = GW[0] * vm[j], e2 = GW[0] * vs[j];
#pragma unroll
			for (int k = 1; k < 11; k++) { mu += GW[k] * vm[j + k]; e2 += GW[k] * vs[j + k]; }
			body(j, mu, e2);
		}
	}

	// Vertical pass of the backward: from the horizontally filtered (dm/dmu1, dm/dE11) pairs h_p and dm/dE12 scalars h_q
	//   dL/dx(p) = up [ w_l1 sign(x - y) + w_ssim ( (W * dmu1)(p) + 2 x(p) (W * dE11)(p) + y(p) (W * dE12)(p) ) ]
	// for the N pixels of column gx from row gy0 on, whose image values are px / py (load_own)
	template <int N, int SP, int SQ>
	__device__ __forceinline__ void vgrad_pass(const v2f (*h_p)[SP], const float (*h_q)[SQ], int row0, int col, const float* __restrict__ upstream,
	                                           float w_l1, float w_ssim, const float (&px)[N], const float (&py)[N], int gx, int gy0, int H, int W,
	                                           size_t plane, float* __restrict__ dL_dimg1)
	{
		v2f vp[10 + N];
		float vq[10 + N];
#pragma unroll
		for (int r = 0; r < 10 + N; r++) { vp[r] = h_p[row0 + r][col]; vq[r] = h_q[row0 + r][col]; }
		const float up = upstream[0];
#pragma unroll
		for (int j = 0; j < N; j++)
		{
			v2f ab = GW[0] * vp[j];
			float d = GW[0] * vq[j];
#pragma unroll
			for (int k = 1; k < 11; k++) { ab += GW[k] * vp[j + k]; d += GW[k] * vq[j + k]; }
			const int gy = gy0 + j;
			if (gx < W && gy < H)
			{
				const size_t o = plane + (size_t)gy * W + gx;
				const float x = px[j], y = py[j];
				const float diff = x - y;
				const float sgn = diff > 0.f ? 1.f : (diff < 0.f ? -1.f : 0.f);
				dL_dimg1[o] = up * (w_l1 * sgn + w_ssim * (ab.x + 2.f * x * ab.y + y * d));
			}
		}
	}

	// SSIM of one pixel, m = A B / (Cc D), with what its derivatives need
	struct Ssim { float m, A, B, rC, rD, inv, mu1, mu2; };
	// ... from the means, sigma_12 and sigma_1^2 + sigma_2^2 (the two variances only ever enter SSIM as their sum)
	__device__ __forceinline__ Ssim ssim_of(float mu1, float mu2, float sg12, float sg_sum)
	{
		const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
		const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
		Ssim s;
		s.mu1 = mu1; s.mu2 = mu2;
		s.A = 2.f * mu12 + C1; s.B = 2.f * sg12 + C2;
		const float Cc = mu1_sq + mu2_sq + C1, D = sg_sum + C2;
		// 1 / Cc and 1 / D by v_rcp_f32 (1 ulp): three IEEE divisions were a seventh of the forward kernel's instructions
		s.rC = __builtin_amdgcn_rcpf(Cc); s.rD = __builtin_amdgcn_rcpf(D);
		s.inv = s.rC * s.rD;
		s.m = s.A * s.B * s.inv;
		return s;
	}
	// ... from the windows mu = (E[u], E[v]) and e2 = (E[u^2], E[v^2]) of u = x + y, v = x - y:  mu1, mu2 = (E[u] +- E[v]) / 2,
	// E[x^2] + E[y^2] = (E[u^2] + E[v^2]) / 2,  E[xy] = (E[u^2] - E[v^2]) / 4
	__device__ __forceinline__ Ssim ssim_from_uv(v2f mu, v2f e2)
	{
		const float mu1 = 0.5f * (mu.x + mu.y), mu2 = 0.5f * (mu.x - mu.y);
		const float e_sum = 0.5f * (e2.x + e2.y), e12 = 0.25f * (e2.x - e2.y);
		const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
		return ssim_of(mu1, mu2, e12 - mu12, e_sum - (mu1_sq + mu2_sq));
	}
	// total derivative of m w.r.t. mu1 (through A, B, Cc, D), and w.r.t. the raw moments E[x^2], E[xy]
	__device__ __forceinline__ void ssim_derivs(const Ssim& s, float& dm_dmu1, float& dm_de11, float& dm_de12)
	{
		const float dm_dA = s.B * s.inv, dm_dB = s.A * s.inv, dm_dC = -s.m * s.rC, dm_dD = -s.m * s.rD;
		dm_dmu1 = dm_dA * 2.f * s.mu2 - dm_dB * 2.f * s.mu2 + dm_dC * 2.f * s.mu1 - dm_dD * 2.f * s.mu1;
		dm_de11 = dm_dD;
		dm_de12 = 2.f * dm_dB;
	}

	// Per-tile sums of N values per thread: a wave shuffle tree, then one partial per wave in red[k][0 .. 3] (valid after the
	// barrier this ends with).  sum4 adds the four in the order its kernel has always used (fixed: the sums are deterministic).
	template <int N>
	__device__ __forceinline__ void tile_reduce(float (&v)[N], float (*red)[STHREADS / WAVE], int tid)
	{
#pragma unroll
		for (int o = 32; o > 0; o >>= 1)
		{
#pragma unroll
			for (int k = 0; k < N; k++) v[k] += __shfl_down(v[k], o);
		}
		if ((tid & 63) == 0)
		{
#pragma unroll
			for (int k = 0; k < N; k++) red[k][tid >> 6] = v[k];
		}
		__syncthreads();
	}
	template <bool PAIRWISE>
	__device__ __forceinline__ float sum4(const float* r) { return PAIRWISE ? (r[0] + r[1]) + (r[2] + r[3]) : r[0] + r[1] + r[2] + r[3]; }
}
