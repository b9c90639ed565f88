// frame_resize.hip -- 8-bit frames resized on the device, byte for byte what the reference's loader gets from PIL (gfx950).
//
//   loadCam             utils/camera_utils.py:19-49     PILtoTorch(image, resolution)
//   PILtoTorch          utils/general_utils.py:22-28    pil_image.resize(resolution)      (Pillow's default filter: BICUBIC)
//   CameraDataset       utils/data_utils.py:20-23       RGBA composited over the background before the resize
//
// Pillow resizes 8-bit images in integer arithmetic: per axis a table of fixed-point taps (22 fractional bits) per output index,
//   out = clip(0, 255, (2^21 + sum_x k[x] * in[xmin + x]) >> 22)              int32 accumulator, arithmetic shift
// the horizontal pass first, into an intermediate ROUNDED TO uint8, the vertical pass over that; a pass whose axis keeps its length
// is skipped; RGBA is premultiplied before and divided by the new alpha afterwards.  The tables are built on the host in float64
// (fdgs/resize.py) and uploaded; the kernels here do integer work only.  The one floating-point step of this file is the
// compositing kernel's float64 formula, so the translation unit is built with FP contraction off (build.sh).
//
// Fused kernel (the usual case): a workgroup takes a tile of TW x TH output pixels.  The taps' bounds are monotonic, so the source
// window of the tile is [bounds of the first column, bounds of the last column) x [.. rows ..).  Phase 1 loads that window into LDS,
// a wave per row, with dword loads from the dword at or below the row's first byte (rows are Ws*C bytes: with C = 3 their alignment
// changes from row to row, the row's shift 0..3 is kept implicit in its address); byte loads when the frame array itself does not
// start on a dword, and for a dword that would reach past the end of the array.  RGBA: premultiplied in place.  Phase 2 is the
// horizontal pass LDS -> LDS (uint8 intermediate of the window's rows x TW columns); a lane takes one column and four rows, so a tap
// is loaded once for four rows.  Phase 3 is the vertical pass LDS -> global, a lane per output pixel (the tap is the same for a whole
// row of lanes).  An unchanged axis is an identity tap in the same code.  The host picks the largest tile whose window fits the LDS
// budget from the sizes alone (the window of T outputs spans at most ksize + (T - 1) * scale + 2 inputs).
//
// Two-launch path (any ksize: a window that does not fit LDS even for a 1 x 1 tile, e.g. 20000 -> 2 columns): one lane per output
// pixel straight from global memory, horizontal pass into `scratch`, vertical pass from there.
//
// Tables from the caller are not trusted with memory: every bound is clamped to the axis and to the staged window.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include "fdgs_common.h"

namespace fdgs
{
	constexpr int RS_THREADS = 256;
	constexpr int RS_WAVES = RS_THREADS / WAVE;
	constexpr int RS_LDS_BUDGET = 48 * 1024;   // bytes of dynamic LDS per workgroup: three workgroups per CU
	constexpr int RS_ROWS = 4;                 // rows per lane in the horizontal pass
	constexpr int RS_ONE = 1 << 22, RS_HALF = 1 << 21;
	constexpr int64_t RS_MAX_FRAME = ((int64_t)1 << 31) - 4096;   // bytes of one frame: offsets inside a frame are ints

	static std::atomic<int> g_resize_path{ 0 };   // fdgs_debug_frames_resize_path

	struct ResizeArgs
	{
		const uint8_t* src; const int32_t* index; uint8_t* dst;
		const int32_t *kx, *bx, *ky, *by;
		int N, Hs, Ws, Hd, Wd;
		int ksx, ksy;               // 0: the axis keeps its length (identity)
		int tw_shift, th;           // tile: (1 << tw_shift) x th output pixels
		int cols_cap, rows_cap;     // staged window, at most
		int pitch;                  // bytes of a staged source row (a multiple of 4, >= cols_cap * C + 3)
		int vec_src, vec_dst;       // the arrays start on a dword
	};

	struct Taps { int lo, n; const int32_t* k; };   // inputs [lo, lo + n) with weights k[0 .. n); k == nullptr: weight 1.0

	__device__ __forceinline__ Taps resize_taps(const int32_t* __restrict__ k, const int32_t* __restrict__ bnd, int ks, int n_in, int i)
	{
		if (ks == 0) return Taps{ i, 1, nullptr };
		int lo = bnd[2 * i], n = bnd[2 * i + 1];
		lo = min(max(lo, 0), n_in - 1);
		n = min(max(n, 0), min(ks, n_in - lo));
		return Taps{ lo, n, k + (size_t)i * ks };
	}

	__device__ __forceinline__ int resize_clip(int acc) { return min(max(acc >> 22, 0), 255); }

	__device__ __forceinline__ uint32_t resize_premul(uint32_t c, uint32_t a)
	{
		const uint32_t t = c * a + 128u;
		return ((t >> 8) + t) >> 8;
	}

	__device__ __forceinline__ uint32_t resize_unpremul(uint32_t c, uint32_t a)
	{
		if (a == 0u || a == 255u) return c;
		return min(255u, (255u * c) / a);
	}

	template <int C>
	__device__ __forceinline__ void resize_store_pixel(uint8_t* __restrict__ q, const int* v, bool dword)
	{
		if constexpr (C == 4)
		{
			const uint32_t a = (uint32_t)v[3];
			const uint32_t r = resize_unpremul((uint32_t)v[0], a), g = resize_unpremul((uint32_t)v[1], a), b = resize_unpremul((uint32_t)v[2], a);
			if (dword) *reinterpret_cast<uint32_t*>(q) = r | (g << 8) | (b << 16) | (a << 24);
			else { q[0] = (uint8_t)r; q[1] = (uint8_t)g; q[2] = (uint8_t)b; q[3] = (uint8_t)a; }
		}
		else { q[0] = (uint8_t)v[0]; q[1] = (uint8_t)v[1]; q[2] = (uint8_t)v[2]; }
	}

	template <int C>
	__global__ void __launch_bounds__(RS_THREADS) frames_resize_fused_kernel(ResizeArgs a)
	{
		extern __shared__ __attribute__((aligned(16))) uint8_t rs_lds[];
		const int b = blockIdx.y;
		const int n = a.index[b];
		if (n < 0 || n >= a.N) return;   // (uniform over the workgroup)
		const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
		const int TW = 1 << a.tw_shift;
		const int tiles_x = (a.Wd + TW - 1) >> a.tw_shift;
		const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
		const int x0 = tx << a.tw_shift, y0 = ty * a.th;
		const int tw = min(TW, a.Wd - x0), th = min(a.th, a.Hd - y0);

		// the tile's source window (monotonic bounds: first and last column / row decide)
		const Taps fx = resize_taps(a.kx, a.bx, a.ksx, a.Ws, x0), lx = resize_taps(a.kx, a.bx, a.ksx, a.Ws, x0 + tw - 1);
		const Taps fy = resize_taps(a.ky, a.by, a.ksy, a.Hs, y0), ly = resize_taps(a.ky, a.by, a.ksy, a.Hs, y0 + th - 1);
		const int c0 = fx.lo, ncols = min(max(lx.lo + lx.n - c0, 0), min(a.cols_cap, a.Ws - c0));
		const int r0 = fy.lo, nrows = min(max(ly.lo + ly.n - r0, 0), min(a.rows_cap, a.Hs - r0));

		const int frame_bytes = a.Hs * a.Ws * C;
		const uint8_t* __restrict__ frame = a.src + (size_t)n * frame_bytes;
		const uint8_t* src_end = a.src + (size_t)a.N * frame_bytes;
		const int base_mod = (int)((uintptr_t)frame & 3u), smask = a.vec_src ? 3 : 0;   // byte path: rows are staged without a shift
		const int pitch = a.pitch, ipitch = TW * C;
		uint8_t* patch = rs_lds;
		uint8_t* inter = rs_lds + (((size_t)a.rows_cap * pitch + 15) & ~(size_t)15);

		// phase 1: the window, a wave per row
		for (int i = wave; i < nrows; i += RS_WAVES)
		{
			const int off = ((r0 + i) * a.Ws + c0) * C;
			uint8_t* row = patch + i * pitch;
			if (a.vec_src)
			{
				const int shift = (base_mod + off) & smask;
				const uint8_t* p0 = frame + (off - shift);
				const int nd = (shift + ncols * C + 3) >> 2;
				for (int j = lane; j < nd; j += WAVE)
				{
					const uint8_t* q = p0 + 4 * j;
					uint32_t w = 0u;
					if (q + 4 <= src_end) w = *reinterpret_cast<const uint32_t*>(q);
					else
						for (int k = 0; k < 4; k++)
							if (q + k < src_end) w |= (uint32_t)q[k] << (8 * k);
					*reinterpret_cast<uint32_t*>(row + 4 * j) = w;
				}
			}
			else
			{
				const uint8_t* p = frame + off;
				for (int j = lane; j < ncols * C; j += WAVE) row[j] = p[j];
			}
		}
		__syncthreads();
		if constexpr (C == 4)
		{
			for (int i = wave; i < nrows; i += RS_WAVES)
			{
				uint8_t* row = patch + i * pitch + ((base_mod + ((r0 + i) * a.Ws + c0) * C) & smask);
				for (int j = lane; j < ncols; j += WAVE)
				{
					uint8_t* q = row + 4 * j;
					const uint32_t al = q[3];
					q[0] = (uint8_t)resize_premul(q[0], al); q[1] = (uint8_t)resize_premul(q[1], al); q[2] = (uint8_t)resize_premul(q[2], al);
				}
			}
			__syncthreads();
		}

		// phase 2: horizontal pass, window rows x tile columns -> uint8 intermediate; a lane takes one column of RS_ROWS rows
		const int ngroups = (nrows + RS_ROWS - 1) / RS_ROWS;
		for (int it = tid; it < (ngroups << a.tw_shift); it += RS_THREADS)
		{
			const int g = it >> a.tw_shift, xl = it & (TW - 1);
			if (xl >= tw) continue;
			const Taps t = resize_taps(a.kx, a.bx, a.ksx, a.Ws, x0 + xl);
			const int lo = max(t.lo, c0), hi = min(t.lo + t.n, c0 + ncols);
			const uint8_t* rows[RS_ROWS];
			int acc[RS_ROWS][C];
#pragma unroll
			for (int r = 0; r < RS_ROWS; r++)
			{
				const int i = min(g * RS_ROWS + r, nrows - 1);
				rows[r] = patch + i * pitch + ((base_mod + ((r0 + i) * a.Ws + c0) * C) & smask);
#pragma unroll
				for (int ch = 0; ch < C; ch++) acc[r][ch] = RS_HALF;
			}
			for (int s = lo; s < hi; s++)
			{
				const int k = t.k ? t.k[s - t.lo] : RS_ONE;
				const int o = (s - c0) * C;
#pragma unroll
				for (int r = 0; r < RS_ROWS; r++)
#pragma unroll
					for (int ch = 0; ch < C; ch++) acc[r][ch] += __mul24(k, (int)rows[r][o + ch]);
			}
#pragma unroll
			for (int r = 0; r < RS_ROWS; r++)
			{
				const int i = g * RS_ROWS + r;
				if (i < nrows)
				{
					uint8_t* q = inter + i * ipitch + xl * C;
#pragma unroll
					for (int ch = 0; ch < C; ch++) q[ch] = (uint8_t)resize_clip(acc[r][ch]);
				}
			}
		}
		__syncthreads();

		// phase 3: vertical pass, intermediate -> the tile's output pixels
		uint8_t* __restrict__ out = a.dst + (size_t)b * ((size_t)a.Hd * a.Wd * C);
		for (int it = tid; it < (th << a.tw_shift); it += RS_THREADS)
		{
			const int yl = it >> a.tw_shift, xl = it & (TW - 1);
			if (xl >= tw) continue;
			const Taps t = resize_taps(a.ky, a.by, a.ksy, a.Hs, y0 + yl);
			const int lo = max(t.lo, r0), hi = min(t.lo + t.n, r0 + nrows);
			int acc[C];
#pragma unroll
			for (int ch = 0; ch < C; ch++) acc[ch] = RS_HALF;
			for (int s = lo; s < hi; s++)
			{
				const int k = t.k ? t.k[s - t.lo] : RS_ONE;
				const uint8_t* p = inter + (s - r0) * ipitch + xl * C;
#pragma unroll
				for (int ch = 0; ch < C; ch++) acc[ch] += __mul24(k, (int)p[ch]);
			}
#pragma unroll
			for (int ch = 0; ch < C; ch++) acc[ch] = resize_clip(acc[ch]);
			resize_store_pixel<C>(out + ((size_t)(y0 + yl) * a.Wd + (x0 + xl)) * C, acc, a.vec_dst != 0);
		}
	}

	// ---- the two-launch path: one pass, a lane per output pixel, straight from global memory -----------------------------------------
	struct PassArgs
	{
		const uint8_t* in; const int32_t* index; uint8_t* out;
		const int32_t *k, *bnd;
		int N, Hi, Wi, Ho, Wo, ks;
		int gather;            // in is the frame array (frame index[b]); otherwise the intermediate (frame b)
		int premul, unpremul;  // RGBA: first / last pass of the resize
		int vec_out;
	};

	template <int C, bool HORIZ>
	__global__ void __launch_bounds__(RS_THREADS) frames_resize_pass_kernel(PassArgs a)
	{
		const int b = blockIdx.y;
		const int n = a.index[b];
		if (n < 0 || n >= a.N) return;
		const int p = blockIdx.x * RS_THREADS + threadIdx.x;   // < 2^31: the host checks the frame's bytes
		if (p >= a.Ho * a.Wo) return;
		const int y = p / a.Wo, x = p - y * a.Wo;
		const Taps t = resize_taps(a.k, a.bnd, a.ks, HORIZ ? a.Wi : a.Hi, HORIZ ? x : y);
		const uint8_t* __restrict__ s = a.in + (size_t)(a.gather ? n : b) * ((size_t)a.Hi * a.Wi * C)
			+ (HORIZ ? ((size_t)y * a.Wi + t.lo) * C : ((size_t)t.lo * a.Wi + x) * C);
		const size_t step = HORIZ ? (size_t)C : (size_t)a.Wi * C;
		int acc[C];
#pragma unroll
		for (int ch = 0; ch < C; ch++) acc[ch] = RS_HALF;
		for (int j = 0; j < t.n; j++, s += step)
		{
			const int k = t.k[j];
			uint32_t v[C];
#pragma unroll
			for (int ch = 0; ch < C; ch++) v[ch] = s[ch];
			if constexpr (C == 4)
				if (a.premul) { v[0] = resize_premul(v[0], v[3]); v[1] = resize_premul(v[1], v[3]); v[2] = resize_premul(v[2], v[3]); }
#pragma unroll
			for (int ch = 0; ch < C; ch++) acc[ch] += __mul24(k, (int)v[ch]);
		}
#pragma unroll
		for (int ch = 0; ch < C; ch++) acc[ch] = resize_clip(acc[ch]);
		uint8_t* q = a.out + ((size_t)b * ((size_t)a.Ho * a.Wo) + p) * C;
		if constexpr (C == 4)
		{
			if (!a.unpremul)   // the intermediate stays premultiplied
			{
				if (a.vec_out) *reinterpret_cast<uint32_t*>(q) = (uint32_t)acc[0] | ((uint32_t)acc[1] << 8) | ((uint32_t)acc[2] << 16) | ((uint32_t)acc[3] << 24);
				else { q[0] = (uint8_t)acc[0]; q[1] = (uint8_t)acc[1]; q[2] = (uint8_t)acc[2]; q[3] = (uint8_t)acc[3]; }
				return;
			}
		}
		resize_store_pixel<C>(q, acc, a.vec_out != 0);
	}

	// neither axis changes: dst[b] = src[index[b]], dwords when both arrays and the frame size allow
	__global__ void __launch_bounds__(RS_THREADS) frames_copy_kernel(const uint8_t* __restrict__ src, const int32_t* __restrict__ index, uint8_t* __restrict__ dst,
	                                                                 int N, int frame_bytes, int vec)
	{
		const int b = blockIdx.y;
		const int n = index[b];
		if (n < 0 || n >= N) return;
		const uint8_t* s = src + (size_t)n * frame_bytes;
		uint8_t* d = dst + (size_t)b * frame_bytes;
		const int stride = gridDim.x * RS_THREADS;
		if (vec)
			for (int i = blockIdx.x * RS_THREADS + threadIdx.x; i < frame_bytes / 4; i += stride)
				reinterpret_cast<uint32_t*>(d)[i] = reinterpret_cast<const uint32_t*>(s)[i];
		else
			for (int i = blockIdx.x * RS_THREADS + threadIdx.x; i < frame_bytes; i += stride) d[i] = s[i];
	}

	// ---- RGBA over a background, the reference readers' float64 formula ---------------------------------------------------------------
	__device__ __forceinline__ uint32_t composite_byte(uint32_t c, double na, double rest)
	{
		const double v = ((double)c / 255.0) * na + rest;
		return (uint32_t)(int)floor(v * 255.0);   // in [0, 255] for every (c, a)
	}

	template <int CO>
	__global__ void __launch_bounds__(RS_THREADS) frames_composite_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, long long pixels,
	                                                                      double bg, int vec_src, int vec_dst)
	{
		const long long stride = (long long)gridDim.x * RS_THREADS;
		for (long long p = (long long)blockIdx.x * RS_THREADS + threadIdx.x; p < pixels; p += stride)
		{
			const uint8_t* s = src + p * 4;
			uint32_t r, g, b, al;
			if (vec_src)
			{
				const uint32_t w = *reinterpret_cast<const uint32_t*>(s);
				r = w & 255u; g = (w >> 8) & 255u; b = (w >> 16) & 255u; al = w >> 24;
			}
			else { r = s[0]; g = s[1]; b = s[2]; al = s[3]; }
			const double na = (double)al / 255.0;
			const double rest = bg * (1.0 - na);
			r = composite_byte(r, na, rest); g = composite_byte(g, na, rest); b = composite_byte(b, na, rest);
			uint8_t* q = dst + p * CO;
			if (CO == 4 && vec_dst) *reinterpret_cast<uint32_t*>(q) = r | (g << 8) | (b << 16) | (al << 24);
			else
			{
				q[0] = (uint8_t)r; q[1] = (uint8_t)g; q[2] = (uint8_t)b;
				if constexpr (CO == 4) q[3] = (uint8_t)al;
			}
		}
	}

	// ---- host side ----------------------------------------------------------------------------------------------------------------
	// Pillow's tap count for an axis n_in -> n_out, float64 with every operation rounded on its own
	static int resize_ksize(int n_in, int n_out)
	{
		const double scale = (double)n_in / (double)n_out;
		const double filterscale = scale < 1.0 ? 1.0 : scale;
		const double support = 2.0 * filterscale;
		return (int)ceil(support) * 2 + 1;
	}

	// inputs the taps of T consecutive outputs span, at most (T = 1: ksize; each further output moves the window by `scale`)
	static int64_t resize_span(int n_in, int n_out, int ks, int T)
	{
		if (n_in == n_out) return T;
		const int64_t span = (int64_t)ks + (int64_t)((double)(T - 1) * ((double)n_in / (double)n_out)) + 2;
		return span < n_in ? span : n_in;
	}

	struct ResizePlan { bool fused; int tw_shift, th, cols_cap, rows_cap, pitch; size_t lds; };

	static ResizePlan resize_plan(int Hs, int Ws, int Hd, int Wd, int C, int ksx, int ksy)
	{
		static const int tiles[][2] = { { 6, 16 }, { 5, 16 }, { 5, 8 }, { 4, 8 }, { 4, 4 }, { 3, 4 }, { 2, 2 }, { 1, 2 }, { 0, 1 } };
		ResizePlan P{};
		if (g_resize_path.load() == 1) return P;
		for (const auto& t : tiles)
		{
			const int TW = 1 << t[0], TH = t[1];
			const int64_t cols = resize_span(Ws, Wd, ksx, TW), rows = resize_span(Hs, Hd, ksy, TH);
			const int64_t pitch = (cols * C + 3 + 3) / 4 * 4;
			const int64_t lds = ((rows * pitch + 15) / 16 * 16) + rows * TW * C;
			if (lds > RS_LDS_BUDGET) continue;
			P.fused = true; P.tw_shift = t[0]; P.th = TH; P.cols_cap = (int)cols; P.rows_cap = (int)rows; P.pitch = (int)pitch; P.lds = (size_t)lds;
			// a tile as large as the image is one workgroup: take smaller tiles until the frame gives the chip something to do
			if ((int64_t)div_up(Wd, TW) * div_up(Hd, TH) >= 64 || t[0] == 0) break;
		}
		return P;
	}

	static const char* resize_check(int64_t N, int Hs, int Ws, int C, int64_t B, int64_t M, int Hd, int Wd)
	{
		if (C != 3 && C != 4) return "C must be 3 (RGB) or 4 (RGBA)";
		if (N <= 0 || Hs <= 0 || Ws <= 0 || Hd <= 0 || Wd <= 0 || B <= 0 || M <= 0) return "bad sizes (N, Hs, Ws, B, M, Hd, Wd must be positive)";
		if (B > 65535 || B > M) return "bad sizes (B <= 65535 and B <= M)";
		if ((int64_t)Hs * Ws * C > RS_MAX_FRAME || (int64_t)Hd * Wd * C > RS_MAX_FRAME || (int64_t)Hs * Wd * C > RS_MAX_FRAME)
			return "bad sizes (a frame, its result and the intermediate must stay below 2^31 - 4096 bytes each)";
		return nullptr;
	}
}

using namespace fdgs;

extern "C" void fdgs_debug_frames_resize_path(int32_t path) { g_resize_path.store(path == 1 ? 1 : 0); }

extern "C" int64_t fdgs_frames_resize_scratch_bytes(int32_t B, int32_t Hs, int32_t Ws, int32_t Hd, int32_t Wd, int32_t C)
{
	if (resize_check(1, Hs, Ws, C, B, B, Hd, Wd)) return -1;
	if (Hs == Hd || Ws == Wd) return 0;
	if (resize_plan(Hs, Ws, Hd, Wd, C, resize_ksize(Ws, Wd), resize_ksize(Hs, Hd)).fused) return 0;
	return (int64_t)B * Hs * Wd * C;
}

extern "C" int fdgs_frames_resize(const uint8_t* src, int32_t N, int32_t Hs, int32_t Ws, int32_t C, const int32_t* index, int32_t B,
                                  uint8_t* dst, int32_t M, int32_t Hd, int32_t Wd, const int32_t* kx, const int32_t* bx, int32_t ksize_x,
                                  const int32_t* ky, const int32_t* by, int32_t ksize_y, void* scratch, void* stream_v)
{
	if (const char* bad = resize_check(N, Hs, Ws, C, B, M, Hd, Wd)) return fail(FDGS_ERR_INVALID_ARG, "fdgs_frames_resize: %s", bad);
	if (!src || !index || !dst || !kx || !bx || !ky || !by) return fail(FDGS_ERR_INVALID_ARG, "fdgs_frames_resize: missing pointer");
	if (ksize_x != resize_ksize(Ws, Wd) || ksize_y != resize_ksize(Hs, Hd))
		return fail(FDGS_ERR_INVALID_ARG, "fdgs_frames_resize: ksize (%d, %d) disagrees with the sizes: %d -> %d columns take %d taps, %d -> %d rows %d",
		            ksize_x, ksize_y, Ws, Wd, resize_ksize(Ws, Wd), Hs, Hd, resize_ksize(Hs, Hd));
	hipStream_t stream = (hipStream_t)stream_v;
	const bool do_x = Ws != Wd, do_y = Hs != Hd;
	const int vec_src = (uintptr_t)src % 4 == 0, vec_dst = (uintptr_t)dst % 4 == 0;
	const dim3 block(RS_THREADS);
	if (!do_x && !do_y)
	{
		const int fb = Hs * Ws * C;
		const int vec = vec_src && vec_dst && fb % 4 == 0;
		const int units = vec ? fb / 4 : fb;
		const dim3 grid((unsigned)std::min(div_up(units, RS_THREADS), 4096), (unsigned)B);
		hipLaunchKernelGGL(frames_copy_kernel, grid, block, 0, stream, src, index, dst, N, fb, vec);
		return launched("fdgs_frames_resize");
	}
	const ResizePlan P = resize_plan(Hs, Ws, Hd, Wd, C, ksize_x, ksize_y);
	if (P.fused)
	{
		ResizeArgs a;
		a.src = src; a.index = index; a.dst = dst; a.kx = kx; a.bx = bx; a.ky = ky; a.by = by;
		a.N = N; a.Hs = Hs; a.Ws = Ws; a.Hd = Hd; a.Wd = Wd;
		a.ksx = do_x ? ksize_x : 0; a.ksy = do_y ? ksize_y : 0;
		a.tw_shift = P.tw_shift; a.th = P.th; a.cols_cap = P.cols_cap; a.rows_cap = P.rows_cap; a.pitch = P.pitch;
		a.vec_src = vec_src; a.vec_dst = vec_dst;
		const int64_t tiles = (int64_t)div_up(Wd, 1 << P.tw_shift) * div_up(Hd, P.th);   // < 2^31: Hd * Wd is
		const dim3 grid((unsigned)tiles, (unsigned)B);
		if (C == 3) hipLaunchKernelGGL((frames_resize_fused_kernel<3>), grid, block, P.lds, stream, a);
		else hipLaunchKernelGGL((frames_resize_fused_kernel<4>), grid, block, P.lds, stream, a);
		return launched("fdgs_frames_resize");
	}
	if (do_x && do_y && !scratch) return fail(FDGS_ERR_INVALID_ARG, "fdgs_frames_resize: missing pointer (scratch of fdgs_frames_resize_scratch_bytes)");
	PassArgs h, v;
	h.in = src; h.index = index; h.out = do_y ? (uint8_t*)scratch : dst; h.k = kx; h.bnd = bx;
	h.N = N; h.Hi = Hs; h.Wi = Ws; h.Ho = Hs; h.Wo = Wd; h.ks = ksize_x; h.gather = 1; h.premul = 1; h.unpremul = !do_y;
	h.vec_out = do_y ? (uintptr_t)scratch % 4 == 0 : vec_dst;
	v.in = do_x ? (const uint8_t*)scratch : src; v.index = index; v.out = dst; v.k = ky; v.bnd = by;
	v.N = N; v.Hi = Hs; v.Wi = Wd; v.Ho = Hd; v.Wo = Wd; v.ks = ksize_y; v.gather = !do_x; v.premul = !do_x; v.unpremul = 1;
	v.vec_out = vec_dst;
	if (do_x)
	{
		const dim3 grid((unsigned)div_up(Hs * Wd, RS_THREADS), (unsigned)B);
		if (C == 3) hipLaunchKernelGGL((frames_resize_pass_kernel<3, true>), grid, block, 0, stream, h);
		else hipLaunchKernelGGL((frames_resize_pass_kernel<4, true>), grid, block, 0, stream, h);
	}
	if (do_y)
	{
		const dim3 grid((unsigned)div_up(Hd * Wd, RS_THREADS), (unsigned)B);
		if (C == 3) hipLaunchKernelGGL((frames_resize_pass_kernel<3, false>), grid, block, 0, stream, v);
		else hipLaunchKernelGGL((frames_resize_pass_kernel<4, false>), grid, block, 0, stream, v);
	}
	return launched("fdgs_frames_resize");
}

extern "C" int fdgs_frames_composite(const uint8_t* src_rgba, int32_t N, int32_t H, int32_t W, int32_t white, int32_t keep_alpha,
                                     uint8_t* dst, void* stream_v)
{
	if (N <= 0 || H <= 0 || W <= 0 || (int64_t)H * W * 4 > RS_MAX_FRAME)
		return fail(FDGS_ERR_INVALID_ARG, "fdgs_frames_composite: bad sizes (N, H, W must be positive, a frame below 2^31 - 4096 bytes)");
	if (!src_rgba || !dst) return fail(FDGS_ERR_INVALID_ARG, "fdgs_frames_composite: missing pointer");
	const long long pixels = (long long)N * H * W;
	const int vec_src = (uintptr_t)src_rgba % 4 == 0, vec_dst = (uintptr_t)dst % 4 == 0;
	const dim3 block(RS_THREADS), grid((unsigned)std::min<long long>((pixels + RS_THREADS - 1) / RS_THREADS, 8192));
	hipStream_t stream = (hipStream_t)stream_v;
	const double bg = white ? 1.0 : 0.0;
	if (keep_alpha) hipLaunchKernelGGL((frames_composite_kernel<4>), grid, block, 0, stream, src_rgba, dst, pixels, bg, vec_src, vec_dst);
	else hipLaunchKernelGGL((frames_composite_kernel<3>), grid, block, 0, stream, src_rgba, dst, pixels, bg, vec_src, vec_dst);
	return launched("fdgs_frames_composite");
}
