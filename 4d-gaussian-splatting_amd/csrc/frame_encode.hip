// frame_encode.hip -- float images written out as 8-bit frames: the inverse of frames.hip (gfx950).
//
//   torchvision.utils.save_image     img.mul(255).add_(0.5).clamp_(0, 255).to(uint8), [C, H, W] -> [H, W, C]
//   easy_cmap                        utils/image_utils.py:21-28     g = clamp((d - min) / (max - min), 0, 1), min / max over the plane
//
// Exactly these fp32 operations in this order per value: t = v * 255.0f; t = t + 0.5f (two roundings: this translation unit is built
// with FP contraction off, build.sh -- a fused multiply-add rounds once and differs next to every (k + 0.5) / 255); then
// q = (uint8) min(max(t, 0), 255), truncating; NaN -> 0 (max(NaN, 0) = 0).  decode(q) = q / 255.0f comes back as q for all 256
// bytes.  The grey plane takes one IEEE subtraction and one IEEE division first, in that order; max == min gives 0 / 0 = NaN -> 0.
//
// A pure streaming kernel, 12 or 16 bytes in and 3 or 4 bytes out per pixel (4 in, 1 out for a grey plane), shaped like
// frames_decode_kernel: an image is a flat array of H*W pixels, a lane takes 4 consecutive pixels with one 16-byte load per input
// plane (declared dword-aligned only: planes 1 and 2 start at H*W floats) and stores three dwords r0 g0 b0 r1 | g1 b1 r2 g2 |
// b2 r3 g3 b3 (RGB), one 16-byte vector (RGBA) or one dword (grey); the last H*W mod 4 pixels are taken one by one.  The stores need
// every frame to start on a dword: frame n starts at n*H*W*C bytes, so shapes with H*W*C not a multiple of 4 (and any pointer that is
// not dword-aligned itself) take the byte-wise path, one pixel per lane.  grid.y = image of the batch; the frame it goes to is read
// from device memory and a number outside [0, N) writes nothing.  Plain vector stores only.
//
// The grey plane's min / max: frames_minmax_kernel, launched ahead of the encode on the same stream -- every workgroup strides over
// its share of the plane (16-byte loads, the tail one by one), reduces over the wave64 with shuffles, over its four waves through LDS
// and writes ONE (min, max) pair into the partials buffer; the encode kernel's workgroups each finish the at most 64 pairs of their
// plane with one more wave reduction.  No atomics.  min / max carry a NaN as torch.min / torch.max do (the whole plane is then 0).
#include <cstdint>
#include <cstdio>
#include <cmath>
#include "fdgs_common.h"

namespace fdgs
{
	constexpr int ENCODE_THREADS = 256;
	constexpr int MINMAX_GROUPS = 64;   // most workgroups (= partial pairs) per plane: one wave finishes them

	typedef uint32_t eu32x4 __attribute__((ext_vector_type(4), aligned(4)));
	typedef uint32_t eu32x3 __attribute__((ext_vector_type(3), aligned(4)));
	typedef float ef32x4 __attribute__((ext_vector_type(4), aligned(4)));

	struct EncodeArgs
	{
		const float* images; const float* alphas; const int32_t* index; uint8_t* frames;
		long long image_stride, alpha_stride;   // floats between two images / planes of the batch
		const float* partials;                  // grey: MINMAX_GROUPS (min, max) pairs per plane
		int N, HW, groups;
	};

	__device__ __forceinline__ uint32_t encode_unit(float v)
	{
		float t = v * 255.0f;
		t = t + 0.5f;
		return (uint32_t)fminf(fmaxf(t, 0.0f), 255.0f);   // fmaxf(NaN, 0) = 0
	}

	// torch.min / torch.max: a NaN wins
	__device__ __forceinline__ float nan_min(float a, float b) { return (a != a) ? a : ((b != b) ? b : fminf(a, b)); }
	__device__ __forceinline__ float nan_max(float a, float b) { return (a != a) ? a : ((b != b) ? b : fmaxf(a, b)); }

	__device__ __forceinline__ float grey_unit(float d, float mn, float range)
	{
		const float g = (d - mn) / range;
		return fminf(fmaxf(g, 0.0f), 1.0f);               // NaN -> 0, as the quantisation would make it
	}

	// One pixel: the byte-wise path and the tail of the vector path.
	template <int C>
	__device__ __forceinline__ void encode_pixel(const float* __restrict__ src, const float* __restrict__ alp, uint8_t* __restrict__ dst, int HW, int p)
	{
		uint8_t* d = dst + (size_t)p * C;
		d[0] = (uint8_t)encode_unit(src[p]);
		d[1] = (uint8_t)encode_unit(src[(size_t)HW + p]);
		d[2] = (uint8_t)encode_unit(src[2 * (size_t)HW + p]);
		if constexpr (C == 4) d[3] = (uint8_t)encode_unit(alp[p]);
	}

	template <int C, bool VEC>
	__global__ void __launch_bounds__(ENCODE_THREADS) frames_encode_kernel(EncodeArgs a)
	{
		const int b = blockIdx.y;
		const int n = a.index[b];
		if (n < 0 || n >= a.N) return;   // (uniform over the workgroup)
		const int HW = a.HW;
		const float* __restrict__ src = a.images + (size_t)b * a.image_stride;
		const float* __restrict__ alp = (C == 4) ? a.alphas + (size_t)b * a.alpha_stride : nullptr;
		uint8_t* __restrict__ dst = a.frames + (size_t)n * HW * C;
		const int t = blockIdx.x * ENCODE_THREADS + threadIdx.x;
		if constexpr (!VEC)
		{
			if (t < HW) encode_pixel<C>(src, alp, dst, HW, t);
			return;
		}
		else
		{
			const int p = 4 * t;   // 4 * t < H W + 1024 < 2^31 (fdgs_frames_encode checks H W)
			if (p >= HW) return;
			if (p + 4 > HW)
			{
				for (int q = p; q < HW; q++) encode_pixel<C>(src, alp, dst, HW, q);
				return;
			}
			const ef32x4 r = *reinterpret_cast<const ef32x4*>(src + p);
			const ef32x4 g = *reinterpret_cast<const ef32x4*>(src + (size_t)HW + p);
			const ef32x4 bl = *reinterpret_cast<const ef32x4*>(src + 2 * (size_t)HW + p);
			uint32_t R[4], G[4], B[4];
#pragma unroll
			for (int k = 0; k < 4; k++) { R[k] = encode_unit(r[k]); G[k] = encode_unit(g[k]); B[k] = encode_unit(bl[k]); }
			if constexpr (C == 3)
			{
				// 12 bytes r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3 (little endian)
				eu32x3 w;
				w[0] = R[0] | (G[0] << 8) | (B[0] << 16) | (R[1] << 24);
				w[1] = G[1] | (B[1] << 8) | (R[2] << 16) | (G[2] << 24);
				w[2] = B[2] | (R[3] << 8) | (G[3] << 16) | (B[3] << 24);
				*reinterpret_cast<eu32x3*>(dst + (size_t)p * 3) = w;
			}
			else
			{
				const ef32x4 al = *reinterpret_cast<const ef32x4*>(alp + p);
				eu32x4 w;
#pragma unroll
				for (int k = 0; k < 4; k++) w[k] = R[k] | (G[k] << 8) | (B[k] << 16) | (encode_unit(al[k]) << 24);
				*reinterpret_cast<eu32x4*>(dst + (size_t)p * 4) = w;
			}
		}
	}

	// (min, max) of a wave64's values in every lane
	__device__ __forceinline__ void wave_minmax(float& mn, float& mx)
	{
		for (int o = 32; o > 0; o >>= 1) { mn = nan_min(mn, __shfl_xor(mn, o)); mx = nan_max(mx, __shfl_xor(mx, o)); }
	}

	// partials[(b * groups + g) * 2 + {0, 1}] = (min, max) over workgroup g's share of plane b.  groups <= MINMAX_GROUPS workgroups
	// per plane, each striding over the plane 4 * ENCODE_THREADS pixels at a time.
	template <bool VEC>
	__global__ void __launch_bounds__(ENCODE_THREADS) frames_minmax_kernel(const float* __restrict__ planes, long long plane_stride, int HW,
	                                                                        int groups, float* __restrict__ partials)
	{
		const int b = blockIdx.y;
		const float* __restrict__ src = planes + (size_t)b * plane_stride;
		float mn = INFINITY, mx = -INFINITY;
		if constexpr (VEC)
		{
			const long long step = 4LL * ENCODE_THREADS * groups;
			for (long long p = 4LL * (blockIdx.x * ENCODE_THREADS + threadIdx.x); p < HW; p += step)
			{
				if (p + 4 <= HW)
				{
					const ef32x4 v = *reinterpret_cast<const ef32x4*>(src + p);
#pragma unroll
					for (int k = 0; k < 4; k++) { mn = nan_min(mn, v[k]); mx = nan_max(mx, v[k]); }
				}
				else
					for (long long q = p; q < HW; q++) { mn = nan_min(mn, src[q]); mx = nan_max(mx, src[q]); }
			}
		}
		else
		{
			const long long step = (long long)ENCODE_THREADS * groups;
			for (long long p = blockIdx.x * ENCODE_THREADS + threadIdx.x; p < HW; p += step) { mn = nan_min(mn, src[p]); mx = nan_max(mx, src[p]); }
		}
		wave_minmax(mn, mx);
		__shared__ float smn[ENCODE_THREADS / 64], smx[ENCODE_THREADS / 64];
		if ((threadIdx.x & 63) == 0) { smn[threadIdx.x >> 6] = mn; smx[threadIdx.x >> 6] = mx; }
		__syncthreads();
		if (threadIdx.x == 0)
		{
			for (int w = 1; w < ENCODE_THREADS / 64; w++) { mn = nan_min(mn, smn[w]); mx = nan_max(mx, smx[w]); }
			float* out = partials + ((size_t)b * groups + blockIdx.x) * 2;
			out[0] = mn; out[1] = mx;
		}
	}

	template <bool VEC>
	__global__ void __launch_bounds__(ENCODE_THREADS) frames_encode_gray_kernel(EncodeArgs a)
	{
		const int b = blockIdx.y;
		const int n = a.index[b];
		if (n < 0 || n >= a.N) return;   // (uniform over the workgroup)
		const int HW = a.HW;
		// finish the plane's min / max: every wave reduces the (at most 64) pairs itself, no barrier
		const int lane = threadIdx.x & 63;
		float mn = INFINITY, mx = -INFINITY;
		if (lane < a.groups)
		{
			const float* pr = a.partials + ((size_t)b * a.groups + lane) * 2;
			mn = pr[0]; mx = pr[1];
		}
		wave_minmax(mn, mx);
		const float range = mx - mn;
		const float* __restrict__ src = a.images + (size_t)b * a.image_stride;
		uint8_t* __restrict__ dst = a.frames + (size_t)n * HW;
		const int t = blockIdx.x * ENCODE_THREADS + threadIdx.x;
		if constexpr (!VEC)
		{
			if (t < HW) dst[t] = (uint8_t)encode_unit(grey_unit(src[t], mn, range));
			return;
		}
		else
		{
			const int p = 4 * t;
			if (p >= HW) return;
			if (p + 4 > HW)
			{
				for (int q = p; q < HW; q++) dst[q] = (uint8_t)encode_unit(grey_unit(src[q], mn, range));
				return;
			}
			const ef32x4 v = *reinterpret_cast<const ef32x4*>(src + p);
			uint32_t w = 0;
#pragma unroll
			for (int k = 0; k < 4; k++) w |= encode_unit(grey_unit(v[k], mn, range)) << (8 * k);
			*reinterpret_cast<uint32_t*>(dst + p) = w;
		}
	}

	static int minmax_groups(int64_t HW)
	{
		const int64_t g = (HW + 4 * ENCODE_THREADS - 1) / (4 * ENCODE_THREADS);
		return (int)(g < 1 ? 1 : (g > MINMAX_GROUPS ? MINMAX_GROUPS : g));
	}
}

using namespace fdgs;

extern "C" int fdgs_frames_encode(const float* images, int64_t image_stride, const float* alphas, int64_t alpha_stride, int32_t B,
                                  int32_t H, int32_t W, int32_t C, uint8_t* frames, int32_t N, const int32_t* index, void* stream_v)
{
	if (C != 3 && C != 4) return fail(FDGS_ERR_INVALID_ARG, "fdgs_frames_encode: C must be 3 (RGB) or 4 (RGBA)");
	const int64_t HW = (int64_t)H * W;
	if (N <= 0 || H <= 0 || W <= 0 || B <= 0 || B > 65535 || HW > ((int64_t)1 << 31) - 4096)
		return fail(FDGS_ERR_INVALID_ARG, "fdgs_frames_encode: bad sizes (N, H, W, B must be positive, B <= 65535, H * W <= 2^31 - 4096)");
	if (!images || !index || !frames || (C == 4 && !alphas)) return fail(FDGS_ERR_INVALID_ARG, "fdgs_frames_encode: missing pointer");
	if (image_stride < 3 * HW || (C == 4 && alpha_stride < HW))
		return fail(FDGS_ERR_INVALID_ARG, "fdgs_frames_encode: image_stride must be at least 3 H W floats and alpha_stride at least H W");
	if (C == 3) alphas = nullptr;
	EncodeArgs a;
	a.images = images; a.alphas = alphas; a.index = index; a.frames = frames;
	a.image_stride = image_stride; a.alpha_stride = alphas ? alpha_stride : 0;
	a.partials = nullptr; a.N = N; a.HW = (int)HW; a.groups = 0;
	// the vector path stores dwords: every frame must start on one, and float pointers are dword-aligned unless the caller cast them
	const bool vec = ((HW * C) % 4 == 0) && ((uintptr_t)frames % 4 == 0) && ((uintptr_t)images % 4 == 0) && ((uintptr_t)alphas % 4 == 0);
	hipStream_t stream = (hipStream_t)stream_v;
	const dim3 block(ENCODE_THREADS);
	if (vec)
	{
		const dim3 grid((unsigned)((HW + 4 * ENCODE_THREADS - 1) / (4 * ENCODE_THREADS)), (unsigned)B);
		if (C == 3) hipLaunchKernelGGL((frames_encode_kernel<3, true>), grid, block, 0, stream, a);
		else hipLaunchKernelGGL((frames_encode_kernel<4, true>), grid, block, 0, stream, a);
	}
	else
	{
		const dim3 grid((unsigned)((HW + ENCODE_THREADS - 1) / ENCODE_THREADS), (unsigned)B);
		if (C == 3) hipLaunchKernelGGL((frames_encode_kernel<3, false>), grid, block, 0, stream, a);
		else hipLaunchKernelGGL((frames_encode_kernel<4, false>), grid, block, 0, stream, a);
	}
	return launched("fdgs_frames_encode");
}

extern "C" int64_t fdgs_frames_encode_gray_scratch_bytes(int32_t B, int32_t H, int32_t W)
{
	const int64_t HW = (int64_t)H * W;
	if (H <= 0 || W <= 0 || B <= 0 || B > 65535 || HW > ((int64_t)1 << 31) - 4096) return -1;
	return (int64_t)B * minmax_groups(HW) * 2 * (int64_t)sizeof(float);
}

extern "C" int fdgs_frames_encode_gray(const float* planes, int64_t plane_stride, int32_t B, int32_t H, int32_t W, uint8_t* frames,
                                       int32_t N, const int32_t* index, void* scratch, void* stream_v)
{
	const int64_t HW = (int64_t)H * W;
	if (N <= 0 || H <= 0 || W <= 0 || B <= 0 || B > 65535 || HW > ((int64_t)1 << 31) - 4096)
		return fail(FDGS_ERR_INVALID_ARG, "fdgs_frames_encode_gray: bad sizes (N, H, W, B must be positive, B <= 65535, H * W <= 2^31 - 4096)");
	if (!planes || !index || !frames || !scratch) return fail(FDGS_ERR_INVALID_ARG, "fdgs_frames_encode_gray: missing pointer");
	if (plane_stride < HW) return fail(FDGS_ERR_INVALID_ARG, "fdgs_frames_encode_gray: plane_stride must be at least H W floats");
	if ((uintptr_t)scratch % 4 != 0) return fail(FDGS_ERR_INVALID_ARG, "fdgs_frames_encode_gray: scratch must be dword-aligned");
	const int groups = minmax_groups(HW);
	EncodeArgs a;
	a.images = planes; a.alphas = nullptr; a.index = index; a.frames = frames;
	a.image_stride = plane_stride; a.alpha_stride = 0;
	a.partials = (const float*)scratch; a.N = N; a.HW = (int)HW; a.groups = groups;
	hipStream_t stream = (hipStream_t)stream_v;
	const dim3 block(ENCODE_THREADS);
	const bool vec_in = (uintptr_t)planes % 4 == 0;
	const dim3 rgrid((unsigned)groups, (unsigned)B);
	if (vec_in) hipLaunchKernelGGL((frames_minmax_kernel<true>), rgrid, block, 0, stream, planes, (long long)plane_stride, (int)HW, groups, (float*)scratch);
	else hipLaunchKernelGGL((frames_minmax_kernel<false>), rgrid, block, 0, stream, planes, (long long)plane_stride, (int)HW, groups, (float*)scratch);
	// one byte per pixel: frame n starts at n*H*W bytes
	const bool vec = vec_in && (HW % 4 == 0) && ((uintptr_t)frames % 4 == 0);
	if (vec)
	{
		const dim3 grid((unsigned)((HW + 4 * ENCODE_THREADS - 1) / (4 * ENCODE_THREADS)), (unsigned)B);
		hipLaunchKernelGGL((frames_encode_gray_kernel<true>), grid, block, 0, stream, a);
	}
	else
	{
		const dim3 grid((unsigned)((HW + ENCODE_THREADS - 1) / ENCODE_THREADS), (unsigned)B);
		hipLaunchKernelGGL((frames_encode_gray_kernel<false>), grid, block, 0, stream, a);
	}
	return launched("fdgs_frames_encode_gray");
}
