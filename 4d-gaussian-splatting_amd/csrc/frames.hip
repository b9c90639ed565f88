// frames.hip -- ground-truth frames kept as 8-bit images, decoded into the float tensors the reference's loader produces (gfx950).
//
//   PILtoTorch          utils/general_utils.py:22-28    v = float(u8) / 255.0, [H, W, C] -> [C, H, W]
//   Camera.__init__     scene/cameras.py:53-57          image *= gt_alpha_mask        (RGBA: mask = a / 255.0, rgb = v * mask)
//
// Exactly these fp32 operations in this order: one IEEE division per value (NOT a multiplication by 1/255.f: that differs for 126 of
// the 256 bytes) and, with an alpha channel, one more division and one product per colour value ((u * a) / 65025 differs for 37 247
// of the 65 536 pairs).  This translation unit is built without fast-math and with FP contraction off (build.sh).
//
// A pure streaming kernel, 1 byte in and 4 bytes out per value.  A frame is a flat array of H*W pixels and so is every output
// plane: pixel p goes to plane offset p, no row structure.  A lane takes 4 consecutive pixels: three dword loads (RGB) or one
// 16-byte load (RGBA), one 16-byte store per output plane; the last H*W mod 4 pixels of a frame are taken one by one.  The loads
// need the frame to start on a dword: frame n starts at n*H*W*C bytes, so RGB frames with H*W not a multiple of 4 (and any frame
// array or output that is not dword-aligned itself) take the byte-wise path, one pixel per lane.  The 16-byte accesses are
// declared dword-aligned only (planes 1 and 2 start at H*W floats, RGBA frames at 4*H*W bytes): global memory takes them at any
// dword.  grid.y = frame of the batch; the frame's number is read from device memory and a number outside [0, N) writes nothing.
#include <cstdint>
#include <cstdio>
#include "fdgs_common.h"

namespace fdgs
{
	constexpr int FRAMES_THREADS = 256;

	typedef uint32_t u32x4 __attribute__((ext_vector_type(4), aligned(4)));
	typedef float f32x4 __attribute__((ext_vector_type(4), aligned(4)));

	struct FramesArgs
	{
		const uint8_t* frames; const int32_t* index; float* out; float* mask;
		long long out_stride, mask_stride;   // floats between two images / masks of the batch
		int N, HW;
	};

	__device__ __forceinline__ float frames_unit(uint32_t byte) { return (float)byte / 255.0f; }

	// One pixel: the byte-wise path and the tail of the vector path.
	template <int C>
	__device__ __forceinline__ void frames_pixel(const uint8_t* __restrict__ src, float* __restrict__ dst, float* __restrict__ msk, int HW, int p)
	{
		const uint8_t* s = src + (size_t)p * C;
		float v0 = frames_unit(s[0]), v1 = frames_unit(s[1]), v2 = frames_unit(s[2]);
		if constexpr (C == 4)
		{
			const float a = frames_unit(s[3]);
			v0 = v0 * a; v1 = v1 * a; v2 = v2 * a;
			if (msk) msk[p] = a;
		}
		dst[p] = v0; dst[(size_t)HW + p] = v1; dst[2 * (size_t)HW + p] = v2;
	}

	template <int C, bool VEC>
	__global__ void __launch_bounds__(FRAMES_THREADS) frames_decode_kernel(FramesArgs a)
	{
		const int b = blockIdx.y;
		const int n = a.index[b];
		if (n < 0 || n >= a.N) return;   // (uniform over the workgroup)
		const int HW = a.HW;
		const uint8_t* __restrict__ src = a.frames + (size_t)n * HW * C;
		float* __restrict__ dst = a.out + (size_t)b * a.out_stride;
		float* __restrict__ msk = (C == 4 && a.mask) ? a.mask + (size_t)b * a.mask_stride : nullptr;
		const int t = blockIdx.x * FRAMES_THREADS + threadIdx.x;
		if constexpr (!VEC)
		{
			if (t < HW) frames_pixel<C>(src, dst, msk, HW, t);
			return;
		}
		else
		{
			const int p = 4 * t;   // 4 * t < H W + 1024 < 2^31 (fdgs_frames_decode checks H W)
			if (p >= HW) return;
			if (p + 4 > HW)
			{
				for (int q = p; q < HW; q++) frames_pixel<C>(src, dst, msk, HW, q);
				return;
			}
			float r[4], g[4], bl[4];
			if constexpr (C == 3)
			{
				// 12 bytes r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3 (little endian)
				const uint32_t* w = reinterpret_cast<const uint32_t*>(src + (size_t)p * 3);
				const uint32_t w0 = w[0], w1 = w[1], w2 = w[2];
				r[0] = frames_unit(w0 & 255u);         g[0] = frames_unit((w0 >> 8) & 255u);  bl[0] = frames_unit((w0 >> 16) & 255u);
				r[1] = frames_unit(w0 >> 24);          g[1] = frames_unit(w1 & 255u);         bl[1] = frames_unit((w1 >> 8) & 255u);
				r[2] = frames_unit((w1 >> 16) & 255u); g[2] = frames_unit(w1 >> 24);          bl[2] = frames_unit(w2 & 255u);
				r[3] = frames_unit((w2 >> 8) & 255u);  g[3] = frames_unit((w2 >> 16) & 255u); bl[3] = frames_unit(w2 >> 24);
			}
			else
			{
				const u32x4 w = *reinterpret_cast<const u32x4*>(src + (size_t)p * 4);
				float al[4];
#pragma unroll
				for (int k = 0; k < 4; k++)
				{
					const uint32_t x = w[k];
					al[k] = frames_unit(x >> 24);
					r[k] = frames_unit(x & 255u) * al[k];
					g[k] = frames_unit((x >> 8) & 255u) * al[k];
					bl[k] = frames_unit((x >> 16) & 255u) * al[k];
				}
				if (msk) *reinterpret_cast<f32x4*>(msk + p) = f32x4{ al[0], al[1], al[2], al[3] };
			}
			*reinterpret_cast<f32x4*>(dst + p) = f32x4{ r[0], r[1], r[2], r[3] };
			*reinterpret_cast<f32x4*>(dst + (size_t)HW + p) = f32x4{ g[0], g[1], g[2], g[3] };
			*reinterpret_cast<f32x4*>(dst + 2 * (size_t)HW + p) = f32x4{ bl[0], bl[1], bl[2], bl[3] };
		}
	}
}

using namespace fdgs;

extern "C" int fdgs_frames_decode(const uint8_t* frames, int32_t N, int32_t H, int32_t W, int32_t C, const int32_t* index, int32_t B,
                                  float* out, int64_t out_stride, float* mask_out, int64_t mask_stride, void* stream_v)
{
	if (C != 3 && C != 4) return fail(FDGS_ERR_INVALID_ARG, "fdgs_frames_decode: C must be 3 (RGB) or 4 (RGBA)");
	const int64_t HW = (int64_t)H * W;
	if (N <= 0 || H <= 0 || W <= 0 || B <= 0 || B > 65535 || HW > ((int64_t)1 << 31) - 4096)
		return fail(FDGS_ERR_INVALID_ARG, "fdgs_frames_decode: bad sizes (N, H, W, B must be positive, B <= 65535, H * W <= 2^31 - 4096)");
	if (!frames || !index || !out) return fail(FDGS_ERR_INVALID_ARG, "fdgs_frames_decode: missing pointer");
	if (out_stride < 3 * HW || (mask_out && mask_stride < HW))
		return fail(FDGS_ERR_INVALID_ARG, "fdgs_frames_decode: out_stride must be at least 3 H W floats and mask_stride at least H W");
	if (C == 3) mask_out = nullptr;
	FramesArgs a;
	a.frames = frames; a.index = index; a.out = out; a.mask = mask_out;
	a.out_stride = out_stride; a.mask_stride = mask_out ? mask_stride : 0;
	a.N = N; a.HW = (int)HW;
	// the vector path loads dwords: every frame must start on one, and float pointers are dword-aligned unless the caller cast them
	const bool vec = ((HW * C) % 4 == 0) && ((uintptr_t)frames % 4 == 0) && ((uintptr_t)out % 4 == 0) && ((uintptr_t)mask_out % 4 == 0);
	hipStream_t stream = (hipStream_t)stream_v;
	const dim3 block(FRAMES_THREADS);
	if (vec)
	{
		const dim3 grid((unsigned)((HW + 4 * FRAMES_THREADS - 1) / (4 * FRAMES_THREADS)), (unsigned)B);
		if (C == 3) hipLaunchKernelGGL((frames_decode_kernel<3, true>), grid, block, 0, stream, a);
		else hipLaunchKernelGGL((frames_decode_kernel<4, true>), grid, block, 0, stream, a);
	}
	else
	{
		const dim3 grid((unsigned)((HW + FRAMES_THREADS - 1) / FRAMES_THREADS), (unsigned)B);
		if (C == 3) hipLaunchKernelGGL((frames_decode_kernel<3, false>), grid, block, 0, stream, a);
		else hipLaunchKernelGGL((frames_decode_kernel<4, false>), grid, block, 0, stream, a);
	}
	return launched("fdgs_frames_decode");
}
