// scan.h -- the prefix sums and wave reductions of the integer kernels, on two levels (tilebin.hip, radix_sort.hip, compact.h).
//   wave    wave_inclusive_sum / wave_sum / wave_max: shuffles only, no LDS and no barrier -- a single wave may call them under
//           `if (tid < WAVE)`
//   block   block_rank / block_scan_counts: the wave level plus a carry over the waves through THREADS / WAVE words of LDS
// Integer sums in a fixed order: exact and reproducible.
#pragma once
#include "fdgs_common.h"

namespace fdgs
{
	// inclusive prefix sum over the lanes of the calling wave (lane WAVE - 1 ends up with the wave's sum)
	__device__ __forceinline__ uint32_t wave_inclusive_sum(uint32_t x)
	{
		const int lane = threadIdx.x & (WAVE - 1);
#pragma unroll
		for (int d = 1; d < WAVE; d <<= 1)
		{
			const uint32_t y = __shfl_up(x, d);
			if (lane >= d) x += y;
		}
		return x;
	}
	// the same over 64-bit values (sums of 32-bit weights that no 32-bit word holds: mcmc.hip)
	__device__ __forceinline__ uint64_t wave_inclusive_sum(uint64_t x)
	{
		const int lane = threadIdx.x & (WAVE - 1);
#pragma unroll
		for (int d = 1; d < WAVE; d <<= 1)
		{
			const uint64_t y = (uint64_t)__shfl_up((unsigned long long)x, d);
			if (lane >= d) x += y;
		}
		return x;
	}
	// sum / maximum over the lanes of the calling wave; every lane gets it
	__device__ __forceinline__ uint32_t wave_sum(uint32_t x)
	{
#pragma unroll
		for (int d = 1; d < WAVE; d <<= 1) x += (uint32_t)__shfl_xor((int)x, d);
		return x;
	}
	__device__ __forceinline__ uint32_t wave_max(uint32_t x)
	{
#pragma unroll
		for (int d = 1; d < WAVE; d <<= 1) x = max(x, (uint32_t)__shfl_xor((int)x, d));
		return x;
	}

	// exclusive rank of v among the workgroup's THREADS threads, in thread order; total: the workgroup's sum (every thread gets it).
	// s_wave: THREADS / WAVE words of LDS; every thread of the workgroup must call.
	template <int THREADS>
	__device__ __forceinline__ uint32_t block_rank(uint32_t v, uint32_t* s_wave, uint32_t& total)
	{
		const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
		const uint32_t x = wave_inclusive_sum(v);
		__syncthreads();                                  // the previous call's readers are done with s_wave[]
		if (lane == WAVE - 1) s_wave[wave] = x;
		__syncthreads();
		uint32_t before = 0;
		total = 0;
#pragma unroll
		for (int w = 0; w < THREADS / WAVE; w++)
		{
			const uint32_t c = s_wave[w];
			if (w < wave) before += c;
			total += c;
		}
		return before + x - v;
	}

	// block_rank over 64-bit values; s_wave: THREADS / WAVE 64-bit words of LDS
	template <int THREADS>
	__device__ __forceinline__ uint64_t block_rank(uint64_t v, uint64_t* s_wave, uint64_t& total)
	{
		const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
		const uint64_t x = wave_inclusive_sum(v);
		__syncthreads();
		if (lane == WAVE - 1) s_wave[wave] = x;
		__syncthreads();
		uint64_t before = 0;
		total = 0;
#pragma unroll
		for (int w = 0; w < THREADS / WAVE; w++)
		{
			const uint64_t c = s_wave[w];
			if (w < wave) before += c;
			total += c;
		}
		return before + x - v;
	}

	// one workgroup of THREADS threads: counts[0 .. n) -> their exclusive scan, in place; returns the sum (every thread gets it)
	template <int THREADS>
	__device__ __forceinline__ uint32_t block_scan_counts(uint32_t* __restrict__ counts, const int n, uint32_t* s_wave)
	{
		uint32_t carry = 0;
		for (int base = 0; base < n; base += THREADS)
		{
			const int i = base + (int)threadIdx.x;
			const uint32_t v = i < n ? counts[i] : 0u;
			uint32_t total;
			const uint32_t before = block_rank<THREADS>(v, s_wave, total);
			if (i < n) counts[i] = carry + before;
			carry += total;
		}
		return carry;
	}
}
