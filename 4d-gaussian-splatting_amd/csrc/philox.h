// philox.h -- Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11), the counter-based
// generator of seed.hip and mcmc.hip: no state, any draw can be made on its own, the same words on every run.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fdgs
{
	__device__ __forceinline__ uint4 philox4x32_10(uint4 c, uint2 k)
	{
#pragma unroll
		for (int r = 0; r < 10; r++)
		{
			const uint32_t hi0 = __umulhi(0xD2511F53u, c.x), lo0 = 0xD2511F53u * c.x;
			const uint32_t hi1 = __umulhi(0xCD9E8D57u, c.z), lo1 = 0xCD9E8D57u * c.z;
			c = make_uint4(hi1 ^ c.y ^ k.x, lo1, hi0 ^ c.w ^ k.y, lo0);
			k.x += 0x9E3779B9u; k.y += 0xBB67AE85u;
		}
		return c;
	}
	// the key of a 64-bit seed: (low word, high word)
	static inline uint2 philox_key(const uint64_t seed) { return make_uint2((uint32_t)(seed & 0xffffffffull), (uint32_t)(seed >> 32)); }
}
