// mesh_common.h -- what the mesh translation units (mesh.hip, mesh_simplify.hip) share: the size limits, the absent-face rule and the
// host-side argument checks of fdgs_mesh_in.  The flag scans they both use are block_scan.h.
#pragma once
#include "fdgs_common.h"
#include "block_scan.h"

namespace fdgs
{
	constexpr int MESH_THREADS = 256;
	constexpr int MESH_SCAN_THREADS = 1024;
	constexpr int MESH_MAX = 1 << 28;                    // V, F below it: 3 F and 3 face + corner stay int32

	__device__ __forceinline__ bool face_present(const int32_t* __restrict__ faces, int f, int V, int& a, int& b, int& c)
	{
		a = faces[3 * (size_t)f + 0]; b = faces[3 * (size_t)f + 1]; c = faces[3 * (size_t)f + 2];
		return (uint32_t)a < (uint32_t)V && (uint32_t)b < (uint32_t)V && (uint32_t)c < (uint32_t)V;
	}

	// the first position of the ascending keys[0 .. n) whose key is >= v
	__device__ __forceinline__ int lower_bound_u32(const uint32_t* __restrict__ keys, const int n, const uint32_t v)
	{
		int lo = 0, hi = n;
		while (lo < hi)
		{
			const int mid = lo + (hi - lo) / 2;
			if (keys[mid] < v) lo = mid + 1;
			else hi = mid;
		}
		return lo;
	}

	static bool mesh_sizes_ok(int64_t V, int64_t F) { return V >= 0 && F >= 0 && V < MESH_MAX && F < MESH_MAX; }
	static int mesh_in_args(const char* fn, const fdgs_mesh_in* m)
	{
		if (!m) return fail(FDGS_ERR_INVALID_ARG, "%s: mesh must not be NULL", fn);
		CHECK_STRUCT_IN(fn, m, fdgs_mesh_in);
		if (m->V < 0 || m->F < 0) return fail(FDGS_ERR_INVALID_ARG, "%s: V and F must not be negative", fn);
		if (!mesh_sizes_ok(m->V, m->F)) return fail(FDGS_ERR_INVALID_ARG, "%s: need V < 2^28 and F < 2^28", fn);
		if (m->F > 0 && !m->faces) return fail(FDGS_ERR_INVALID_ARG, "%s: faces must not be NULL with F > 0", fn);
		return FDGS_OK;
	}
	static size_t blocks_of(size_t n) { return (n + MESH_THREADS - 1) / MESH_THREADS; }
}
