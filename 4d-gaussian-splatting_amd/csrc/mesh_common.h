// mesh_common.h -- what the translation units that make or take meshes (tsdf.hip, mesh.hip, mesh_simplify.hip) share: the size limits,
// the absent-face rule, the rows of sorted incidences, and the host-side argument checks of fdgs_mesh_in and fdgs_surface_out.
// The flag scans they all use are compact.h.
#pragma once
#include "fdgs_common.h"
#include "compact.h"

namespace fdgs
{
	constexpr int MESH_THREADS = COMPACT_THREADS;
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

	// row_start[r], r in [0, R]: the first sorted position whose key is >= r (row r is [row_start[r], row_start[r + 1])).
	// R = rows, or the smaller of rows and *rows_dev where the number of rows is a count still on the device.
	template <int THREADS>
	__global__ void __launch_bounds__(THREADS) rows_from_sorted_keys_kernel(const uint32_t* __restrict__ keys, const int n, const int rows,
	                                                                        const int32_t* __restrict__ rows_dev, int32_t* __restrict__ row_start)
	{
		const int r = blockIdx.x * THREADS + threadIdx.x;
		if (r > rows || (rows_dev && r > *rows_dev)) return;
		row_start[r] = lower_bound_u32(keys, n, (uint32_t)r);
	}

	static bool finite_f(float v) { return v - v == 0.f; }
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
	static size_t blocks_of(size_t n) { return compact_blocks(n); }

	// What an entry point that writes a mesh does with its fdgs_surface_out.  The capacities count only where an array was given:
	// a call without vertex arrays (without faces) emits no vertex (no face) and still counts them.
	struct SurfaceOut
	{
		bool any_vertex;
		int vcap, fcap;
	};
	static int surface_out_args(const char* fn, const fdgs_surface_out* out, SurfaceOut& o)
	{
		if (!out) return fail(FDGS_ERR_INVALID_ARG, "%s: out must not be NULL", fn);
		CHECK_STRUCT_IN(fn, out, fdgs_surface_out);
		if (!out->n_vertices || !out->n_faces) return fail(FDGS_ERR_INVALID_ARG, "%s: n_vertices and n_faces must not be NULL", fn);
		if (out->vertex_capacity < 0 || out->face_capacity < 0) return fail(FDGS_ERR_INVALID_ARG, "%s: capacities must not be negative", fn);
		o.any_vertex = out->vertices || out->normals || out->colors;
		o.vcap = o.any_vertex ? out->vertex_capacity : 0;
		o.fcap = out->faces ? out->face_capacity : 0;
		return FDGS_OK;
	}
	// the mesh of nothing: both counts 0, no array touched
	static int surface_out_empty(const char* fn, const fdgs_surface_out* out, hipStream_t stream)
	{
		for (int32_t* n : { out->n_vertices, out->n_faces })
		{
			const hipError_t e = hipMemsetAsync(n, 0, sizeof(int32_t), stream);
			if (e != hipSuccess) return fail(FDGS_ERR_HIP, "%s: memset: %s", fn, hipGetErrorString(e));
		}
		return FDGS_OK;
	}
}
