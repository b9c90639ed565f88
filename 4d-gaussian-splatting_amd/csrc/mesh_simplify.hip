// mesh_simplify.hip -- vertex-clustering simplification of a mesh on the device (gfx950), with mean or quadric placement of the
// cluster vertices (fdgs_mesh_simplify).  The statement is in include/fdgs.h; tests/simplify_oracle.py is the same statement in numpy.
// Float32 in the written operation order, the quadric sums and their solve in float64 (built with FP contraction off).  No float
// atomics, no integer atomics either: every count is a flag scan.  One lane owns a vertex, a sorted position, a cluster row or a face;
// every loop is bounded by a row length or by log2 of an array length, nothing waits for another thread.
//
//   cells      one lane per vertex: (cell, vertex) pairs; a vertex with a non-finite coordinate carries the key nx ny nz
//   sort       radix_sort_pairs by cell (stable: a row's members in ascending vertex index)
//   heads      (compact.h: count, scan, emit) one lane per sorted position: "a row starts here"; the total is the cluster count;
//              emit: vertex_map[vertex] = cluster (-1 without a cell), cluster_start[cluster] = the row's first position
//   -- the vertex count is known; with faces: --
//   face keys  one lane per face: the mapped triple rotated to its smallest index, or (V, V, V) for a face that cannot survive
//   3 x sort   by third, second, first index (the keys of the second and third sort are gathered through the order so far)
//   unique     one lane per sorted position: keep[face] = "a candidate, and the triple differs from the previous position's"
//   kept faces (compact.h: count, scan)  -- the face count is known; the emitting call goes on: --
//   cluster    one lane per cluster: mean position (cell units), colour, normal along the row; mean placement writes the vertex
//   incidences / sort / rows / quadric   (quadric placement) (cluster, 3 face + corner) sorted by cluster, one lane per cluster sums
//              its row's ten float64 numbers in order and solves the stabilised 3 x 3 system by Cramer's rule
//   kept faces (emit)  one lane per face: survivors to their rank, as the mapped triple without rotation
#include "mesh_common.h"
#include <math.h>

namespace fdgs
{
	constexpr int64_t SIMPLIFY_MAX_CELLS = (int64_t)1 << 30;

	struct SimplifyArgs
	{
		int V, F;
		const float *vertices, *normals, *colors;
		const int32_t* faces;
		float ox, oy, oz, h;
		int nx, ny, nz;
		uint32_t ncells;                    // nx ny nz: the key of a vertex without a cell
		int placement;
		double stabilise;
		int32_t* map;                       // [V] vertex -> cluster, -1 without a cell
		int32_t* user_map;                  // the caller's copy of it, or NULL
		int32_t* cluster_start;             // [V] the first sorted position of every cluster's row
		float* mean;                        // [V, 3] every cluster's mean position in cell units
		uint32_t* canon[3];                 // [F] each: the canonical triple
		uint8_t* keep;                      // [F] 1 for a surviving face
		int32_t *n_vertices, *n_faces;
		int vcap, fcap;
		float *out_vertices, *out_normals, *out_colors;
		int32_t* out_faces;
	};

	// ---- the grid ----
	__device__ __forceinline__ bool finite3(float x, float y, float z) { return __builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z); }
	__device__ __forceinline__ int cell_axis(float p, float o, float h, int n)
	{
		const float f = floorf((p - o) / h);                 // p finite: f is a number or +-inf, never NaN
		return f >= (float)n ? n - 1 : (f > 0.f ? (int)f : 0);
	}
	__device__ __forceinline__ float centre_axis(int i, float o, float h) { return o + ((float)i + 0.5f) * h; }
	struct Cell { float cx, cy, cz; };
	__device__ __forceinline__ Cell cell_centre(const SimplifyArgs& a, uint32_t cell)
	{
		const int i = (int)(cell % (uint32_t)a.nx), j = (int)((cell / (uint32_t)a.nx) % (uint32_t)a.ny), k = (int)(cell / ((uint32_t)a.nx * (uint32_t)a.ny));
		Cell c;
		c.cx = centre_axis(i, a.ox, a.h); c.cy = centre_axis(j, a.oy, a.h); c.cz = centre_axis(k, a.oz, a.h);
		return c;
	}
	__device__ __forceinline__ float clamp_half(float x) { return fminf(fmaxf(x, -0.5f), 0.5f); }
	__device__ __forceinline__ double clamp_half(double x) { return fmin(fmax(x, -0.5), 0.5); }

	// ---- clusters ----
	__global__ void __launch_bounds__(MESH_THREADS) simplify_cells_kernel(const SimplifyArgs a, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals)
	{
		const int v = blockIdx.x * MESH_THREADS + threadIdx.x;
		if (v >= a.V) return;
		const size_t r = 3 * (size_t)v;
		const float x = a.vertices[r], y = a.vertices[r + 1], z = a.vertices[r + 2];
		uint32_t key = a.ncells;
		if (finite3(x, y, z))
		{
			const int i = cell_axis(x, a.ox, a.h, a.nx), j = cell_axis(y, a.oy, a.h, a.ny), k = cell_axis(z, a.oz, a.h, a.nz);
			key = ((uint32_t)k * (uint32_t)a.ny + (uint32_t)j) * (uint32_t)a.nx + (uint32_t)i;
		}
		keys[v] = key;
		vals[v] = (uint32_t)v;
	}

	// the heads of the sorted cells' rows: position i starts a row if it has a cell and it differs from the one before
	struct SimplifyHeads
	{
		SimplifyArgs a;
		const uint32_t *keys, *vals;
		struct Item {};
		__host__ __device__ int size() const { return a.V; }
		__device__ uint32_t count(int i, Item&, bool) const { return keys[i] != a.ncells && (i == 0 || keys[i - 1] != keys[i]) ? 1u : 0u; }
		__device__ void emit(int i, uint32_t head, uint32_t rank, const Item&) const
		{
			// the heads before a position that has a cell include its own row's, unless it is that head
			const int32_t cluster = keys[i] == a.ncells ? -1 : (int32_t)(head ? rank : rank - 1u);
			const uint32_t v = vals[i];
			a.map[v] = cluster;
			if (a.user_map) a.user_map[v] = cluster;
			if (head) a.cluster_start[rank] = i;
		}
	};

	// one lane per cluster: the sums along its row, in ascending vertex index
	__global__ void __launch_bounds__(MESH_THREADS) simplify_cluster_kernel(const SimplifyArgs a, const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals)
	{
		const int c = blockIdx.x * MESH_THREADS + threadIdx.x;
		if (c >= a.V || c >= *a.n_vertices) return;
		const int s = a.cluster_start[c];
		const uint32_t cell = keys[s];
		const Cell ce = cell_centre(a, cell);
		float sx = 0.f, sy = 0.f, sz = 0.f, cr = 0.f, cg = 0.f, cb = 0.f, nx = 0.f, ny = 0.f, nz = 0.f;
		int n = 0;
		for (int i = s; i < a.V && keys[i] == cell; i++, n++)
		{
			const size_t r = 3 * (size_t)vals[i];
			sx = sx + (a.vertices[r] - ce.cx) / a.h;
			sy = sy + (a.vertices[r + 1] - ce.cy) / a.h;
			sz = sz + (a.vertices[r + 2] - ce.cz) / a.h;
			if (a.out_colors) { cr = cr + a.colors[r]; cg = cg + a.colors[r + 1]; cb = cb + a.colors[r + 2]; }
			if (a.out_normals) { nx = nx + a.normals[r]; ny = ny + a.normals[r + 1]; nz = nz + a.normals[r + 2]; }
		}
		const float fn = (float)n;
		const float mx = sx / fn, my = sy / fn, mz = sz / fn;
		const size_t d = 3 * (size_t)c;
		a.mean[d] = mx; a.mean[d + 1] = my; a.mean[d + 2] = mz;
		if (c >= a.vcap) return;
		if (a.out_vertices && a.placement == 0)
		{
			a.out_vertices[d] = ce.cx + a.h * clamp_half(mx);
			a.out_vertices[d + 1] = ce.cy + a.h * clamp_half(my);
			a.out_vertices[d + 2] = ce.cz + a.h * clamp_half(mz);
		}
		if (a.out_colors) { a.out_colors[d] = cr / fn; a.out_colors[d + 1] = cg / fn; a.out_colors[d + 2] = cb / fn; }
		if (a.out_normals)
		{
			const float len2 = (nx * nx + ny * ny) + nz * nz;
			if (len2 > 0.f)
			{
				const float len = sqrtf(len2);
				nx = nx / len; ny = ny / len; nz = nz / len;
			}
			else nx = ny = nz = 0.f;
			a.out_normals[d] = nx; a.out_normals[d + 1] = ny; a.out_normals[d + 2] = nz;
		}
	}

	// ---- quadric placement ----
	// keys[3 f + k] = the cluster of corner k of face f (V for an absent face or a vertex without a cell), vals[3 f + k] = 3 f + k
	__global__ void __launch_bounds__(MESH_THREADS) simplify_incidences_kernel(const SimplifyArgs a, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals)
	{
		const int f = blockIdx.x * MESH_THREADS + threadIdx.x;
		if (f >= a.F) return;
		int c[3];
		const bool present = face_present(a.faces, f, a.V, c[0], c[1], c[2]);
#pragma unroll
		for (int k = 0; k < 3; k++)
		{
			const int32_t m = present ? a.map[c[k]] : -1;
			keys[3 * (size_t)f + k] = m >= 0 ? (uint32_t)m : (uint32_t)a.V;
			vals[3 * (size_t)f + k] = 3u * (uint32_t)f + k;
		}
	}

	__global__ void __launch_bounds__(MESH_THREADS) simplify_quadric_kernel(const SimplifyArgs a, const uint32_t* __restrict__ cell_keys, const uint32_t* __restrict__ vals,
	                                                                        const int32_t* __restrict__ row_start)
	{
		const int c = blockIdx.x * MESH_THREADS + threadIdx.x;
		if (c >= a.V || c >= *a.n_vertices || c >= a.vcap) return;
		const Cell ce = cell_centre(a, cell_keys[a.cluster_start[c]]);
		const float h = a.h;
		double a00 = 0., a01 = 0., a02 = 0., a11 = 0., a12 = 0., a22 = 0., b0 = 0., b1 = 0., b2 = 0.;
		for (int i = row_start[c]; i < row_start[c + 1]; i++)
		{
			const int32_t* face = a.faces + 3 * (size_t)(vals[i] / 3u);
			const size_t ra = 3 * (size_t)face[0], rb = 3 * (size_t)face[1], rc = 3 * (size_t)face[2];
			const float ax = (a.vertices[ra] - ce.cx) / h, ay = (a.vertices[ra + 1] - ce.cy) / h, az = (a.vertices[ra + 2] - ce.cz) / h;
			const float bx = (a.vertices[rb] - ce.cx) / h, by = (a.vertices[rb + 1] - ce.cy) / h, bz = (a.vertices[rb + 2] - ce.cz) / h;
			const float cx = (a.vertices[rc] - ce.cx) / h, cy = (a.vertices[rc + 1] - ce.cy) / h, cz = (a.vertices[rc + 2] - ce.cz) / h;
			const float ux = bx - ax, uy = by - ay, uz = bz - az, wx = cx - ax, wy = cy - ay, wz = cz - az;
			const float nx = uy * wz - uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx;
			const float l = sqrtf((nx * nx + ny * ny) + nz * nz);
			const float d = -((nx * ax + ny * ay) + nz * az);
			if (l > 0.f && __builtin_isfinite(l) && __builtin_isfinite(d))
			{
				const double X = nx, Y = ny, Z = nz, D = d, L = l;
				a00 = a00 + (X * X) / L; a01 = a01 + (X * Y) / L; a02 = a02 + (X * Z) / L;
				a11 = a11 + (Y * Y) / L; a12 = a12 + (Y * Z) / L; a22 = a22 + (Z * Z) / L;
				b0 = b0 + (X * D) / L; b1 = b1 + (Y * D) / L; b2 = b2 + (Z * D) / L;
			}
		}
		const size_t o = 3 * (size_t)c;
		const double mx = a.mean[o], my = a.mean[o + 1], mz = a.mean[o + 2];
		double x = mx, y = my, z = mz;
		const double trace = (a00 + a11) + a22;
		if (trace != 0.)
		{
			const double lam = (a.stabilise * trace) / 3.;
			const double m00 = a00 + lam, m11 = a11 + lam, m22 = a22 + lam;
			const double r0 = lam * mx - b0, r1 = lam * my - b1, r2 = lam * mz - b2;
			const double c00 = m11 * m22 - a12 * a12, c01 = a02 * a12 - a01 * m22, c02 = a01 * a12 - a02 * m11;
			const double c11 = m00 * m22 - a02 * a02, c12 = a01 * a02 - m00 * a12, c22 = m00 * m11 - a01 * a01;
			const double det = (m00 * c00 + a01 * c01) + a02 * c02;
			if (det > 0.)
			{
				x = ((c00 * r0 + c01 * r1) + c02 * r2) / det;
				y = ((c01 * r0 + c11 * r1) + c12 * r2) / det;
				z = ((c02 * r0 + c12 * r1) + c22 * r2) / det;
			}
		}
		a.out_vertices[o] = ce.cx + h * (float)clamp_half(x);
		a.out_vertices[o + 1] = ce.cy + h * (float)clamp_half(y);
		a.out_vertices[o + 2] = ce.cz + h * (float)clamp_half(z);
	}

	// ---- faces ----
	// the mapped triple of a face that can survive: present, every corner in a cluster, three different clusters
	__device__ __forceinline__ bool mapped_face(const SimplifyArgs& a, int f, int& i, int& j, int& k)
	{
		int x, y, z;
		if (f >= a.F || !face_present(a.faces, f, a.V, x, y, z)) return false;
		i = a.map[x]; j = a.map[y]; k = a.map[z];
		return i >= 0 && j >= 0 && k >= 0 && i != j && j != k && i != k;
	}

	__global__ void __launch_bounds__(MESH_THREADS) simplify_face_keys_kernel(const SimplifyArgs a, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals)
	{
		const int f = blockIdx.x * MESH_THREADS + threadIdx.x;
		if (f >= a.F) return;
		int i, j, k;
		uint32_t c0 = (uint32_t)a.V, c1 = (uint32_t)a.V, c2 = (uint32_t)a.V;
		if (mapped_face(a, f, i, j, k))
		{
			if (i < j && i < k) { c0 = i; c1 = j; c2 = k; }
			else if (j < k) { c0 = j; c1 = k; c2 = i; }
			else { c0 = k; c1 = i; c2 = j; }
		}
		a.canon[0][f] = c0; a.canon[1][f] = c1; a.canon[2][f] = c2;
		keys[f] = c2;
		vals[f] = (uint32_t)f;
	}

	// the next sort's keys: a component of the canonical triple, in the order the sorts so far left
	__global__ void __launch_bounds__(MESH_THREADS) simplify_gather_kernel(const uint32_t* __restrict__ canon, const uint32_t* __restrict__ vals, const int F,
	                                                                       uint32_t* __restrict__ keys)
	{
		const int i = blockIdx.x * MESH_THREADS + threadIdx.x;
		if (i < F) keys[i] = canon[vals[i]];
	}

	__global__ void __launch_bounds__(MESH_THREADS) simplify_unique_kernel(const SimplifyArgs a, const uint32_t* __restrict__ order)
	{
		const int i = blockIdx.x * MESH_THREADS + threadIdx.x;
		if (i >= a.F) return;
		const uint32_t f = order[i];
		const uint32_t c0 = a.canon[0][f], c1 = a.canon[1][f], c2 = a.canon[2][f];
		bool first = c0 != (uint32_t)a.V;
		if (first && i > 0)
		{
			const uint32_t g = order[i - 1];
			first = a.canon[0][g] != c0 || a.canon[1][g] != c1 || a.canon[2][g] != c2;
		}
		a.keep[f] = first ? 1 : 0;
	}

	// the faces simplify_unique_kernel kept, as their mapped triples
	struct SimplifyFaces
	{
		SimplifyArgs a;
		struct Item {};
		__host__ __device__ int size() const { return a.F; }
		__device__ uint32_t count(int f, Item&, bool) const { return a.keep[f] ? 1u : 0u; }
		__device__ void emit(int f, uint32_t kept, uint32_t rank, const Item&) const
		{
			if (!kept || rank >= (uint32_t)a.fcap) return;
			int i, j, k;
			mapped_face(a, f, i, j, k);
			const size_t d = 3 * (size_t)rank;
			a.out_faces[d] = i; a.out_faces[d + 1] = j; a.out_faces[d + 2] = k;
		}
	};

	// ---- host side ----
	struct SimplifyLayout { size_t vkeys[2], vvals[2], fkeys[2], fvals[2], hist, map, cluster_start, mean, row_start, canon[3], keep, vcounts, fcounts, total; };
	static SimplifyLayout simplify_layout(int V, int F)
	{
		SimplifyLayout L;
		ScratchCursor c;
		const size_t n = 3 * (size_t)F;
		for (int k = 0; k < 2; k++) L.vkeys[k] = c.take((size_t)V * 4);
		for (int k = 0; k < 2; k++) L.vvals[k] = c.take((size_t)V * 4);
		for (int k = 0; k < 2; k++) L.fkeys[k] = c.take(n * 4);
		for (int k = 0; k < 2; k++) L.fvals[k] = c.take(n * 4);
		int sb = sort_blocks(V);
		if (sort_blocks(F) > sb) sb = sort_blocks(F);
		if (sort_blocks((int)n) > sb) sb = sort_blocks((int)n);
		L.hist = c.take((size_t)RADIX * ((size_t)sb + 1) * 4);
		L.map = c.take((size_t)V * sizeof(int32_t));
		L.cluster_start = c.take((size_t)V * sizeof(int32_t));
		L.mean = c.take(3 * (size_t)V * sizeof(float));
		L.row_start = c.take(((size_t)V + 1) * sizeof(int32_t));
		for (int k = 0; k < 3; k++) L.canon[k] = c.take((size_t)F * 4);
		L.keep = c.take((size_t)F);
		L.vcounts = c.take(blocks_of((size_t)V) * sizeof(uint32_t));
		L.fcounts = c.take(blocks_of((size_t)F) * sizeof(uint32_t));
		L.total = c.o;
		return L;
	}
	static int bits_of(uint32_t largest_key)
	{
		int bits = 0;
		while (bits < 32 && (largest_key >> bits) != 0) bits++;
		return div_up(bits, RADIX_BITS) * RADIX_BITS;
	}
}

using namespace fdgs;

extern "C" size_t fdgs_mesh_simplify_scratch_bytes(int32_t V, int32_t F)
{
	return mesh_sizes_ok(V, F) ? simplify_layout(V, F).total : 0;
}

extern "C" int fdgs_mesh_simplify(const fdgs_mesh_in* mesh, const fdgs_mesh_simplify_params* params, const fdgs_surface_out* out, void* scratch,
                                  void* stream_v)
{
	const char* fn = "fdgs_mesh_simplify";
	if (const int rc = mesh_in_args(fn, mesh)) return rc;
	if (!params) return fail(FDGS_ERR_INVALID_ARG, "%s: params must not be NULL", fn);
	CHECK_STRUCT_IN(fn, params, fdgs_mesh_simplify_params);
	if (!(params->cell > 0.f) || !finite_f(params->cell)) return fail(FDGS_ERR_INVALID_ARG, "%s: cell must be positive and finite", fn);
	if (!finite_f(params->origin[0]) || !finite_f(params->origin[1]) || !finite_f(params->origin[2])) return fail(FDGS_ERR_INVALID_ARG, "%s: origin must be finite", fn);
	if (params->nx < 1 || params->ny < 1 || params->nz < 1) return fail(FDGS_ERR_INVALID_ARG, "%s: the grid dimensions nx, ny, nz must be at least 1", fn);
	const int64_t ncells = (int64_t)params->nx * params->ny;     // < 2^62
	if (ncells > SIMPLIFY_MAX_CELLS || ncells * params->nz > SIMPLIFY_MAX_CELLS) return fail(FDGS_ERR_INVALID_ARG, "%s: the grid must not have more than 2^30 cells", fn);
	if (!(params->stabilise >= 0.f)) return fail(FDGS_ERR_INVALID_ARG, "%s: stabilise must not be negative or NaN", fn);
	if (params->placement != FDGS_SIMPLIFY_MEAN && params->placement != FDGS_SIMPLIFY_QUADRIC) return fail(FDGS_ERR_INVALID_ARG, "%s: placement must be 0 (mean) or 1 (quadric)", fn);
	SurfaceOut so;
	if (const int rc = surface_out_args(fn, out, so)) return rc;
	const int V = mesh->V, F = mesh->F;
	if (V > 0 && !mesh->vertices) return fail(FDGS_ERR_INVALID_ARG, "%s: the mesh's vertices must not be NULL with V > 0", fn);
	if ((out->normals && !mesh->normals) || (out->colors && !mesh->colors)) return fail(FDGS_ERR_INVALID_ARG, "%s: an output array needs its input array", fn);
	if (V > 0 && !scratch) return fail(FDGS_ERR_INVALID_ARG, "%s: scratch must not be NULL with V > 0", fn);
	hipStream_t stream = (hipStream_t)stream_v;
	if (V == 0) return surface_out_empty(fn, out, stream);        // no vertex: every face is absent
	if (F == 0) HIP_TRY(hipMemsetAsync(out->n_faces, 0, sizeof(int32_t), stream), "fdgs_mesh_simplify: memset");
	const SimplifyLayout L = simplify_layout(V, F);
	char* base = reinterpret_cast<char*>(scratch);
	auto u32 = [&](size_t off) { return reinterpret_cast<uint32_t*>(base + off); };
	SimplifyArgs a;
	a.V = V; a.F = F;
	a.vertices = mesh->vertices; a.normals = mesh->normals; a.colors = mesh->colors; a.faces = mesh->faces;
	a.ox = params->origin[0]; a.oy = params->origin[1]; a.oz = params->origin[2]; a.h = params->cell;
	a.nx = params->nx; a.ny = params->ny; a.nz = params->nz; a.ncells = (uint32_t)(ncells * params->nz);
	a.placement = params->placement; a.stabilise = (double)params->stabilise;
	a.map = reinterpret_cast<int32_t*>(base + L.map); a.user_map = params->vertex_map;
	a.cluster_start = reinterpret_cast<int32_t*>(base + L.cluster_start);
	a.mean = reinterpret_cast<float*>(base + L.mean);
	for (int k = 0; k < 3; k++) a.canon[k] = u32(L.canon[k]);
	a.keep = reinterpret_cast<uint8_t*>(base + L.keep);
	a.n_vertices = out->n_vertices; a.n_faces = out->n_faces;
	a.out_vertices = out->vertices; a.out_normals = out->normals; a.out_colors = out->colors; a.out_faces = out->faces;
	a.vcap = so.vcap; a.fcap = so.fcap;
	const int vb = (int)blocks_of((size_t)V), fb = (int)blocks_of((size_t)F);
	const dim3 T(MESH_THREADS);
	uint32_t* hist = u32(L.hist);
	const char* sort = "fdgs_mesh_simplify: sort";

	// clusters
	uint32_t* vkeys[2] = { u32(L.vkeys[0]), u32(L.vkeys[1]) };
	uint32_t* vvals[2] = { u32(L.vvals[0]), u32(L.vvals[1]) };
	int vres = 0;
	hipLaunchKernelGGL(simplify_cells_kernel, dim3(vb), T, 0, stream, a, vkeys[0], vvals[0]);
	HIP_TRY(radix_sort_pairs(vkeys, vvals, V, 0, bits_of(a.ncells), hist, stream, &vres), sort);
	const uint32_t *cell_keys = vkeys[vres], *cell_vals = vvals[vres];
	compact_enqueue(Compaction<SimplifyHeads>{ { a, cell_keys, cell_vals }, u32(L.vcounts), out->n_vertices, 1u, true }, stream);

	// faces: which survive
	Compaction<SimplifyFaces> kept{ { a }, u32(L.fcounts), out->n_faces, 1u, false };
	if (F > 0)
	{
		uint32_t* keys[2] = { u32(L.fkeys[0]), u32(L.fkeys[1]) };
		uint32_t* vals[2] = { u32(L.fvals[0]), u32(L.fvals[1]) };
		const int bits = bits_of((uint32_t)V);
		hipLaunchKernelGGL(simplify_face_keys_kernel, dim3(fb), T, 0, stream, a, keys[0], vals[0]);
		for (int component = 2; component >= 0; component--)
		{
			int res = 0;
			HIP_TRY(radix_sort_pairs(keys, vals, F, 0, bits, hist, stream, &res), sort);
			if (res) { uint32_t* t = keys[0]; keys[0] = keys[1]; keys[1] = t; t = vals[0]; vals[0] = vals[1]; vals[1] = t; }
			if (component > 0) hipLaunchKernelGGL(simplify_gather_kernel, dim3(fb), T, 0, stream, a.canon[component - 1], vals[0], F, keys[0]);
		}
		hipLaunchKernelGGL(simplify_unique_kernel, dim3(fb), T, 0, stream, a, vals[0]);
		compact_enqueue(kept, stream);                       // count and scan; the emit comes last
	}

	// the emitting call
	if (so.any_vertex)
	{
		hipLaunchKernelGGL(simplify_cluster_kernel, dim3(vb), T, 0, stream, a, cell_keys, cell_vals);
		if (a.out_vertices && a.placement == FDGS_SIMPLIFY_QUADRIC)
		{
			uint32_t* keys[2] = { u32(L.fkeys[0]), u32(L.fkeys[1]) };
			uint32_t* vals[2] = { u32(L.fvals[0]), u32(L.fvals[1]) };
			int32_t* row_start = reinterpret_cast<int32_t*>(base + L.row_start);
			const int n = 3 * F;
			int res = 0;
			if (F > 0)
			{
				hipLaunchKernelGGL(simplify_incidences_kernel, dim3(fb), T, 0, stream, a, keys[0], vals[0]);
				HIP_TRY(radix_sort_pairs(keys, vals, n, 0, bits_of((uint32_t)V), hist, stream, &res), sort);
			}
			hipLaunchKernelGGL(rows_from_sorted_keys_kernel<MESH_THREADS>, dim3((int)blocks_of((size_t)V + 1)), T, 0, stream, keys[res], n, V,
			                   (const int32_t*)out->n_vertices, row_start);
			hipLaunchKernelGGL(simplify_quadric_kernel, dim3(vb), T, 0, stream, a, cell_keys, vals[res], row_start);
		}
	}
	kept.emit = a.out_faces != nullptr;
	compact_emit(kept, stream);
	return launched("fdgs_mesh_simplify");
}
