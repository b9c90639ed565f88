// mesh.hip -- cleaning and smoothing the meshes fdgs_surface_extract leaves on the device (gfx950): connected components
// (fdgs_mesh_components), component filtering with order-preserving compaction (fdgs_mesh_compact) and Taubin smoothing with
// recomputed normals (fdgs_mesh_smooth).  Conventions: include/fdgs.h.  A face with an index outside [0, V) is absent everywhere:
// face_present() (mesh_common.h, shared with mesh_simplify.hip) is the one place that reads a face's indices before they are used as addresses.
//
// Components.  A lock-free union-find over parent[V] (parent[v] <= v always; a root is its own parent):
//   hook      one lane per face: unite (a, b) and (a, c).  unite = find both roots, compare-and-swap the larger root onto the
//             smaller; a failed swap returns that root's new, strictly smaller parent and the retry goes on from there -- every loop
//             here walks a strictly decreasing chain of indices, none waits for another thread.  find halves paths as it goes.
//   (host)    reads one flag: did any face see two different roots?  No: done.  Yes: compress, hook again (the check) -- 32 at most.
//   compress  one lane per vertex: parent[v] = its root (the only store to parent[v] in that launch)
// One hook pass unites everything (the swap is the linearisation point), so the second finds nothing to do; the result is checked
// on the device whatever the memory system did in between.  A component's root is its smallest index, whatever the schedule.
//   roots (count / scan / emit) / assign   dense ids = the compaction (compact.h) of "v is a root"
//   vertex count / face count      wave-aggregated integer atomics; all a `labelled` call runs (ids from an earlier call)
//
// Compaction, shaped as tsdf.hip's extraction: two passes of compact.h (vertices, faces) that share their scan launch.
//
// Smoothing.  pairs (vertex, 3 face + corner) -> radix_sort_pairs by vertex (stable: rows in ascending 3 face + corner; absent faces'
// corners carry the key V and end up behind every row) -> row starts by binary search -> the two other corners of every incidence,
// once -> boundary flags, once -> 2 x iterations passes between two position buffers, one lane per vertex summing its row in order
// -> normals.  Float32 in the operation order of the written statement (built with FP contraction off).  No float atomics.
#include "mesh_common.h"
#include <math.h>

namespace fdgs
{
	constexpr int MESH_MAX_ROUNDS = 32;

	// ---- components ----
	// parent[] is read and written by many workgroups in one launch: every access is a relaxed agent-scope atomic (no stale cache line)
	__device__ __forceinline__ int cc_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
	__device__ __forceinline__ void cc_store(int32_t* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

	// the root above x.  x strictly decreases: at most x steps.  halve: x's parent becomes its grandparent (an ancestor either way)
	template <bool HALVE>
	__device__ __forceinline__ int cc_find(int32_t* parent, int x)
	{
		int p = cc_load(parent + x);
		while (p != x)
		{
			const int g = cc_load(parent + p);
			if (HALVE && g != p) cc_store(parent + x, g);
			x = p;
			p = g;
		}
		return x;
	}

	// true if a and b were under different roots when looked at
	__device__ __forceinline__ bool cc_unite(int32_t* parent, int a, int b)
	{
		int ra = cc_find<true>(parent, a), rb = cc_find<true>(parent, b);
		const bool differed = ra != rb;
		while (ra != rb)
		{
			const int hi = ra > rb ? ra : rb, lo = ra > rb ? rb : ra;
			const int old = atomicCAS(parent + hi, hi, lo);
			if (old == hi) break;                            // hi was still a root and now hangs under lo
			ra = cc_find<true>(parent, old);                 // old < hi: max(ra, rb) went down
			rb = cc_find<true>(parent, lo);
		}
		return differed;
	}

	__global__ void __launch_bounds__(MESH_THREADS) cc_init_kernel(int32_t* __restrict__ parent, const int V)
	{
		const int v = blockIdx.x * MESH_THREADS + threadIdx.x;
		if (v < V) parent[v] = v;
	}

	__global__ void __launch_bounds__(MESH_THREADS) cc_hook_kernel(const int32_t* __restrict__ faces, const int F, const int V, int32_t* parent,
	                                                               int32_t* changed)
	{
		const int f = blockIdx.x * MESH_THREADS + threadIdx.x;
		int a, b, c;
		if (f >= F || !face_present(faces, f, V, a, b, c)) return;
		const bool ab = cc_unite(parent, a, b), ac = cc_unite(parent, a, c);
		if (ab || ac) cc_store(changed, 1);
	}

	__global__ void __launch_bounds__(MESH_THREADS) cc_compress_kernel(int32_t* parent, const int V)
	{
		const int v = blockIdx.x * MESH_THREADS + threadIdx.x;
		if (v < V) cc_store(parent + v, cc_find<false>(parent, v));
	}

	// the roots' dense ids, into their own rows of vertex_component
	struct CcRoots
	{
		const int32_t* parent;
		int V;
		int32_t* vertex_component;
		struct Item {};
		__host__ __device__ int size() const { return V; }
		__device__ uint32_t count(int v, Item&, bool) const { return parent[v] == v ? 1u : 0u; }
		__device__ void emit(int v, uint32_t root, uint32_t rank, const Item&) const { if (root) vertex_component[v] = (int32_t)rank; }
	};

	// counts[c] += 1 for every lane with valid set, one atomic per distinct c of the wave.  Every lane of the wave must call;
	// each turn of the loop retires the first pending lane and all lanes with its c.
	__device__ __forceinline__ void wave_count(int32_t* counts, int c, bool valid)
	{
		const int lane = threadIdx.x & (WAVE - 1);
		unsigned long long todo = __ballot(valid);
		while (todo)
		{
			const int leader = __ffsll((long long)todo) - 1;
			const int lc = __shfl(c, leader);
			const unsigned long long same = __ballot(valid && c == lc);
			if (lane == leader) atomicAdd(counts + lc, (int32_t)__popcll(same));
			todo &= ~same;
		}
	}

	// the other vertices take their root's id (a root's row is not written here)
	__global__ void __launch_bounds__(MESH_THREADS) cc_assign_kernel(const int32_t* __restrict__ parent, const int V, int32_t* vertex_component)
	{
		const int v = blockIdx.x * MESH_THREADS + threadIdx.x;
		if (v >= V) return;
		const int r = parent[v];
		if (r != v) vertex_component[v] = vertex_component[r];
	}

	// vertices and faces per component; an id outside [0, cap) is counted nowhere
	__global__ void __launch_bounds__(MESH_THREADS) cc_vertex_count_kernel(const int32_t* __restrict__ vertex_component, const int V,
	                                                                       int32_t* component_vertices, const int cap)
	{
		const int v = blockIdx.x * MESH_THREADS + threadIdx.x;
		const int id = v < V ? vertex_component[v] : 0;
		wave_count(component_vertices, id, v < V && (uint32_t)id < (uint32_t)cap);
	}

	__global__ void __launch_bounds__(MESH_THREADS) cc_face_count_kernel(const int32_t* __restrict__ faces, const int F, const int V,
	                                                                     const int32_t* __restrict__ vertex_component, int32_t* component_faces, const int cap)
	{
		const int f = blockIdx.x * MESH_THREADS + threadIdx.x;
		int a, b, c, id = 0;
		bool valid = false;
		if (f < F && face_present(faces, f, V, a, b, c))
		{
			id = vertex_component[a];
			valid = (uint32_t)id < (uint32_t)cap;
		}
		wave_count(component_faces, id, valid);
	}

	// ---- compaction ----
	struct CompactArgs
	{
		int V, F, C;
		const float *vertices, *normals, *colors;
		const int32_t *faces, *vertex_component;
		const uint8_t* keep;
		int32_t* map;                 // [V] old vertex -> new vertex, -1 for a dropped one
		int vcap, fcap;
		float *out_vertices, *out_normals, *out_colors;
		int32_t* out_faces;
	};

	__device__ __forceinline__ bool vertex_kept(const CompactArgs& a, int v)
	{
		const int c = a.vertex_component[v];
		return (uint32_t)c < (uint32_t)a.C && a.keep[c] != 0;
	}
	struct CompactVertices
	{
		CompactArgs a;
		struct Item {};
		__host__ __device__ int size() const { return a.V; }
		__device__ uint32_t count(int v, Item&, bool) const { return vertex_kept(a, v) ? 1u : 0u; }
		__device__ void emit(int v, uint32_t kept, uint32_t rank, const Item&) const
		{
			a.map[v] = kept ? (int32_t)rank : -1;
			if (!kept || rank >= (uint32_t)a.vcap) return;
			const size_t s = 3 * (size_t)v, d = 3 * (size_t)rank;
			if (a.out_vertices) { a.out_vertices[d] = a.vertices[s]; a.out_vertices[d + 1] = a.vertices[s + 1]; a.out_vertices[d + 2] = a.vertices[s + 2]; }
			if (a.out_normals) { a.out_normals[d] = a.normals[s]; a.out_normals[d + 1] = a.normals[s + 1]; a.out_normals[d + 2] = a.normals[s + 2]; }
			if (a.out_colors) { a.out_colors[d] = a.colors[s]; a.out_colors[d + 1] = a.colors[s + 1]; a.out_colors[d + 2] = a.colors[s + 2]; }
		}
	};

	struct CompactFaces
	{
		CompactArgs a;
		struct Item { int i, j, k; };
		__host__ __device__ int size() const { return a.F; }
		__device__ uint32_t count(int f, Item& c, bool) const { return face_present(a.faces, f, a.V, c.i, c.j, c.k) && vertex_kept(a, c.i) ? 1u : 0u; }
		__device__ void emit(int, uint32_t kept, uint32_t rank, const Item& c) const
		{
			if (!kept || rank >= (uint32_t)a.fcap) return;
			const size_t d = 3 * (size_t)rank;
			a.out_faces[d] = a.map[c.i]; a.out_faces[d + 1] = a.map[c.j]; a.out_faces[d + 2] = a.map[c.k];
		}
	};

	// ---- smoothing ----
	// keys[3 f + k] = corner k of face f (V for an absent face), vals[3 f + k] = 3 f + k
	__global__ void __launch_bounds__(MESH_THREADS) smooth_pairs_kernel(const int32_t* __restrict__ faces, const int F, const int V,
	                                                                    uint32_t* __restrict__ keys, uint32_t* __restrict__ vals)
	{
		const int f = blockIdx.x * MESH_THREADS + threadIdx.x;
		if (f >= F) return;
		int c[3];
		const bool present = face_present(faces, f, V, c[0], c[1], c[2]);
#pragma unroll
		for (int k = 0; k < 3; k++)
		{
			keys[3 * (size_t)f + k] = present ? (uint32_t)c[k] : (uint32_t)V;
			vals[3 * (size_t)f + k] = 3u * (uint32_t)f + k;
		}
	}

	// the other two corners of every incidence, in ascending corner index.  n_rows = row_start[V]: the incidences of present faces
	__global__ void __launch_bounds__(MESH_THREADS) smooth_others_kernel(const int32_t* __restrict__ faces, const uint32_t* __restrict__ vals,
	                                                                     const int32_t* __restrict__ row_start, const int V, const int n, int2* __restrict__ others)
	{
		const int i = blockIdx.x * MESH_THREADS + threadIdx.x;
		if (i >= n || i >= row_start[V]) return;
		const uint32_t val = vals[i], f = val / 3u, k = val - 3u * f;
		const int32_t* face = faces + 3 * (size_t)f;
		others[i] = make_int2(face[k == 0 ? 1 : 0], face[k == 2 ? 1 : 2]);
	}

	// boundary[v] = 1 if some index occurs among the other corners of exactly one incidence of v's row
	__global__ void __launch_bounds__(MESH_THREADS) smooth_boundary_kernel(const int2* __restrict__ others, const int32_t* __restrict__ row_start, const int V,
	                                                                       uint8_t* __restrict__ boundary)
	{
		const int v = blockIdx.x * MESH_THREADS + threadIdx.x;
		if (v >= V) return;
		const int s = row_start[v], e = row_start[v + 1];
		bool found = false;
		for (int i = s; i < e && !found; i++)
		{
			const int2 o = others[i];
			int nx = 0, ny = 0;
			for (int j = s; j < e; j++)
			{
				const int2 q = others[j];
				nx += (q.x == o.x || q.y == o.x) ? 1 : 0;
				ny += (q.x == o.y || q.y == o.y) ? 1 : 0;
			}
			found = nx == 1 || ny == 1;
		}
		boundary[v] = found ? 1 : 0;
	}

	__global__ void __launch_bounds__(MESH_THREADS) smooth_pass_kernel(const float* __restrict__ src, float* __restrict__ dst, const int2* __restrict__ others,
	                                                                   const int32_t* __restrict__ row_start, const uint8_t* __restrict__ pinned, const int V,
	                                                                   const float t)
	{
		const int v = blockIdx.x * MESH_THREADS + threadIdx.x;
		if (v >= V) return;
		const size_t r = 3 * (size_t)v;
		float px = src[r], py = src[r + 1], pz = src[r + 2];
		const int s = row_start[v], e = row_start[v + 1];
		if (e > s && !(pinned && pinned[v]))
		{
			float sx = 0.f, sy = 0.f, sz = 0.f;
			for (int i = s; i < e; i++)
			{
				const int2 o = others[i];
				const size_t a = 3 * (size_t)o.x, b = 3 * (size_t)o.y;
				sx = sx + (src[a] + src[b]);
				sy = sy + (src[a + 1] + src[b + 1]);
				sz = sz + (src[a + 2] + src[b + 2]);
			}
			const float d = (float)(2 * (e - s));
			px = px + t * (sx / d - px);
			py = py + t * (sy / d - py);
			pz = pz + t * (sz / d - pz);
		}
		dst[r] = px; dst[r + 1] = py; dst[r + 2] = pz;
	}

	__global__ void __launch_bounds__(MESH_THREADS) smooth_normals_kernel(const float* __restrict__ pos, const int32_t* __restrict__ faces,
	                                                                      const uint32_t* __restrict__ vals, const int32_t* __restrict__ row_start, const int V,
	                                                                      float* __restrict__ normals)
	{
		const int v = blockIdx.x * MESH_THREADS + threadIdx.x;
		if (v >= V) return;
		float nx = 0.f, ny = 0.f, nz = 0.f;
		for (int i = row_start[v]; i < row_start[v + 1]; i++)
		{
			const int32_t* face = faces + 3 * (size_t)(vals[i] / 3u);
			const size_t a = 3 * (size_t)face[0], b = 3 * (size_t)face[1], c = 3 * (size_t)face[2];
			const float ux = pos[b] - pos[a], uy = pos[b + 1] - pos[a + 1], uz = pos[b + 2] - pos[a + 2];
			const float wx = pos[c] - pos[a], wy = pos[c + 1] - pos[a + 1], wz = pos[c + 2] - pos[a + 2];
			nx = nx + (uy * wz - uz * wy);
			ny = ny + (uz * wx - ux * wz);
			nz = nz + (ux * wy - uy * wx);
		}
		const float len2 = (nx * nx + ny * ny) + nz * nz;
		if (len2 > 0.f)
		{
			const float len = sqrtf(len2);
			nx = nx / len; ny = ny / len; nz = nz / len;
		}
		else nx = ny = nz = 0.f;
		const size_t r = 3 * (size_t)v;
		normals[r] = nx; normals[r + 1] = ny; normals[r + 2] = nz;
	}

	// ---- host side ---- (argument checks of fdgs_mesh_in: mesh_common.h)
	struct ComponentsLayout { size_t parent, counts, flag, total; };
	static ComponentsLayout components_layout(int V)
	{
		ComponentsLayout L;
		ScratchCursor c;
		L.flag = c.take(16);                    // a block of its own at the start: the memset's target
		L.parent = c.take((size_t)V * sizeof(int32_t));
		L.counts = c.take(blocks_of((size_t)V) * sizeof(uint32_t));
		L.total = c.o;
		return L;
	}
	struct CompactLayout { size_t map, vcounts, fcounts, total; };
	static CompactLayout compact_layout(int V, int F)
	{
		CompactLayout L;
		ScratchCursor c;
		L.map = c.take((size_t)V * sizeof(int32_t));
		L.vcounts = c.take(blocks_of((size_t)V) * sizeof(uint32_t));
		L.fcounts = c.take(blocks_of((size_t)F) * sizeof(uint32_t));
		L.total = c.o;
		return L;
	}
	struct SmoothLayout { size_t keys[2], vals[2], hist, row_start, others, tmp, boundary, total; };
	static SmoothLayout smooth_layout(int V, int F)
	{
		SmoothLayout L;
		ScratchCursor c;
		const size_t n = 3 * (size_t)F;
		for (int k = 0; k < 2; k++) L.keys[k] = c.take(n * 4);
		for (int k = 0; k < 2; k++) L.vals[k] = c.take(n * 4);
		L.hist = c.take((size_t)RADIX * (sort_blocks((int)n) + 1) * 4);
		L.row_start = c.take(((size_t)V + 1) * sizeof(int32_t));
		L.others = c.take(n * sizeof(int2));
		L.tmp = c.take(3 * (size_t)V * sizeof(float));
		L.boundary = c.take((size_t)V);
		L.total = c.o;
		return L;
	}
}

using namespace fdgs;

extern "C" size_t fdgs_mesh_components_scratch_bytes(int32_t V, int32_t F)
{
	return mesh_sizes_ok(V, F) ? components_layout(V).total : 0;
}

extern "C" int fdgs_mesh_components(const fdgs_mesh_in* mesh, const fdgs_mesh_components_out* out, void* scratch, void* stream_v)
{
	const char* fn = "fdgs_mesh_components";
	if (const int rc = mesh_in_args(fn, mesh)) return rc;
	if (!out) return fail(FDGS_ERR_INVALID_ARG, "%s: out must not be NULL", fn);
	CHECK_STRUCT_IN(fn, out, fdgs_mesh_components_out);
	if (out->capacity < 0) return fail(FDGS_ERR_INVALID_ARG, "%s: capacity must not be negative", fn);
	if (!out->labelled && !out->n_components) return fail(FDGS_ERR_INVALID_ARG, "%s: n_components must not be NULL", fn);
	const int V = mesh->V, F = mesh->F;
	if (V > 0 && !out->vertex_component) return fail(FDGS_ERR_INVALID_ARG, "%s: vertex_component must not be NULL with V > 0", fn);
	if (V > 0 && !out->labelled && !scratch) return fail(FDGS_ERR_INVALID_ARG, "%s: scratch must not be NULL with V > 0", fn);
	hipStream_t stream = (hipStream_t)stream_v;
	if (out->rounds) *out->rounds = 0;
	const int cap = out->capacity;
	int32_t* cv = cap > 0 ? out->component_vertices : nullptr;
	int32_t* cf = cap > 0 ? out->component_faces : nullptr;
	const int vb = (int)blocks_of((size_t)V), fb = (int)blocks_of((size_t)F);
	if (!out->labelled)
	{
		if (V == 0)
		{
			HIP_TRY(hipMemsetAsync(out->n_components, 0, sizeof(int32_t), stream), "fdgs_mesh_components: memset");
			return FDGS_OK;
		}
		const ComponentsLayout L = components_layout(V);
		char* base = reinterpret_cast<char*>(scratch);
		int32_t* flag = reinterpret_cast<int32_t*>(base + L.flag);
		int32_t* parent = reinterpret_cast<int32_t*>(base + L.parent);
		uint32_t* counts = reinterpret_cast<uint32_t*>(base + L.counts);
		hipLaunchKernelGGL(cc_init_kernel, dim3(vb), dim3(MESH_THREADS), 0, stream, parent, V);
		int rounds = 0;
		for (bool done = F == 0; !done;)
		{
			if (rounds == MESH_MAX_ROUNDS) return fail(FDGS_ERR_HIP, "fdgs_mesh_components: no convergence within 32 hook passes");
			int32_t changed = 0;
			HIP_TRY(hipMemsetAsync(flag, 0, 16, stream), "fdgs_mesh_components: memset");
			hipLaunchKernelGGL(cc_hook_kernel, dim3(fb), dim3(MESH_THREADS), 0, stream, mesh->faces, F, V, parent, flag);
			rounds++;
			HIP_TRY(hipMemcpyAsync(&changed, flag, sizeof changed, hipMemcpyDeviceToHost, stream), "fdgs_mesh_components: reading the convergence flag");
			HIP_TRY(hipStreamSynchronize(stream), "fdgs_mesh_components: reading the convergence flag");
			done = changed == 0;
			if (!done) hipLaunchKernelGGL(cc_compress_kernel, dim3(vb), dim3(MESH_THREADS), 0, stream, parent, V);
		}
		if (out->rounds) *out->rounds = rounds;
		// here every parent[v] is v's root, the smallest index of its component
		compact_enqueue(Compaction<CcRoots>{ { parent, V, out->vertex_component }, counts, out->n_components, 1u, true }, stream);
		hipLaunchKernelGGL(cc_assign_kernel, dim3(vb), dim3(MESH_THREADS), 0, stream, parent, V, out->vertex_component);
	}
	if (cv) HIP_TRY(hipMemsetAsync(cv, 0, (size_t)cap * sizeof(int32_t), stream), "fdgs_mesh_components: memset");
	if (cf) HIP_TRY(hipMemsetAsync(cf, 0, (size_t)cap * sizeof(int32_t), stream), "fdgs_mesh_components: memset");
	if (cv && V > 0) hipLaunchKernelGGL(cc_vertex_count_kernel, dim3(vb), dim3(MESH_THREADS), 0, stream, out->vertex_component, V, cv, cap);
	if (cf && V > 0 && F > 0)
		hipLaunchKernelGGL(cc_face_count_kernel, dim3(fb), dim3(MESH_THREADS), 0, stream, mesh->faces, F, V, out->vertex_component, cf, cap);
	return launched("fdgs_mesh_components");
}

extern "C" size_t fdgs_mesh_compact_scratch_bytes(int32_t V, int32_t F)
{
	return mesh_sizes_ok(V, F) ? compact_layout(V, F).total : 0;
}

extern "C" int fdgs_mesh_compact(const fdgs_mesh_in* mesh, const int32_t* vertex_component, const uint8_t* keep, int32_t n_components,
                                 const fdgs_surface_out* out, void* scratch, void* stream_v)
{
	const char* fn = "fdgs_mesh_compact";
	if (const int rc = mesh_in_args(fn, mesh)) return rc;
	SurfaceOut so;
	if (const int rc = surface_out_args(fn, out, so)) return rc;
	if (n_components < 0) return fail(FDGS_ERR_INVALID_ARG, "%s: n_components must not be negative", fn);
	if (n_components > 0 && !keep) return fail(FDGS_ERR_INVALID_ARG, "%s: keep must not be NULL with n_components > 0", fn);
	const int V = mesh->V, F = mesh->F;
	if (V > 0 && !vertex_component) return fail(FDGS_ERR_INVALID_ARG, "%s: vertex_component must not be NULL with V > 0", fn);
	if ((out->vertices && !mesh->vertices) || (out->normals && !mesh->normals) || (out->colors && !mesh->colors))
		return fail(FDGS_ERR_INVALID_ARG, "%s: an output array needs its input array", fn);
	if (V > 0 && !scratch) return fail(FDGS_ERR_INVALID_ARG, "%s: scratch must not be NULL with V > 0", fn);
	hipStream_t stream = (hipStream_t)stream_v;
	if (V == 0) return surface_out_empty(fn, out, stream);        // no vertex: every face is absent
	const CompactLayout L = compact_layout(V, F);
	char* base = reinterpret_cast<char*>(scratch);
	CompactArgs a;
	a.V = V; a.F = F; a.C = n_components;
	a.vertices = mesh->vertices; a.normals = mesh->normals; a.colors = mesh->colors; a.faces = mesh->faces;
	a.vertex_component = vertex_component; a.keep = keep;
	a.map = reinterpret_cast<int32_t*>(base + L.map);
	a.out_vertices = out->vertices; a.out_normals = out->normals; a.out_colors = out->colors; a.out_faces = out->faces;
	a.vcap = so.vcap; a.fcap = so.fcap;
	// the faces go through the map the vertex emit writes: asked for faces alone, the vertices are emitted too (into no array)
	compact_enqueue(Compaction<CompactVertices>{ { a }, reinterpret_cast<uint32_t*>(base + L.vcounts), out->n_vertices, 1u, so.any_vertex || a.out_faces },
	                Compaction<CompactFaces>{ { a }, reinterpret_cast<uint32_t*>(base + L.fcounts), out->n_faces, 1u, a.out_faces != nullptr }, stream);
	return launched("fdgs_mesh_compact");
}

extern "C" size_t fdgs_mesh_smooth_scratch_bytes(int32_t V, int32_t F)
{
	return mesh_sizes_ok(V, F) ? smooth_layout(V, F).total : 0;
}

extern "C" int fdgs_mesh_smooth(const fdgs_mesh_in* mesh, const fdgs_mesh_smooth_out* out, void* scratch, void* stream_v)
{
	const char* fn = "fdgs_mesh_smooth";
	if (const int rc = mesh_in_args(fn, mesh)) return rc;
	if (!out) return fail(FDGS_ERR_INVALID_ARG, "%s: out must not be NULL", fn);
	CHECK_STRUCT_IN(fn, out, fdgs_mesh_smooth_out);
	if (out->iterations < 0) return fail(FDGS_ERR_INVALID_ARG, "%s: iterations must not be negative", fn);
	if (out->lambda != out->lambda || out->mu != out->mu) return fail(FDGS_ERR_INVALID_ARG, "%s: lambda and mu must not be NaN", fn);
	const int V = mesh->V, F = mesh->F, iterations = out->iterations;
	if (V > 0 && !mesh->vertices) return fail(FDGS_ERR_INVALID_ARG, "%s: the mesh's vertices must not be NULL with V > 0", fn);
	if (V > 0 && iterations > 0 && !out->vertices) return fail(FDGS_ERR_INVALID_ARG, "%s: out vertices must not be NULL with iterations > 0", fn);
	if (V > 0 && !scratch) return fail(FDGS_ERR_INVALID_ARG, "%s: scratch must not be NULL with V > 0", fn);
	if (V == 0) return FDGS_OK;
	hipStream_t stream = (hipStream_t)stream_v;
	const SmoothLayout L = smooth_layout(V, F);
	char* base = reinterpret_cast<char*>(scratch);
	uint32_t* keys[2] = { reinterpret_cast<uint32_t*>(base + L.keys[0]), reinterpret_cast<uint32_t*>(base + L.keys[1]) };
	uint32_t* vals[2] = { reinterpret_cast<uint32_t*>(base + L.vals[0]), reinterpret_cast<uint32_t*>(base + L.vals[1]) };
	int32_t* row_start = reinterpret_cast<int32_t*>(base + L.row_start);
	int2* others = reinterpret_cast<int2*>(base + L.others);
	float* tmp = reinterpret_cast<float*>(base + L.tmp);
	const int n = 3 * F, vb = (int)blocks_of((size_t)V), fb = (int)blocks_of((size_t)F);
	int res = 0;
	if (F > 0)
	{
		int bits = 0;                                        // the keys are 0 .. V
		while (bits < 32 && ((uint32_t)V >> bits) != 0) bits++;
		hipLaunchKernelGGL(smooth_pairs_kernel, dim3(fb), dim3(MESH_THREADS), 0, stream, mesh->faces, F, V, keys[0], vals[0]);
		HIP_TRY(radix_sort_pairs(keys, vals, n, 0, div_up(bits, RADIX_BITS) * RADIX_BITS, reinterpret_cast<uint32_t*>(base + L.hist), stream, &res), "fdgs_mesh_smooth: sort");
	}
	hipLaunchKernelGGL(rows_from_sorted_keys_kernel<MESH_THREADS>, dim3((int)blocks_of((size_t)V + 1)), dim3(MESH_THREADS), 0, stream, keys[res], n, V,
	                   (const int32_t*)nullptr, row_start);
	if (F > 0)
		hipLaunchKernelGGL(smooth_others_kernel, dim3((int)blocks_of((size_t)n)), dim3(MESH_THREADS), 0, stream, mesh->faces, vals[res], row_start, V, n, others);
	uint8_t* boundary = out->boundary ? out->boundary : reinterpret_cast<uint8_t*>(base + L.boundary);
	const bool pin = out->pin_boundary != 0;
	if (out->boundary || (pin && iterations > 0))
		hipLaunchKernelGGL(smooth_boundary_kernel, dim3(vb), dim3(MESH_THREADS), 0, stream, others, row_start, V, boundary);
	const float* pos = mesh->vertices;
	for (int pass = 0; pass < 2 * iterations; pass++)
	{
		float* dst = (pass & 1) ? out->vertices : tmp;       // lambda: -> tmp, mu: -> out
		hipLaunchKernelGGL(smooth_pass_kernel, dim3(vb), dim3(MESH_THREADS), 0, stream, pos, dst, others, row_start, pin ? boundary : nullptr, V,
		                   (pass & 1) ? out->mu : out->lambda);
		pos = dst;
	}
	if (iterations == 0 && out->vertices && out->vertices != mesh->vertices)
		HIP_TRY(hipMemcpyAsync(out->vertices, mesh->vertices, 3 * (size_t)V * sizeof(float), hipMemcpyDeviceToDevice, stream), "fdgs_mesh_smooth: copy");
	if (out->normals)
		hipLaunchKernelGGL(smooth_normals_kernel, dim3(vb), dim3(MESH_THREADS), 0, stream, pos, mesh->faces, vals[res], row_start, V, out->normals);
	return launched("fdgs_mesh_smooth");
}
