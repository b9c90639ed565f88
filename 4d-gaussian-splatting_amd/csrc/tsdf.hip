// tsdf.hip -- a surface from the renderer's depth maps (gfx950): fusion of V views into a truncated signed distance volume
// (fdgs_tsdf_integrate) and surface nets on that volume (fdgs_surface_extract).  Conventions: include/fdgs.h.
//
// Integration.  One thread owns a voxel (x is the fast thread axis: a wave reads and writes 256 contiguous bytes of every array) and
// applies up to TSDF_CHUNK views to it in ascending order with distance, weight, colour and colour weight in registers: the volume is
// read once and written once per chunk, whatever the number of views -- 24 B per voxel each way instead of 24 B per voxel and VIEW.
// What a view contributes are gathers from its depth / alpha / mask / image planes, which neighbouring voxels share.  The views'
// parameters are kernel arguments (wave-uniform: scalar loads), the view matrices are read through their device pointers, uniformly.
// Every update is the same sequence of float32 operations whether it is the first of a chunk or not, and a float32 survives the trip
// through memory unchanged: any chunking is bit-identical to one call per view.  No atomics.  A voxel no view reaches is not written.
//
// Extraction: two passes of compact.h, one lane per voxel each, that share their scan launch.
//   1 cells     (count) a voxel = the cell whose lowest corner it is: active?  -> map[voxel] = 0 / -1, vertices per workgroup
//   2 edges     (count) how many of the voxel's three +x / +y / +z grid edges give a quad (four active cells: the map) -> per workgroup
//   3 scan      exclusive scans of both count arrays (one workgroup each), n_vertices, n_faces = 2 x the quads
//   4 vertices  (emit) rank = workgroup start + rank in the workgroup; map[voxel] = rank; the vertex is computed and stored below the capacity
//   5 faces     (emit) the quads of a voxel's edges, through the map, at 2 * (quad rank)
// A count-only call stops after 3.  Float32 in the operation order of the written statement (built with FP contraction off).
#include "mesh_common.h"
#include <math.h>

namespace fdgs
{
	constexpr int TSDF_THREADS = 256;
	constexpr int TSDF_CHUNK = 16;                       // views per pass over the volume (1232 bytes of kernel arguments: 72 of volume, 1160 of views)
	constexpr int TSDF_MAX_BLOCKS = 256 * 8;             // 256 CUs x 8 workgroups: the rest of the volume is a grid stride away
	constexpr int TSDF_MAX_VOXELS = 1 << 28;             // 3 * voxel + axis and 2 * quads stay int32
	constexpr float TSDF_NEAR = 0.2f;                    // the rasterizer's near plane

	struct TsdfView
	{
		int H, W;
		const float *depth, *alpha, *mask, *image, *vm;
		float alpha_min, fl_x, fl_y, cx, cy, weight;
	};
	struct TsdfViews
	{
		int n;
		TsdfView v[TSDF_CHUNK];
	};
	struct TsdfVol
	{
		int nx, ny, nz, n;
		float ox, oy, oz, s, trunc;
		float *tsdf, *weight, *color, *cweight;
	};

	__global__ void __launch_bounds__(TSDF_THREADS) tsdf_integrate_kernel(const TsdfVol vol, const TsdfViews views)
	{
		const size_t plane = (size_t)vol.n;
		for (int idx = blockIdx.x * TSDF_THREADS + threadIdx.x; idx < vol.n; idx += gridDim.x * TSDF_THREADS)   // n < 2^28, stride <= 2^19
		{
			const int i = idx % vol.nx, jk = idx / vol.nx, j = jk % vol.ny, k = jk / vol.ny;
			const float px = vol.ox + ((float)i + 0.5f) * vol.s;
			const float py = vol.oy + ((float)j + 0.5f) * vol.s;
			const float pz = vol.oz + ((float)k + 0.5f) * vol.s;
			float t = vol.tsdf[idx], wt = vol.weight[idx];
			float c0 = 0.f, c1 = 0.f, c2 = 0.f, cw = 0.f;
			if (vol.color)
			{
				c0 = vol.color[idx]; c1 = vol.color[plane + idx]; c2 = vol.color[2 * plane + idx];
				cw = vol.cweight[idx];
			}
			bool touched = false, ctouched = false;
			for (int n = 0; n < views.n; n++)
			{
				const TsdfView& V = views.v[n];
				const float* m = V.vm;                        // world_view_transform as the rasterizer takes it: view = (p, 1) M
				const float z = ((m[2] * px + m[6] * py) + m[10] * pz) + m[14];
				if (!(z > TSDF_NEAR)) continue;
				const float x = ((m[0] * px + m[4] * py) + m[8] * pz) + m[12];
				const float y = ((m[1] * px + m[5] * py) + m[9] * pz) + m[13];
				const float fu = floorf((V.fl_x * x) / z + V.cx), fv = floorf((V.fl_y * y) / z + V.cy);
				if (!(fu >= 0.f && fu < (float)V.W && fv >= 0.f && fv < (float)V.H)) continue;     // (a NaN fails)
				const int pix = (int)fv * V.W + (int)fu;      // H W < 2^30
				float zp = V.depth[pix];
				if (V.alpha)
				{
					const float a = V.alpha[pix];
					if (!(a >= V.alpha_min)) continue;
					zp = zp / a;
				}
				if (V.mask && !(V.mask[pix] > 0.f)) continue;
				if (!(zp > 0.f && zp < INFINITY)) continue;
				const float sdf = zp - z;
				if (sdf < -vol.trunc) continue;
				const float d = fminf(1.f, sdf / vol.trunc);
				const float w = V.weight;
				const float wn = wt + w;
				t = (wt * t + w * d) / wn;
				wt = wn;
				touched = true;
				if (vol.color && V.image && d < 1.f)
				{
					const size_t hw = (size_t)V.H * V.W;
					const float cn = cw + w;
					c0 = (cw * c0 + w * V.image[pix]) / cn;
					c1 = (cw * c1 + w * V.image[hw + pix]) / cn;
					c2 = (cw * c2 + w * V.image[2 * hw + pix]) / cn;
					cw = cn;
					ctouched = true;
				}
			}
			if (touched) { vol.tsdf[idx] = t; vol.weight[idx] = wt; }
			if (ctouched)
			{
				vol.color[idx] = c0; vol.color[plane + idx] = c1; vol.color[2 * plane + idx] = c2;
				vol.cweight[idx] = cw;
			}
		}
	}

	// ---- surface nets ----
	struct SurfArgs
	{
		int nx, ny, nz, n;
		float ox, oy, oz, s;
		const float *tsdf, *weight, *color;
		float min_weight;
		int32_t* map;                 // [n] per cell (indexed by its lowest corner's voxel): -1 inactive, else 0 and later the vertex index
		int vcap, fcap;
		float *vertices, *normals, *colors;
		int32_t* faces;
	};

	__device__ __forceinline__ bool surf_known(const SurfArgs& a, int v)
	{
		const float w = a.weight[v];
		return w >= a.min_weight && w > 0.f;
	}
	// voxel index of corner m (bit 0: +x, bit 1: +y, bit 2: +z) of the cell whose lowest corner is voxel idx
	__device__ __forceinline__ int surf_corner(const SurfArgs& a, int idx, int m)
	{
		return idx + (m & 1) + ((m >> 1) & 1) * a.nx + (m >> 2) * a.nx * a.ny;
	}

	// what surf_edges finds at a voxel: which edges give a quad, the four cells around each, and whether the voxel itself is inside
	struct SurfQuads
	{
		bool quad[3], inside0;
		int cells[3][4];
	};

	// which of the voxel's three grid edges (towards +x, +y, +z) give a quad; returns how many
	__device__ __forceinline__ uint32_t surf_edges(const SurfArgs& a, int idx, SurfQuads& q)
	{
		q.quad[0] = q.quad[1] = q.quad[2] = false;
		q.inside0 = false;
		const int i = idx % a.nx, jk = idx / a.nx, j = jk % a.ny, k = jk / a.ny;
		const int c[3] = { i, j, k }, d[3] = { a.nx, a.ny, a.nz }, st[3] = { 1, a.nx, a.nx * a.ny };
		if (!surf_known(a, idx)) return 0;
		q.inside0 = a.tsdf[idx] < 0.f;
		uint32_t count = 0;
#pragma unroll
		for (int ax = 0; ax < 3; ax++)
		{
			const int b = (ax + 1) % 3, e = (ax + 2) % 3;
			if (!(c[ax] < d[ax] - 1 && c[b] >= 1 && c[b] <= d[b] - 2 && c[e] >= 1 && c[e] <= d[e] - 2)) continue;
			const int v1 = idx + st[ax];
			if (!surf_known(a, v1) || (a.tsdf[v1] < 0.f) == q.inside0) continue;
			// the four cells around the edge, counter-clockwise seen from +ax (b x e = ax)
			q.cells[ax][0] = a.map[idx - st[b] - st[e]];
			q.cells[ax][1] = a.map[idx - st[e]];
			q.cells[ax][2] = a.map[idx];
			q.cells[ax][3] = a.map[idx - st[b]];
			q.quad[ax] = q.cells[ax][0] >= 0 && q.cells[ax][1] >= 0 && q.cells[ax][2] >= 0 && q.cells[ax][3] >= 0;
			count += q.quad[ax] ? 1u : 0u;
		}
		return count;
	}

	// the cells that carry a vertex.  The count pass decides it and leaves map[voxel] = 0 / -1 (the edges pass reads that); the emit
	// pass reads the decision back from the map and replaces it by the vertex index.
	struct SurfVertices
	{
		SurfArgs a;
		struct Item {};
		__host__ __device__ int size() const { return a.n; }
		__device__ uint32_t count(int idx, Item&, bool emitting) const
		{
			if (emitting) return a.map[idx] >= 0 ? 1u : 0u;
			bool active = false;
			const int i = idx % a.nx, jk = idx / a.nx, j = jk % a.ny, k = jk / a.ny;
			if (i < a.nx - 1 && j < a.ny - 1 && k < a.nz - 1)
			{
				bool all = true;
				int inside = 0;
#pragma unroll
				for (int m = 0; m < 8; m++)
				{
					const int v = surf_corner(a, idx, m);
					all = all && surf_known(a, v);
					inside += a.tsdf[v] < 0.f ? 1 : 0;
				}
				active = all && inside > 0 && inside < 8;
			}
			a.map[idx] = active ? 0 : -1;
			return active ? 1u : 0u;
		}
		__device__ void emit(int idx, uint32_t active, uint32_t rank, const Item&) const
		{
			if (!active) return;
			a.map[idx] = (int32_t)rank;
			if (rank >= (uint32_t)a.vcap) return;
			float tv[8];
#pragma unroll
			for (int m = 0; m < 8; m++) tv[m] = a.tsdf[surf_corner(a, idx, m)];
			// the 12 edges, axis by axis: corner m0 (without the axis bit) to m0 | axis bit
			float sx = 0.f, sy = 0.f, sz = 0.f, cr = 0.f, cg = 0.f, cb = 0.f;
			int crossings = 0;
			const size_t plane = (size_t)a.n;
#pragma unroll
			for (int ax = 0; ax < 3; ax++)
			{
#pragma unroll
				for (int q = 0; q < 4; q++)
				{
					const int lo = q & 1, hi = q >> 1;                 // the two other bits, in ascending bit order
					const int m0 = ax == 0 ? (lo << 1) | (hi << 2) : (ax == 1 ? lo | (hi << 2) : lo | (hi << 1));
					const int m1 = m0 | (1 << ax);
					const float fa = tv[m0], fb = tv[m1];
					if ((fa < 0.f) == (fb < 0.f)) continue;
					const float t = fa / (fa - fb);
					sx += ax == 0 ? t : (float)(m0 & 1);
					sy += ax == 1 ? t : (float)((m0 >> 1) & 1);
					sz += ax == 2 ? t : (float)(m0 >> 2);
					crossings++;
					if (a.colors && a.color)
					{
						const int v0 = surf_corner(a, idx, m0), v1 = surf_corner(a, idx, m1);
						const float r0 = a.color[v0], g0 = a.color[plane + v0], b0 = a.color[2 * plane + v0];
						const float r1 = a.color[v1], g1 = a.color[plane + v1], b1 = a.color[2 * plane + v1];
						cr += r0 + t * (r1 - r0);
						cg += g0 + t * (g1 - g0);
						cb += b0 + t * (b1 - b0);
					}
				}
			}
			const float nf = (float)crossings;                        // >= 3 in an active cell
			const int i = idx % a.nx, jk = idx / a.nx, j = jk % a.ny, k = jk / a.ny;
			const size_t r = (size_t)rank;
			if (a.vertices)
			{
				a.vertices[3 * r + 0] = a.ox + (((float)i + 0.5f) + sx / nf) * a.s;
				a.vertices[3 * r + 1] = a.oy + (((float)j + 0.5f) + sy / nf) * a.s;
				a.vertices[3 * r + 2] = a.oz + (((float)k + 0.5f) + sz / nf) * a.s;
			}
			if (a.colors)
			{
				a.colors[3 * r + 0] = cr / nf; a.colors[3 * r + 1] = cg / nf; a.colors[3 * r + 2] = cb / nf;
			}
			if (a.normals)
			{
				// the trilinear gradient at the cell centre: the mean of the four corner differences per axis
				const float gx = (((tv[1] - tv[0]) + (tv[3] - tv[2])) + ((tv[5] - tv[4]) + (tv[7] - tv[6]))) * 0.25f;
				const float gy = (((tv[2] - tv[0]) + (tv[3] - tv[1])) + ((tv[6] - tv[4]) + (tv[7] - tv[5]))) * 0.25f;
				const float gz = (((tv[4] - tv[0]) + (tv[5] - tv[1])) + ((tv[6] - tv[2]) + (tv[7] - tv[3]))) * 0.25f;
				const float len2 = (gx * gx + gy * gy) + gz * gz;
				float nx = 0.f, ny = 0.f, nz = 0.f;
				if (len2 > 1e-20f)
				{
					const float len = sqrtf(len2);
					nx = gx / len; ny = gy / len; nz = gz / len;
				}
				a.normals[3 * r + 0] = nx; a.normals[3 * r + 1] = ny; a.normals[3 * r + 2] = nz;
			}
		}
	};

	// the quads of a voxel's three edges, two triangles each
	struct SurfFaces
	{
		SurfArgs a;
		typedef SurfQuads Item;
		__host__ __device__ int size() const { return a.n; }
		__device__ uint32_t count(int idx, Item& q, bool) const { return surf_edges(a, idx, q); }
		__device__ void emit(int, uint32_t, uint32_t rank, const Item& q) const
		{
#pragma unroll
			for (int ax = 0; ax < 3; ax++)
			{
				if (!q.quad[ax]) continue;
				// counter-clockwise seen from +ax: the normal points to +ax, right where this end is the inside one
				const int q0 = q.cells[ax][0], q1 = q.inside0 ? q.cells[ax][1] : q.cells[ax][3], q2 = q.cells[ax][2], q3 = q.inside0 ? q.cells[ax][3] : q.cells[ax][1];
				const size_t f = 2 * (size_t)rank;
				if (f < (size_t)a.fcap) { a.faces[3 * f + 0] = q0; a.faces[3 * f + 1] = q1; a.faces[3 * f + 2] = q2; }
				if (f + 1 < (size_t)a.fcap) { a.faces[3 * f + 3] = q0; a.faces[3 * f + 4] = q2; a.faces[3 * f + 5] = q3; }
				rank++;
			}
		}
	};

	// scratch of fdgs_surface_extract for n voxels: the cells' vertex indices and the per-block vertex / face counts
	struct SurfaceLayout { size_t map, vcounts, fcounts, total; };
	static SurfaceLayout surface_layout(size_t n)
	{
		SurfaceLayout L;
		ScratchCursor c;
		const size_t nb = compact_blocks(n);
		L.map = c.take(n * sizeof(int32_t));
		L.vcounts = c.take(nb * sizeof(uint32_t));
		L.fcounts = c.take(nb * sizeof(uint32_t));
		L.total = c.o;
		return L;
	}
	static bool positive_f(float v) { return v > 0.f && v < INFINITY; }

	// FDGS_OK: the volume is fine and `v` is filled in; otherwise the entry point `fn` fails with what is wrong with it
	static int tsdf_volume_args(const char* fn, const fdgs_tsdf_volume* in, TsdfVol& v)
	{
		if (!in) return fail(FDGS_ERR_INVALID_ARG, "%s: volume must not be NULL", fn);
		CHECK_STRUCT_IN(fn, in, fdgs_tsdf_volume);
		if (in->nx < 0 || in->ny < 0 || in->nz < 0) return fail(FDGS_ERR_INVALID_ARG, "%s: nx, ny, nz must not be negative", fn);
		if ((int64_t)in->nx * in->ny >= TSDF_MAX_VOXELS || (int64_t)in->nx * in->ny * in->nz >= TSDF_MAX_VOXELS) return fail(FDGS_ERR_INVALID_ARG, "%s: need nx * ny * nz < 2^28", fn);
		if (!in->tsdf || !in->weight) return fail(FDGS_ERR_INVALID_ARG, "%s: tsdf and weight must not be NULL", fn);
		if (!positive_f(in->voxel_size)) return fail(FDGS_ERR_INVALID_ARG, "%s: voxel_size (s) must be positive and finite", fn);
		if (!positive_f(in->trunc)) return fail(FDGS_ERR_INVALID_ARG, "%s: trunc must be positive and finite", fn);
		if (!finite_f(in->origin[0]) || !finite_f(in->origin[1]) || !finite_f(in->origin[2])) return fail(FDGS_ERR_INVALID_ARG, "%s: origin must be finite", fn);
		if ((in->color != nullptr) != (in->cweight != nullptr)) return fail(FDGS_ERR_INVALID_ARG, "%s: color and cweight must be given together", fn);
		v.nx = in->nx; v.ny = in->ny; v.nz = in->nz; v.n = in->nx * in->ny * in->nz;
		v.ox = in->origin[0]; v.oy = in->origin[1]; v.oz = in->origin[2]; v.s = in->voxel_size; v.trunc = in->trunc;
		v.tsdf = in->tsdf; v.weight = in->weight; v.color = in->color; v.cweight = in->cweight;
		return FDGS_OK;
	}

	static int tsdf_view_args(const char* fn, const fdgs_tsdf_view& in, TsdfView& v)
	{
		CHECK_STRUCT_IN(fn, &in, fdgs_tsdf_view);
		if (in.H <= 0 || in.W <= 0 || (int64_t)in.H * in.W >= ((int64_t)1 << 30)) return fail(FDGS_ERR_INVALID_ARG, "%s: a view needs H, W > 0 and H * W < 2^30", fn);
		if (!in.depth || !in.viewmatrix) return fail(FDGS_ERR_INVALID_ARG, "%s: a view's depth and viewmatrix must not be NULL", fn);
		if (in.alpha && !positive_f(in.alpha_min)) return fail(FDGS_ERR_INVALID_ARG, "%s: alpha_min must be positive and finite (zp = depth / alpha)", fn);
		if (!positive_f(in.fl_x) || !positive_f(in.fl_y)) return fail(FDGS_ERR_INVALID_ARG, "%s: fl_x and fl_y must be positive and finite", fn);
		if (!finite_f(in.cx) || !finite_f(in.cy)) return fail(FDGS_ERR_INVALID_ARG, "%s: cx and cy must be finite", fn);
		if (!positive_f(in.view_weight)) return fail(FDGS_ERR_INVALID_ARG, "%s: view_weight must be positive and finite", fn);
		v.H = in.H; v.W = in.W; v.depth = in.depth; v.alpha = in.alpha; v.mask = in.mask; v.image = in.image; v.vm = in.viewmatrix;
		v.alpha_min = in.alpha_min; v.fl_x = in.fl_x; v.fl_y = in.fl_y; v.cx = in.cx; v.cy = in.cy; v.weight = in.view_weight;
		return FDGS_OK;
	}
}

using namespace fdgs;

extern "C" int fdgs_tsdf_integrate(const fdgs_tsdf_volume* volume, int32_t num_views, const fdgs_tsdf_view* views, void* stream)
{
	TsdfVol vol;
	if (const int rc = tsdf_volume_args("fdgs_tsdf_integrate", volume, vol)) return rc;
	if (num_views < 0 || (num_views > 0 && !views)) return fail(FDGS_ERR_INVALID_ARG, "fdgs_tsdf_integrate: num_views must not be negative, views not NULL");
	TsdfView probe;
	for (int n = 0; n < num_views; n++)
		if (const int rc = tsdf_view_args("fdgs_tsdf_integrate", views[n], probe)) return rc;
	if (vol.n == 0 || num_views == 0) return FDGS_OK;
	const int blocks = div_up(vol.n, TSDF_THREADS);
	const dim3 grid(blocks < TSDF_MAX_BLOCKS ? blocks : TSDF_MAX_BLOCKS);
	for (int first = 0; first < num_views; first += TSDF_CHUNK)
	{
		TsdfViews chunk;
		chunk.n = num_views - first < TSDF_CHUNK ? num_views - first : TSDF_CHUNK;
		for (int n = 0; n < TSDF_CHUNK; n++) (void)tsdf_view_args("fdgs_tsdf_integrate", views[first + (n < chunk.n ? n : 0)], chunk.v[n]);   // (checked above; unused slots: a valid view)
		hipLaunchKernelGGL(tsdf_integrate_kernel, grid, dim3(TSDF_THREADS), 0, (hipStream_t)stream, vol, chunk);
	}
	return launched("fdgs_tsdf_integrate");
}

extern "C" size_t fdgs_surface_extract_scratch_bytes(int32_t nx, int32_t ny, int32_t nz)
{
	if (nx < 2 || ny < 2 || nz < 2 || (int64_t)nx * ny >= TSDF_MAX_VOXELS || (int64_t)nx * ny * nz >= TSDF_MAX_VOXELS) return 0;
	return surface_layout((size_t)nx * ny * nz).total;
}

extern "C" int fdgs_surface_extract(const fdgs_tsdf_volume* volume, float min_weight, const fdgs_surface_out* out, void* scratch, void* stream_v)
{
	TsdfVol vol;
	if (const int rc = tsdf_volume_args("fdgs_surface_extract", volume, vol)) return rc;
	SurfaceOut so;
	if (const int rc = surface_out_args("fdgs_surface_extract", out, so)) return rc;
	if (min_weight != min_weight) return fail(FDGS_ERR_INVALID_ARG, "fdgs_surface_extract: min_weight must not be NaN");
	hipStream_t stream = (hipStream_t)stream_v;
	if (vol.nx < 2 || vol.ny < 2 || vol.nz < 2) return surface_out_empty("fdgs_surface_extract", out, stream);   // no cell: nothing is launched that indexes the volume
	if (!scratch) return fail(FDGS_ERR_INVALID_ARG, "fdgs_surface_extract: scratch must not be NULL");
	SurfArgs a;
	a.nx = vol.nx; a.ny = vol.ny; a.nz = vol.nz; a.n = vol.n;
	a.ox = vol.ox; a.oy = vol.oy; a.oz = vol.oz; a.s = vol.s;
	a.tsdf = vol.tsdf; a.weight = vol.weight; a.color = vol.color;
	a.min_weight = min_weight;
	const SurfaceLayout L = surface_layout((size_t)vol.n);
	char* base = reinterpret_cast<char*>(scratch);
	a.map = reinterpret_cast<int32_t*>(base + L.map);
	a.vertices = out->vertices; a.normals = out->normals; a.colors = out->colors; a.faces = out->faces;
	a.vcap = so.vcap; a.fcap = so.fcap;
	// the faces go through the map the vertex emit writes: asked for faces alone, the vertices are emitted too (into no array)
	compact_enqueue(Compaction<SurfVertices>{ { a }, reinterpret_cast<uint32_t*>(base + L.vcounts), out->n_vertices, 1u, so.any_vertex || a.faces },
	                Compaction<SurfFaces>{ { a }, reinterpret_cast<uint32_t*>(base + L.fcounts), out->n_faces, 2u, a.faces != nullptr }, stream);
	return launched("fdgs_surface_extract");
}
