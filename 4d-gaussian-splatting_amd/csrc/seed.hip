// seed.hip -- starting a run from a point cloud (include/fdgs_seed.h) for gfx950: voxel-grid thinning in (x, y, z, t), counter-based
// random clouds, and the initial model written straight into the flat bucket.  What the reference does on the host before
// iteration 0: np.random.randint over the cloud (scene/dataset_readers.py:339-355), np.random clouds (:329-331, :357-371) and a dozen
// PyTorch launches (scene/gaussian_model.py:259-300).
//
// Everything is per point and memory-bound; wave64, 256-thread workgroups, no float atomics, every result bit-reproducible.
//   thin     keys       one lane per point: four float32 cell indices -> two 32-bit key words (x y | z t)
//            sort       the library's stable radix sort twice, low word then high word (LSD over the 64-bit key)
//            cells      compact.h over the sorted points: a point whose key differs from its predecessor's heads a cell; the emit pass
//                       has that lane walk the cell's run and sum its members one after the other (float32, compensated).  The stable
//                       sort left them in ascending point index, so the sums are sequential in the original order.
//   random   Philox4x32-10, one counter per point: no state, any point can be drawn on its own
//   init     one lane per four consecutive floats of the bucket, whatever segment they fall into: whole float4 stores
// Built with FP contraction off: floor((v - origin) * inv_cell) and u * extent + lo are two roundings each, as a numpy float32
// restatement computes them.
#pragma clang fp contract(off)
#include "fdgs_common.h"
#include "compact.h"
#include "philox.h"
#include "../../include/fdgs_seed.h"
#include <cmath>

namespace fdgs
{
	constexpr int SEED_THREADS = 256;
	static_assert(SEED_THREADS % WAVE == 0 && SEED_THREADS == COMPACT_THREADS, "256-thread workgroups throughout");

	// ---- thinning ----
	struct SeedThinLayout { size_t klo, khi, key[2], val[2], hist, counts, total; };
	static inline SeedThinLayout seed_thin_layout(int N)
	{
		SeedThinLayout L;
		ScratchCursor c;
		const size_t n = (size_t)(N > 0 ? N : 1);
		L.klo = c.take(n * 4);
		L.khi = c.take(n * 4);
		for (int k = 0; k < 2; k++) L.key[k] = c.take(n * 4);
		for (int k = 0; k < 2; k++) L.val[k] = c.take(n * 4);
		L.hist = c.take((size_t)RADIX * (sort_blocks((int)n) + 1) * 4);
		L.counts = c.take(compact_blocks(n) * 4);
		L.total = c.o;
		return L;
	}

	struct SeedGrid { float origin[4], inv_cell[4]; };

	__device__ __forceinline__ uint32_t seed_cell(const float v, const float origin, const float inv_cell)
	{
		const float f = floorf((v - origin) * inv_cell);
		if (!(f >= 0.f)) return 0u;                                       // below the origin, NaN
		return f >= (float)(FDGS_SEED_AXIS_CELLS - 1) ? (uint32_t)(FDGS_SEED_AXIS_CELLS - 1) : (uint32_t)f;
	}

	__global__ void __launch_bounds__(SEED_THREADS) seed_key_kernel(const int N, const float* __restrict__ xyz, const float* __restrict__ t,
	                                                                const SeedGrid g, uint32_t* __restrict__ klo, uint32_t* __restrict__ khi,
	                                                                uint32_t* __restrict__ key, uint32_t* __restrict__ val)
	{
		const int i = blockIdx.x * SEED_THREADS + threadIdx.x;
		if (i >= N) return;
		const uint32_t ix = seed_cell(xyz[3 * (size_t)i + 0], g.origin[0], g.inv_cell[0]);
		const uint32_t iy = seed_cell(xyz[3 * (size_t)i + 1], g.origin[1], g.inv_cell[1]);
		const uint32_t iz = seed_cell(xyz[3 * (size_t)i + 2], g.origin[2], g.inv_cell[2]);
		const uint32_t it = t != nullptr ? seed_cell(t[i], g.origin[3], g.inv_cell[3]) : 0u;
		const uint32_t lo = (iz << FDGS_SEED_AXIS_BITS) | it, hi = (ix << FDGS_SEED_AXIS_BITS) | iy;
		klo[i] = lo; khi[i] = hi;
		key[i] = lo; val[i] = (uint32_t)i;
	}

	// dst[i] = src[idx[i]] (dst may be the buffer the sort reads next; never src or idx)
	__global__ void __launch_bounds__(SEED_THREADS) seed_gather_kernel(const int N, const uint32_t* __restrict__ src, const uint32_t* __restrict__ idx,
	                                                                   uint32_t* __restrict__ dst)
	{
		const int i = blockIdx.x * SEED_THREADS + threadIdx.x;
		if (i < N) dst[i] = src[idx[i]];
	}

	// compact.h's Pass over the sorted points: one output per cell, written by the lane of the cell's first point
	struct SeedCellPass
	{
		int N, capacity;
		const uint32_t *shi, *slo, *order;          // [N] the sorted keys' two words and the point each position holds
		const float *xyz, *rgb, *t;
		uint64_t* out_key; float *out_xyz, *out_rgb, *out_t; int32_t *out_count, *out_first;
		struct Item {};
		__host__ __device__ int size() const { return N; }
		__device__ uint32_t count(const int i, Item&, const bool) const
		{
			return i == 0 || shi[i] != shi[i - 1] || slo[i] != slo[i - 1] ? 1u : 0u;
		}
		__device__ void emit(const int i, const uint32_t n, const uint32_t rank, const Item&) const
		{
			if (n == 0u || rank >= (uint32_t)capacity) return;
			const uint32_t hi = shi[i], lo = slo[i];
			const uint32_t first = order[i];
			// compensated (Kahan) sums, one member after the other: the error of a sum stays at one rounding of the result however long the run
			float3 p = ld3(xyz, first), pc = make_float3(0.f, 0.f, 0.f);
			float3 c = rgb != nullptr ? ld3(rgb, first) : make_float3(0.f, 0.f, 0.f), cc = make_float3(0.f, 0.f, 0.f);
			float tt = t != nullptr ? t[first] : 0.f, tc = 0.f;
			int j = i + 1;
			for (; j < N && shi[j] == hi && slo[j] == lo; j++)
			{
				const uint32_t o = order[j];
				const float3 q = ld3(xyz, o);
				kahan_add(p.x, pc.x, q.x); kahan_add(p.y, pc.y, q.y); kahan_add(p.z, pc.z, q.z);
				if (rgb != nullptr) { const float3 d = ld3(rgb, o); kahan_add(c.x, cc.x, d.x); kahan_add(c.y, cc.y, d.y); kahan_add(c.z, cc.z, d.z); }
				if (t != nullptr) kahan_add(tt, tc, t[o]);
			}
			const int members = j - i;
			const float m = (float)members;
			out_key[rank] = ((uint64_t)hi << 32) | (uint64_t)lo;
			out_count[rank] = members;
			out_first[rank] = (int32_t)first;
			st3(out_xyz, rank, make_float3(p.x / m, p.y / m, p.z / m));
			if (rgb != nullptr) st3(out_rgb, rank, make_float3(c.x / m, c.y / m, c.z / m));
			if (t != nullptr) out_t[rank] = tt / m;
		}
		// sum += x with the running compensation comp (Kahan 1965); exact operation order, no contraction, no reassociation
		__device__ static void kahan_add(float& sum, float& comp, const float x)
		{
			const float y = x - comp;
			const float next = sum + y;
			comp = (next - sum) - y;
			sum = next;
		}
		__device__ static float3 ld3(const float* a, const size_t k) { return make_float3(a[3 * k], a[3 * k + 1], a[3 * k + 2]); }
		__device__ static void st3(float* a, const size_t k, const float3 v) { a[3 * k] = v.x; a[3 * k + 1] = v.y; a[3 * k + 2] = v.z; }
	};

	// ---- Philox4x32-10 (philox.h) ----
	__device__ __forceinline__ float seed_uniform(const uint32_t w) { return (float)(w >> 8) * 5.9604644775390625e-08f; }   // 2^-24, exact

	struct SeedRandomParams { float p[6]; };

	__global__ void __launch_bounds__(SEED_THREADS) seed_random_kernel(const int N, const uint2 key, const uint32_t stream_id, const int shape,
	                                                                   const SeedRandomParams a, float* __restrict__ out,
	                                                                   uint32_t* __restrict__ words, float* __restrict__ uniforms)
	{
		const int i = blockIdx.x * SEED_THREADS + threadIdx.x;
		if (i >= N) return;
		const uint4 w = philox4x32_10(make_uint4((uint32_t)i, stream_id, 0u, 0u), key);
		const float u0 = seed_uniform(w.x), u1 = seed_uniform(w.y), u2 = seed_uniform(w.z), u3 = seed_uniform(w.w);
		if (words != nullptr) reinterpret_cast<uint4*>(words)[i] = w;
		if (uniforms != nullptr) reinterpret_cast<float4*>(uniforms)[i] = make_float4(u0, u1, u2, u3);
		if (shape == FDGS_SEED_BOX)
		{
			out[3 * (size_t)i + 0] = u0 * a.p[3] + a.p[0];
			out[3 * (size_t)i + 1] = u1 * a.p[4] + a.p[1];
			out[3 * (size_t)i + 2] = u2 * a.p[5] + a.p[2];
		}
		else if (shape == FDGS_SEED_SPHERE)
		{
			const float r = a.p[0];
			float sp, cp;
			sincosf(6.283185307179586f * u0, &sp, &cp);
			const float c = 2.f * u1 - 1.f;
			const float s = sqrtf(fmaxf(1.f - c * c, 0.f));
			out[3 * (size_t)i + 0] = r * s * cp;
			out[3 * (size_t)i + 1] = r * s * sp;
			out[3 * (size_t)i + 2] = r * c;
		}
		else
			out[i] = (u0 * 1.2f - 0.1f) * a.p[1] + a.p[0];
	}

	// ---- the initial model ----
	struct SeedInitArgs
	{
		int P, M, dim4;
		const float *xyz, *rgb, *t, *dist2;
		float opacity_raw, scaling_t_raw;
		float* flat;
	};

	// element e of the flat bucket (include/fdgs_seed.h: xyz | opacity | scaling | rotation | t | scaling_t | rotation_r | features)
	__device__ __forceinline__ float seed_init_value(const SeedInitArgs& a, const uint32_t e)
	{
		const uint32_t P = (uint32_t)a.P;
		if (e < 3u * P) return a.xyz[e];
		if (e < 4u * P) return a.opacity_raw;
		// log(sqrt(x)) as half the float64 logarithm, rounded once: the float32 chain loses the result's low bits to the square root's
		// rounding wherever x is near 1
		if (e < 7u * P) return (float)(0.5 * log((double)fmaxf(a.dist2[(e - 4u * P) / 3u], 1e-7f)));
		if (e < 11u * P) return ((e - 7u * P) & 3u) == 0u ? 1.f : 0.f;
		if (e < 12u * P) return a.dim4 ? a.t[e - 11u * P] : 0.f;
		if (e < 13u * P) return a.dim4 ? a.scaling_t_raw : 0.f;
		if (e < 17u * P) return ((e - 13u * P) & 3u) == 0u ? 1.f : 0.f;
		const uint32_t f = e - 17u * P, row = 3u * (uint32_t)a.M;
		const uint32_t p = f / row, r = f - p * row;
		return r < 3u ? (a.rgb[3u * p + r] - 0.5f) / 0.28209479177387814f : 0.f;
	}

	__global__ void __launch_bounds__(SEED_THREADS) seed_init_kernel(const SeedInitArgs a, const uint32_t total)
	{
		const uint32_t e = 4u * (blockIdx.x * (uint32_t)SEED_THREADS + threadIdx.x);
		if (e >= total) return;
		if (e + 4u <= total && (reinterpret_cast<uintptr_t>(a.flat) & 15) == 0)
			reinterpret_cast<float4*>(a.flat)[e >> 2] = make_float4(seed_init_value(a, e), seed_init_value(a, e + 1u), seed_init_value(a, e + 2u),
			                                                        seed_init_value(a, e + 3u));
		else
			for (uint32_t k = e; k < total && k < e + 4u; k++) a.flat[k] = seed_init_value(a, k);
	}
}

extern "C" size_t fdgs_seed_thin_scratch_bytes(int32_t N) { return fdgs::seed_thin_layout(N).total; }

extern "C" int fdgs_seed_thin(int32_t N, const float* xyz, const float* rgb, const float* t, const float* origin, const float* inv_cell,
                              int32_t count_only, int32_t capacity, uint64_t* out_key, float* out_xyz, float* out_rgb, float* out_t,
                              int32_t* out_count, int32_t* out_first, int32_t* n_cells, void* scratch, void* stream_v)
{
	using namespace fdgs;
	if (N < 0 || N >= (1 << 28)) return fail(FDGS_ERR_INVALID_ARG, "fdgs_seed_thin: N=%d is not in [0, 2^28)", N);
	if (capacity < 0) return fail(FDGS_ERR_INVALID_ARG, "fdgs_seed_thin: capacity=%d is negative", capacity);
	if (!origin || !inv_cell || !n_cells) return fail(FDGS_ERR_INVALID_ARG, "fdgs_seed_thin: origin / inv_cell / n_cells must not be NULL");
	SeedGrid g;
	for (int k = 0; k < 4; k++)
	{
		g.origin[k] = origin[k]; g.inv_cell[k] = inv_cell[k];
		if (!std::isfinite(origin[k])) return fail(FDGS_ERR_INVALID_ARG, "fdgs_seed_thin: origin[%d] is not finite", k);
		if (!(inv_cell[k] > 0.f) || !std::isfinite(inv_cell[k]))
			return fail(FDGS_ERR_INVALID_ARG, "fdgs_seed_thin: inv_cell[%d]=%g is not positive and finite", k, (double)inv_cell[k]);
	}
	hipStream_t stream = (hipStream_t)stream_v;
	if (N == 0)
	{
		HIP_TRY(hipMemsetAsync(n_cells, 0, sizeof(int32_t), stream), "fdgs_seed_thin: hipMemsetAsync");
		return FDGS_OK;
	}
	if (!xyz || !scratch) return fail(FDGS_ERR_INVALID_ARG, "fdgs_seed_thin: xyz / scratch must not be NULL");
	if (!count_only && (!out_key || !out_xyz || !out_count || !out_first || (rgb && !out_rgb) || (t && !out_t)))
		return fail(FDGS_ERR_INVALID_ARG, "fdgs_seed_thin: an output is NULL (out_key / out_xyz / out_count / out_first, out_rgb with rgb, out_t with t)");
	const SeedThinLayout L = seed_thin_layout(N);
	char* s = (char*)scratch;
	uint32_t* klo = (uint32_t*)(s + L.klo);
	uint32_t* khi = (uint32_t*)(s + L.khi);
	uint32_t* key[2] = { (uint32_t*)(s + L.key[0]), (uint32_t*)(s + L.key[1]) };
	uint32_t* val[2] = { (uint32_t*)(s + L.val[0]), (uint32_t*)(s + L.val[1]) };
	uint32_t* hist = (uint32_t*)(s + L.hist);
	const int nb = div_up(N, SEED_THREADS);
	hipLaunchKernelGGL(seed_key_kernel, dim3(nb), dim3(SEED_THREADS), 0, stream, N, xyz, t, g, klo, khi, key[0], val[0]);
	int res = 0;
	HIP_TRY(radix_sort_pairs(key, val, N, 0, 32, hist, stream, &res), "fdgs_seed_thin: radix_sort_pairs");
	// the second, more significant word, in the order the first sort left: the sort takes its input from the first buffer of the pair
	uint32_t* key2[2] = { key[res ^ 1], key[res] };
	uint32_t* val2[2] = { val[res], val[res ^ 1] };
	hipLaunchKernelGGL(seed_gather_kernel, dim3(nb), dim3(SEED_THREADS), 0, stream, N, khi, val2[0], key2[0]);
	HIP_TRY(radix_sort_pairs(key2, val2, N, 0, 32, hist, stream, &res), "fdgs_seed_thin: radix_sort_pairs");
	uint32_t* shi = key2[res];
	uint32_t* order = val2[res];
	uint32_t* slo = key2[res ^ 1];
	hipLaunchKernelGGL(seed_gather_kernel, dim3(nb), dim3(SEED_THREADS), 0, stream, N, klo, order, slo);
	Compaction<SeedCellPass> c;
	c.pass = SeedCellPass{ N, capacity, shi, slo, order, xyz, rgb, t, out_key, out_xyz, out_rgb, out_t, out_count, out_first };
	c.counts = (uint32_t*)(s + L.counts);
	c.total = n_cells;
	c.factor = 1u;
	c.emit = !count_only;
	compact_enqueue(c, stream);
	return launched("fdgs_seed_thin");
}

extern "C" int fdgs_seed_random(int32_t N, uint64_t seed, uint32_t stream_id, int32_t shape, const float* params, float* out, uint32_t* words,
                                float* uniforms, void* stream_v)
{
	using namespace fdgs;
	if (N < 0) return fail(FDGS_ERR_INVALID_ARG, "fdgs_seed_random: N=%d is negative", N);
	if (shape != FDGS_SEED_BOX && shape != FDGS_SEED_SPHERE && shape != FDGS_SEED_TIME)
		return fail(FDGS_ERR_INVALID_ARG, "fdgs_seed_random: unknown shape %d", shape);
	if (!params) return fail(FDGS_ERR_INVALID_ARG, "fdgs_seed_random: params must not be NULL");
	if (N == 0) return FDGS_OK;
	if (!out) return fail(FDGS_ERR_INVALID_ARG, "fdgs_seed_random: out must not be NULL");
	SeedRandomParams a;
	for (int k = 0; k < 6; k++) a.p[k] = params[k];
	const uint2 key = philox_key(seed);
	hipLaunchKernelGGL(seed_random_kernel, dim3(div_up(N, SEED_THREADS)), dim3(SEED_THREADS), 0, (hipStream_t)stream_v, N, key, stream_id, shape, a, out,
	                   words, uniforms);
	return launched("fdgs_seed_random");
}

extern "C" int fdgs_seed_init(int32_t P, int32_t M, int32_t gaussian_dim, const float* xyz, const float* rgb, const float* t, const float* dist2,
                              float opacity_raw, float scaling_t_raw, float* flat, void* stream_v)
{
	using namespace fdgs;
	if (P < 0 || M < 1) return fail(FDGS_ERR_INVALID_ARG, "fdgs_seed_init: bad sizes P=%d M=%d", P, M);
	if (gaussian_dim != 3 && gaussian_dim != 4) return fail(FDGS_ERR_INVALID_ARG, "fdgs_seed_init: gaussian_dim=%d is neither 3 nor 4", gaussian_dim);
	const long long total = (long long)P * (17 + 3 * (long long)M);
	if (total >= (1ll << 31)) return fail(FDGS_ERR_INVALID_ARG, "fdgs_seed_init: P=%d M=%d is a bucket of 2^31 floats or more", P, M);
	if (P == 0) return FDGS_OK;
	if (!xyz || !rgb || !dist2 || !flat) return fail(FDGS_ERR_INVALID_ARG, "fdgs_seed_init: xyz / rgb / dist2 / flat must not be NULL");
	if (gaussian_dim == 4 && !t) return fail(FDGS_ERR_INVALID_ARG, "fdgs_seed_init: t must not be NULL with gaussian_dim == 4");
	const SeedInitArgs a{ P, M, gaussian_dim == 4, xyz, rgb, t, dist2, opacity_raw, scaling_t_raw, flat };
	const long long lanes = (total + 3) / 4;
	hipLaunchKernelGGL(seed_init_kernel, dim3((unsigned)((lanes + SEED_THREADS - 1) / SEED_THREADS)), dim3(SEED_THREADS), 0, (hipStream_t)stream_v, a,
	                   (uint32_t)total);
	return launched("fdgs_seed_init");
}
