// knn.hip -- distCUDA2: mean squared distance to the three nearest neighbours (gfx950).
//
// SURVEY.md section 8f rank 4, second half: the only other native code the reference runs by default, once at
// initialisation, to size the initial Gaussians (scene/gaussian_model.py:274; simple-knn/simple_knn.cu).
// Same plan as the reference -- Morton order, boxes of 1024 consecutive points, exact search with box pruning --
// re-cut for wave64 / LDS:
//   * bounds and Morton codes stay on the device (the reference copies min / max to the host: two syncs);
//   * the (code, index) pairs go through this library's own radix sort (radix_sort.hip);
//   * the search runs one workgroup per 256 consecutive (Morton-sorted, hence spatially close) queries; a candidate
//     box that ANY of them still needs is staged once into LDS and scanned from there by the lanes that need it,
//     instead of every thread gathering every candidate point from global memory (simple_knn.cu:176-188).
// The result does not depend on the search order; the arithmetic that defines it is kept literally and the TU is
// compiled with FP contraction off:  d = (dx*dx + dy*dy) + dz*dz ;  mean = ((b0 + b1) + b2) / 3  -> bit-exact vs the oracle.
#include "fdgs_common.h"
#include <cfloat>

namespace fdgs
{
	constexpr int KNN_BOX = 1024;       // simple_knn.cu:12
	constexpr int KNN_THREADS = 256;

	struct KnnLayout { size_t code[2], idx[2], hist, boxes, bounds, total; };
	static inline KnnLayout knn_layout(int P)
	{
		KnnLayout L;
		ScratchCursor c;
		const size_t p = (size_t)(P > 0 ? P : 1);
		for (int i = 0; i < 2; i++) L.code[i] = c.take(p * 4);
		for (int i = 0; i < 2; i++) L.idx[i] = c.take(p * 4);
		L.hist = c.take((size_t)RADIX * (sort_blocks((int)p) + 1) * 4);
		L.boxes = c.take((size_t)div_up((int)p, KNN_BOX) * 6 * 4);
		L.bounds = c.take(6 * 4);
		L.total = c.o;
		return L;
	}

	// min / max over all points AND the origin (cub::DeviceReduce with init {0,0,0}, simple_knn.cu:198-205)
	// (the query search: over the sources and the queries, so that every query's Morton code is in range too)
	__global__ void __launch_bounds__(1024) knn_bounds_kernel(int P, const float* __restrict__ pts, int P2, const float* __restrict__ pts2,
	                                                          float* __restrict__ bounds)
	{
		__shared__ float red[6][1024 / WAVE];
		float mn[3] = { 0.f, 0.f, 0.f }, mx[3] = { 0.f, 0.f, 0.f };
		for (int i = threadIdx.x; i < P; i += 1024)
			for (int k = 0; k < 3; k++) { const float v = pts[3 * (size_t)i + k]; mn[k] = fminf(mn[k], v); mx[k] = fmaxf(mx[k], v); }
		for (int i = threadIdx.x; i < P2; i += 1024)
			for (int k = 0; k < 3; k++) { const float v = pts2[3 * (size_t)i + k]; mn[k] = fminf(mn[k], v); mx[k] = fmaxf(mx[k], v); }
		for (int k = 0; k < 3; k++)
			for (int o = 32; o > 0; o >>= 1) { mn[k] = fminf(mn[k], __shfl_xor(mn[k], o)); mx[k] = fmaxf(mx[k], __shfl_xor(mx[k], o)); }
		const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
		if (lane == 0) for (int k = 0; k < 3; k++) { red[k][wave] = mn[k]; red[3 + k][wave] = mx[k]; }
		__syncthreads();
		if (threadIdx.x < 6)
		{
			float v = red[threadIdx.x][0];
			for (int w = 1; w < 1024 / WAVE; w++) v = threadIdx.x < 3 ? fminf(v, red[threadIdx.x][w]) : fmaxf(v, red[threadIdx.x][w]);
			bounds[threadIdx.x] = v;
		}
	}

	__device__ __forceinline__ uint32_t prep_morton(uint32_t x)   // simple_knn.cu:45-52
	{
		x = (x | (x << 16)) & 0x030000FF;
		x = (x | (x << 8)) & 0x0300F00F;
		x = (x | (x << 4)) & 0x030C30C3;
		x = (x | (x << 2)) & 0x09249249;
		return x;
	}

	__global__ void __launch_bounds__(256) knn_morton_kernel(int P, const float* __restrict__ pts, const float* __restrict__ bounds,
	                                                         uint32_t* __restrict__ codes, uint32_t* __restrict__ idx)
	{
		const int i = blockIdx.x * blockDim.x + threadIdx.x;
		if (i >= P) return;
		uint32_t c[3];
		for (int k = 0; k < 3; k++)   // simple_knn.cu:54-61; an axis of zero extent (every point on the origin's plane) gets code 0
		{
			const float ext = bounds[3 + k] - bounds[k];
			c[k] = ext > 0.f ? prep_morton((uint32_t)(((pts[3 * (size_t)i + k] - bounds[k]) / ext) * ((1 << 10) - 1))) : 0u;
		}
		codes[i] = c[0] | (c[1] << 1) | (c[2] << 2);
		idx[i] = (uint32_t)i;
	}

	// one workgroup per box of BOX Morton-consecutive points (simple_knn.cu:77-122)
	template <int BOX>
	__global__ void __launch_bounds__(KNN_THREADS) knn_box_bounds_kernel(int P, const float* __restrict__ pts, const uint32_t* __restrict__ order,
	                                                                     float* __restrict__ boxes)
	{
		__shared__ float red[6][KNN_THREADS / WAVE];
		float mn[3] = { FLT_MAX, FLT_MAX, FLT_MAX }, mx[3] = { -FLT_MAX, -FLT_MAX, -FLT_MAX };
		for (int j = threadIdx.x; j < BOX; j += KNN_THREADS)
		{
			const int i = blockIdx.x * BOX + j;
			if (i < P)
				for (int k = 0; k < 3; k++) { const float v = pts[3 * (size_t)order[i] + k]; mn[k] = fminf(mn[k], v); mx[k] = fmaxf(mx[k], v); }
		}
		for (int k = 0; k < 3; k++)
			for (int o = 32; o > 0; o >>= 1) { mn[k] = fminf(mn[k], __shfl_xor(mn[k], o)); mx[k] = fmaxf(mx[k], __shfl_xor(mx[k], o)); }
		const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
		if (lane == 0) for (int k = 0; k < 3; k++) { red[k][wave] = mn[k]; red[3 + k][wave] = mx[k]; }
		__syncthreads();
		if (threadIdx.x < 6)
		{
			float v = red[threadIdx.x][0];
			for (int w = 1; w < KNN_THREADS / WAVE; w++) v = threadIdx.x < 3 ? fminf(v, red[threadIdx.x][w]) : fmaxf(v, red[threadIdx.x][w]);
			boxes[6 * (size_t)blockIdx.x + threadIdx.x] = v;
		}
	}

	__device__ __forceinline__ void update_k_best(float px, float py, float pz, float qx, float qy, float qz, float* knn)
	{
		// simple_knn.cu:131-145, K = 3
		const float dx = qx - px, dy = qy - py, dz = qz - pz;
		float dist = (dx * dx + dy * dy) + dz * dz;
#pragma unroll
		for (int j = 0; j < 3; j++)
			if (knn[j] > dist) { const float t = knn[j]; knn[j] = dist; dist = t; }
	}

	__device__ __forceinline__ float dist_box_point(const float* box, float px, float py, float pz)
	{
		// simple_knn.cu:124-134
		float dx = 0.f, dy = 0.f, dz = 0.f;
		if (px < box[0] || px > box[3]) dx = fminf(fabsf(px - box[0]), fabsf(px - box[3]));
		if (py < box[1] || py > box[4]) dy = fminf(fabsf(py - box[1]), fabsf(py - box[4]));
		if (pz < box[2] || pz > box[5]) dz = fminf(fabsf(pz - box[2]), fabsf(pz - box[5]));
		return dx * dx + dy * dy + dz * dz;
	}

	__global__ void __launch_bounds__(KNN_THREADS) knn_mean_dist_kernel(int P, const float* __restrict__ pts, const uint32_t* __restrict__ order,
	                                                                    const float* __restrict__ boxes, float* __restrict__ dists)
	{
		__shared__ float sx[KNN_BOX], sy[KNN_BOX], sz[KNN_BOX];
		__shared__ int s_need;
		const int idx = blockIdx.x * KNN_THREADS + threadIdx.x;
		const bool valid = idx < P;
		float px = 0.f, py = 0.f, pz = 0.f;
		uint32_t me = 0;
		if (valid) { me = order[idx]; px = pts[3 * (size_t)me]; py = pts[3 * (size_t)me + 1]; pz = pts[3 * (size_t)me + 2]; }
		float best[3] = { FLT_MAX, FLT_MAX, FLT_MAX };
		if (valid)
			for (int i = max(0, idx - 3); i <= min(P - 1, idx + 3); i++)   // simple_knn.cu:164-169
			{
				if (i == idx) continue;
				const uint32_t o = order[i];
				update_k_best(px, py, pz, pts[3 * (size_t)o], pts[3 * (size_t)o + 1], pts[3 * (size_t)o + 2], best);
			}
		const float reject = best[2];
		best[0] = FLT_MAX; best[1] = FLT_MAX; best[2] = FLT_MAX;

		const int nboxes = (P + KNN_BOX - 1) / KNN_BOX;
		for (int b = 0; b < nboxes; b++)
		{
			bool need = false;
			if (valid)
			{
				const float d = dist_box_point(boxes + 6 * (size_t)b, px, py, pz);
				need = !(d > reject || d > best[2]);                        // simple_knn.cu:178-180
			}
			if (threadIdx.x == 0) s_need = 0;
			__syncthreads();
			if (need) s_need = 1;
			__syncthreads();
			if (s_need == 0) continue;                                       // nobody in this workgroup needs the box
			const int first = b * KNN_BOX, cnt = min(KNN_BOX, P - first);
			for (int j = threadIdx.x; j < cnt; j += KNN_THREADS)
			{
				const uint32_t o = order[first + j];
				sx[j] = pts[3 * (size_t)o]; sy[j] = pts[3 * (size_t)o + 1]; sz[j] = pts[3 * (size_t)o + 2];
			}
			__syncthreads();
			if (need)
				for (int j = 0; j < cnt; j++)
				{
					if (first + j == idx) continue;                          // :185
					update_k_best(px, py, pz, sx[j], sy[j], sz[j], best);
				}
			__syncthreads();
		}
		if (valid) dists[me] = ((best[0] + best[1]) + best[2]) / 3.0f;       // :191
	}
}

extern "C" size_t fdgs_knn_scratch_bytes(int32_t P) { return fdgs::knn_layout(P).total; }

extern "C" int fdgs_dist2_knn3(int32_t P, const float* points, float* mean_dist2, void* scratch, void* stream_v)
{
	using namespace fdgs;
	if (P < 0) return fail(FDGS_ERR_INVALID_ARG, "fdgs_dist2_knn3: P=%d is negative", P);
	if (P == 0) return FDGS_OK;
	if (!points || !mean_dist2 || !scratch) return fail(FDGS_ERR_INVALID_ARG, "fdgs_dist2_knn3: points / mean_dist2 / scratch must not be NULL");
	hipStream_t stream = (hipStream_t)stream_v;
	const KnnLayout L = knn_layout(P);
	char* s = (char*)scratch;
	uint32_t* codes[2] = { (uint32_t*)(s + L.code[0]), (uint32_t*)(s + L.code[1]) };
	uint32_t* idx[2] = { (uint32_t*)(s + L.idx[0]), (uint32_t*)(s + L.idx[1]) };
	float* bounds = (float*)(s + L.bounds);
	float* boxes = (float*)(s + L.boxes);
	hipLaunchKernelGGL(knn_bounds_kernel, dim3(1), dim3(1024), 0, stream, P, points, 0, nullptr, bounds);
	hipLaunchKernelGGL(knn_morton_kernel, dim3(div_up(P, 256)), dim3(256), 0, stream, P, points, bounds, codes[0], idx[0]);
	int res = 0;
	HIP_TRY(radix_sort_pairs(codes, idx, P, 0, 32, (uint32_t*)(s + L.hist), stream, &res), "fdgs_dist2_knn3: radix_sort_pairs");
	const int nboxes = div_up(P, KNN_BOX);
	hipLaunchKernelGGL(knn_box_bounds_kernel<KNN_BOX>, dim3(nboxes), dim3(KNN_THREADS), 0, stream, P, points, idx[res], boxes);
	hipLaunchKernelGGL(knn_mean_dist_kernel, dim3(div_up(P, KNN_THREADS)), dim3(KNN_THREADS), 0, stream, P, points, idx[res], boxes, mean_dist2);
	return launched("fdgs_dist2_knn3");
}

// ---- k-nearest-neighbour query: drop-in for pointops2's knnquery (utils/general_utils.py:170-184) ----------------------
// Exact k nearest sources of every query, rows sorted by (d2, source index): d2 = (dx*dx + dy*dy) + dz*dz in fp32 (this TU is
// built with FP contraction off).  Same plan as distCUDA2 above, re-tuned for k ~ 20:
//   * sources and queries are Morton-sorted with one set of bounds (over both); the sources are cut into boxes of 256;
//   * every query seeds its list, and with it a reject bound, from the 2k sources around its own Morton position;
//   * one workgroup per 256 consecutive sorted queries first marks, in an LDS bitmask, every box that any of its queries
//     cannot reject, then walks the marked boxes in order, staging each once into LDS; a lane scans a staged box only if the box
//     can still hold a better point than its current k-th;
//   * the k best live in VGPRs as a sorted list of (d2, index), KC >= k entries of which the first KC - k are pads below any
//     distance, so that the worst entry is always the last one (static register indices only).
// Differences from the reference: its heap breaks exact ties in an order that depends on the scan; here the lower source index
// wins.  Like the reference's initial heap, a slot no source fills holds d2 = 1e10, index 0, and a source at d2 >= 1e10 is never
// taken.
namespace fdgs
{
	constexpr int KNNQ_BOX = 256;
	constexpr int KNNQ_MASK_WORDS = 2048;             // LDS bitmask of boxes: at most 65536 boxes = 16.7 M sources per batch
	constexpr float KNNQ_EMPTY = 1e10f;               // knnquery_cuda_kernel.cu's initial heap distance

	struct KnnQueryLayout { size_t scode[2], sidx[2], qcode[2], qidx[2], hist, boxes, bounds, total; };
	static inline KnnQueryLayout knn_query_layout(int n, int m)
	{
		KnnQueryLayout L;
		ScratchCursor c;
		const size_t pn = (size_t)(n > 0 ? n : 1), pm = (size_t)(m > 0 ? m : 1);
		for (int i = 0; i < 2; i++) L.scode[i] = c.take(pm * 4);
		for (int i = 0; i < 2; i++) L.sidx[i] = c.take(pm * 4);
		for (int i = 0; i < 2; i++) L.qcode[i] = c.take(pn * 4);
		for (int i = 0; i < 2; i++) L.qidx[i] = c.take(pn * 4);
		L.hist = c.take((size_t)RADIX * (sort_blocks((int)(pn > pm ? pn : pm)) + 1) * 4);
		L.boxes = c.take((size_t)div_up((int)pm, KNNQ_BOX) * 6 * 4);
		L.bounds = c.take(6 * 4);
		L.total = c.o;
		return L;
	}

	__device__ __forceinline__ bool knn_less(float d, uint32_t i, float bd, uint32_t bi) { return d < bd || (d == bd && i < bi); }

	template <int KC>
	__device__ __forceinline__ void knn_insert(float (&bd)[KC], uint32_t (&bi)[KC], float d, uint32_t i)
	{
		if (!knn_less(d, i, bd[KC - 1], bi[KC - 1])) return;
		bd[KC - 1] = d; bi[KC - 1] = i;
#pragma unroll
		for (int j = KC - 1; j > 0; j--)
			if (knn_less(bd[j], bi[j], bd[j - 1], bi[j - 1]))
			{
				const float td = bd[j]; bd[j] = bd[j - 1]; bd[j - 1] = td;
				const uint32_t ti = bi[j]; bi[j] = bi[j - 1]; bi[j - 1] = ti;
			}
	}

	template <int KC>
	__device__ __forceinline__ void knn_reset(float (&bd)[KC], uint32_t (&bi)[KC], int k)
	{
#pragma unroll
		for (int j = 0; j < KC; j++) { bd[j] = j < KC - k ? -1.f : KNNQ_EMPTY; bi[j] = 0; }
	}

	__device__ __forceinline__ float knn_d2(float px, float py, float pz, float qx, float qy, float qz)
	{
		const float dx = qx - px, dy = qy - py, dz = qz - pz;
		return (dx * dx + dy * dy) + dz * dz;
	}

	template <int KC>
	__global__ void __launch_bounds__(KNN_THREADS) knn_query_kernel(int n, int m, int k, const float* __restrict__ x, const float* __restrict__ src,
	                                                                const uint32_t* __restrict__ qorder, const uint32_t* __restrict__ qcodes,
	                                                                const uint32_t* __restrict__ sorder, const uint32_t* __restrict__ scodes,
	                                                                const float* __restrict__ boxes, int64_t* __restrict__ out_idx,
	                                                                float* __restrict__ out_d2)
	{
		__shared__ float sx[KNNQ_BOX], sy[KNNQ_BOX], sz[KNNQ_BOX];
		__shared__ uint32_t si[KNNQ_BOX];
		__shared__ uint32_t need_mask[KNNQ_MASK_WORDS];
		const int q = blockIdx.x * KNN_THREADS + threadIdx.x;
		const bool valid = q < n;
		const int nboxes = (m + KNNQ_BOX - 1) / KNNQ_BOX, nwords = (nboxes + 31) / 32;
		for (int w = threadIdx.x; w < nwords; w += KNN_THREADS) need_mask[w] = 0u;

		float px = 0.f, py = 0.f, pz = 0.f;
		uint32_t me = 0;
		float bd[KC];
		uint32_t bi[KC];
		knn_reset(bd, bi, k);
		int wb = 0, we = 0;                               // the seed window, in the sources' sorted order
		if (valid)
		{
			me = qorder[q];
			px = x[3 * (size_t)me]; py = x[3 * (size_t)me + 1]; pz = x[3 * (size_t)me + 2];
			// seed: the 2k sources around the query's own position in the sources' Morton order
			const uint32_t code = qcodes[q];
			int lo = 0, hi = m;
			while (lo < hi) { const int mid = (lo + hi) >> 1; if (scodes[mid] < code) lo = mid + 1; else hi = mid; }
			wb = min(max(0, lo - k), max(0, m - 2 * k));
			we = min(m, wb + 2 * k);
			for (int j = wb; j < we; j++)
			{
				const uint32_t o = sorder[j];
				knn_insert(bd, bi, knn_d2(px, py, pz, src[3 * (size_t)o], src[3 * (size_t)o + 1], src[3 * (size_t)o + 2]), o);
			}
		}
		// the k-th distance of any k sources bounds the true k-th from above; ties at it must still be scanned (box distance <= d2 in fp32
		// too).  The seeded list is kept: the box scan below skips the window's sources, so that none enters twice.
		const float reject = bd[KC - 1];
		__syncthreads();

		const int lane = threadIdx.x & (WAVE - 1);
		for (int b = 0; b < nboxes; b++)
		{
			const bool need = valid && !(dist_box_point(boxes + 6 * (size_t)b, px, py, pz) > reject);
			if (__ballot(need) != 0ull && lane == 0) atomicOr(&need_mask[b >> 5], 1u << (b & 31));
		}
		__syncthreads();

		for (int w = 0; w < nwords; w++)
		{
			uint32_t word = need_mask[w];
			while (word != 0u)
			{
				const int b = w * 32 + (__ffs(word) - 1);
				word &= word - 1u;
				const int first = b * KNNQ_BOX, cnt = min(KNNQ_BOX, m - first);
				for (int j = threadIdx.x; j < cnt; j += KNN_THREADS)
				{
					const uint32_t o = sorder[first + j];
					sx[j] = src[3 * (size_t)o]; sy[j] = src[3 * (size_t)o + 1]; sz[j] = src[3 * (size_t)o + 2]; si[j] = o;
				}
				__syncthreads();
				if (valid)
				{
					const float d = dist_box_point(boxes + 6 * (size_t)b, px, py, pz);
					if (!(d > reject || d > bd[KC - 1]))
						for (int j = 0; j < cnt; j++)
							if (first + j < wb || first + j >= we) knn_insert(bd, bi, knn_d2(px, py, pz, sx[j], sy[j], sz[j]), si[j]);
				}
				__syncthreads();
			}
		}
		if (valid)
		{
			int64_t* oi = out_idx + (size_t)me * k;
			float* od = out_d2 + (size_t)me * k;
#pragma unroll
			for (int j = 0; j < KC; j++)
				if (j >= KC - k) { oi[j - (KC - k)] = (int64_t)bi[j]; od[j - (KC - k)] = bd[j]; }
		}
	}

	template <int KC>
	static void knn_query_launch(int n, int m, int k, const float* x, const float* src, const KnnQueryLayout& L, char* s, int qres, int sres,
	                             int64_t* idx, float* d2, hipStream_t stream)
	{
		hipLaunchKernelGGL(knn_query_kernel<KC>, dim3(div_up(n, KNN_THREADS)), dim3(KNN_THREADS), 0, stream, n, m, k, x, src,
		                   (const uint32_t*)(s + L.qidx[qres]), (const uint32_t*)(s + L.qcode[qres]), (const uint32_t*)(s + L.sidx[sres]),
		                   (const uint32_t*)(s + L.scode[sres]), (const float*)(s + L.boxes), idx, d2);
	}
}

extern "C" size_t fdgs_knn_query_scratch_bytes(int32_t n, int32_t m) { return fdgs::knn_query_layout(n, m).total; }

extern "C" int fdgs_knn_query(int32_t b, int32_t n, int32_t m, int32_t k, const float* x, const float* src, int64_t* idx, float* dist2,
                              void* scratch, void* stream_v)
{
	using namespace fdgs;
	if (b < 0 || n < 0 || m < 0) return fail(FDGS_ERR_INVALID_ARG, "fdgs_knn_query: negative size");
	if (k < 1 || k > FDGS_KNN_MAX_K) return fail(FDGS_ERR_INVALID_ARG, "fdgs_knn_query: k must be in [1, 64]");
	if ((int64_t)div_up(m > 0 ? m : 1, KNNQ_BOX) > (int64_t)KNNQ_MASK_WORDS * 32)
		return fail(FDGS_ERR_INVALID_ARG, "fdgs_knn_query: more than 16777216 sources per batch");
	if (b == 0 || n == 0) return FDGS_OK;
	if (!x || !idx || !dist2 || !scratch || (m > 0 && !src)) return fail(FDGS_ERR_INVALID_ARG, "fdgs_knn_query: missing pointer");
	hipStream_t stream = (hipStream_t)stream_v;
	const KnnQueryLayout L = knn_query_layout(n, m);
	char* s = (char*)scratch;
	float* bounds = (float*)(s + L.bounds);
	for (int bb = 0; bb < b; bb++)
	{
		const float* xb = x + (size_t)bb * n * 3;
		const float* sb = src + (size_t)bb * m * 3;
		int sres = 0, qres = 0;
		hipLaunchKernelGGL(knn_bounds_kernel, dim3(1), dim3(1024), 0, stream, m, sb, n, xb, bounds);
		uint32_t* scode[2] = { (uint32_t*)(s + L.scode[0]), (uint32_t*)(s + L.scode[1]) };
		uint32_t* sidx[2] = { (uint32_t*)(s + L.sidx[0]), (uint32_t*)(s + L.sidx[1]) };
		uint32_t* qcode[2] = { (uint32_t*)(s + L.qcode[0]), (uint32_t*)(s + L.qcode[1]) };
		uint32_t* qidx[2] = { (uint32_t*)(s + L.qidx[0]), (uint32_t*)(s + L.qidx[1]) };
		if (m > 0)
		{
			hipLaunchKernelGGL(knn_morton_kernel, dim3(div_up(m, 256)), dim3(256), 0, stream, m, sb, bounds, scode[0], sidx[0]);
			HIP_TRY(radix_sort_pairs(scode, sidx, m, 0, 32, (uint32_t*)(s + L.hist), stream, &sres), "fdgs_knn_query: radix_sort_pairs");
			hipLaunchKernelGGL(knn_box_bounds_kernel<KNNQ_BOX>, dim3(div_up(m, KNNQ_BOX)), dim3(KNN_THREADS), 0, stream, m, sb, sidx[sres],
			                   (float*)(s + L.boxes));
		}
		hipLaunchKernelGGL(knn_morton_kernel, dim3(div_up(n, 256)), dim3(256), 0, stream, n, xb, bounds, qcode[0], qidx[0]);
		HIP_TRY(radix_sort_pairs(qcode, qidx, n, 0, 32, (uint32_t*)(s + L.hist), stream, &qres), "fdgs_knn_query: radix_sort_pairs");
		int64_t* ib = idx + (size_t)bb * n * k;
		float* db = dist2 + (size_t)bb * n * k;
		if (k <= 4) knn_query_launch<4>(n, m, k, xb, sb, L, s, qres, sres, ib, db, stream);
		else if (k <= 8) knn_query_launch<8>(n, m, k, xb, sb, L, s, qres, sres, ib, db, stream);
		else if (k <= 16) knn_query_launch<16>(n, m, k, xb, sb, L, s, qres, sres, ib, db, stream);
		else if (k <= 20) knn_query_launch<20>(n, m, k, xb, sb, L, s, qres, sres, ib, db, stream);
		else if (k <= 32) knn_query_launch<32>(n, m, k, xb, sb, L, s, qres, sres, ib, db, stream);
		else knn_query_launch<64>(n, m, k, xb, sb, L, s, qres, sres, ib, db, stream);
	}
	return launched("fdgs_knn_query");
}

// Test hook (include/fdgs.h): where the stages above lie in the scratch buffer of a finished call.  Host arithmetic only.
extern "C" int fdgs_debug_knn_stage_offsets(int32_t query, int32_t n, int32_t m, int64_t* offsets)
{
	using namespace fdgs;
	if (!offsets || n < 0 || m < 0) return fail(FDGS_ERR_INVALID_ARG, "fdgs_debug_knn_stage_offsets: bad arguments");
	if (query)
	{
		const KnnQueryLayout L = knn_query_layout(n, m);
		const int sres = radix_sort_result_buffer(m, 0, 32), qres = radix_sort_result_buffer(n, 0, 32);
		offsets[FDGS_KNN_STAGE_BOUNDS] = (int64_t)L.bounds;
		offsets[FDGS_KNN_STAGE_BOXES] = (int64_t)L.boxes;
		offsets[FDGS_KNN_STAGE_SRC_CODES] = (int64_t)L.scode[sres];
		offsets[FDGS_KNN_STAGE_SRC_ORDER] = (int64_t)L.sidx[sres];
		offsets[FDGS_KNN_STAGE_QUERY_CODES] = (int64_t)L.qcode[qres];
		offsets[FDGS_KNN_STAGE_QUERY_ORDER] = (int64_t)L.qidx[qres];
		offsets[FDGS_KNN_STAGE_NBOXES] = m > 0 ? div_up(m, KNNQ_BOX) : 0;
		offsets[FDGS_KNN_STAGE_BOX] = KNNQ_BOX;
	}
	else
	{
		const KnnLayout L = knn_layout(m);
		const int res = radix_sort_result_buffer(m, 0, 32);
		offsets[FDGS_KNN_STAGE_BOUNDS] = (int64_t)L.bounds;
		offsets[FDGS_KNN_STAGE_BOXES] = (int64_t)L.boxes;
		offsets[FDGS_KNN_STAGE_SRC_CODES] = (int64_t)L.code[res];
		offsets[FDGS_KNN_STAGE_SRC_ORDER] = (int64_t)L.idx[res];
		offsets[FDGS_KNN_STAGE_QUERY_CODES] = -1;
		offsets[FDGS_KNN_STAGE_QUERY_ORDER] = -1;
		offsets[FDGS_KNN_STAGE_NBOXES] = m > 0 ? div_up(m, KNN_BOX) : 0;
		offsets[FDGS_KNN_STAGE_BOX] = KNN_BOX;
	}
	return FDGS_OK;
}
