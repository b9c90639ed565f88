// compress.hip -- storing a trained model small: k-means over the non-DC SH rows (assignment on the f32-input MFMA, a reproducible
// weighted update through the stable radix sort), per-column quantisation and the decode straight into a flat parameter bucket.
// C ABI: fdgs_kmeans_assign / _update / _scratch_bytes, fdgs_quantize_columns, fdgs_compact_decode (include/fdgs.h).
//
// Built with FP contraction off: every expression below is the IEEE operations as written, so a numpy float32 restatement
// (tests/compress_oracle.py) matches the quantise / decode kernels bit for bit.  No float atomics anywhere in this file.
#include "fdgs_common.h"
#include <math.h>

namespace fdgs
{
	constexpr int KM_THREADS = 256;   // 4 waves
	constexpr int KM_ROWS = 128;      // rows of x per workgroup: one 32-row MFMA tile per wave, its A fragments held in registers
	constexpr int KM_COLS = 64;       // codebook rows per LDS tile: two 32-column MFMA tiles (two independent accumulators per wave)
	constexpr int KM_MAX_D = 192;
	constexpr int KM_MAX_K = 65536;
	typedef float km_f32x16 __attribute__((ext_vector_type(16)));

	struct KmLayout { size_t cnorm, keys[2], vals[2], hist, seg_lo, seg_hi, total; };
	static inline KmLayout km_layout(int N, int K)
	{
		KmLayout L;
		ScratchCursor c;
		const size_t n = (size_t)(N > 0 ? N : 1), k = (size_t)(K > 0 ? K : 1);
		L.cnorm = c.take(k * 4);
		for (int i = 0; i < 2; i++) L.keys[i] = c.take(n * 4);
		for (int i = 0; i < 2; i++) L.vals[i] = c.take(n * 4);
		L.hist = c.take((size_t)RADIX * (sort_blocks((int)n) + 1) * 4);
		L.seg_lo = c.take(k * 4);
		L.seg_hi = c.take(k * 4);
		L.total = c.o;
		return L;
	}

	// ---- assignment ----
	// score(n, k) = |c_k|^2 - 2 x_n . c_k  (the |x_n|^2 every k shares is left out).  |c_k|^2 is a d-ordered sum, the dot product the
	// MFMA's d-ordered fma chain: both depend on the VALUES of row k alone, never on where the row sits in a tile, so two equal codebook
	// rows score bit-identically and the lowest k wins the tie.
	__global__ void kmeans_cnorm_kernel(int K, int D, const float* __restrict__ c, float* __restrict__ cn)
	{
		const int k = blockIdx.x * blockDim.x + threadIdx.x;
		if (k >= K) return;
		const float* r = c + (size_t)k * D;
		float s = 0.f;
		for (int d = 0; d < D; d++) s = s + r[d] * r[d];
		cn[k] = s;
	}

	// STEPS: k-steps of v_mfma_f32_32x32x2_f32 that cover D (2 STEPS >= D; the tail is zero-padded in registers / LDS, and
	// fma(0, 0, acc) leaves acc as it is).  Lane l of a wave holds A[row l & 31][d = 2 s + (l >> 5)] of its 32 rows for every step s --
	// the whole x tile lives in STEPS registers for the launch -- and reads B[d = 2 s + (l >> 5)][column l & 31] from the LDS tile
	// (row-major codebook rows at an odd pitch: the 32 lanes of a half-wave hit 32 banks).  The accumulator has its column on the lane and
	// 16 rows in registers (row = (r & 3) + 8 (r >> 2) + 4 (l >> 5)), so the running (best score, best k) of those 16 rows over the
	// columns this lane sees stays in registers across all tiles; one 32-lane reduction per row at the very end.
	template <int STEPS>
	__global__ void __launch_bounds__(KM_THREADS) kmeans_assign_kernel(int N, int K, int D, const float* __restrict__ x, const float* __restrict__ c,
	                                                                    const float* __restrict__ cn, int32_t* __restrict__ index)
	{
		constexpr int DP = 2 * STEPS, PITCH = DP + 1;
		__shared__ float tile[KM_COLS * PITCH];
		const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
		const int col = lane & 31, half = lane >> 5;
		const long long row0 = (long long)blockIdx.x * KM_ROWS + wave * 32;
		const bool wave_live = row0 < N;
		const long long row = row0 + col;
		const bool row_ok = row < N;
		const float* xr = x + (size_t)(row_ok ? row : 0) * D;
		float a[STEPS];
#pragma unroll
		for (int s = 0; s < STEPS; s++)
		{
			const int d = 2 * s + half;
			a[s] = (row_ok && d < D) ? xr[d] : 0.f;
		}
		float best[16];
		int bestk[16];
#pragma unroll
		for (int r = 0; r < 16; r++) { best[r] = INFINITY; bestk[r] = 0; }

		for (int k0 = 0; k0 < K; k0 += KM_COLS)
		{
			__syncthreads();
			for (int i = threadIdx.x; i < KM_COLS * DP; i += KM_THREADS)
			{
				const int j = i / DP, d = i - j * DP;
				const int k = k0 + j;
				tile[j * PITCH + d] = (k < K && d < D) ? c[(size_t)k * D + d] : 0.f;
			}
			__syncthreads();
			if (!wave_live) continue;
			const int ka = k0 + col, kb = k0 + 32 + col;
			const bool second = k0 + 32 < K;   // wave-uniform
			const float cna = ka < K ? cn[ka] : INFINITY;
			const float cnb = kb < K ? cn[kb] : INFINITY;
			const float* ta = tile + col * PITCH + half;
			const float* tb = ta + 32 * PITCH;
			km_f32x16 acc0 = { 0 }, acc1 = { 0 };
			if (second)
			{
#pragma unroll
				for (int s = 0; s < STEPS; s++)
				{
					acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], ta[2 * s], acc0, 0, 0, 0);
					acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], tb[2 * s], acc1, 0, 0, 0);
				}
			}
			else
			{
#pragma unroll
				for (int s = 0; s < STEPS; s++) acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], ta[2 * s], acc0, 0, 0, 0);
			}
			// strict <: an equal score never replaces an earlier (lower) k; a column at or beyond K scores +inf
#pragma unroll
			for (int r = 0; r < 16; r++)
			{
				const float s0 = cna - 2.f * acc0[r];
				if (s0 < best[r]) { best[r] = s0; bestk[r] = ka; }
			}
			if (second)
			{
#pragma unroll
				for (int r = 0; r < 16; r++)
				{
					const float s1 = cnb - 2.f * acc1[r];
					if (s1 < best[r]) { best[r] = s1; bestk[r] = kb; }
				}
			}
		}
		if (!wave_live) return;
#pragma unroll
		for (int r = 0; r < 16; r++)
		{
			float b = best[r];
			int bk = bestk[r];
#pragma unroll
			for (int off = 16; off >= 1; off >>= 1)   // stays inside the 32 lanes that share these rows
			{
				const float ob = __shfl_xor(b, off);
				const int ok = __shfl_xor(bk, off);
				if (ob < b || (ob == b && ok < bk)) { b = ob; bk = ok; }
			}
			const long long out_row = row0 + (r & 3) + 8 * (r >> 2) + 4 * half;
			if (col == 0 && out_row < N) index[out_row] = bk;
		}
	}

	// the winning squared distance, as the direct sum
	__global__ void kmeans_dist_kernel(int N, int K, int D, const float* __restrict__ x, const float* __restrict__ c, const int32_t* __restrict__ index,
	                                   float* __restrict__ dist2)
	{
		const long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x;
		if (n >= N) return;
		const int k = min(max(index[n], 0), K - 1);
		const float* xr = x + (size_t)n * D;
		const float* cr = c + (size_t)k * D;
		float s = 0.f;
		for (int d = 0; d < D; d++)
		{
			const float t = xr[d] - cr[d];
			s = s + t * t;
		}
		dist2[n] = s;
	}

	// ---- update ----
	__global__ void kmeans_pairs_kernel(int N, const int32_t* __restrict__ index, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals)
	{
		const long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x;
		if (n >= N) return;
		keys[n] = (uint32_t)index[n];
		vals[n] = (uint32_t)n;
	}

	// [lo, hi) of every cluster's run in the sorted keys (both zero-filled before: an empty cluster keeps lo == hi == 0)
	__global__ void kmeans_segments_kernel(int N, int K, const uint32_t* __restrict__ keys, uint32_t* __restrict__ seg_lo, uint32_t* __restrict__ seg_hi)
	{
		const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
		if (i >= N) return;
		const uint32_t k = keys[i];
		if (k >= (uint32_t)K) return;   // an index outside the codebook belongs to no cluster
		if (i == 0 || keys[i - 1] != k) seg_lo[k] = (uint32_t)i;
		if (i == N - 1 || keys[i + 1] != k) seg_hi[k] = (uint32_t)(i + 1);
	}

	// One workgroup per cluster, one thread per component: the rows of the cluster are summed in ascending row id (the sort is stable),
	// so the result does not depend on scheduling.  Every thread carries the same weight sum.
	__global__ void __launch_bounds__(KM_MAX_D) kmeans_update_kernel(int K, int D, const float* __restrict__ x, const float* __restrict__ w,
	                                                                 const uint32_t* __restrict__ rows, const uint32_t* __restrict__ seg_lo,
	                                                                 const uint32_t* __restrict__ seg_hi, float* __restrict__ c, int32_t* __restrict__ counts)
	{
		const int k = blockIdx.x;
		const int d = threadIdx.x;
		const uint32_t lo = seg_lo[k], hi = seg_hi[k];
		if (counts && d == 0) counts[k] = (int32_t)(hi - lo);
		if (d >= D || hi <= lo) return;
		float sum = 0.f, wsum = 0.f;
		for (uint32_t i = lo; i < hi; i++)
		{
			const uint32_t n = rows[i];
			const float wn = w ? w[n] : 1.f;
			sum = sum + wn * x[(size_t)n * D + d];
			wsum = wsum + wn;
		}
		if (wsum > 0.f) c[(size_t)k * D + d] = sum / wsum;   // no weight: the row stays
	}

	// ---- column quantisation ----
	template <typename Q>
	__global__ void quantize_columns_kernel(long long total, int C, const float* __restrict__ x, const float* __restrict__ lo, const float* __restrict__ inv,
	                                        float qmax, Q* __restrict__ q)
	{
		const long long stride = (long long)gridDim.x * blockDim.x;
		for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride)
		{
			const int col = (int)(i % C);
			const float t = rintf((x[i] - lo[col]) * inv[col]);
			q[i] = (Q)fminf(fmaxf(t, 0.f), qmax);
		}
	}

	// ---- decode ----
	// Row p of `out` is C + D floats: the C columns (8 / 16 bit: lo + q * step; 32: the stored float, bit for bit), then -- D > 0 --
	// row index[p] (p itself without an index) of `rows` [K, D].  A thread produces four consecutive floats of one output row and, where
	// the rows start on 16 bytes, stores them as one float4; the loads of a wave are consecutive dwords of q / of one codebook row.
	template <int BITS>
	__device__ __forceinline__ float decode_value(const void* q, const float* lo, const float* step, long long p, int C, int col)
	{
		if (BITS == 32) return ((const float*)q)[p * C + col];
		const float v = BITS == 8 ? (float)((const uint8_t*)q)[p * C + col] : (float)((const uint16_t*)q)[p * C + col];
		return lo[col] + v * step[col];
	}

	template <int BITS, bool VEC>
	__global__ void compact_decode_kernel(long long P, int C, const void* __restrict__ q, const float* __restrict__ lo, const float* __restrict__ step,
	                                      int D, const float* __restrict__ rows, const int32_t* __restrict__ index, int K, float* __restrict__ out)
	{
		const int pitch = C + D, groups = (pitch + 3) >> 2;
		const long long total = P * groups, stride = (long long)gridDim.x * blockDim.x;
		for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride)
		{
			const long long p = i / groups;
			const int f0 = (int)(i - p * groups) * 4;
			const float* src = nullptr;
			if (D > 0)
			{
				const long long k = index ? (long long)min(max(index[p], 0), K - 1) : p;
				src = rows + (size_t)k * D;
			}
			float v[4];
#pragma unroll
			for (int e = 0; e < 4; e++)
			{
				const int f = f0 + e;
				v[e] = f < C ? decode_value<BITS>(q, lo, step, p, C, f) : (f < pitch ? src[f - C] : 0.f);
			}
			float* dst = out + (size_t)p * pitch + f0;
			if (VEC) *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);   // (pitch is a multiple of 4 here)
			else
			{
#pragma unroll
				for (int e = 0; e < 4; e++) if (f0 + e < pitch) dst[e] = v[e];
			}
		}
	}

	static inline int stream_grid(long long total, int threads)
	{
		const long long b = (total + threads - 1) / threads;
		return (int)(b < 1 ? 1 : (b > 8192 ? 8192 : b));
	}

	template <int BITS>
	static void launch_decode(long long P, int C, const void* q, const float* lo, const float* step, int D, const float* rows, const int32_t* index,
	                          int K, float* out, hipStream_t stream)
	{
		const int pitch = C + D;
		const long long total = P * ((pitch + 3) >> 2);
		const int grid = stream_grid(total, 256);
		if (pitch % 4 == 0 && ((uintptr_t)out & 15) == 0)
			hipLaunchKernelGGL((compact_decode_kernel<BITS, true>), dim3(grid), dim3(256), 0, stream, P, C, q, lo, step, D, rows, index, K, out);
		else
			hipLaunchKernelGGL((compact_decode_kernel<BITS, false>), dim3(grid), dim3(256), 0, stream, P, C, q, lo, step, D, rows, index, K, out);
	}
}

using namespace fdgs;

extern "C" size_t fdgs_kmeans_scratch_bytes(int32_t N, int32_t K) { return km_layout(N, K).total; }

static const char* km_sizes_bad(int32_t N, int32_t K, int32_t D)
{
	if (N < 1) return "N must be at least 1";
	if (K < 1 || K > KM_MAX_K) return "K must be within 1..65536";
	if (D < 1 || D > KM_MAX_D) return "D must be within 1..192";
	return nullptr;
}

extern "C" int fdgs_kmeans_assign(int32_t N, int32_t K, int32_t D, const float* x, const float* c, int32_t* index, float* dist2, void* scratch,
                                  void* stream_v)
{
	if (const char* bad = km_sizes_bad(N, K, D)) return fail(FDGS_ERR_INVALID_ARG, "fdgs_kmeans_assign: %s (N=%d K=%d D=%d)", bad, N, K, D);
	if (!x || !c || !index || !scratch) return fail(FDGS_ERR_INVALID_ARG, "fdgs_kmeans_assign: x / c / index / scratch must not be NULL");
	hipStream_t stream = (hipStream_t)stream_v;
	float* cn = (float*)((char*)scratch + km_layout(N, K).cnorm);
	hipLaunchKernelGGL(kmeans_cnorm_kernel, dim3(div_up(K, 256)), dim3(256), 0, stream, K, D, c, cn);
	const dim3 grid((unsigned)(((long long)N + KM_ROWS - 1) / KM_ROWS)), block(KM_THREADS);
	if (D <= 16) hipLaunchKernelGGL(kmeans_assign_kernel<8>, grid, block, 0, stream, N, K, D, x, c, cn, index);
	else if (D <= 48) hipLaunchKernelGGL(kmeans_assign_kernel<24>, grid, block, 0, stream, N, K, D, x, c, cn, index);
	else if (D <= 96) hipLaunchKernelGGL(kmeans_assign_kernel<48>, grid, block, 0, stream, N, K, D, x, c, cn, index);
	else if (D <= 144) hipLaunchKernelGGL(kmeans_assign_kernel<72>, grid, block, 0, stream, N, K, D, x, c, cn, index);
	else hipLaunchKernelGGL(kmeans_assign_kernel<96>, grid, block, 0, stream, N, K, D, x, c, cn, index);
	if (dist2) hipLaunchKernelGGL(kmeans_dist_kernel, dim3((unsigned)(((long long)N + 255) / 256)), dim3(256), 0, stream, N, K, D, x, c, index, dist2);
	return launched("fdgs_kmeans_assign");
}

extern "C" int fdgs_kmeans_update(int32_t N, int32_t K, int32_t D, const float* x, const int32_t* index, const float* w, float* c, int32_t* counts,
                                  void* scratch, void* stream_v)
{
	if (const char* bad = km_sizes_bad(N, K, D)) return fail(FDGS_ERR_INVALID_ARG, "fdgs_kmeans_update: %s (N=%d K=%d D=%d)", bad, N, K, D);
	if (!x || !index || !c || !scratch) return fail(FDGS_ERR_INVALID_ARG, "fdgs_kmeans_update: x / index / c / scratch must not be NULL");
	hipStream_t stream = (hipStream_t)stream_v;
	const KmLayout L = km_layout(N, K);
	char* s = (char*)scratch;
	uint32_t* keys[2] = { (uint32_t*)(s + L.keys[0]), (uint32_t*)(s + L.keys[1]) };
	uint32_t* vals[2] = { (uint32_t*)(s + L.vals[0]), (uint32_t*)(s + L.vals[1]) };
	uint32_t* seg_lo = (uint32_t*)(s + L.seg_lo);
	uint32_t* seg_hi = (uint32_t*)(s + L.seg_hi);
	const unsigned nb = (unsigned)(((long long)N + 255) / 256);
	hipLaunchKernelGGL(kmeans_pairs_kernel, dim3(nb), dim3(256), 0, stream, N, index, keys[0], vals[0]);
	const int bits = K <= 256 ? 8 : 16;   // whole radix passes over the keys 0 .. K - 1
	int res = 0;
	HIP_TRY(radix_sort_pairs(keys, vals, N, 0, bits, (uint32_t*)(s + L.hist), stream, &res), "fdgs_kmeans_update: radix_sort_pairs");
	HIP_TRY(hipMemsetAsync(seg_lo, 0, (size_t)K * 4, stream), "fdgs_kmeans_update: hipMemsetAsync");
	HIP_TRY(hipMemsetAsync(seg_hi, 0, (size_t)K * 4, stream), "fdgs_kmeans_update: hipMemsetAsync");
	hipLaunchKernelGGL(kmeans_segments_kernel, dim3(nb), dim3(256), 0, stream, N, K, keys[res], seg_lo, seg_hi);
	hipLaunchKernelGGL(kmeans_update_kernel, dim3(K), dim3(KM_MAX_D), 0, stream, K, D, x, w, vals[res], seg_lo, seg_hi, c, counts);
	return launched("fdgs_kmeans_update");
}

extern "C" int fdgs_quantize_columns(int32_t P, int32_t C, const float* x, const float* lo, const float* inv, int32_t qmax, void* q, void* stream_v)
{
	if (P < 0 || C < 1 || (int64_t)P * C >= ((int64_t)1 << 40)) return fail(FDGS_ERR_INVALID_ARG, "fdgs_quantize_columns: need P >= 0, C >= 1");
	if (qmax != 255 && qmax != 65535) return fail(FDGS_ERR_INVALID_ARG, "fdgs_quantize_columns: qmax must be 255 (uint8) or 65535 (uint16)");
	if (P == 0) return FDGS_OK;
	if (!x || !lo || !inv || !q) return fail(FDGS_ERR_INVALID_ARG, "fdgs_quantize_columns: x / lo / inv / q must not be NULL");
	hipStream_t stream = (hipStream_t)stream_v;
	const long long total = (long long)P * C;
	const int grid = stream_grid(total, 256);
	if (qmax == 255) hipLaunchKernelGGL(quantize_columns_kernel<uint8_t>, dim3(grid), dim3(256), 0, stream, total, C, x, lo, inv, 255.f, (uint8_t*)q);
	else hipLaunchKernelGGL(quantize_columns_kernel<uint16_t>, dim3(grid), dim3(256), 0, stream, total, C, x, lo, inv, 65535.f, (uint16_t*)q);
	return launched("fdgs_quantize_columns");
}

extern "C" int fdgs_compact_decode(int32_t P, int32_t C, int32_t bits, const void* q, const float* lo, const float* step, int32_t D, const float* rows,
                                   const int32_t* index, int32_t K, float* out, void* stream_v)
{
	if (P < 0 || C < 0 || D < 0 || C + (int64_t)D < 1 || C + (int64_t)D > (1 << 20))
		return fail(FDGS_ERR_INVALID_ARG, "fdgs_compact_decode: need P >= 0, C >= 0, D >= 0 and 1 <= C + D <= 2^20");
	if (bits != 8 && bits != 16 && bits != 32) return fail(FDGS_ERR_INVALID_ARG, "fdgs_compact_decode: bits must be 8, 16 or 32");
	if (D > 0 && index && K < 1) return fail(FDGS_ERR_INVALID_ARG, "fdgs_compact_decode: an index needs K >= 1 rows");
	if (P == 0) return FDGS_OK;
	if (!out || (C > 0 && (!q || (bits != 32 && (!lo || !step)))) || (D > 0 && !rows))
		return fail(FDGS_ERR_INVALID_ARG, "fdgs_compact_decode: out / q / lo / step / rows must not be NULL where they are read");
	hipStream_t stream = (hipStream_t)stream_v;
	if (bits == 8) launch_decode<8>(P, C, q, lo, step, D, rows, index, K, out, stream);
	else if (bits == 16) launch_decode<16>(P, C, q, lo, step, D, rows, index, K, out, stream);
	else launch_decode<32>(P, C, q, lo, step, D, rows, index, K, out, stream);
	return launched("fdgs_compact_decode");
}
