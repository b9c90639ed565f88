// compact.h -- order-preserving compaction of a whole array in three launches (time_slice.hip, tsdf.hip, mesh.hip, mesh_simplify.hip):
//   count   every workgroup's number of outputs                               compact_count_kernel<THREADS, Pass>
//   scan    one workgroup per count array: the workgroups' first ranks, the total       compact_scan_kernel
//   emit    rank = the workgroup's first rank + the rank inside the workgroup            compact_emit_kernel<THREADS, Pass>
// Integer sums in a fixed order (the workgroup scans of scan.h): exact and reproducible.  What is counted and what is written is a Pass, a small trivially copyable
// struct handed to both kernels by value:
//   __host__ __device__ int size() const                how many elements there are
//   typename Item                                       what count() hands to emit() inside the emit kernel (registers of one thread)
//   uint32_t count(int i, Item& item, bool emitting)    how many outputs element i < size() produces.  It runs in both kernels, so what it
//                                                       stores for later passes it stores under !emitting (a constant where it is inlined)
//   void emit(int i, uint32_t n, uint32_t rank, const Item& item)     for every i < size(): its n outputs go to rank, rank + 1, ...
#pragma once
#include "scan.h"

namespace fdgs
{
	constexpr int COMPACT_THREADS = 256;                 // the count and emit kernels' workgroup
	constexpr int COMPACT_SCAN_THREADS = 1024;           // one scan chunk: the counts of 1024 workgroups
	static size_t compact_blocks(size_t n) { return (n + COMPACT_THREADS - 1) / COMPACT_THREADS; }

	template <int THREADS, class Pass>
	__global__ void __launch_bounds__(THREADS) compact_count_kernel(const Pass p, uint32_t* __restrict__ counts)
	{
		__shared__ uint32_t s_wave[THREADS / WAVE];
		const int i = blockIdx.x * THREADS + threadIdx.x;
		typename Pass::Item item;
		uint32_t total;
		block_rank<THREADS>(i < p.size() ? p.count(i, item, false) : 0u, s_wave, total);
		if (threadIdx.x == 0) counts[blockIdx.x] = total;
	}

	template <int THREADS, class Pass>
	__global__ void __launch_bounds__(THREADS) compact_emit_kernel(const Pass p, const uint32_t* __restrict__ counts)
	{
		__shared__ uint32_t s_wave[THREADS / WAVE];
		const int i = blockIdx.x * THREADS + threadIdx.x;
		typename Pass::Item item;
		const uint32_t n = i < p.size() ? p.count(i, item, true) : 0u;
		uint32_t total;
		const uint32_t rank = counts[blockIdx.x] + block_rank<THREADS>(n, s_wave, total);
		if (i < p.size()) p.emit(i, n, rank, item);
	}

	// one workgroup per job: counts[0 .. n) -> their exclusive scan in place, factor x the sum -> *total
	struct ScanJob { uint32_t* counts; int n; uint32_t factor; int32_t* total; };
	struct ScanJobs { ScanJob job[2]; };
	template <int THREADS>
	__global__ void __launch_bounds__(THREADS) compact_scan_kernel(const ScanJobs jobs)
	{
		__shared__ uint32_t s_wave[THREADS / WAVE];
		const ScanJob& j = jobs.job[blockIdx.x];
		const uint32_t sum = block_scan_counts<THREADS>(j.counts, j.n, s_wave);
		if (threadIdx.x == 0) *j.total = (int32_t)(j.factor * sum);
	}

	// ---- host side ----
	// One compaction: its pass, the scratch words of its workgroups' counts (compact_blocks(pass.size()) of them), where the total
	// goes and what it is multiplied with, and whether the caller wants more than the total.
	template <class Pass>
	struct Compaction { Pass pass; uint32_t* counts; int32_t* total; uint32_t factor; bool emit; };

	template <class Pass>
	static void compact_count(const Compaction<Pass>& c, hipStream_t stream)
	{
		const int nb = (int)compact_blocks((size_t)c.pass.size());
		if (nb > 0) hipLaunchKernelGGL((compact_count_kernel<COMPACT_THREADS, Pass>), dim3(nb), dim3(COMPACT_THREADS), 0, stream, c.pass, c.counts);
	}
	template <class Pass>
	static void compact_emit(const Compaction<Pass>& c, hipStream_t stream)
	{
		const int nb = (int)compact_blocks((size_t)c.pass.size());
		if (c.emit && nb > 0) hipLaunchKernelGGL((compact_emit_kernel<COMPACT_THREADS, Pass>), dim3(nb), dim3(COMPACT_THREADS), 0, stream, c.pass, c.counts);
	}
	// the scan of one count array, or of two in one launch (an array without a count is fine: its total is 0)
	static void compact_scan(const ScanJob& a, hipStream_t stream)
	{
		hipLaunchKernelGGL(compact_scan_kernel<COMPACT_SCAN_THREADS>, dim3(1), dim3(COMPACT_SCAN_THREADS), 0, stream, ScanJobs{ { a, a } });
	}
	static void compact_scan(const ScanJob& a, const ScanJob& b, hipStream_t stream)
	{
		hipLaunchKernelGGL(compact_scan_kernel<COMPACT_SCAN_THREADS>, dim3(2), dim3(COMPACT_SCAN_THREADS), 0, stream, ScanJobs{ { a, b } });
	}
	template <class Pass>
	static ScanJob scan_job(const Compaction<Pass>& c) { return ScanJob{ c.counts, (int)compact_blocks((size_t)c.pass.size()), c.factor, c.total }; }

	// count, scan, emit of one compaction ...
	template <class A>
	static void compact_enqueue(const Compaction<A>& a, hipStream_t stream)
	{
		compact_count(a, stream);
		compact_scan(scan_job(a), stream);
		compact_emit(a, stream);
	}
	// ... and of two that share their scan launch: count, count, scan, emit, emit (b's emit may read what a's wrote)
	template <class A, class B>
	static void compact_enqueue(const Compaction<A>& a, const Compaction<B>& b, hipStream_t stream)
	{
		compact_count(a, stream);
		compact_count(b, stream);
		compact_scan(scan_job(a), scan_job(b), stream);
		compact_emit(a, stream);
		compact_emit(b, stream);
	}
}
