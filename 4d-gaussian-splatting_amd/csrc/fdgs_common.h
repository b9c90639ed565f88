// fdgs_common.h -- internal declarations shared by the HIP translation units of libfdgs.so.
//
// Scratch-buffer layouts, launch geometry constants and the host-side entry
// point of each stage.  Written for gfx950 only (wave64, 256 CUs / 8 XCDs).
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <stddef.h>
#include <stdint.h>
#include "../../include/fdgs.h"

namespace fdgs
{
	constexpr int TILE_X = 16;          // reference config.h:16-17 (the tile grid defines key/range indexing)
	constexpr int TILE_Y = 16;
	constexpr int WAVE = 64;            // gfx950 wavefront
	constexpr int SORT_THREADS = 256;   // radix sort workgroup
	constexpr int SORT_ITEMS = 16;      // keys per thread (large inputs: 4096 keys per workgroup)
	constexpr int SORT_ITEMS_SMALL = 4; // keys per thread for inputs <= 1 M keys (1024 per workgroup: fills the chip)
	static inline int sort_items_for(int n) { return n <= (1 << 20) ? SORT_ITEMS_SMALL : SORT_ITEMS; }
	static inline int sort_blocks(int n) { return (n + SORT_THREADS * sort_items_for(n) - 1) / (SORT_THREADS * sort_items_for(n)); }
	constexpr int RADIX_BITS = 8;
	constexpr int RADIX = 1 << RADIX_BITS;
	constexpr int GRAD_ACC_WORDS = 16;  // packed per-Gaussian gradient accumulator record (64 B = one cache line)

	static inline size_t align_up(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }
	static inline int div_up(int a, int b) { return (a + b - 1) / b; }

	// The one error path of the entry points (defined in capi.hip): records the formatted message as this thread's fdgs_last_error()
	// and returns code.  Every non-zero return of an entry point goes through it, so the text always belongs to the call that failed.
	int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
	// the end of an entry point `fn` that launched kernels: FDGS_OK, or the launch error under its name
	static inline int launched(const char* fn)
	{
		const hipError_t e = hipGetLastError();
		return e == hipSuccess ? FDGS_OK : fail(FDGS_ERR_HIP, "%s: %s", fn, hipGetErrorString(e));
	}
	// a HIP runtime call (or a launcher that returns hipError_t) inside an entry point
#define HIP_TRY(expr, what)                                                                                 \
	do {                                                                                                    \
		hipError_t e__ = (expr);                                                                            \
		if (e__ != hipSuccess) return ::fdgs::fail(FDGS_ERR_HIP, "%s: %s", what, hipGetErrorString(e__));   \
	} while (0)
	// every struct of the ABI starts with its own size as the caller's header defined it: a caller built against another fdgs.h
	// is turned away here instead of the library reading past the end of a shorter struct.  CHECK_STRUCT_IN: the message starts
	// with the entry point's name, as the other messages of that entry point do.
#define CHECK_STRUCT_IN(fn, ptr, type)                                                                                    \
	do {                                                                                                                  \
		if ((ptr)->struct_size != (uint32_t)sizeof(type))                                                                 \
			return ::fdgs::fail(FDGS_ERR_INVALID_ARG, "%s%s" #type ".struct_size is %u, this library (FDGS_VERSION %d) expects %zu: built against another fdgs.h?", \
			                    fn, *(fn) ? ": " : "", (unsigned)(ptr)->struct_size, FDGS_VERSION, sizeof(type));         \
	} while (0)
#define CHECK_STRUCT(ptr, type) CHECK_STRUCT_IN("", ptr, type)

	// hands out the members of a scratch layout front to back, each at the default alignment; `o` ends as the total
	struct ScratchCursor
	{
		size_t o = 0;
		size_t take(size_t bytes) { const size_t at = o; o = align_up(o + bytes); return at; }
	};

	// Packed per-Gaussian blend record, 3 x float4 = 48 B, written by preprocess and
	// gathered by both blend kernels (one record instead of the reference's four arrays
	// means2D / conic_opacity / rgb / depths + the flow input):
	//   a = (x, y, conic.x, conic.y)   b = (conic.z, opacity, r, g)   c = (b, depth, flow.x, flow.y)
	// Loads / stores of data that is touched ONCE per optimizer step and is larger than the 256 MB Infinity Cache -- the two Adam moments
	// of the SH coefficients (0.69 GB at C3, 0.77 GB at C5): non-temporal, so that they neither wait for cache lines nor push out what
	// IS used again (the coefficients themselves -- the next forward reads them -- stay ordinary accesses).  Measured on MI355X
	// (profiles/HISTORY.md, round 6): fused SH flush + Adam 214 -> 180 us (1.08 GB: 6.0 TB/s), step +1.5 % at C3, +2.3 % at C5;
	// coefficients non-temporal as well: 190 us; the GEOMETRY parameters' moments (41 MB at C3: they live in that cache from step to
	// step) non-temporal: step -1 ... -2 %, left alone.  -DFDGS_STREAM_PLAIN: ordinary accesses (A/B).
#ifndef FDGS_STREAM_PLAIN
	typedef float fdgs_v4f __attribute__((ext_vector_type(4)));
	__device__ __forceinline__ float4 stream_ld(const float4* p)
	{
		const fdgs_v4f v = __builtin_nontemporal_load(reinterpret_cast<const fdgs_v4f*>(p));
		return make_float4(v.x, v.y, v.z, v.w);
	}
	__device__ __forceinline__ void stream_st(float4* p, float4 x)
	{
		fdgs_v4f v = { x.x, x.y, x.z, x.w };
		__builtin_nontemporal_store(v, reinterpret_cast<fdgs_v4f*>(p));
	}
#else
	__device__ __forceinline__ float4 stream_ld(const float4* p) { return *p; }
	__device__ __forceinline__ void stream_st(float4* p, float4 x) { *p = x; }
#endif

	struct GeomLayout
	{
		size_t records, depths, cov3D, tiles_touched, rect, clamped;
		size_t total;
	};
	static inline GeomLayout geom_layout(int P)
	{
		GeomLayout L;
		ScratchCursor c;
		const size_t p = (size_t)(P > 0 ? P : 1);
		L.records = c.take(p * 48);
		L.depths = c.take(p * 4);
		L.cov3D = c.take(p * 24);
		L.tiles_touched = c.take(p * 4);
		L.rect = c.take(p * 8);
		L.clamped = c.take(p);
		L.total = c.o;
		return L;
	}

	// Tile binning (tilebin.hip): one instance counter per tile, padded to whole uint4s
	static inline size_t bin_counter_words(int T) { return ((size_t)T + 3) & ~(size_t)3; }
	// The tile-order area (ImageLayout::tile_order, 3 T + 16 words): [0, T) the order; at align4(T) the scan's copy of the tile
	// counts (whole uint4 stores: the offset is a multiple of 4 words for every T); behind it T words of scratch
	__host__ __device__ static inline int tile_order_counts_off(int T) { return (T + 3) & ~3; }
	__host__ __device__ static inline int tile_order_tmp_off(int T) { return 2 * ((T + 3) & ~3) + 4; }

	struct ImageLayout
	{
		size_t final_T, n_contrib, ranges;
		size_t tile_counters;   // [T] instance counts -> exclusive starts -> ends (count / scan / scatter passes)
		size_t bin_ctl;         // { R, longest tile list } written by the scan, read back by the host
		size_t tile_order;      // [T] the order in which the blend kernels take the tiles (all tiles, longest lists first; position p
		                        // goes to XCD p % 8), written by one workgroup of the scatter launch from the
		                        // [T] counts the scan leaves behind it (tile_order_counts_off); [T] words of scratch behind those
		size_t total;
	};
	static inline ImageLayout image_layout(int W, int H)
	{
		ImageLayout L;
		ScratchCursor c;
		const size_t n = (size_t)W * H;
		const size_t t = (size_t)div_up(W, TILE_X) * div_up(H, TILE_Y);
		L.final_T = c.take(n * 4);
		L.n_contrib = c.take(n * 4);
		L.ranges = c.take(t * 8);
		L.tile_counters = c.take(bin_counter_words((int)t) * 4);
		L.bin_ctl = c.take(16);
		L.tile_order = c.take((3 * t + 16) * 4);
		L.total = c.o;
		return L;
	}

	// Binning buffer: the sorted instance list the blend kernels walk, the unsorted (depth bits, id) pairs of the
	// scatter pass, and -- only when some tile's list is longer than the LDS sort takes -- R keys of global scratch.
	struct BinLayout
	{
		size_t point_list, cull_bits, pairs, big_scratch, total;
		uint32_t cull_stride;   // 64-bit words per sub-block plane of cull_bits
	};
	// cull_bits: what the blend forward's per-block cull decided, one bit per (list entry, 8x8 block), kept for the blend backward
	// (which used to run the same test again: a tenth of its instructions).  Four planes (one per sub-block of a tile) of
	// cull_stride 64-bit words; the 64 entries [64 c, 64 c + 64) of tile t's list sit in word (list start >> 6) + t + c of the
	// plane -- consecutive tiles never share a word (the + t), and the index stays below (R >> 6) + T + 1.
	static inline BinLayout bin_layout(int R, bool with_big_scratch, int T)
	{
		BinLayout L;
		ScratchCursor c;
		const size_t r = (size_t)(R > 0 ? R : 1);
		L.point_list = c.take(r * 4);
		L.cull_stride = (uint32_t)((r >> 6) + (size_t)(T > 0 ? T : 0) + 2);
		L.cull_bits = c.take((size_t)L.cull_stride * 4 * 8);
		L.pairs = c.take(r * 8);
		L.big_scratch = c.take(with_big_scratch ? r * 8 : 0);
		L.total = c.o;
		return L;
	}

	// ---- stage launchers (each enqueues on `stream`, returns hipError_t) ----

	hipError_t launch_preprocess_fwd(const fdgs_scene& s, const fdgs_forward_out& out, char* geom, uint32_t* bin_counters, int part,
	                                 hipStream_t stream);   // part 0: one launch; 1 / 2: geometry / colour halves

	// SH colours of several views of the same Gaussians in one pass over the coefficients (after the views' part-1 launches)
	hipError_t launch_colour_batch(int nviews, const fdgs_scene* const* views, const fdgs_forward_out* const* outs, char* const* geoms,
	                               hipStream_t stream);

	// Stable LSD radix sort of (key,value) u32 pairs on key bits [bit_lo, bit_hi) (radix_sort.hip; used by knn.hip and regularize.hip).
	// keys[0]/vals[0] hold the input; *result receives the index (0/1) of the buffers holding the output.
	hipError_t radix_sort_pairs(uint32_t* keys[2], uint32_t* vals[2], int n, int bit_lo, int bit_hi,
	                            uint32_t* hist, hipStream_t stream, int* result);
	// the *result of that call, known without running it: every pass of RADIX_BITS bits swaps the buffers
	static inline int radix_sort_result_buffer(int n, int bit_lo, int bit_hi)
	{
		return n > 0 && bit_hi > bit_lo ? ((bit_hi - bit_lo + RADIX_BITS - 1) / RADIX_BITS) & 1 : 0;
	}

	// Tile binning (tilebin.hip).  What its passes share, handed to the launchers and on to the kernels by value:
	struct TileBinArgs
	{
		uint32_t* counters;    // bin_counter_words(T) words, zero on entry of the count pass (cleared by preprocess_fwd, the forward's first
		                       // kernel); after the scan they hold every tile list's start, after the scatter its end
		uint2* pairs;          // [capacity] unsorted (depth bits, id) pairs: scatter -> sort
		uint32_t* point_list;  // [capacity] the tiles' sorted lists
		uint2* ranges;         // [T] (start, end) of every tile's list
		uint32_t* ctl;         // ctl[0] = R, ctl[1] = longest tile list
		uint32_t capacity;     // the instances pairs / point_list hold
		uint32_t* order;       // optional, the tile-order area (3 T + 16 words, see ImageLayout) of COMPACT lists: the scan leaves a copy of the
		                       // tile counts at order + tile_order_counts_off(T), one extra workgroup of the scatter launch turns it into the
		                       // blend kernels' tile order, and the sort takes the tiles in that order too (longest lists first)
		int T, grid_x;
		uint32_t sparse_cap;   // != 0: SPARSE lists (fdgs_forward_out.sparse_lists): no count / scan pass runs, the counters start from zero, tile
		                       // t's list goes to [t * sparse_cap, (t + 1) * sparse_cap) of pairs / point_list; after the scatter the counters hold
		                       // the tiles' counts
	};
	// Who tells the host {R, longest list}: the scan, or with sparse lists one extra workgroup of the sort's main instance (which then writes the
	// tile order too: what the scan + scatter launches do for compact lists).  ctl == NULL: nobody (a sort launch of compact lists).
	struct TileReport
	{
		uint32_t* ctl;         // ctl[0] = R, ctl[1] = longest tile list
		uint32_t* box;         // optional: device pointer of a pinned host mailbox {R, longest, ticket} the kernel writes directly
		uint32_t ticket;
		uint32_t* order_out;   // sort only, optional: the tile-order area the blend kernels' order goes to
	};
	hipError_t launch_tile_count(const uint16_t* rect, int P, const TileBinArgs& a, hipStream_t stream);
	hipError_t launch_tile_scan(const TileBinArgs& a, const TileReport& to, hipStream_t stream);
	// scatter / sort may be launched before the host knows num_rendered (see lists_do_not_fit, tilebin.hip)
	hipError_t launch_tile_scatter(const uint16_t* rect, const float* depths, int P, const TileBinArgs& a, hipStream_t stream);
	// max_count: the longest list PROVIDED FOR; big_scratch: `capacity` 64-bit keys, needed when max_count > tile_sort_lds_cap()
	hipError_t launch_tile_sort(const TileBinArgs& a, int max_count, void* big_scratch, const TileReport& rep, hipStream_t stream);
	int tile_sort_lds_cap();                                   // lists longer than this need the global scratch
	void tile_sort_debug_limits(int lds_cap, int rank_max);    // test hook (fdgs_debug_tile_sort_limits); <= 0 restores the default

	// tile_order: NULL = tiles in index order
	// cull_bits / cull_stride (BinLayout; NULL: not kept) and ctl (the image buffer's control words): the forward leaves the plane
	// stride in ctl[2] and the plane array's offset from the start of the binning buffer (in 64-bit words) in ctl[3] for the backward
	hipError_t launch_blend_fwd(const fdgs_scene& s, const fdgs_forward_out& out, const float* records,
	                            const uint32_t* point_list, const uint32_t* ranges, const uint32_t* tile_order,
	                            float* final_T, uint32_t* n_contrib, unsigned long long* cull_bits, uint32_t cull_stride, uint32_t cull_word_off,
	                            uint32_t* ctl, hipStream_t stream);

	// What a finished forward left in its three scratch buffers, as the kernels that walk its lists again take it (the blend backward,
	// contribution.hip, features.hip, fdgs_debug_views).
	struct FinishedForward
	{
		int W, H, gx, ntiles;
		const float4* records;        // [P] 48-byte blend records
		const uint32_t* point_list;   // the tiles' sorted lists
		const uint2* ranges;          // [ntiles] (start, end) of every tile's list
		const uint32_t* tile_order;   // the order the blend kernels take the tiles in; NULL = index order
		const float* final_T;         // [H, W]
		const uint32_t* n_contrib;    // [H, W]
		const uint32_t* ctl;          // the image buffer's control words (ctl[2..3]: the cull planes, see launch_blend_fwd)
	};
	// The only place that knows point_list sits at the front of the binning buffer whatever layout the forward chose (sparse or
	// compact lists, cull planes, sort scratch); num_rendered < 0: not known (a lazy forward) -- the ranges carry what the kernels need.
	static inline FinishedForward finished_forward(int P, int W, int H, int num_rendered, const void* geom, const void* bin, const void* img,
	                                               bool use_tile_order)
	{
		const GeomLayout GL = geom_layout(P);
		const ImageLayout IL = image_layout(W, H);
		const BinLayout BL = bin_layout(num_rendered, false, 0);
		const char* g = (const char*)geom;
		const char* b = (const char*)bin;
		const char* i = (const char*)img;
		FinishedForward ff;
		ff.W = W; ff.H = H; ff.gx = div_up(W, TILE_X); ff.ntiles = ff.gx * div_up(H, TILE_Y);
		ff.records = (const float4*)(g + GL.records);
		ff.point_list = b ? (const uint32_t*)(b + BL.point_list) : nullptr;
		ff.ranges = (const uint2*)(i + IL.ranges);
		ff.tile_order = use_tile_order ? (const uint32_t*)(i + IL.tile_order) : nullptr;
		ff.final_T = (const float*)(i + IL.final_T);
		ff.n_contrib = (const uint32_t*)(i + IL.n_contrib);
		ff.ctl = (const uint32_t*)(i + IL.bin_ctl);
		return ff;
	}

	hipError_t launch_blend_bwd(const fdgs_scene& s, const fdgs_backward_in& in, const fdgs_backward_out& out, const FinishedForward& ff,
	                            hipStream_t stream);

	// per-Gaussian contribution statistics and the per-pixel ID map of a finished forward (contribution.hip)
	hipError_t launch_contribution(const fdgs_contribution_in& in, const fdgs_contribution_out& out, const FinishedForward& ff, hipStream_t stream);

	// per-Gaussian feature channels blended with a finished forward's weights, and the adjoint (features.hip)
	hipError_t launch_feature_blend(const fdgs_feature_in& in, float* out, const FinishedForward& ff, hipStream_t stream);
	hipError_t launch_feature_blend_bwd(const fdgs_feature_in& in, const float* dL_dout, float* dL_dfeatures, const FinishedForward& ff,
	                                    hipStream_t stream);

	// SH / 4D-SH backward (coalesced); must run after the blend backward and before launch_preprocess_bwd
	hipError_t launch_sh_bwd(const fdgs_scene& s, const fdgs_backward_in& in, const fdgs_backward_out& out,
	                         const char* geom, hipStream_t stream);

	// SH backward (deferred mode: stage records + mean / time gradient) of several views in one pass over the coefficients
	hipError_t launch_sh_bwd_batch(int nviews, const fdgs_scene* const* views, const fdgs_backward_in* const* ins,
	                               const fdgs_backward_out* const* outs, hipStream_t stream);

	// once per optimizer step: dL_dsh from the staged per-view records of the deferred SH backward (sh_bwd.hip)
	hipError_t launch_sh_flush(int P, int D, int D_t, int M, int gaussian_dim, int force_sh_3d, int analytic, int nviews,
	                           const float* stages, float* dL_dsh, int accumulate, hipStream_t stream);

	// once per optimizer step, instead of launch_sh_flush + Adam over the SH segment: the summed SH gradient is built in LDS and
	// consumed by the Adam update in the same kernel (sh_bwd.hip); dL_dsh (optional) also receives it
	struct AdamScalars { float lr_head_bc1, lr_bc1, b1, b2, eps, inv_sqrt_bc2; };
	hipError_t launch_sh_adam(int P, int D, int D_t, int M, int gaussian_dim, int force_sh_3d, int analytic, int nviews,
	                          const float* stages, float* params, float* exp_avg, float* exp_avg_sq, float* dL_dsh,
	                          const AdamScalars& k, hipStream_t stream);

	hipError_t launch_preprocess_bwd(const fdgs_scene& s, const fdgs_backward_in& in, const fdgs_backward_out& out,
	                                 const char* geom, hipStream_t stream);

	// camera gradients (camera_bwd.hip): after the blend + SH backward, before launch_preprocess_bwd; grad_accum is only read
	size_t camera_bwd_scratch_bytes(int P);
	hipError_t launch_camera_bwd(const fdgs_scene& s, const fdgs_backward_in& in, const float* grad_accum, const fdgs_camera_grads& out,
	                             void* scratch, hipStream_t stream);

	hipError_t launch_mark_visible(int P, const float* means3D, const float* viewmatrix, uint8_t* present, hipStream_t stream);

	hipError_t launch_block_reaches_debug(int n, const float* tuples, uint8_t* out, hipStream_t stream);

	// One element of torch.optim.Adam (no amsgrad / weight decay; train.py:247-249), shared by adam.hip and the fused SH
	// update of sh_bwd.hip so that both round identically: explicit FMAs, independent of the translation unit's contraction mode.
	__device__ __forceinline__ void adam_update(float& p, float& m, float& v, float g, float lr_bc1, float b1, float b2, float eps,
	                                            float inv_sqrt_bc2)
	{
		m = fmaf(b1, m, (1.f - b1) * g);
		v = fmaf(b2, v, ((1.f - b2) * g) * g);
		const float denom = fmaf(sqrtf(v), inv_sqrt_bc2, eps);
		p = fmaf(-lr_bc1, m / denom, p);
	}

	// a 4D model at one timestamp as compact 3D Gaussians (time_slice.hip): flags + counts, scan, write + SH fold
	size_t time_slice_scratch_bytes(int P);
	hipError_t launch_time_slice(const fdgs_slice_in& in, const fdgs_slice_out& out, void* scratch, hipStream_t stream);
	hipError_t launch_model_transform(const fdgs_transform_in& in, const fdgs_transform_out& out, hipStream_t stream);

	hipError_t launch_activations(int P, const float* opacity_raw, const float* scales_raw, const float* scales_t_raw, const float* rot_raw,
	                              const float* rot_r_raw, float* opacity, float* scales, float* scales_t, float* rot, float* rot_r, hipStream_t stream);
}
