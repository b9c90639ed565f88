// sh_eval.h -- the spherical-harmonics evaluation that the forward colour (preprocess_fwd.hip: preprocess_fwd_kernel and
// colour_batch_kernel), the SH backward and its flush (sh_bwd.hip: sh_bwd_kernel, sh_bwd_batch_kernel, sh_flush_kernel) and the
// time slice (time_slice.hip) share, each piece ONCE:
//   the block plan (sh_plan) and the float4 flag of the launchers (sh_rows_vec_ok);
//   the time factors cos(2 pi k dt / T) and their dt derivative (sh_time_factor, sh_time_factor_dt);
//   the view direction (sh_view_dir), the basis tables (sh_tables, sh_values, sh_basis_4d);
//   the forward of one view: sh_colour_block per staged coefficient block, then sh_colour_finish (preprocess_fwd_kernel writes
//   sh_colour_block out, for its register budget: see there);
//   the backward of one view: the liveness test (sh_live), ShBwdEval::begin / block per staged block / finish, and the basis
//   of block 0 that multiplies dL_dRGB (sh_grad_basis0: Q1), which the flush uses as well;
//   the row walker of the staging loops (RowWalk).
// The kernels of a pair differ in how the coefficient rows get into LDS, and in nothing else.
//
// Every piece carries a quirk of the reference: Q1 dL_dsh[1] = l[0] * dRGB in the 4D path, Q2 the sign
// of d cos / dt, Q3 the last time block overwrites dRGB / dt, Q4 the backward's view direction comes from the SHIFTED mean
// (the forward's from the input mean); the truncated REF_PI and the double promotions of l[6] and of the time factors.
// fdgs_scene.analytic_sh_grad (opt-in) switches Q1-Q3 to the analytic gradient of the forward pass.
//
// The translation units that include this are built with -ffp-contract=off -fno-slp-vectorize: the kernels that share a
// function here make the same IEEE operations in the same order.
#pragma once
#pragma clang fp contract(off)
#include "fdgs_common.h"
#include "fdgs_math.h"

namespace fdgs
{
	// host: a row of M coefficients can move as float4s -- 3 M floats are whole float4s and every given pointer is 16-byte aligned
	template <typename... T>
	inline bool sh_rows_vec_ok(int M, const T*... ptr)
	{
		return (3 * M) % 4 == 0 && ((... | reinterpret_cast<uintptr_t>(ptr)) & 15) == 0;
	}

	// ---- time factor of coefficient block blk = 1, 2: cos(2 pi blk dt / T), evaluated in double as the reference writes it
	// (forward.cu:133-192) -- and its dt derivative as the backward has it: Q2, the sign of d cos / dt (backward.cu:303, 384);
	// analytic: d cos(u) / dt = -sin(u) du/dt ----
	__device__ __forceinline__ float sh_time_factor(int blk, float dir_t, float time_duration)
	{
		return (blk == 1) ? (float)cos(2 * REF_PI * dir_t / time_duration) : (float)cos(2 * REF_PI * dir_t * 2 / time_duration);
	}
	__device__ __forceinline__ float sh_time_factor_dt(int blk, float dir_t, float time_duration, bool analytic)
	{
		const float d = (blk == 1) ? (float)(sin(2 * REF_PI * dir_t / time_duration) * 2 * REF_PI / time_duration)
		                           : (float)(sin(2 * REF_PI * dir_t * 2 / time_duration) * 2 * REF_PI * 2 / time_duration);
		return analytic ? -d : d;
	}

	// ---- view direction: mean - campos and its normalisation.  Q4 is the caller's: the forward passes the UN-shifted input mean
	// (forward.cu:480-482), the backward the forward's SHIFTED out_means3D.  (dot3 is the sum x x + y y + z z left to right, which is
	// what the backward used to write out: one body serves both.) ----
	__device__ __forceinline__ float3 sh_view_dir(float3 mean, const float* __restrict__ campos, float3& dir_orig)
	{
		dir_orig = sub3(mean, ld3(campos, 0));
		const float len = sqrtf(dot3(dir_orig, dir_orig));
		return make_float3(dir_orig.x / len, dir_orig.y / len, dir_orig.z / len);
	}

	// ---- which coefficient blocks of a row are active ----
	// Block 0 = the plain SH sum over ncoef0 coefficients; blocks 1 / 2 = all 16 basis values times cos(2 pi k dt / T), k = 1, 2:
	// only the 4D path at degree 3 has them (forward.cu:133-192).
	struct ShPlan
	{
		bool sh3d;        // 3D SH: no time blocks, no double promotion, Q1 does not apply
		int ncoef0, nblocks;
		int act_floats;   // floats of a row the active degrees read and write
	};
	__host__ __device__ inline ShPlan sh_plan(int D, int D_t, int gaussian_dim, int force_sh_3d, int M)
	{
		ShPlan p;
		p.sh3d = (gaussian_dim == 3 || force_sh_3d);
		p.ncoef0 = min(16, (D + 1) * (D + 1));
		p.nblocks = (!p.sh3d && D > 2) ? 1 + min(max(D_t, 0), 2) : 1;
		p.act_floats = (p.nblocks - 1) * 48 + 3 * (p.nblocks > 1 ? 16 : p.ncoef0);   // (fdgs_scene validation: M holds them)
		(void)M;
		return p;
	}

	// ---- basis values and derivatives (forward.cu:87-131, backward.cu:172-263); entries the reference has no term for stay zero ----
	// promote: the 4D path's double promotion in l[6]
	__device__ __forceinline__ void sh_tables(int deg, float x, float y, float z, bool promote, float* l, float* dX, float* dY, float* dZ)
	{
#pragma unroll
		for (int k = 0; k < 16; k++) { l[k] = 0.f; dX[k] = 0.f; dY[k] = 0.f; dZ[k] = 0.f; }
		l[0] = SH_C0;
		if (deg > 0)
		{
			l[1] = -1 * SH_C1 * y; l[2] = SH_C1 * z; l[3] = -1 * SH_C1 * x;
			dY[1] = -1 * SH_C1; dZ[2] = SH_C1; dX[3] = -1 * SH_C1;
			if (deg > 1)
			{
				const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
				l[4] = SH_C2[0] * xy; l[5] = SH_C2[1] * yz;
				l[6] = promote ? (float)(SH_C2[2] * (2.0 * zz - xx - yy)) : SH_C2[2] * (2.f * zz - xx - yy);
				l[7] = SH_C2[3] * xz; l[8] = SH_C2[4] * (xx - yy);
				dX[4] = SH_C2[0] * y; dY[4] = SH_C2[0] * x;
				dY[5] = SH_C2[1] * z; dZ[5] = SH_C2[1] * y;
				dX[6] = -2 * SH_C2[2] * x; dY[6] = -2 * SH_C2[2] * y; dZ[6] = 4 * SH_C2[2] * z;
				dX[7] = SH_C2[3] * z; dZ[7] = SH_C2[3] * x;
				dX[8] = 2 * SH_C2[4] * x; dY[8] = -2 * SH_C2[4] * y;
				if (deg > 2)
				{
					l[9] = SH_C3[0] * y * (3 * xx - yy);
					l[10] = SH_C3[1] * xy * z;
					l[11] = SH_C3[2] * y * (4 * zz - xx - yy);
					l[12] = SH_C3[3] * z * (2 * zz - 3 * xx - 3 * yy);
					l[13] = SH_C3[4] * x * (4 * zz - xx - yy);
					l[14] = SH_C3[5] * z * (xx - yy);
					l[15] = SH_C3[6] * x * (xx - 3 * yy);
					dX[9] = SH_C3[0] * y * 6 * x;               dY[9] = SH_C3[0] * (3 * xx - 3 * yy);
					dX[10] = SH_C3[1] * yz;                     dY[10] = SH_C3[1] * xz;                     dZ[10] = SH_C3[1] * xy;
					dX[11] = -SH_C3[2] * y * 2 * x;             dY[11] = SH_C3[2] * (4 * zz - xx - 3 * yy);  dZ[11] = SH_C3[2] * y * 8 * z;
					dX[12] = -SH_C3[3] * z * 6 * x;             dY[12] = -SH_C3[3] * z * 6 * y;             dZ[12] = SH_C3[3] * (6 * zz - 3 * xx - 3 * yy);
					dX[13] = SH_C3[4] * (4 * zz - 3 * xx - yy);  dY[13] = -SH_C3[4] * x * 2 * y;             dZ[13] = SH_C3[4] * x * 8 * z;
					dX[14] = SH_C3[5] * z * 2 * x;              dY[14] = -SH_C3[5] * z * 2 * y;             dZ[14] = SH_C3[5] * (xx - yy);
					dX[15] = SH_C3[6] * (3 * xx - 3 * yy);      dY[15] = -SH_C3[6] * x * 6 * y;
				}
			}
		}
	}
	// basis values only (sh_tables without the derivative tables)
	__device__ __forceinline__ void sh_values(int deg, float x, float y, float z, bool promote, float* l)
	{
		float dX[16], dY[16], dZ[16];
		sh_tables(deg, x, y, z, promote, l, dX, dY, dZ);
	}

	// dL_dRGB of a Gaussian as the blend backward left it in words 0..2 of its accumulator record, clamped channels zeroed
	// (backward.cu:158-161)
	__device__ __forceinline__ float3 sh_colour_gradient(const float* gacc, const uint8_t* clamped, int idx)
	{
		const float4 w = *reinterpret_cast<const float4*>(gacc + (size_t)idx * GRAD_ACC_WORDS);
		float3 dRGB = make_float3(w.x, w.y, w.z);
		const uint8_t cl = clamped[idx];
		if (cl & 1) dRGB.x = 0.f;
		if (cl & 2) dRGB.y = 0.f;
		if (cl & 4) dRGB.z = 0.f;
		return dRGB;
	}
	// A Gaussian is LIVE in a view when it is visible (backward.cu:873) and a colour gradient is left after clamping: every output
	// of the SH backward is linear in dRGB, so the others only get their zeros.  The accumulator record is read only where visible.
	__device__ __forceinline__ bool sh_live(const int32_t* radii, const float* gacc, const uint8_t* clamped, int idx, float3& dRGB)
	{
		dRGB = make_float3(0.f, 0.f, 0.f);
		if (!(radii[idx] > 0)) return false;
		dRGB = sh_colour_gradient(gacc, clamped, idx);
		return dRGB.x != 0.f || dRGB.y != 0.f || dRGB.z != 0.f;
	}
	// the basis value that multiplies dRGB in dL_dsh for coefficient k of block 0 (lk = l[k], l0 = l[0]).  Q1: the 4D path of the
	// reference uses the degree-0 basis for coefficient 1 (backward.cu:190).  sh_bwd_kernel<false> and sh_flush_kernel have to make
	// the same additions: both ask here.
	__device__ __forceinline__ float sh_grad_basis0(int k, float lk, float l0, const ShPlan& plan, bool analytic)
	{
		return (k == 1 && !plan.sh3d && !analytic) ? l0 : lk;
	}

	// ------------------------------------------------------------------------------------------------
	// Forward: colour from the coefficient row, block by block
	// ------------------------------------------------------------------------------------------------
	// 3D SH (forward.cu:20-71); returns the un-clamped colour + 0.5.  The reference writes this path term by term, not from a
	// table: its evaluation order is kept as it is.
	__device__ inline float3 sh_color_3d(int deg, const float* __restrict__ sh, float3 dir)
	{
		float3 result = scl3(SH_C0, ld3(sh, 0));
		if (deg > 0)
		{
			const float x = dir.x, y = dir.y, z = dir.z;
			result = sub3(add3(sub3(result, scl3(SH_C1 * y, ld3(sh, 1))), scl3(SH_C1 * z, ld3(sh, 2))), scl3(SH_C1 * x, ld3(sh, 3)));
			if (deg > 1)
			{
				const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
				result = add3(result, scl3(SH_C2[0] * xy, ld3(sh, 4)));
				result = add3(result, scl3(SH_C2[1] * yz, ld3(sh, 5)));
				result = add3(result, scl3(SH_C2[2] * (2.0f * zz - xx - yy), ld3(sh, 6)));
				result = add3(result, scl3(SH_C2[3] * xz, ld3(sh, 7)));
				result = add3(result, scl3(SH_C2[4] * (xx - yy), ld3(sh, 8)));
				if (deg > 2)
				{
					result = add3(result, scl3(SH_C3[0] * y * (3.0f * xx - yy), ld3(sh, 9)));
					result = add3(result, scl3(SH_C3[1] * xy * z, ld3(sh, 10)));
					result = add3(result, scl3(SH_C3[2] * y * (4.0f * zz - xx - yy), ld3(sh, 11)));
					result = add3(result, scl3(SH_C3[3] * z * (2.0f * zz - 3.0f * xx - 3.0f * yy), ld3(sh, 12)));
					result = add3(result, scl3(SH_C3[4] * x * (4.0f * zz - xx - yy), ld3(sh, 13)));
					result = add3(result, scl3(SH_C3[5] * z * (xx - yy), ld3(sh, 14)));
					result = add3(result, scl3(SH_C3[6] * x * (xx - 3.0f * yy), ld3(sh, 15)));
				}
			}
		}
		return make_float3(result.x + 0.5f, result.y + 0.5f, result.z + 0.5f);
	}
	__device__ __forceinline__ float3 sh_weighted(const float* l, const float* __restrict__ sh, int lo, int hi, int off)
	{
		float3 acc = scl3(l[lo - off], ld3(sh, lo));
#pragma unroll
		for (int k = lo + 1; k <= hi; k++) acc = add3(acc, scl3(l[k - off], ld3(sh, k)));
		return acc;
	}
	// 4D SH (forward.cu:73-195), split by coefficient block so each block of 16 coefficients can be staged through
	// LDS on its own.  Evaluation order inside and across blocks is the reference's.
	__device__ __forceinline__ float3 sh4d_block0(int deg, const float* l, const float* __restrict__ sh)
	{
		float3 result = scl3(l[0], ld3(sh, 0));
		if (deg > 0)
		{
			result = add3(result, sh_weighted(l, sh, 1, 3, 0));
			if (deg > 1)
			{
				result = add3(result, sh_weighted(l, sh, 4, 8, 0));
				if (deg > 2) result = add3(result, sh_weighted(l, sh, 9, 15, 0));
			}
		}
		return result;
	}
	// basis values of the forward's 4D path (forward.cu:87-131): sh_values with promote, entries beyond the degree left unset
	// (sh4d_block0 does not read them; zeroing them as sh_tables does costs the forward kernels 15 registers)
	__device__ __forceinline__ void sh_basis_4d(int deg, float x, float y, float z, float* l)
	{
		l[0] = SH_C0;
		if (deg > 0)
		{
			l[1] = -1 * SH_C1 * y; l[2] = SH_C1 * z; l[3] = -1 * SH_C1 * x;
			if (deg > 1)
			{
				const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
				l[4] = SH_C2[0] * xy;
				l[5] = SH_C2[1] * yz;
				l[6] = (float)(SH_C2[2] * (2.0 * zz - xx - yy));
				l[7] = SH_C2[3] * xz;
				l[8] = SH_C2[4] * (xx - yy);
				if (deg > 2)
				{
					l[9] = SH_C3[0] * y * (3 * xx - yy);
					l[10] = SH_C3[1] * xy * z;
					l[11] = SH_C3[2] * y * (4 * zz - xx - yy);
					l[12] = SH_C3[3] * z * (2 * zz - 3 * xx - 3 * yy);
					l[13] = SH_C3[4] * x * (4 * zz - xx - yy);
					l[14] = SH_C3[5] * z * (xx - yy);
					l[15] = SH_C3[6] * x * (xx - 3 * yy);
				}
			}
		}
	}
	// One view's colour, a staged coefficient block at a time: c after block blk from c before it.  row: the block's 16 x 3 staged
	// floats; dir: sh_view_dir of the INPUT mean (Q4); l: sh_basis_4d(deg, dir) in the 4D path, not read in the 3D path.
	__device__ __forceinline__ float3 sh_colour_block(int blk, const ShPlan& plan, int deg, const float* l, const float* __restrict__ row,
	                                                  float3 dir, float dir_t, float time_duration, float3 c)
	{
		if (blk == 0) return plan.sh3d ? sh_color_3d(deg, row, dir) : sh4d_block0(deg, l, row);
		return add3(c, scl3(sh_time_factor(blk, dir_t, time_duration), sh_weighted(l, row, 0, 15, 0)));
	}
	// ... and after the last block: the + 0.5 (sh_color_3d has added it already), which channels are clamped, the clamped colour
	__device__ __forceinline__ float3 sh_colour_finish(const ShPlan& plan, float3 c, uint8_t& clampbits)
	{
		if (!plan.sh3d) c = make_float3(c.x + 0.5f, c.y + 0.5f, c.z + 0.5f);
		clampbits = (uint8_t)((c.x < 0 ? 1 : 0) | (c.y < 0 ? 2 : 0) | (c.z < 0 ? 4 : 0));
		return make_float3(fmaxf(c.x, 0.0f), fmaxf(c.y, 0.0f), fmaxf(c.z, 0.0f));
	}

	// ------------------------------------------------------------------------------------------------
	// Backward of one (Gaussian, view): begin, block for every staged coefficient block in order, finish
	// ------------------------------------------------------------------------------------------------
	__device__ __forceinline__ float3 sel3(bool c, float3 a, float3 b) { return make_float3(c ? a.x : b.x, c ? a.y : b.y, c ? a.z : b.z); }
	struct ShBwdEval
	{
		float3 dir_orig, dir, dRGB;
		float dir_t;
		float l[16], dX[16], dY[16], dZ[16];
		float3 gx, gy, gz, gt;   // d colour / d dir.x, .y, .z and / dt, channel by channel
		float tk_stage[2];       // cos factors of the two time blocks (deferred mode hands them to the flush)

		// mean: the forward's SHIFTED out_means3D (Q4); t: the Gaussian's ts (not read for 3D SH); dRGB_: sh_live's
		__device__ __forceinline__ void begin(const ShPlan& plan, int deg, float3 mean, const float* __restrict__ campos, float t, float timestamp,
		                                      float3 dRGB_)
		{
			dir = sh_view_dir(mean, campos, dir_orig);
			dRGB = dRGB_;
			dir_t = plan.sh3d ? 0.f : t - timestamp;
			sh_tables(deg, dir.x, dir.y, dir.z, !plan.sh3d, l, dX, dY, dZ);
			const float3 zero = make_float3(0.f, 0.f, 0.f);
			gx = zero; gy = zero; gz = zero; gt = zero;
			tk_stage[0] = 0.f; tk_stage[1] = 0.f;
		}
		// row: the nk x 3 staged coefficients of block blk.  WRITE_DSH: they are overwritten with this view's dL_dsh, basis x time
		// factor x dRGB (sh_bwd_kernel<false>)
		template <bool WRITE_DSH>
		__device__ __forceinline__ void block(const ShPlan& plan, bool analytic, float time_duration, float* row, int nk, int blk)
		{
			float tk = 1.f, dtk_dt = 0.f;
			if (blk > 0)
			{
				tk = sh_time_factor(blk, dir_t, time_duration);
				dtk_dt = sh_time_factor_dt(blk, dir_t, time_duration, analytic);
			}
			// (the members are assigned unconditionally, values selected: a store under a branch or a dynamic index sends the state to scratch)
			tk_stage[0] = (blk == 1) ? tk : tk_stage[0];
			tk_stage[1] = (blk == 2) ? tk : tk_stage[1];
			float3 st = make_float3(0.f, 0.f, 0.f), sx = st, sy = st, sz = st;
#pragma unroll
			for (int k = 0; k < 16; k++)   // fully unrolled: the tables stay in registers (no dynamic indexing)
			{
				if (k < nk)
				{
					const float3 s = ld3(row, k);
					if (WRITE_DSH) st3(row, k, scl3(blk == 0 ? sh_grad_basis0(k, l[k], l[0], plan, analytic) : tk * l[k], dRGB));
					st = add3(st, scl3(l[k], s));
					sx = add3(sx, scl3(dX[k], s));
					sy = add3(sy, scl3(dY[k], s));
					sz = add3(sz, scl3(dZ[k], s));
				}
			}
			const bool first = blk == 0;
			const float3 tx = add3(gx, scl3(tk, sx)), ty = add3(gy, scl3(tk, sy)), tz = add3(gz, scl3(tk, sz));
			const float3 tt = scl3(dtk_dt, st), at = add3(gt, tt);
			gx = sel3(first, sx, tx); gy = sel3(first, sy, ty); gz = sel3(first, sz, tz);
			gt = sel3(first, gt, sel3(analytic, at, tt)); // Q3: overwrite, not accumulate
		}
		// the two stage records -- what the flush needs to rebuild this view's contribution basis(dir) x time factor x dRGB to dL_dsh --
		// and words 12..15 of the accumulator record: the mean gradient through the view direction, the time gradient
		__device__ __forceinline__ float4 finish(const ShPlan& plan, float4& stage0, float4& stage1) const
		{
			stage0 = make_float4(dRGB.x, dRGB.y, dRGB.z, tk_stage[0]);
			stage1 = make_float4(dir.x, dir.y, dir.z, tk_stage[1]);
			const float3 dmean = dnormvdv(dir_orig, make_float3(dot3(gx, dRGB), dot3(gy, dRGB), dot3(gz, dRGB)));
			return make_float4(dmean.x, dmean.y, dmean.z, plan.sh3d ? 0.f : dot3(gt, dRGB));
		}
	};

	// ------------------------------------------------------------------------------------------------
	// Moving rows between memory and a wave-private LDS tile
	// ------------------------------------------------------------------------------------------------
	// A wave walks `rows` x rc elements linearly, element e = lane, lane + 64, ... = (row g, position q of the row)
	struct RowWalk
	{
		int g, q, dg, dq, rc;
		__device__ __forceinline__ RowWalk(int lane, int rc_) : g(lane / rc_), q(lane - (lane / rc_) * rc_), dg(WAVE / rc_), dq(WAVE - (WAVE / rc_) * rc_), rc(rc_) {}
		__device__ __forceinline__ void step() { g += dg; q += dq; if (q >= rc) { q -= rc; g++; } }
	};
}
