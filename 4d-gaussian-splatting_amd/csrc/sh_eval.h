// sh_eval.h -- the spherical-harmonics pieces that the forward colour (preprocess_fwd.hip) and the SH backward and its flush
// (sh_bwd.hip) share, each ONCE: the block plan, the basis tables, the forward's block sums, the colour
// gradient and the row walker.
//
// Every piece carries a quirk of the reference: Q1 dL_dsh[1] = l[0] * dRGB in the 4D path, Q2 the sign
// of d cos / dt, Q3 the last time block overwrites dRGB / dt, Q4 the backward's view direction comes from the SHIFTED mean
// (the forward's from the input mean); the truncated REF_PI and the double promotions of l[6] and of the time factors.
// fdgs_scene.analytic_sh_grad (opt-in) switches Q1-Q3 to the analytic gradient of the forward pass.
//
// The two translation units that include this are built with -ffp-contract=off -fno-slp-vectorize: the kernels that share a
// function here make the same IEEE operations in the same order.
#pragma once
#pragma clang fp contract(off)
#include "fdgs_common.h"
#include "fdgs_math.h"

namespace fdgs
{
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
