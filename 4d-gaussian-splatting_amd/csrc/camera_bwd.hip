// camera_bwd.hip -- gradient of the loss with respect to the CAMERA of a view (gfx950): dL/dviewmatrix [4,4], dL/dprojmatrix [4,4],
// dL/dcampos [3] and dL/dtimestamp [1], 36 sums over the P Gaussians of the view.
//
// Runs between the two halves of the backward (fdgs_backward_out.stage_mask 1, then this, then 2): the blend + SH backward have left
// every Gaussian's conic gradient, pixel-position moments, depth carrier, opacity and colour gradient in words 0-11 of its accumulator
// record, the geometry backward has not consumed (and, with grad_accum_clean, re-zeroed) them yet.  The record is only READ here.
//
// What is differentiated is the forward as it computes, with every discrete decision held constant (culls,
// radii, tile lists, n_contrib, the alpha and T cut-offs) -- NOT the reference backward's quirks Q1-Q7: the camera is no parameter of
// the reference, there is nothing to be bug-compatible with.
//   viewmatrix  <- t = (mean, 1) V[:, 0:3]   (EWA Jacobian J(t), the depth carrier)   and   W = V[0:3, 0:3]^T in T = J W
//   projmatrix  <- p_hom.x, .y, .w -> pixel position                                   (the depth column gets nothing)
//   campos      <- the SH view direction, from the UN-shifted input mean (Q4: what the forward uses)
//   timestamp   <- the temporal marginal; rot_4d: the conditional mean shift c12 / cov_t * dt (moves t and p_hom);
//                  4D SH: the time factors cos(2 pi k (ts - timestamp) / T)
// On a lane clamped at 1.3 tanfov the forward has tx = lim * tz: J02 = -fx lim / tz there, so dJ02/dtx = 0 and
// dJ02/dtz = fx lim / tz^2 = fx tx / tz^3 -- half of the unclamped 2 fx tx / tz^3.
//
// No atomics, bitwise reproducible: one lane per Gaussian (culled: zeros), a fixed-order wave reduction, the four waves of a block
// summed in order through LDS -> partials[block][36]; a second, single-block kernel sums the partials in fixed order in double.
// The geometry sums (24 live values) are reduced before the colour / time part starts, so the two halves' registers do not add up.
#pragma clang fp contract(off)
#include "fdgs_common.h"
#include "fdgs_math.h"
#include "sh_eval.h"

namespace fdgs
{
	constexpr int CAM_SUMS = 36;       // viewmatrix 0-15, projmatrix 16-31, campos 32-34, timestamp 35
	constexpr int CAM_THREADS = 256;
	constexpr int CAM_WAVES = CAM_THREADS / WAVE;
	constexpr int CAM_FIN_GROUPS = 7;  // the finish kernel: 7 x 36 = 252 lanes, group g takes the blocks g, g + 7, ...

	struct CamArgs
	{
		int P, D, D_t, M;
		const float *means_in, *shs, *ts, *scales, *scales_t, *rotations, *rotations_r, *cov3D_precomp;
		const float *viewmatrix, *projmatrix, *campos;
		float scale_modifier, prefilter_var, tan_fovx, tan_fovy, focal_x, focal_y, timestamp, time_duration, half_w, half_h;
		int rot_4d, gaussian_dim, force_sh_3d, raw;
		const int32_t* radii; const float* means; /* out_means3D */
		const float* cov3D; const uint8_t* clamped; const float* gacc; const float4* records;
		float* partials;
	};

	// sum over the 64 lanes, in lane 0; the same tree whatever the values: reproducible
	__device__ __forceinline__ float cam_wave_sum(float v)
	{
#pragma unroll
		for (int off = WAVE / 2; off > 0; off >>= 1) v += __shfl_down(v, off, WAVE);
		return v;
	}

	__global__ void __launch_bounds__(CAM_THREADS) camera_bwd_kernel(const CamArgs a)
	{
		__shared__ float red[CAM_WAVES][CAM_SUMS];
		const int idx = blockIdx.x * CAM_THREADS + threadIdx.x;
		const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
		if (threadIdx.x < CAM_WAVES * CAM_SUMS) (&red[0][0])[threadIdx.x] = 0.f;   // the structurally zero entries stay exactly 0
		__syncthreads();
		const bool visible = idx < a.P && a.radii[idx] > 0;
		float dts = 0.f;

		// ---------------- geometry: viewmatrix and projmatrix, the timestamp through marginal and mean shift ----------------
		{
			float dvm[4][3], dpm[4][3];   // [row][column]; the projection's columns 0, 1, 3
#pragma unroll
			for (int r = 0; r < 4; r++)
#pragma unroll
				for (int j = 0; j < 3; j++) { dvm[r][j] = 0.f; dpm[r][j] = 0.f; }
			if (visible)
			{
				const float4* rec = reinterpret_cast<const float4*>(a.gacc + (size_t)idx * GRAD_ACC_WORDS);
				const float4 r0 = rec[0], r1 = rec[1], r2 = rec[2];
				const float4 ra = a.records[3 * (size_t)idx + 0], rb = a.records[3 * (size_t)idx + 1];
				const float cA = ra.z, cB = ra.w, cC = rb.x, o_eff = rb.y;
				// the record's moments of q = G dL/dalpha (blend_bwd.hip) -> dL/d(NDC position), dL/dconic (A, B, C), dL/d(effective opacity)
				const float gx = -o_eff * a.half_w * (cA * r1.z + cB * r1.w);
				const float gy = -o_eff * a.half_h * (cB * r1.z + cC * r1.w);
				const float gA = -0.5f * o_eff * r2.x, gB = -o_eff * r2.z, gC = -0.5f * o_eff * r2.y;
				const float g_depth = r0.w, g_op = r2.w;
				const float3 mean = ld3(a.means, idx);
				const float hom[4] = { mean.x, mean.y, mean.z, 1.0f };
				const float* m = a.viewmatrix;
				const float* pm = a.projmatrix;
				const float t0 = m[0] * mean.x + m[4] * mean.y + m[8] * mean.z + m[12];
				const float t1 = m[1] * mean.x + m[5] * mean.y + m[9] * mean.z + m[13];
				const float tz = m[2] * mean.x + m[6] * mean.y + m[10] * mean.z + m[14];
				const float limx = 1.3f * a.tan_fovx, limy = 1.3f * a.tan_fovy;
				const float txtz = t0 / tz, tytz = t1 / tz;
				const bool clx = txtz < -limx || txtz > limx, cly = tytz < -limy || tytz > limy;
				const float tx = fminf(limx, fmaxf(-limx, txtz)) * tz, ty = fminf(limy, fmaxf(-limy, tytz)) * tz;
				const float itz = 1.0f / tz, itz2 = itz * itz, itz3 = itz2 * itz;
				const float J00 = a.focal_x * itz, J02 = -(a.focal_x * tx) * itz2, J11 = a.focal_y * itz, J12 = -(a.focal_y * ty) * itz2;
				const float* c3 = (a.cov3D_precomp ? a.cov3D_precomp : a.cov3D) + 6 * (size_t)idx;
				const float S[3][3] = { { c3[0], c3[1], c3[2] }, { c3[1], c3[3], c3[4] }, { c3[2], c3[4], c3[5] } };
				// A = J W (2 x 3), cov2D = A Sigma A^T
				float A0[3], A1[3], AS0[3], AS1[3];
#pragma unroll
				for (int r = 0; r < 3; r++) { A0[r] = J00 * m[4 * r] + J02 * m[4 * r + 2]; A1[r] = J11 * m[4 * r + 1] + J12 * m[4 * r + 2]; }
#pragma unroll
				for (int s = 0; s < 3; s++)
				{
					AS0[s] = A0[0] * S[0][s] + A0[1] * S[1][s] + A0[2] * S[2][s];
					AS1[s] = A1[0] * S[0][s] + A1[1] * S[1][s] + A1[2] * S[2][s];
				}
				const float ca = (AS0[0] * A0[0] + AS0[1] * A0[1] + AS0[2] * A0[2]) + 0.3f;
				const float cb = AS0[0] * A1[0] + AS0[1] * A1[1] + AS0[2] * A1[2];
				const float cc = (AS1[0] * A1[0] + AS1[1] * A1[1] + AS1[2] * A1[2]) + 0.3f;
				const float det = ca * cc - cb * cb;
				const float inv2 = 1.0f / (det * det);
				// conic = (cc, -cb, ca) / det
				const float dLa = inv2 * (-cc * cc * gA + cb * cc * gB - cb * cb * gC);
				const float dLb = inv2 * (2.f * cb * cc * gA - (det + 2.f * cb * cb) * gB + 2.f * ca * cb * gC);
				const float dLc = inv2 * (-cb * cb * gA + ca * cb * gB - ca * ca * gC);
				float D0[3], D1[3];   // dL/dA
#pragma unroll
				for (int r = 0; r < 3; r++) { D0[r] = 2.f * dLa * AS0[r] + dLb * AS1[r]; D1[r] = dLb * AS0[r] + 2.f * dLc * AS1[r]; }
				const float gJ00 = D0[0] * m[0] + D0[1] * m[4] + D0[2] * m[8];
				const float gJ02 = D0[0] * m[2] + D0[1] * m[6] + D0[2] * m[10];
				const float gJ11 = D1[0] * m[1] + D1[1] * m[5] + D1[2] * m[9];
				const float gJ12 = D1[0] * m[2] + D1[1] * m[6] + D1[2] * m[10];
				// J(t): a clamped lane has tx = lim tz (see the header comment)
				float dt[3];
				dt[0] = clx ? 0.f : -a.focal_x * itz2 * gJ02;
				dt[1] = cly ? 0.f : -a.focal_y * itz2 * gJ12;
				dt[2] = -a.focal_x * itz2 * gJ00 - a.focal_y * itz2 * gJ11 + (clx ? 1.f : 2.f) * (a.focal_x * tx) * itz3 * gJ02
				        + (cly ? 1.f : 2.f) * (a.focal_y * ty) * itz3 * gJ12 + g_depth;
				// pixel position: p_hom = (mean, 1) P, pix = ((p_hom.xy / (p_hom.w + 1e-7) + 1) (W, H) - 1) / 2
				const float ph0 = pm[0] * mean.x + pm[4] * mean.y + pm[8] * mean.z + pm[12];
				const float ph1 = pm[1] * mean.x + pm[5] * mean.y + pm[9] * mean.z + pm[13];
				const float ph3 = pm[3] * mean.x + pm[7] * mean.y + pm[11] * mean.z + pm[15];
				const float pw = 1.0f / (ph3 + 0.0000001f);
				float dph[3];
				dph[0] = gx * pw; dph[1] = gy * pw; dph[2] = -(gx * ph0 + gy * ph1) * pw * pw;
#pragma unroll
				for (int r = 0; r < 4; r++)
#pragma unroll
					for (int j = 0; j < 3; j++) { dvm[r][j] = hom[r] * dt[j]; dpm[r][j] = hom[r] * dph[j]; }
				// the rotation block W in T = J W
#pragma unroll
				for (int r = 0; r < 3; r++) { dvm[r][0] += D0[r] * J00; dvm[r][1] += D1[r] * J11; dvm[r][2] += D0[r] * J02 + D1[r] * J12; }

				if (a.cov3D_precomp == nullptr && a.gaussian_dim == 4)
				{
					if (a.rot_4d)
					{
						float3 sc = ld3(a.scales, idx);
						float sct = a.scales_t[idx];
						float4 q = reinterpret_cast<const float4*>(a.rotations)[idx], qr = reinterpret_cast<const float4*>(a.rotations_r)[idx];
						float unused;
						if (a.raw) { activate(sc, q, &unused); activate(sct, qr, &unused); }
						const M4 Sigma = cov4_build(sc, sct, a.scale_modifier, q, qr).Sigma;
						const float cov_t = Sigma.c[3][3];
						const float dtime = a.timestamp - a.ts[idx];
						// marginal = exp(-dt^2 / 2 var): d/d timestamp = -marginal dt / var; the effective opacity is opacity * marginal
						dts += g_op * o_eff * (-dtime / prefiltered_var(cov_t, a.prefilter_var));
						// mean = p + c12 / cov_t * dt: d mean / d timestamp = c12 / cov_t
#pragma unroll
						for (int r = 0; r < 3; r++)
						{
							const float dmean = (m[4 * r] * dt[0] + m[4 * r + 1] * dt[1] + m[4 * r + 2] * dt[2])
							                    + (pm[4 * r] * dph[0] + pm[4 * r + 1] * dph[1] + pm[4 * r + 3] * dph[2]);
							dts += dmean * (Sigma.c[r][3] / cov_t);
						}
					}
					else
					{
						const float dtime = a.ts[idx] - a.timestamp;   // (the other sign: as the forward has it)
						const float sigma = (a.raw ? expf(a.scales_t[idx]) : a.scales_t[idx]) * a.scale_modifier;
						dts += g_op * o_eff * (dtime / prefiltered_var(sigma, a.prefilter_var));
					}
				}
			}
#pragma unroll
			for (int r = 0; r < 4; r++)
#pragma unroll
				for (int j = 0; j < 3; j++)
				{
					const float sv = cam_wave_sum(dvm[r][j]), sp = cam_wave_sum(dpm[r][j]);
					if (lane == 0) { red[wave][4 * r + j] = sv; red[wave][16 + 4 * r + (j == 2 ? 3 : j)] = sp; }
				}
		}

		// ---------------- colour: campos through the SH view direction, the timestamp through the 4D-SH time factors ----------------
		{
			float3 dcam = make_float3(0.f, 0.f, 0.f);
			if (visible && a.shs)
			{
				const float3 dRGB = sh_colour_gradient(a.gacc, a.clamped, idx);
				const ShPlan plan = sh_plan(a.D, a.D_t, a.gaussian_dim, a.force_sh_3d, a.M);
				const float3 v = sub3(ld3(a.means_in, idx), ld3(a.campos, 0));   // Q4: the un-shifted mean
				const float inv = 1.0f / sqrtf(dot3(v, v));
				const float3 d = scl3(inv, v);
				float l[16], dX[16], dY[16], dZ[16];
				sh_tables(a.D, d.x, d.y, d.z, false, l, dX, dY, dZ);
				const float* sh = a.shs + (size_t)idx * a.M * 3;
				float3 dd = make_float3(0.f, 0.f, 0.f);   // dL/d(unit direction)
				for (int b = 0; b < plan.nblocks; b++)
				{
					const int n = b == 0 ? plan.ncoef0 : 16;
					float val = 0.f;
					float3 g = make_float3(0.f, 0.f, 0.f);
#pragma unroll
					for (int k = 0; k < 16; k++)
					{
						if (k < n)
						{
							const float w = dot3(dRGB, ld3(sh, 16 * b + k));
							val += l[k] * w; g.x += dX[k] * w; g.y += dY[k] * w; g.z += dZ[k] * w;
						}
					}
					float ck = 1.f;
					if (b > 0)
					{
						// colour += cos(2 pi b (ts - timestamp) / T) * block b: d/d timestamp = +sin(.) 2 pi b / T
						const float wq = (float)(2.0 * REF_PI) * (float)b / a.time_duration;
						const float ang = wq * (a.ts[idx] - a.timestamp);
						ck = cosf(ang);
						dts += val * sinf(ang) * wq;
					}
					dd.x += ck * g.x; dd.y += ck * g.y; dd.z += ck * g.z;
				}
				// d (v / |v|): (I - d d^T) / |v|; campos enters as -v
				const float along = dot3(d, dd);
				dcam = make_float3(-(dd.x - d.x * along) * inv, -(dd.y - d.y * along) * inv, -(dd.z - d.z * along) * inv);
			}
			const float s0 = cam_wave_sum(dcam.x), s1 = cam_wave_sum(dcam.y), s2 = cam_wave_sum(dcam.z), s3 = cam_wave_sum(dts);
			if (lane == 0) { red[wave][32] = s0; red[wave][33] = s1; red[wave][34] = s2; red[wave][35] = s3; }
		}
		__syncthreads();
		if (threadIdx.x < CAM_SUMS)
		{
			float s = red[0][threadIdx.x];
#pragma unroll
			for (int w = 1; w < CAM_WAVES; w++) s += red[w][threadIdx.x];
			a.partials[(size_t)blockIdx.x * CAM_SUMS + threadIdx.x] = s;
		}
	}

	struct CamOut { float *vm, *pm, *campos, *ts; float scale; int accumulate; };

	// one block: partials [nblocks][36] -> the 36 outputs, summed in fixed order in double
	__global__ void __launch_bounds__(CAM_THREADS) camera_finish_kernel(const float* __restrict__ partials, const int nblocks, const CamOut o)
	{
		__shared__ double red[CAM_FIN_GROUPS][CAM_SUMS];
		const int tid = threadIdx.x, col = tid % CAM_SUMS, grp = tid / CAM_SUMS;
		if (grp < CAM_FIN_GROUPS)
		{
			double s = 0.0;
			for (int b = grp; b < nblocks; b += CAM_FIN_GROUPS) s += (double)partials[(size_t)b * CAM_SUMS + col];
			red[grp][col] = s;
		}
		__syncthreads();
		if (tid >= CAM_SUMS) return;
		double s = red[0][tid];
#pragma unroll
		for (int g = 1; g < CAM_FIN_GROUPS; g++) s += red[g][tid];
		float* dst = tid < 16 ? (o.vm ? o.vm + tid : nullptr) : tid < 32 ? (o.pm ? o.pm + (tid - 16) : nullptr)
		             : tid < 35 ? (o.campos ? o.campos + (tid - 32) : nullptr) : o.ts;
		if (dst == nullptr) return;
		const float v = (float)s * o.scale;
		*dst = o.accumulate ? *dst + v : v;
	}

	size_t camera_bwd_scratch_bytes(int P) { return align_up((size_t)(P > 0 ? div_up(P, CAM_THREADS) : 1) * CAM_SUMS * sizeof(float)); }

	hipError_t launch_camera_bwd(const fdgs_scene& s, const fdgs_backward_in& in, const float* grad_accum, const fdgs_camera_grads& out,
	                             void* scratch, hipStream_t stream)
	{
		const int nblocks = s.P > 0 ? div_up(s.P, CAM_THREADS) : 0;
		float* partials = reinterpret_cast<float*>(scratch);
		if (nblocks > 0)
		{
			const GeomLayout L = geom_layout(s.P);
			const char* geom = reinterpret_cast<const char*>(in.geom_buffer);
			CamArgs a;
			a.P = s.P; a.D = s.D; a.D_t = s.D_t; a.M = s.M;
			a.means_in = s.means3D; a.shs = s.shs; a.ts = s.ts; a.scales = s.scales; a.scales_t = s.scales_t;
			a.rotations = s.rotations; a.rotations_r = s.rotations_r; a.cov3D_precomp = s.cov3D_precomp;
			a.viewmatrix = s.viewmatrix; a.projmatrix = s.projmatrix; a.campos = s.campos;
			a.scale_modifier = s.scale_modifier; a.prefilter_var = s.prefilter_var;
			a.tan_fovx = s.tan_fovx; a.tan_fovy = s.tan_fovy;
			a.focal_y = s.H / (2.0f * s.tan_fovy); a.focal_x = s.W / (2.0f * s.tan_fovx);
			a.timestamp = s.timestamp; a.time_duration = s.time_duration;
			a.half_w = 0.5f * s.W; a.half_h = 0.5f * s.H;
			a.rot_4d = s.rot_4d; a.gaussian_dim = s.gaussian_dim; a.force_sh_3d = s.force_sh_3d; a.raw = s.raw_params;
			a.radii = in.radii; a.means = in.out_means3D;
			a.cov3D = reinterpret_cast<const float*>(geom + L.cov3D);
			a.clamped = reinterpret_cast<const uint8_t*>(geom + L.clamped);
			a.gacc = grad_accum;
			a.records = reinterpret_cast<const float4*>(geom + L.records);
			a.partials = partials;
			hipLaunchKernelGGL(camera_bwd_kernel, dim3(nblocks), dim3(CAM_THREADS), 0, stream, a);
			const hipError_t e = hipGetLastError();
			if (e != hipSuccess) return e;
		}
		const CamOut o{ out.dL_dviewmatrix, out.dL_dprojmatrix, out.dL_dcampos, out.dL_dtimestamp, out.scale, out.accumulate };
		hipLaunchKernelGGL(camera_finish_kernel, dim3(1), dim3(CAM_THREADS), 0, stream, partials, nblocks, o);
		return hipGetLastError();
	}
}
