// flow.hip -- per-Gaussian screen motion between two views (fdgs_gaussian_flow_forward / _backward) for gfx950.
//
//   flow_i = pix(mu_i(timestamp_to); target camera) - pix(mu_i(timestamp); source camera)
// mu_i(t): the mean as the forward preprocess has it at time t -- with rot_4d gaussian_at_time's conditional mean
// p + Sigma[0:3,3] / Sigma[3,3] * (t - t_i) from the same cov4_build call (fdgs_math.h), otherwise the plain mean; pix: the
// preprocess's own mean -> pixel expressions (pre_geometry: xform4x4, 1 / (w + 1e-7f), the double-promoted ndc2Pix).  Both ends go
// through ONE device function (flow_end), so equal timestamps and one camera give exactly (0, 0), and where the forward keeps a
// Gaussian in both views the flow is the difference of its two blend records' positions bit for bit (tests/test_gpu_flow.py).
// A Gaussian whose view-space z <= 0.2 at either end (the forward's near cull) has flow (0, 0) and no gradient.  The temporal cull
// is not applied: the rasterizer never reads those rows.
//
// One launch each, one lane per Gaussian, no atomics: forward and backward are bitwise reproducible.  The forward moves about 72
// bytes per Gaussian (17 floats in, 2 out): it is bound by the launch up to a few hundred thousand Gaussians.
// The backward is the analytic gradient of the forward as written (the cameras are constants):
//   g_j = J_pix(mu_j)^T (+-dL_dflow)      d p = g_0 + g_1      d w = g_0 (t_0 - t_i) + g_1 (t_1 - t_i)      d t_i = -w . (g_0 + g_1)
//   w = c / c_t, c = Sigma[0:3,3], c_t = Sigma[3,3]:   d c = d w / c_t,   d c_t = -(d w . c) / c_t^2
// then cov4_backward with a dSigma that is non-zero in the time row and column only, the scale modifier (cov4_backward differentiates
// with respect to modifier * scale) and, for raw parameters, exp and act_normalize_bwd.
// Built with FP contraction off and without the SLP vectorizer, as preprocess_fwd.hip: the means must be the forward's bits.
#pragma clang fp contract(off)
#include "fdgs_common.h"
#include "fdgs_math.h"

namespace fdgs
{
	constexpr int FLOW_THREADS = 256;

	struct FlowArgs
	{
		int P, W, H;
		const float *means3D, *ts, *scales, *scales_t, *rotations, *rotations_r;
		const float *vm0, *pm0, *vm1, *pm1;   // source and target camera (the same pointers: one camera)
		float t0, t1, mod;
		int rot_4d, raw;
		float* flows;
		const float* dL_dflows; float scale;
		float *d_means3D, *d_ts, *d_scales, *d_scales_t, *d_rotations, *d_rotations_r;
	};

	// What the kernels need of one Gaussian: the mean and, with rot_4d, the 4D covariance the forward builds and the velocity
	// w = Sigma[0:3,3] / Sigma[3,3] (the quotient gaussian_at_time multiplies by dt)
	struct FlowGauss { float3 p; Cov4 c; float3 sc; float sct; float4 q, qr; float inv_q, inv_qr; float ti; float3 w; };

	__device__ __forceinline__ void flow_gauss(const FlowArgs& a, const size_t i, FlowGauss& g)
	{
		g.p = ld3(a.means3D, i);
		g.w = make_float3(0.f, 0.f, 0.f);
		g.ti = 0.f; g.inv_q = 1.f; g.inv_qr = 1.f;
		if (a.rot_4d)
		{
			g.sc = ld3(a.scales, i);
			g.sct = a.scales_t[i];
			// scalar loads: a slice of a flat parameter bucket need not be 16-byte aligned
			g.q = make_float4(a.rotations[4 * i], a.rotations[4 * i + 1], a.rotations[4 * i + 2], a.rotations[4 * i + 3]);
			g.qr = make_float4(a.rotations_r[4 * i], a.rotations_r[4 * i + 1], a.rotations_r[4 * i + 2], a.rotations_r[4 * i + 3]);
			if (a.raw) { activate(g.sc, g.q, &g.inv_q); activate(g.sct, g.qr, &g.inv_qr); }
			g.ti = a.ts[i];
			g.c = cov4_build(g.sc, g.sct, a.mod, g.q, g.qr);
			const float cov_t = g.c.Sigma.c[3][3];
			g.w = make_float3(g.c.Sigma.c[0][3] / cov_t, g.c.Sigma.c[1][3] / cov_t, g.c.Sigma.c[2][3] / cov_t);
		}
	}
	// gaussian_at_time's mean at `timestamp`: p + c12 / cov_t * dt, dt = timestamp - t_i
	__device__ __forceinline__ float3 flow_mean(const FlowArgs& a, const FlowGauss& g, const float timestamp)
	{
		float3 m = g.p;
		if (a.rot_4d)
		{
			const float dt = timestamp - g.ti;
			m.x += g.w.x * dt; m.y += g.w.y * dt; m.z += g.w.z * dt;
		}
		return m;
	}

	// One end of the flow: the near cull and the pixel position of pre_geometry (preprocess_fwd.hip), expression for expression
	struct FlowEnd { bool ok; float2 pix; float hx, hy, pw; };
	__device__ __forceinline__ FlowEnd flow_end(const float3 mean, const float* __restrict__ viewmatrix, const float* __restrict__ projmatrix,
	                                            const int W, const int H)
	{
		FlowEnd e;
		const float3 p_view = xform4x3(mean, viewmatrix);
		e.ok = !(p_view.z <= 0.2f);
		const float4 p_hom = xform4x4(mean, projmatrix);
		const float p_w = 1.0f / (p_hom.w + 0.0000001f);
		const float p_proj_x = p_hom.x * p_w, p_proj_y = p_hom.y * p_w;
		e.pix.x = (float)(((p_proj_x + 1.0) * W - 1.0) * 0.5);
		e.pix.y = (float)(((p_proj_y + 1.0) * H - 1.0) * 0.5);
		e.hx = p_hom.x; e.hy = p_hom.y; e.pw = p_w;
		return e;
	}
	// J_pix(mean)^T (gx, gy):  pix.x = ((hx pw + 1) W - 1) / 2,  pw = 1 / (hw + 1e-7),  h = proj * (mean, 1)
	__device__ __forceinline__ float3 flow_end_bwd(const FlowEnd& e, const float* __restrict__ m, const int W, const int H, const float gx, const float gy)
	{
		const float ax = gx * (0.5f * (float)W) * e.pw, ay = gy * (0.5f * (float)H) * e.pw;   // d L / d hx, d L / d hy
		const float aw = -(ax * e.hx + ay * e.hy) * e.pw;                                       // d L / d hw
		return make_float3(ax * m[0] + ay * m[1] + aw * m[3], ax * m[4] + ay * m[5] + aw * m[7], ax * m[8] + ay * m[9] + aw * m[11]);
	}

	__global__ void __launch_bounds__(FLOW_THREADS) flow_forward_kernel(const FlowArgs a)
	{
		const int tid = blockIdx.x * FLOW_THREADS + threadIdx.x;
		if (tid >= a.P) return;
		const size_t i = (size_t)tid;
		FlowGauss g;
		flow_gauss(a, i, g);
		const FlowEnd e0 = flow_end(flow_mean(a, g, a.t0), a.vm0, a.pm0, a.W, a.H);
		const FlowEnd e1 = flow_end(flow_mean(a, g, a.t1), a.vm1, a.pm1, a.W, a.H);
		const bool ok = e0.ok && e1.ok;
		a.flows[2 * i] = ok ? e1.pix.x - e0.pix.x : 0.f;
		a.flows[2 * i + 1] = ok ? e1.pix.y - e0.pix.y : 0.f;
	}

	__global__ void __launch_bounds__(FLOW_THREADS) flow_backward_kernel(const FlowArgs a)
	{
		const int tid = blockIdx.x * FLOW_THREADS + threadIdx.x;
		if (tid >= a.P) return;
		const size_t i = (size_t)tid;
		FlowGauss g;
		flow_gauss(a, i, g);
		const FlowEnd e0 = flow_end(flow_mean(a, g, a.t0), a.vm0, a.pm0, a.W, a.H);
		const FlowEnd e1 = flow_end(flow_mean(a, g, a.t1), a.vm1, a.pm1, a.W, a.H);
		if (!(e0.ok && e1.ok)) return;   // the flow is the constant (0, 0): nothing to add
		const float gx = a.scale * a.dL_dflows[2 * i], gy = a.scale * a.dL_dflows[2 * i + 1];
		const float3 g0 = flow_end_bwd(e0, a.pm0, a.W, a.H, -gx, -gy);
		const float3 g1 = flow_end_bwd(e1, a.pm1, a.W, a.H, gx, gy);
		const float3 gp = add3(g0, g1);
		if (a.d_means3D) { float* o = a.d_means3D + 3 * i; o[0] += gp.x; o[1] += gp.y; o[2] += gp.z; }
		if (!a.rot_4d) return;

		const float dt0 = a.t0 - g.ti, dt1 = a.t1 - g.ti;
		if (a.d_ts) a.d_ts[i] += -dot3(g.w, gp);
		if (!a.d_scales && !a.d_scales_t && !a.d_rotations && !a.d_rotations_r) return;
		const float dw[3] = { g0.x * dt0 + g1.x * dt1, g0.y * dt0 + g1.y * dt1, g0.z * dt0 + g1.z * dt1 };
		const float ct = g.c.Sigma.c[3][3];
		const float c12[3] = { g.c.Sigma.c[0][3], g.c.Sigma.c[1][3], g.c.Sigma.c[2][3] };
		const float ddot = dw[0] * c12[0] + dw[1] * c12[1] + dw[2] * c12[2];
		M4 dSig;
#pragma unroll
		for (int j = 0; j < 4; j++)
#pragma unroll
			for (int r = 0; r < 4; r++) dSig.c[j][r] = 0.f;
#pragma unroll
		for (int r = 0; r < 3; r++) { const float d = 0.5f * (dw[r] / ct); dSig.c[r][3] = d; dSig.c[3][r] = d; }
		dSig.c[3][3] = -ddot / (ct * ct);
		float3 dscale;
		float dscale_t;
		float4 drot, drot_r;
		cov4_backward(g.c, dSig, dscale, dscale_t, drot, drot_r);
		dscale = scl3(a.mod, dscale); dscale_t *= a.mod;   // cov4_backward: with respect to modifier * scale
		if (a.raw)
		{
			dscale.x *= g.sc.x; dscale.y *= g.sc.y; dscale.z *= g.sc.z; dscale_t *= g.sct;   // d exp
			drot = act_normalize_bwd(g.q, g.inv_q, drot);
			drot_r = act_normalize_bwd(g.qr, g.inv_qr, drot_r);
		}
		if (a.d_scales) { float* o = a.d_scales + 3 * i; o[0] += dscale.x; o[1] += dscale.y; o[2] += dscale.z; }
		if (a.d_scales_t) a.d_scales_t[i] += dscale_t;
		if (a.d_rotations) { float* o = a.d_rotations + 4 * i; o[0] += drot.x; o[1] += drot.y; o[2] += drot.z; o[3] += drot.w; }
		if (a.d_rotations_r) { float* o = a.d_rotations_r + 4 * i; o[0] += drot_r.x; o[1] += drot_r.y; o[2] += drot_r.z; o[3] += drot_r.w; }
	}

	// FDGS_OK: the arguments are fine and `a` is filled in; otherwise the entry point `fn` fails with what is wrong with them
	static int flow_args(const char* fn, const fdgs_flow_in* in, FlowArgs& a)
	{
		if (!in) return fail(FDGS_ERR_INVALID_ARG, "%s: in must not be NULL", fn);
		CHECK_STRUCT_IN(fn, in, fdgs_flow_in);
		if (in->P < 0) return fail(FDGS_ERR_INVALID_ARG, "%s: P must not be negative", fn);
		if (in->W <= 0 || in->H <= 0) return fail(FDGS_ERR_INVALID_ARG, "%s: W and H must be positive", fn);
		if (!in->viewmatrix || !in->projmatrix) return fail(FDGS_ERR_INVALID_ARG, "%s: viewmatrix / projmatrix must not be NULL", fn);
		if ((in->viewmatrix_to == nullptr) != (in->projmatrix_to == nullptr)) return fail(FDGS_ERR_INVALID_ARG, "%s: viewmatrix_to and projmatrix_to come together (both NULL: the same camera)", fn);
		if (in->gaussian_dim != 3 && in->gaussian_dim != 4) return fail(FDGS_ERR_INVALID_ARG, "%s: gaussian_dim must be 3 or 4", fn);
		if (in->rot_4d && in->gaussian_dim != 4) return fail(FDGS_ERR_INVALID_ARG, "%s: rot_4d needs gaussian_dim == 4", fn);
		if (in->P > 0 && !in->means3D) return fail(FDGS_ERR_INVALID_ARG, "%s: means3D must not be NULL", fn);
		if (in->P > 0 && in->rot_4d && (!in->ts || !in->scales || !in->scales_t || !in->rotations || !in->rotations_r))
			return fail(FDGS_ERR_INVALID_ARG, "%s: rot_4d needs ts / scales / scales_t / rotations / rotations_r", fn);
		a.P = in->P; a.W = in->W; a.H = in->H;
		a.means3D = in->means3D; a.ts = in->ts; a.scales = in->scales; a.scales_t = in->scales_t;
		a.rotations = in->rotations; a.rotations_r = in->rotations_r;
		a.vm0 = in->viewmatrix; a.pm0 = in->projmatrix;
		a.vm1 = in->viewmatrix_to ? in->viewmatrix_to : in->viewmatrix;
		a.pm1 = in->projmatrix_to ? in->projmatrix_to : in->projmatrix;
		a.t0 = in->timestamp; a.t1 = in->timestamp_to; a.mod = in->scale_modifier;
		a.rot_4d = in->rot_4d != 0; a.raw = in->raw_params != 0;
		a.flows = nullptr; a.dL_dflows = nullptr; a.scale = 0.f;
		a.d_means3D = a.d_ts = a.d_scales = a.d_scales_t = a.d_rotations = a.d_rotations_r = nullptr;
		return FDGS_OK;
	}
}

using namespace fdgs;

extern "C" int fdgs_gaussian_flow_forward(const fdgs_flow_in* in, float* flows, void* stream)
{
	FlowArgs a;
	if (const int rc = flow_args("fdgs_gaussian_flow_forward", in, a)) return rc;
	if (a.P == 0) return FDGS_OK;
	if (!flows) return fail(FDGS_ERR_INVALID_ARG, "fdgs_gaussian_flow_forward: flows must not be NULL");
	a.flows = flows;
	hipLaunchKernelGGL(flow_forward_kernel, dim3(div_up(a.P, FLOW_THREADS)), dim3(FLOW_THREADS), 0, (hipStream_t)stream, a);
	return launched("fdgs_gaussian_flow_forward");
}

extern "C" int fdgs_gaussian_flow_backward(const fdgs_flow_in* in, const float* dL_dflows, float scale, const fdgs_flow_grads* out, void* stream)
{
	FlowArgs a;
	if (const int rc = flow_args("fdgs_gaussian_flow_backward", in, a)) return rc;
	if (!out) return fail(FDGS_ERR_INVALID_ARG, "fdgs_gaussian_flow_backward: out must not be NULL");
	CHECK_STRUCT_IN("fdgs_gaussian_flow_backward", out, fdgs_flow_grads);
	if (a.P == 0) return FDGS_OK;
	if (!dL_dflows) return fail(FDGS_ERR_INVALID_ARG, "fdgs_gaussian_flow_backward: dL_dflows must not be NULL");
	a.dL_dflows = dL_dflows; a.scale = scale;
	a.d_means3D = out->d_means3D; a.d_ts = out->d_ts; a.d_scales = out->d_scales; a.d_scales_t = out->d_scales_t;
	a.d_rotations = out->d_rotations; a.d_rotations_r = out->d_rotations_r;
	if (!a.d_means3D && !a.d_ts && !a.d_scales && !a.d_scales_t && !a.d_rotations && !a.d_rotations_r) return FDGS_OK;
	hipLaunchKernelGGL(flow_backward_kernel, dim3(div_up(a.P, FLOW_THREADS)), dim3(FLOW_THREADS), 0, (hipStream_t)stream, a);
	return launched("fdgs_gaussian_flow_backward");
}
