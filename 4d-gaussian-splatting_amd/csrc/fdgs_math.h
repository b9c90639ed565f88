// fdgs_math.h -- small fixed-size vector / matrix helpers for the per-Gaussian kernels, and the temporal model built from them:
// the 4D / 3D covariance and their backwards, the temporal marginal, the activations of raw parameters and gaussian_at_time.
//
// The forward preprocess has to reproduce the reference's float results BIT-EXACTLY
// wherever they feed integers (radius, tile rectangle, tile count, depth-key bits),
// so these helpers fix one evaluation order: matrix products accumulate
// k = 0,1,2(,3) left to right, dot3 = (x+y)+z, dot4 = (x+y)+(z+w) -- the order the
// reference's GLM expressions evaluate in (glm/detail/type_mat3x3.inl:486,
// type_mat4x4.inl:630, func_geometric.inl:48-65).  Translation units that need
// bit-exactness are compiled with FP contraction off (no FMA fusion).
#pragma once
#include <hip/hip_runtime.h>

namespace fdgs
{
	struct M3 { float c[3][3]; };   // c[column][row]
	struct M4 { float c[4][4]; };

	__device__ __forceinline__ M3 mul(const M3& A, const M3& B)
	{
		M3 R;
#pragma unroll
		for (int j = 0; j < 3; j++)
#pragma unroll
			for (int i = 0; i < 3; i++)
				R.c[j][i] = A.c[0][i] * B.c[j][0] + A.c[1][i] * B.c[j][1] + A.c[2][i] * B.c[j][2];
		return R;
	}
	__device__ __forceinline__ M3 transpose(const M3& A)
	{
		M3 R;
#pragma unroll
		for (int j = 0; j < 3; j++)
#pragma unroll
			for (int i = 0; i < 3; i++) R.c[j][i] = A.c[i][j];
		return R;
	}
	__device__ __forceinline__ M4 mul(const M4& A, const M4& B)
	{
		M4 R;
#pragma unroll
		for (int j = 0; j < 4; j++)
#pragma unroll
			for (int i = 0; i < 4; i++)
				R.c[j][i] = A.c[0][i] * B.c[j][0] + A.c[1][i] * B.c[j][1] + A.c[2][i] * B.c[j][2] + A.c[3][i] * B.c[j][3];
		return R;
	}
	__device__ __forceinline__ M4 transpose(const M4& A)
	{
		M4 R;
#pragma unroll
		for (int j = 0; j < 4; j++)
#pragma unroll
			for (int i = 0; i < 4; i++) R.c[j][i] = A.c[i][j];
		return R;
	}
	__device__ __forceinline__ M4 diag4(float a, float b, float c, float d)
	{
		M4 S;
#pragma unroll
		for (int j = 0; j < 4; j++)
#pragma unroll
			for (int i = 0; i < 4; i++) S.c[j][i] = 0.0f;
		S.c[0][0] = a; S.c[1][1] = b; S.c[2][2] = c; S.c[3][3] = d;
		return S;
	}
	__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz)
	{
		return ax * bx + ay * by + az * bz;
	}
	__device__ __forceinline__ float dot4(const float* a, const float* b)
	{
		return (a[0] * b[0] + a[1] * b[1]) + (a[2] * b[2] + a[3] * b[3]);
	}
	__device__ __forceinline__ float3 ld3(const float* p, size_t i) { return make_float3(p[3 * i], p[3 * i + 1], p[3 * i + 2]); }
	__device__ __forceinline__ void st3(float* p, size_t i, float3 v) { p[3 * i] = v.x; p[3 * i + 1] = v.y; p[3 * i + 2] = v.z; }
	__device__ __forceinline__ float3 add3(float3 a, float3 b) { return make_float3(a.x + b.x, a.y + b.y, a.z + b.z); }
	__device__ __forceinline__ float3 sub3(float3 a, float3 b) { return make_float3(a.x - b.x, a.y - b.y, a.z - b.z); }
	__device__ __forceinline__ float3 scl3(float s, float3 a) { return make_float3(s * a.x, s * a.y, s * a.z); }
	__device__ __forceinline__ float dot3(float3 a, float3 b) { return dot3(a.x, a.y, a.z, b.x, b.y, b.z); }
	// backward of v / |v| (auxiliary.h:108-118): the geometry backward's and the SH backward's view direction
	__device__ __forceinline__ float3 dnormvdv(float3 v, float3 dv)
	{
		const float sum2 = v.x * v.x + v.y * v.y + v.z * v.z;
		const float invsum32 = 1.0f / sqrtf(sum2 * sum2 * sum2);
		float3 r;
		r.x = ((+sum2 - v.x * v.x) * dv.x - v.y * v.x * dv.y - v.z * v.x * dv.z) * invsum32;
		r.y = (-v.x * v.y * dv.x + (sum2 - v.y * v.y) * dv.y - v.z * v.y * dv.z) * invsum32;
		r.z = (-v.x * v.z * dv.x - v.y * v.z * dv.y + (sum2 - v.z * v.z) * dv.z) * invsum32;
		return r;
	}

	// Left / right isoclinic factors of the 4D rotation, column-major
	// (reference forward.cu:315-327): R4 = M_r * M_l.
	__device__ __forceinline__ void build_Ml_Mr(const float4 rot, const float4 rot_r, M4& L, M4& Rr)
	{
		const float a = rot.x, b = rot.y, c = rot.z, d = rot.w;
		const float p = rot_r.x, q = rot_r.y, r = rot_r.z, s = rot_r.w;
		const float l[4][4] = { { a, b, -c, d }, { -b, a, d, c }, { c, -d, a, b }, { -d, -c, -b, a } };
		const float m[4][4] = { { p, q, -r, -s }, { -q, p, s, -r }, { r, -s, p, -q }, { s, r, q, p } };
#pragma unroll
		for (int j = 0; j < 4; j++)
#pragma unroll
			for (int i = 0; i < 4; i++) { L.c[j][i] = l[j][i]; Rr.c[j][i] = m[j][i]; }
	}

	// The 4D covariance Sigma = M^T M, M = S (M_r M_l) (reference forward.cu:279-352) and its backward (backward.cu:689-834):
	// dSig (symmetric, the off-diagonal halves already split) -> d scale (x, y, z, t) and d rot / rot_r of the NORMALISED quaternions.
	struct Cov4 { M4 Ml, Mr, R, M, Sigma; float scl[4]; };
	__device__ __forceinline__ Cov4 cov4_build(const float3 sc, float sct, float mod, const float4 q, const float4 qr)
	{
		Cov4 c;
		c.scl[0] = mod * sc.x; c.scl[1] = mod * sc.y; c.scl[2] = mod * sc.z; c.scl[3] = mod * sct;
		const M4 S = diag4(c.scl[0], c.scl[1], c.scl[2], c.scl[3]);
		build_Ml_Mr(q, qr, c.Ml, c.Mr);
		c.R = mul(c.Mr, c.Ml);
		c.M = mul(S, c.R);
		c.Sigma = mul(transpose(c.M), c.M);
		return c;
	}
	__device__ __forceinline__ void cov4_backward(const Cov4& c, const M4& dSig, float3& dscale, float& dscale_t, float4& drot, float4& drot_r)
	{
		M4 M2;
#pragma unroll
		for (int j = 0; j < 4; j++)
#pragma unroll
			for (int i = 0; i < 4; i++) M2.c[j][i] = 2.0f * c.M.c[j][i];
		const M4 dM = mul(M2, dSig);
		const M4 Rt = transpose(c.R);
		M4 dMt = transpose(dM);
		dscale.x = dot4(Rt.c[0], dMt.c[0]);
		dscale.y = dot4(Rt.c[1], dMt.c[1]);
		dscale.z = dot4(Rt.c[2], dMt.c[2]);
		dscale_t = dot4(Rt.c[3], dMt.c[3]);
#pragma unroll
		for (int k = 0; k < 4; k++)
#pragma unroll
			for (int i = 0; i < 4; i++) dMt.c[k][i] *= c.scl[k];
		const M4 A = mul(dMt, c.Mr);
		drot.x = A.c[0][0] + A.c[1][1] + A.c[2][2] + A.c[3][3];
		drot.y = -A.c[0][1] + A.c[1][0] - A.c[2][3] + A.c[3][2];
		drot.z = A.c[0][2] - A.c[1][3] - A.c[2][0] + A.c[3][1];
		drot.w = -A.c[0][3] - A.c[1][2] + A.c[2][1] + A.c[3][0];
		const M4 B = mul(c.Ml, dMt);
		drot_r.x = B.c[0][0] + B.c[1][1] + B.c[2][2] + B.c[3][3];
		drot_r.y = -B.c[0][1] + B.c[1][0] + B.c[2][3] - B.c[3][2];
		drot_r.z = B.c[0][2] + B.c[1][3] - B.c[2][0] - B.c[3][1];
		drot_r.w = B.c[0][3] - B.c[1][2] + B.c[2][1] - B.c[3][0];
	}

	// quaternion (w,x,y,z) -> rotation, column-major (reference forward.cu:251-262)
	__device__ __forceinline__ M3 quat_to_R(const float4 q)
	{
		const float r = q.x, x = q.y, y = q.z, z = q.w;
		M3 R;
		R.c[0][0] = 1.f - 2.f * (y * y + z * z); R.c[0][1] = 2.f * (x * y - r * z); R.c[0][2] = 2.f * (x * z + r * y);
		R.c[1][0] = 2.f * (x * y + r * z); R.c[1][1] = 1.f - 2.f * (x * x + z * z); R.c[1][2] = 2.f * (y * z - r * x);
		R.c[2][0] = 2.f * (x * z - r * y); R.c[2][1] = 2.f * (y * z + r * x); R.c[2][2] = 1.f - 2.f * (x * x + y * y);
		return R;
	}

	// The reference model's activations (scene/gaussian_model.py:55-66, 179-219), used when fdgs_scene.raw_params != 0
	__device__ __forceinline__ float act_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }
	__device__ __forceinline__ float4 act_normalize(const float4 v, float* inv_norm)
	{
		const float n = sqrtf((v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w));
		const float inv = 1.0f / fmaxf(n, 1e-12f); // F.normalize eps
		*inv_norm = inv;
		return make_float4(v.x * inv, v.y * inv, v.z * inv, v.w * inv);
	}
	// d/dv of v / |v| applied to g:  (g - q (q . g)) / |v|
	__device__ __forceinline__ float4 act_normalize_bwd(const float4 q, float inv_norm, const float4 g)
	{
		const float d = (q.x * g.x + q.y * g.y) + (q.z * g.z + q.w * g.w);
		return make_float4((g.x - q.x * d) * inv_norm, (g.y - q.y * d) * inv_norm, (g.z - q.z * d) * inv_norm, (g.w - q.w * d) * inv_norm);
	}

	// Raw parameters -> what the covariances are built from: exp on the scales, F.normalize on the quaternions (the inverse norm
	// goes back to the caller: act_normalize_bwd needs it)
	__device__ __forceinline__ float3 act_exp3(const float3 s) { return make_float3(expf(s.x), expf(s.y), expf(s.z)); }
	__device__ __forceinline__ void activate(float3& sc, float4& q, float* inv_norm) { sc = act_exp3(sc); q = act_normalize(q, inv_norm); }
	__device__ __forceinline__ void activate(float& sct, float4& qr, float* inv_norm) { sct = expf(sct); qr = act_normalize(qr, inv_norm); }

	// The 3D covariance Sigma = M^T M, M = S R (reference forward.cu:242-276) and its backward (backward.cu:621-684): dSig as for
	// cov4_backward -> d scale and d rot of the NORMALISED quaternion q that R was built from.
	struct Cov3 { M3 R, M, Sigma; float scl[3]; };
	__device__ __forceinline__ Cov3 cov3_build(const float3 sc, float mod, const float4 q)
	{
		Cov3 c;
		c.scl[0] = mod * sc.x; c.scl[1] = mod * sc.y; c.scl[2] = mod * sc.z;
		M3 S;
#pragma unroll
		for (int j = 0; j < 3; j++)
#pragma unroll
			for (int i = 0; i < 3; i++) S.c[j][i] = 0.0f;
		S.c[0][0] = c.scl[0]; S.c[1][1] = c.scl[1]; S.c[2][2] = c.scl[2];
		c.R = quat_to_R(q);
		c.M = mul(S, c.R);
		c.Sigma = mul(transpose(c.M), c.M);
		return c;
	}
	__device__ __forceinline__ void cov3_backward(const Cov3& c, const float4 q, const M3& dSig, float3& dscale, float4& drot)
	{
		const float r = q.x, x = q.y, y = q.z, z = q.w;
		M3 M2;
#pragma unroll
		for (int j = 0; j < 3; j++)
#pragma unroll
			for (int i = 0; i < 3; i++) M2.c[j][i] = 2.0f * c.M.c[j][i];
		const M3 dM = mul(M2, dSig);
		const M3 Rt = transpose(c.R);
		M3 dMt = transpose(dM);
		dscale.x = dot3(Rt.c[0][0], Rt.c[0][1], Rt.c[0][2], dMt.c[0][0], dMt.c[0][1], dMt.c[0][2]);
		dscale.y = dot3(Rt.c[1][0], Rt.c[1][1], Rt.c[1][2], dMt.c[1][0], dMt.c[1][1], dMt.c[1][2]);
		dscale.z = dot3(Rt.c[2][0], Rt.c[2][1], Rt.c[2][2], dMt.c[2][0], dMt.c[2][1], dMt.c[2][2]);
#pragma unroll
		for (int k = 0; k < 3; k++)
#pragma unroll
			for (int i = 0; i < 3; i++) dMt.c[k][i] *= c.scl[k];
#define DD(i, j) dMt.c[i][j]
		drot.x = 2 * z * (DD(0, 1) - DD(1, 0)) + 2 * y * (DD(2, 0) - DD(0, 2)) + 2 * x * (DD(1, 2) - DD(2, 1));
		drot.y = 2 * y * (DD(1, 0) + DD(0, 1)) + 2 * z * (DD(2, 0) + DD(0, 2)) + 2 * r * (DD(1, 2) - DD(2, 1)) - 4 * x * (DD(2, 2) + DD(1, 1));
		drot.z = 2 * x * (DD(1, 0) + DD(0, 1)) + 2 * r * (DD(2, 0) - DD(0, 2)) + 2 * z * (DD(1, 2) + DD(2, 1)) - 4 * y * (DD(2, 2) + DD(0, 0));
		drot.w = 2 * r * (DD(0, 1) - DD(1, 0)) + 2 * x * (DD(2, 0) + DD(0, 2)) + 2 * y * (DD(1, 2) + DD(2, 1)) - 4 * z * (DD(1, 1) + DD(0, 0));
#undef DD
	}
	// the symmetric gradient matrix the two covariance backwards take, from the six gradients of the upper triangle: the
	// off-diagonal halves split
	__device__ __forceinline__ M3 sym_split(const float* d)
	{
		M3 S;
		S.c[0][0] = d[0]; S.c[0][1] = 0.5f * d[1]; S.c[0][2] = 0.5f * d[2];
		S.c[1][0] = 0.5f * d[1]; S.c[1][1] = d[3]; S.c[1][2] = 0.5f * d[4];
		S.c[2][0] = 0.5f * d[2]; S.c[2][1] = 0.5f * d[4]; S.c[2][2] = d[5];
		return S;
	}

	// The 1-D temporal marginal exp(-dt^2 / 2 var) with the reference's double promotion of the exponent (forward.cu:334-336,
	// 431-437) over the prefiltered variance (prefilter_var <= 0: none).  The cull is marginal > 0.05.
	__device__ __forceinline__ float prefiltered_var(float var, float prefilter_var) { return (prefilter_var > 0.0) ? (prefilter_var + var) : var; }
	__device__ __forceinline__ float temporal_marginal(float dt, float var, float prefilter_var)
	{
		return expf((float)(-0.5 * dt * dt / prefiltered_var(var, prefilter_var)));
	}

	// ---- The temporal model: what a Gaussian of the model is at time `timestamp` ----
	// rot_4d: the mean and covariance of the 4D Gaussian conditioned on t (forward.cu:279-352); otherwise the plain 3D covariance
	// (forward.cu:242-276) and, for gaussian_dim == 4, the marginal of an independent temporal axis whose VARIANCE is scales_t
	// (forward.cu:431-437); either way the opacity times the marginal, and no Gaussian whose marginal is <= 0.05.  This is the one
	// statement of it: the forward preprocess continues from here with the view transform, the time slice stores it.  The geometry
	// backward differentiates the same cov4_build / cov3_build / temporal_marginal; its conditioning step reads Sigma[3][k] where
	// this one reads Sigma[k][3] (Q7) and stays its own.
	// `in`: the parameters AS STORED (raw: the activations run here).  Mean shift, conditional covariance and the opacity product
	// exist only for a Gaussian that is alive; `alive` starts as `valid` and, on the rot_4d path, is the marginal's test alone.
	struct GaussIn { float3 p; float opacity; float3 sc; float sct; float4 q, qr; float t; };
	struct GaussAtTime { bool alive; float3 mean; float cov[6]; float opacity; };
	__device__ __forceinline__ void gaussian_at_time(const GaussIn& in, const bool valid, const int raw, const int rot_4d, const int gaussian_dim,
	                                                 const float mod, const float prefilter_var, const float timestamp,
	                                                 const float* __restrict__ cov_precomp, GaussAtTime& o)
	{
		o.alive = valid; o.mean = in.p;
		o.opacity = raw ? act_sigmoid(in.opacity) : in.opacity;
#pragma unroll
		for (int k = 0; k < 6; k++) o.cov[k] = 0.f;
		float unused;
		if (cov_precomp != nullptr)
		{
#pragma unroll
			for (int k = 0; k < 6; k++) o.cov[k] = cov_precomp[k];
		}
		else if (rot_4d)
		{
			float3 sc = in.sc;
			float sct = in.sct;
			float4 q = in.q, qr = in.qr;
			if (raw) { activate(sc, q, &unused); activate(sct, qr, &unused); }
			const float dt = timestamp - in.t;
			const M4 Sigma = cov4_build(sc, sct, mod, q, qr).Sigma;
			const float cov_t = Sigma.c[3][3];
			const float marginal_t = temporal_marginal(dt, cov_t, prefilter_var);
			o.alive = marginal_t > 0.05;
			if (o.alive)
			{
				o.opacity *= marginal_t;
				const float c12[3] = { Sigma.c[0][3], Sigma.c[1][3], Sigma.c[2][3] };
				o.cov[0] = Sigma.c[0][0] - (c12[0] * c12[0]) / cov_t;
				o.cov[1] = Sigma.c[0][1] - (c12[1] * c12[0]) / cov_t;
				o.cov[2] = Sigma.c[0][2] - (c12[2] * c12[0]) / cov_t;
				o.cov[3] = Sigma.c[1][1] - (c12[1] * c12[1]) / cov_t;
				o.cov[4] = Sigma.c[1][2] - (c12[2] * c12[1]) / cov_t;
				o.cov[5] = Sigma.c[2][2] - (c12[2] * c12[2]) / cov_t;
				o.mean.x += c12[0] / cov_t * dt;
				o.mean.y += c12[1] / cov_t * dt;
				o.mean.z += c12[2] / cov_t * dt;
			}
		}
		else
		{
			float3 sc = in.sc;
			float4 q = in.q;
			if (raw) activate(sc, q, &unused);
			const M3 Sigma = cov3_build(sc, mod, q).Sigma;
			o.cov[0] = Sigma.c[0][0]; o.cov[1] = Sigma.c[0][1]; o.cov[2] = Sigma.c[0][2];
			o.cov[3] = Sigma.c[1][1]; o.cov[4] = Sigma.c[1][2]; o.cov[5] = Sigma.c[2][2];
			if (gaussian_dim == 4)
			{
				const float dt = in.t - timestamp;   // (the other sign than above: as the reference has it)
				const float sigma = (raw ? expf(in.sct) : in.sct) * mod;
				const float marginal_t = temporal_marginal(dt, sigma, prefilter_var);
				if (marginal_t <= 0.05) o.alive = false;
				else o.opacity *= marginal_t;
			}
		}
	}

	// SH constants (reference auxiliary.h:23-40)
	__device__ constexpr float SH_C0 = 0.28209479177387814f;
	__device__ constexpr float SH_C1 = 0.4886025119029199f;
	__device__ constexpr float SH_C2[5] = { 1.0925484305920792f, -1.0925484305920792f, 0.31539156525252005f, -1.0925484305920792f, 0.5462742152960396f };
	__device__ constexpr float SH_C3[7] = { -0.5900435899266435f, 2.890611442640554f, -0.4570457994644658f, 0.3731763325901154f, -0.4570457994644658f, 1.445305721320277f, -0.5900435899266435f };
	constexpr double REF_PI = 3.14159265; // the reference's truncated pi (auxiliary.h:20), double

	// view * p with the translation row (auxiliary.h:59-67), view stored transposed
	__device__ __forceinline__ float3 xform4x3(const float3 p, const float* __restrict__ m)
	{
		return make_float3(m[0] * p.x + m[4] * p.y + m[8] * p.z + m[12],
		                   m[1] * p.x + m[5] * p.y + m[9] * p.z + m[13],
		                   m[2] * p.x + m[6] * p.y + m[10] * p.z + m[14]);
	}
	__device__ __forceinline__ float4 xform4x4(const float3 p, const float* __restrict__ m)
	{
		return make_float4(m[0] * p.x + m[4] * p.y + m[8] * p.z + m[12],
		                   m[1] * p.x + m[5] * p.y + m[9] * p.z + m[13],
		                   m[2] * p.x + m[6] * p.y + m[10] * p.z + m[14],
		                   m[3] * p.x + m[7] * p.y + m[11] * p.z + m[15]);
	}

	// The EWA projection shared by forward (forward.cu:198-237) and backward (backward.cu:509-537).
	struct Cov2D
	{
		float3 t;          // clamped view-space mean
		float txtz, tytz;
		M3 T, Vrk, W;
		float a, b, c;     // cov2D entries before the +0.3 low-pass
	};
	__device__ __forceinline__ Cov2D project_cov(const float3 mean, float focal_x, float focal_y, float tan_fovx, float tan_fovy,
	                                              const float* cov3D, const float* __restrict__ vm)
	{
		Cov2D o;
		float3 t = xform4x3(mean, vm);
		const float limx = 1.3f * tan_fovx, limy = 1.3f * tan_fovy;
		o.txtz = t.x / t.z; o.tytz = t.y / t.z;
		t.x = fminf(limx, fmaxf(-limx, o.txtz)) * t.z;
		t.y = fminf(limy, fmaxf(-limy, o.tytz)) * t.z;
		M3 J;
		J.c[0][0] = focal_x / t.z; J.c[0][1] = 0.0f; J.c[0][2] = -(focal_x * t.x) / (t.z * t.z);
		J.c[1][0] = 0.0f; J.c[1][1] = focal_y / t.z; J.c[1][2] = -(focal_y * t.y) / (t.z * t.z);
		J.c[2][0] = 0.0f; J.c[2][1] = 0.0f; J.c[2][2] = 0.0f;
		o.W.c[0][0] = vm[0]; o.W.c[0][1] = vm[4]; o.W.c[0][2] = vm[8];
		o.W.c[1][0] = vm[1]; o.W.c[1][1] = vm[5]; o.W.c[1][2] = vm[9];
		o.W.c[2][0] = vm[2]; o.W.c[2][1] = vm[6]; o.W.c[2][2] = vm[10];
		o.T = mul(o.W, J);
		o.Vrk.c[0][0] = cov3D[0]; o.Vrk.c[0][1] = cov3D[1]; o.Vrk.c[0][2] = cov3D[2];
		o.Vrk.c[1][0] = cov3D[1]; o.Vrk.c[1][1] = cov3D[3]; o.Vrk.c[1][2] = cov3D[4];
		o.Vrk.c[2][0] = cov3D[2]; o.Vrk.c[2][1] = cov3D[4]; o.Vrk.c[2][2] = cov3D[5];
		const M3 cov = mul(mul(transpose(o.T), transpose(o.Vrk)), o.T);
		o.a = cov.c[0][0]; o.b = cov.c[0][1]; o.c = cov.c[1][1];
		o.t = t;
		return o;
	}
}
