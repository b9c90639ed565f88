// model_transform.hip -- a model's raw parameters under a similarity transform x' = s R x + T, t' = a t + b (fdgs_model_transform)
// for gfx950.
//
// Two launches, no atomics, no scratch memory:
//   1 geometry   one lane per Gaussian, raw parameters in, raw parameters out.  Three modes (a template parameter: the closed forms
//                must not carry the registers of the eigen-decomposition):
//                  0  gaussian_dim 3, or 4 without rot_4d: q' = q_R * q, scales += log s, scales_t += 2 log a (a variance)
//                  1  rot_4d, s == a: R4' = R4 diag(R, 1)^T = M_r(q_r) M_r(u) M_l(q_l) M_l(v) -- the two isoclinic families commute and are
//                     closed under the product -- so q_l' = q_l * v, q_r' = q_r * u: two quaternion products, no trigonometry
//                  2  rot_4d, s != a: A Sigma A^T with A = diag(s R, a) has other eigenvectors: cyclic Jacobi on the 4x4 in double, the
//                     eigenvector with the largest |time component| becomes axis 3, R4' = V^T is factored back into (q_l', q_r') through
//                     its rank-1 coefficient matrix K[a][b] = <M_r(e_a) M_l(e_b), R4'> / 4 = q_r[a] q_l[b]
//                Quaternion products and the sums with log s / log a are formed in double and rounded once; the mean is fp32 in a fixed
//                order (the error bar of tests/test_gpu_edit.py counts its roundings).  What the transform leaves alone -- a rotation,
//                scale or time map that is the identity to 0 ulp -- is copied, not recomputed: the identity returns the input bit for
//                bit, also for a component that is -0.
//   2 SH rows    the [P,M,3] tensor is a flat run of 16-coefficient blocks (M = 16, 32, 48; 3 M floats for M = 4, 9).  A workgroup stages
//                256 consecutive blocks through LDS with coalesced 16-byte accesses (block stride 49 dwords: the lanes' ds_read_b32 of
//                one coefficient fall on distinct banks), one lane rotates one block in place there -- bands 1-3 of the three channels,
//                c' = D c, D wave-uniform in kernel arguments (scalar registers) -- and the tile goes back the way it came.  Each sum is
//                pairwise and starts from +0: at most 4 roundings per term, and a block of zeros stays +0.  Coefficient 0 is never
//                touched.  in == out is fine: a workgroup reads its blocks before it writes them, and no other workgroup's.
#pragma clang fp contract(off)
#include "fdgs_common.h"
#include "fdgs_math.h"

namespace fdgs
{
	struct XformArgs
	{
		int P;
		const float *xyz, *ts, *scales, *scales_t, *rot, *rot_r;
		float *o_xyz, *o_ts, *o_scales, *o_scales_t, *o_rot, *o_rot_r;
		float R[9], T[3], s, a, b;     // the mean's fp32 path
		double Rd[9], sd, ad;          // mode 2
		double q[4], u[4], v[4], log_s, log_st;   // log_st: what scales_t gains (log a; 2 log a where it is a variance)
		int keep_xyz, keep_rot, keep_t, keep_scale, keep_scale_t;   // the identity to 0 ulp: copy
	};

	// M_l / M_r of build_Ml_Mr (fdgs_math.h) in double; the literals are the COLUMNS, entry (row i, column j) is l[j][i]
	__device__ __forceinline__ void Ml_d(const double* q, double (&l)[4][4])
	{
		const double a = q[0], b = q[1], c = q[2], d = q[3];
		const double t[4][4] = { { a, b, -c, d }, { -b, a, d, c }, { c, -d, a, b }, { -d, -c, -b, a } };
#pragma unroll
		for (int j = 0; j < 4; j++)
#pragma unroll
			for (int i = 0; i < 4; i++) l[j][i] = t[j][i];
	}
	__device__ __forceinline__ void Mr_d(const double* q_, double (&m)[4][4])
	{
		const double p = q_[0], q = q_[1], r = q_[2], s = q_[3];
		const double t[4][4] = { { p, q, -r, -s }, { -q, p, s, -r }, { r, -s, p, -q }, { s, r, q, p } };
#pragma unroll
		for (int j = 0; j < 4; j++)
#pragma unroll
			for (int i = 0; i < 4; i++) m[j][i] = t[j][i];
	}
	// M_l(x) M_l(y) = M_l(z): column 0 of M_l(z) is M_l(x) times column 0 of M_l(y), and column 0 is (z0, z1, -z2, z3)
	__device__ __forceinline__ void iso_mul_l(const double* x, const double* y, double* z)
	{
		double l[4][4];
		Ml_d(x, l);
		const double c0[4] = { y[0], y[1], -y[2], y[3] };
		double r[4];
#pragma unroll
		for (int i = 0; i < 4; i++) r[i] = (l[0][i] * c0[0] + l[1][i] * c0[1]) + (l[2][i] * c0[2] + l[3][i] * c0[3]);
		z[0] = r[0]; z[1] = r[1]; z[2] = -r[2]; z[3] = r[3];
	}
	// the same for M_r: column 0 is (z0, z1, -z2, -z3)
	__device__ __forceinline__ void iso_mul_r(const double* x, const double* y, double* z)
	{
		double m[4][4];
		Mr_d(x, m);
		const double c0[4] = { y[0], y[1], -y[2], -y[3] };
		double r[4];
#pragma unroll
		for (int i = 0; i < 4; i++) r[i] = (m[0][i] * c0[0] + m[1][i] * c0[1]) + (m[2][i] * c0[2] + m[3][i] * c0[3]);
		z[0] = r[0]; z[1] = r[1]; z[2] = -r[2]; z[3] = -r[3];
	}
	// Hamilton product x * y of (w, x, y, z) quaternions: R(x * y) = R(x) R(y)
	__device__ __forceinline__ void quat_mul(const double* x, const double* y, double* z)
	{
		z[0] = (x[0] * y[0] - x[1] * y[1]) - (x[2] * y[2] + x[3] * y[3]);
		z[1] = (x[0] * y[1] + x[1] * y[0]) + (x[2] * y[3] - x[3] * y[2]);
		z[2] = (x[0] * y[2] - x[1] * y[3]) + (x[2] * y[0] + x[3] * y[1]);
		z[3] = (x[0] * y[3] + x[1] * y[2]) - (x[2] * y[1] - x[3] * y[0]);
	}

	// ---- mode 2: the coefficient table of the isoclinic factorisation, at compile time from the same two literals ----
	struct IsoTable { signed char e[4][4][4][4]; };   // e[a][b][i][j]: entry (row i, column j) of M_r(e_a) M_l(e_b): 0 or +-1
	constexpr int ml_unit(int b, int i, int j)
	{
		int q[4] = { 0, 0, 0, 0 };
		q[b] = 1;
		const int l[4][4] = { { q[0], q[1], -q[2], q[3] }, { -q[1], q[0], q[3], q[2] }, { q[2], -q[3], q[0], q[1] }, { -q[3], -q[2], -q[1], q[0] } };
		return l[j][i];
	}
	constexpr int mr_unit(int a, int i, int j)
	{
		int q[4] = { 0, 0, 0, 0 };
		q[a] = 1;
		const int m[4][4] = { { q[0], q[1], -q[2], -q[3] }, { -q[1], q[0], q[3], -q[2] }, { q[2], -q[3], q[0], -q[1] }, { q[3], q[2], q[1], q[0] } };
		return m[j][i];
	}
	constexpr IsoTable make_iso_table()
	{
		IsoTable t{};
		for (int a = 0; a < 4; a++)
			for (int b = 0; b < 4; b++)
				for (int i = 0; i < 4; i++)
					for (int j = 0; j < 4; j++)
					{
						int s = 0;
						for (int k = 0; k < 4; k++) s += mr_unit(a, i, k) * ml_unit(b, k, j);
						t.e[a][b][i][j] = (signed char)s;
					}
		return t;
	}
	__device__ constexpr IsoTable ISO = make_iso_table();

	template <int p, int q>
	__device__ __forceinline__ void jacobi4_rotate(double (&A)[4][4], double (&V)[4][4])
	{
		const double apq = A[p][q];
		if (apq == 0.0) return;
		const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
		const double t = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));   // the smaller root: |angle| <= pi / 4
		const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
		for (int k = 0; k < 4; k++)
		{
			if (k == p || k == q) continue;
			const double akp = c * A[k][p] - s * A[k][q], akq = s * A[k][p] + c * A[k][q];
			A[k][p] = akp; A[p][k] = akp; A[k][q] = akq; A[q][k] = akq;
		}
		A[p][p] -= t * apq; A[q][q] += t * apq;
		A[p][q] = 0.0; A[q][p] = 0.0;
#pragma unroll
		for (int k = 0; k < 4; k++)
		{
			const double vp = c * V[k][p] - s * V[k][q], vq = s * V[k][p] + c * V[k][q];
			V[k][p] = vp; V[k][q] = vq;
		}
	}

	// raw (scales, scales_t, q_l, q_r) -> raw parameters of A Sigma A^T, A = diag(s R, a); everything in double
	__device__ inline void redecompose4(const XformArgs& a, const float3 sc_raw, const float sct_raw, const double* ql_raw, const double* qr_raw,
	                                    float* sc_out, float& sct_out, double* ql_out, double* qr_out)
	{
		double ql[4], qr[4];
		{
			const double nl = sqrt((ql_raw[0] * ql_raw[0] + ql_raw[1] * ql_raw[1]) + (ql_raw[2] * ql_raw[2] + ql_raw[3] * ql_raw[3]));
			const double nr = sqrt((qr_raw[0] * qr_raw[0] + qr_raw[1] * qr_raw[1]) + (qr_raw[2] * qr_raw[2] + qr_raw[3] * qr_raw[3]));
			const double il = 1.0 / fmax(nl, 1e-12), ir = 1.0 / fmax(nr, 1e-12);   // F.normalize eps
#pragma unroll
			for (int k = 0; k < 4; k++) { ql[k] = ql_raw[k] * il; qr[k] = qr_raw[k] * ir; }
		}
		const double S[4] = { exp((double)sc_raw.x), exp((double)sc_raw.y), exp((double)sc_raw.z), exp((double)sct_raw) };
		// M = S R4, R4 = M_r M_l; then B = M A^T (so that A Sigma A^T = B^T B): B[k][i] = S_k sum_j R4[k][j] A[i][j]
		double B[4][4];
		{
			double l[4][4], m[4][4];
			Ml_d(ql, l);
			Mr_d(qr, m);
#pragma unroll
			for (int k = 0; k < 4; k++)
			{
				double r4[4];   // row k of R4: sum_n M_r(k, n) M_l(n, j) = sum_n m[n][k] l[j][n]
#pragma unroll
				for (int j = 0; j < 4; j++) r4[j] = S[k] * ((m[0][k] * l[j][0] + m[1][k] * l[j][1]) + (m[2][k] * l[j][2] + m[3][k] * l[j][3]));
#pragma unroll
				for (int i = 0; i < 3; i++) B[k][i] = a.sd * ((r4[0] * a.Rd[3 * i + 0] + r4[1] * a.Rd[3 * i + 1]) + r4[2] * a.Rd[3 * i + 2]);
				B[k][3] = a.ad * r4[3];
			}
		}
		double A[4][4], V[4][4];
#pragma unroll
		for (int i = 0; i < 4; i++)
#pragma unroll
			for (int j = i; j < 4; j++)
			{
				const double v = (B[0][i] * B[0][j] + B[1][i] * B[1][j]) + (B[2][i] * B[2][j] + B[3][i] * B[3][j]);
				A[i][j] = v; A[j][i] = v;
			}
#pragma unroll
		for (int i = 0; i < 4; i++)
#pragma unroll
			for (int j = 0; j < 4; j++) V[i][j] = i == j ? 1.0 : 0.0;
#pragma unroll 1
		for (int sweep = 0; sweep < 12; sweep++)
		{
			const double off = (fabs(A[0][1]) + fabs(A[0][2]) + fabs(A[0][3])) + (fabs(A[1][2]) + fabs(A[1][3]) + fabs(A[2][3]));
			if (!(off > 1e-20 * ((fabs(A[0][0]) + fabs(A[1][1])) + (fabs(A[2][2]) + fabs(A[3][3]))))) break;   // (also NaN)
			jacobi4_rotate<0, 1>(A, V); jacobi4_rotate<0, 2>(A, V); jacobi4_rotate<0, 3>(A, V);
			jacobi4_rotate<1, 2>(A, V); jacobi4_rotate<1, 3>(A, V); jacobi4_rotate<2, 3>(A, V);
		}
		// A = V diag V^T, the columns of V the eigenvectors = the ROWS of R4'.  Axis 3 (scales_t) is the one that points most along time.
		int mt = 0;
		double best = fabs(V[3][0]);
#pragma unroll
		for (int j = 1; j < 4; j++) if (fabs(V[3][j]) > best) { best = fabs(V[3][j]); mt = j; }
		double Rn[4][4], lam[4];   // Rn[axis][i]
#pragma unroll
		for (int axis = 0; axis < 4; axis++)
		{
			const int src = axis == 3 ? mt : axis + (axis >= mt ? 1 : 0);
			lam[axis] = A[0][0];
#pragma unroll
			for (int i = 0; i < 4; i++) Rn[axis][i] = V[i][0];
#pragma unroll
			for (int j = 1; j < 4; j++)
				if (src == j)
				{
					lam[axis] = A[j][j];
#pragma unroll
					for (int i = 0; i < 4; i++) Rn[axis][i] = V[i][j];
				}
		}
		// V is a product of plane rotations (det +1); moving column mt to the end is 3 - mt transpositions
		if ((3 - mt) & 1)
		{
#pragma unroll
			for (int i = 0; i < 4; i++) Rn[0][i] = -Rn[0][i];
		}
		double K[4][4];
#pragma unroll
		for (int x = 0; x < 4; x++)
#pragma unroll
			for (int y = 0; y < 4; y++)
			{
				double acc = 0.0;
#pragma unroll
				for (int i = 0; i < 4; i++)
#pragma unroll
					for (int j = 0; j < 4; j++)
					{
						if (ISO.e[x][y][i][j] > 0) acc += Rn[i][j];
						if (ISO.e[x][y][i][j] < 0) acc -= Rn[i][j];
					}
				K[x][y] = 0.25 * acc;
			}
		// K = q_r q_l^T: q_l from the row of largest norm, q_r = K q_l (its sign then fits by construction)
		double l0 = K[0][0], l1 = K[0][1], l2 = K[0][2], l3 = K[0][3];
		double n2 = (l0 * l0 + l1 * l1) + (l2 * l2 + l3 * l3);
#pragma unroll
		for (int x = 1; x < 4; x++)
		{
			const double c2 = (K[x][0] * K[x][0] + K[x][1] * K[x][1]) + (K[x][2] * K[x][2] + K[x][3] * K[x][3]);
			if (c2 > n2) { n2 = c2; l0 = K[x][0]; l1 = K[x][1]; l2 = K[x][2]; l3 = K[x][3]; }
		}
		double inv = 1.0 / sqrt(n2);
		bool ok = inv < 1e300;   // (false for NaN too)
		ql_out[0] = l0 * inv; ql_out[1] = l1 * inv; ql_out[2] = l2 * inv; ql_out[3] = l3 * inv;
		double r[4];
#pragma unroll
		for (int x = 0; x < 4; x++) r[x] = (K[x][0] * ql_out[0] + K[x][1] * ql_out[1]) + (K[x][2] * ql_out[2] + K[x][3] * ql_out[3]);
		inv = 1.0 / sqrt((r[0] * r[0] + r[1] * r[1]) + (r[2] * r[2] + r[3] * r[3]));
		ok = ok && inv < 1e300;
#pragma unroll
		for (int x = 0; x < 4; x++) qr_out[x] = r[x] * inv;
		if (!ok)   // a covariance with NaN / inf in it
		{
			ql_out[0] = 1.0; ql_out[1] = 0.0; ql_out[2] = 0.0; ql_out[3] = 0.0;
			qr_out[0] = 1.0; qr_out[1] = 0.0; qr_out[2] = 0.0; qr_out[3] = 0.0;
		}
		// scales floored as the slice kernel floors its own: the logarithm stays finite
#pragma unroll
		for (int k = 0; k < 3; k++) sc_out[k] = (float)log(fmax(sqrt(fmax(lam[k], 0.0)), 1e-15));
		sct_out = (float)log(fmax(sqrt(fmax(lam[3], 0.0)), 1e-15));
	}

	constexpr int XFORM_THREADS = 256;

	template <int MODE>
	__global__ void __launch_bounds__(XFORM_THREADS) transform_geometry_kernel(const XformArgs a)
	{
		const int idx = blockIdx.x * blockDim.x + threadIdx.x;
		if (idx >= a.P) return;
		// everything this lane reads, before anything it writes: out may alias in
		const float3 p = ld3(a.xyz, idx);
		const float3 sc = ld3(a.scales, idx);
		const float q_in[4] = { a.rot[4 * (size_t)idx], a.rot[4 * (size_t)idx + 1], a.rot[4 * (size_t)idx + 2], a.rot[4 * (size_t)idx + 3] };
		const bool has_t = a.ts != nullptr, has_st = a.scales_t != nullptr;
		const float t = has_t ? a.ts[idx] : 0.f;
		const float sct = has_st ? a.scales_t[idx] : 0.f;
		float qr_in[4] = { 1.f, 0.f, 0.f, 0.f };
		if (MODE != 0)
		{
#pragma unroll
			for (int k = 0; k < 4; k++) qr_in[k] = a.rot_r[4 * (size_t)idx + k];
		}

		// x' = s (R x) + T, each row left to right: 3 products, 2 sums, 1 product, 1 sum
		float3 o;
		o.x = a.s * ((a.R[0] * p.x + a.R[1] * p.y) + a.R[2] * p.z) + a.T[0];
		o.y = a.s * ((a.R[3] * p.x + a.R[4] * p.y) + a.R[5] * p.z) + a.T[1];
		o.z = a.s * ((a.R[6] * p.x + a.R[7] * p.y) + a.R[8] * p.z) + a.T[2];
		if (a.keep_xyz) o = p;
		const float t_out = a.keep_t ? t : a.a * t + a.b;

		float sc_out[3] = { sc.x, sc.y, sc.z }, sct_out = sct;
		float q_out[4] = { q_in[0], q_in[1], q_in[2], q_in[3] }, qr_out[4] = { qr_in[0], qr_in[1], qr_in[2], qr_in[3] };
		const double qd[4] = { (double)q_in[0], (double)q_in[1], (double)q_in[2], (double)q_in[3] };
		const double qrd[4] = { (double)qr_in[0], (double)qr_in[1], (double)qr_in[2], (double)qr_in[3] };
		if (MODE == 2)
		{
			double zl[4], zr[4];
			redecompose4(a, sc, sct, qd, qrd, sc_out, sct_out, zl, zr);
#pragma unroll
			for (int k = 0; k < 4; k++) { q_out[k] = (float)zl[k]; qr_out[k] = (float)zr[k]; }
		}
		else
		{
			if (!a.keep_rot)
			{
				double z[4];
				if (MODE == 0) quat_mul(a.q, qd, z);
				else iso_mul_l(qd, a.v, z);
#pragma unroll
				for (int k = 0; k < 4; k++) q_out[k] = (float)z[k];
				if (MODE == 1)
				{
					iso_mul_r(qrd, a.u, z);
#pragma unroll
					for (int k = 0; k < 4; k++) qr_out[k] = (float)z[k];
				}
			}
			if (!a.keep_scale)
			{
				sc_out[0] = (float)((double)sc.x + a.log_s); sc_out[1] = (float)((double)sc.y + a.log_s); sc_out[2] = (float)((double)sc.z + a.log_s);
			}
			if (!a.keep_scale_t) sct_out = (float)((double)sct + a.log_st);
		}

		st3(a.o_xyz, idx, o);
		a.o_scales[3 * (size_t)idx] = sc_out[0]; a.o_scales[3 * (size_t)idx + 1] = sc_out[1]; a.o_scales[3 * (size_t)idx + 2] = sc_out[2];
#pragma unroll
		for (int k = 0; k < 4; k++) a.o_rot[4 * (size_t)idx + k] = q_out[k];
		if (has_t) a.o_ts[idx] = t_out;
		if (has_st) a.o_scales_t[idx] = sct_out;
		if (MODE != 0)
		{
#pragma unroll
			for (int k = 0; k < 4; k++) a.o_rot_r[4 * (size_t)idx + k] = qr_out[k];
		}
	}

	// ---- the SH rows ----
	struct ShRotArgs
	{
		int n_items;         // blocks of CB coefficients in the tensor
		const float* in;
		float* out;
		float D[83];         // bands 1, 2, 3 row-major: 9 + 25 + 49
	};
	constexpr int SHROT_THREADS = 256;

	// c' = D c for one band of one channel, in place in the lane's LDS block; t points at the band's first coefficient of the channel
	template <int N>
	__device__ __forceinline__ void rotate_band(float* t, const float* D)
	{
		float c[N], o[N];
#pragma unroll
		for (int k = 0; k < N; k++) c[k] = t[3 * k];
#pragma unroll
		for (int i = 0; i < N; i++)
		{
			float p[N];
#pragma unroll
			for (int j = 0; j < N; j++) p[j] = D[i * N + j] * c[j];
			float sum;
			if constexpr (N == 3) sum = (p[0] + p[1]) + p[2];
			else if constexpr (N == 5) sum = ((p[0] + p[1]) + (p[2] + p[3])) + p[4];
			else sum = ((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + p[6]);
			o[i] = 0.f + sum;   // (-0) + (+0) = +0: a block of zeros stays +0 whatever the signs of D
		}
#pragma unroll
		for (int k = 0; k < N; k++) t[3 * k] = o[k];
	}

	// CB: coefficients per block (16; 4 or 9 for a row that short).  VEC: floats per global access.
	template <int CB, int VEC>
	__global__ void __launch_bounds__(SHROT_THREADS) sh_rotate_kernel(const ShRotArgs a)
	{
		constexpr int BF = 3 * CB, STRIDE = BF | 1;
		__shared__ float tile[SHROT_THREADS * STRIDE];
		const int item0 = blockIdx.x * SHROT_THREADS;
		const int n = min(SHROT_THREADS, a.n_items - item0);
		const size_t f0 = (size_t)item0 * BF;
		const int nf = n * BF;
		const int tid = threadIdx.x;
		const float* src = a.in + f0;
		float* dst = a.out + f0;
		if constexpr (VEC == 4)
		{
			for (int e = 4 * tid; e + 3 < nf; e += 4 * SHROT_THREADS)
			{
				const float4 v = *reinterpret_cast<const float4*>(src + e);   // (f0 and e are multiples of 4, the base is 16-byte aligned)
				const float w[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
				for (int k = 0; k < 4; k++) tile[((e + k) / BF) * STRIDE + (e + k) % BF] = w[k];
			}
			const int e = (nf & ~3) + tid;
			if (e < nf) tile[(e / BF) * STRIDE + e % BF] = src[e];
		}
		else
		{
			for (int e = tid; e < nf; e += SHROT_THREADS) tile[(e / BF) * STRIDE + e % BF] = src[e];
		}
		__syncthreads();
		if (tid < n)
		{
			float* blk = tile + tid * STRIDE;
#pragma unroll
			for (int ch = 0; ch < 3; ch++)
			{
				rotate_band<3>(blk + 3 * 1 + ch, a.D);
				if constexpr (CB >= 9) rotate_band<5>(blk + 3 * 4 + ch, a.D + 9);
				if constexpr (CB >= 16) rotate_band<7>(blk + 3 * 9 + ch, a.D + 34);
			}
		}
		__syncthreads();
		if constexpr (VEC == 4)
		{
			for (int e = 4 * tid; e + 3 < nf; e += 4 * SHROT_THREADS)
			{
				float w[4];
#pragma unroll
				for (int k = 0; k < 4; k++) w[k] = tile[((e + k) / BF) * STRIDE + (e + k) % BF];
				*reinterpret_cast<float4*>(dst + e) = make_float4(w[0], w[1], w[2], w[3]);
			}
			const int e = (nf & ~3) + tid;
			if (e < nf) dst[e] = tile[(e / BF) * STRIDE + e % BF];
		}
		else
		{
			for (int e = tid; e < nf; e += SHROT_THREADS) dst[e] = tile[(e / BF) * STRIDE + e % BF];
		}
	}

	template <int CB>
	static void launch_sh_rotate(const ShRotArgs& a, hipStream_t stream)
	{
		const int nb = div_up(a.n_items, SHROT_THREADS);
		const bool vec = (reinterpret_cast<uintptr_t>(a.in) & 15) == 0 && (reinterpret_cast<uintptr_t>(a.out) & 15) == 0;
		if (vec) hipLaunchKernelGGL((sh_rotate_kernel<CB, 4>), dim3(nb), dim3(SHROT_THREADS), 0, stream, a);
		else hipLaunchKernelGGL((sh_rotate_kernel<CB, 1>), dim3(nb), dim3(SHROT_THREADS), 0, stream, a);
	}

	hipError_t launch_model_transform(const fdgs_transform_in& in, const fdgs_transform_out& out, hipStream_t stream)
	{
		if (in.P <= 0) return hipSuccess;
		bool rot_identity = true;
		for (int i = 0; i < 3; i++)
			for (int j = 0; j < 3; j++) rot_identity = rot_identity && in.rotation[3 * i + j] == (i == j ? 1.0 : 0.0);
		XformArgs a;
		a.P = in.P;
		a.xyz = in.means3D; a.ts = in.ts; a.scales = in.scales; a.scales_t = in.scales_t; a.rot = in.rotations; a.rot_r = in.rotations_r;
		a.o_xyz = out.means3D; a.o_ts = out.ts; a.o_scales = out.scales; a.o_scales_t = out.scales_t; a.o_rot = out.rotations; a.o_rot_r = out.rotations_r;
		if (in.gaussian_dim != 4) { a.ts = nullptr; a.scales_t = nullptr; }
		for (int k = 0; k < 9; k++) { a.R[k] = (float)in.rotation[k]; a.Rd[k] = in.rotation[k]; }
		for (int k = 0; k < 3; k++) a.T[k] = (float)in.translation[k];
		a.s = (float)in.scale; a.a = (float)in.time_scale; a.b = (float)in.time_shift;
		a.sd = in.scale; a.ad = in.time_scale;
		for (int k = 0; k < 4; k++) { a.q[k] = in.quat[k]; a.u[k] = in.iso_u[k]; a.v[k] = in.iso_v[k]; }
		a.log_s = in.log_scale;
		a.log_st = in.rot_4d ? in.log_time_scale : 2.0 * in.log_time_scale;   // a standard deviation with rot_4d, a variance without
		a.keep_rot = rot_identity;
		a.keep_xyz = rot_identity && in.scale == 1.0 && in.translation[0] == 0.0 && in.translation[1] == 0.0 && in.translation[2] == 0.0;
		a.keep_t = in.time_scale == 1.0 && in.time_shift == 0.0;
		a.keep_scale = in.scale == 1.0;
		a.keep_scale_t = in.time_scale == 1.0;
		const int nb = div_up(in.P, XFORM_THREADS);
		if (!in.rot_4d) hipLaunchKernelGGL(transform_geometry_kernel<0>, dim3(nb), dim3(XFORM_THREADS), 0, stream, a);
		else if (in.scale == in.time_scale) hipLaunchKernelGGL(transform_geometry_kernel<1>, dim3(nb), dim3(XFORM_THREADS), 0, stream, a);
		else hipLaunchKernelGGL(transform_geometry_kernel<2>, dim3(nb), dim3(XFORM_THREADS), 0, stream, a);
		hipError_t e = hipGetLastError();
		if (e != hipSuccess || in.shs == nullptr) return e;

		if (rot_identity || in.M < 4)   // nothing rotates: the copy is the whole job
		{
			if (in.shs != out.shs) return hipMemcpyAsync(out.shs, in.shs, (size_t)in.P * in.M * 3 * sizeof(float), hipMemcpyDeviceToDevice, stream);
			return hipSuccess;
		}
		ShRotArgs s;
		s.in = in.shs; s.out = out.shs;
		for (int k = 0; k < 83; k++) s.D[k] = in.sh_rot[k];
		if (in.M >= 16) { s.n_items = in.P * (in.M / 16); launch_sh_rotate<16>(s, stream); }
		else if (in.M == 9) { s.n_items = in.P; launch_sh_rotate<9>(s, stream); }
		else { s.n_items = in.P; launch_sh_rotate<4>(s, stream); }
		return hipGetLastError();
	}
}
