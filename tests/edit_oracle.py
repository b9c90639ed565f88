"""float64 numpy statement of what ``fdgs.edit.transform`` computes, written from the formulas and independent of fdgs.edit:

* the transformed means, times and covariances ``A Sigma A^T``, ``A = diag(s R, a)``, from the model's raw fp32 parameters;
* the covariance a set of raw OUTPUT parameters stands for (``rebuild4`` / ``rebuild3``);
* a float64 decomposition of a 4x4 covariance back into raw parameters (numpy ``eigh``, the isoclinic pair by SVD), whose fp32
  rounding is the yardstick of the GPU tests: no fp32 output can be expected to do better than that;
* SH rotation matrices from a least-squares fit over sampled directions, on a float64 restatement of the basis.
"""
import numpy as np

import slice_oracle as so

EPS32 = 2.0 ** -23


# ---- SH ----
def sh_basis(d):
    """[n,16]: the real SH basis of the kernels (sh_tables in csrc/sh_eval.h), restated from the header in float64."""
    d = np.asarray(d, np.float64)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    c1 = 0.4886025119029199
    c2 = [1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396]
    c3 = [-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658, 1.445305721320277,
          -0.5900435899266435]
    Y = np.zeros((d.shape[0], 16))
    Y[:, 0] = 0.28209479177387814
    Y[:, 1], Y[:, 2], Y[:, 3] = -c1 * y, c1 * z, -c1 * x
    Y[:, 4], Y[:, 5] = c2[0] * x * y, c2[1] * y * z
    Y[:, 6] = c2[2] * (2.0 * z * z - x * x - y * y)
    Y[:, 7], Y[:, 8] = c2[3] * x * z, c2[4] * (x * x - y * y)
    Y[:, 9] = c3[0] * y * (3 * x * x - y * y)
    Y[:, 10] = c3[1] * x * y * z
    Y[:, 11] = c3[2] * y * (4 * z * z - x * x - y * y)
    Y[:, 12] = c3[3] * z * (2 * z * z - 3 * x * x - 3 * y * y)
    Y[:, 13] = c3[4] * x * (4 * z * z - x * x - y * y)
    Y[:, 14] = c3[5] * z * (x * x - y * y)
    Y[:, 15] = c3[6] * x * (x * x - 3 * y * y)
    return Y


def random_directions(n, seed=0):
    d = np.random.default_rng(seed).standard_normal((n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def sh_rotation_fit(R, n=600, seed=11):
    """[16,16]: D with sum_k (D c)_k Y_k(R d) = sum_k c_k Y_k(d), band by band as the least-squares solution of Y(R d) D = Y(d) over
    ``n`` random directions (exactly solvable: the residual is rounding)."""
    R = np.asarray(R, np.float64)
    d = random_directions(n, seed)
    Y, Yr = sh_basis(d), sh_basis(d @ R.T)
    D = np.zeros((16, 16))
    for lo, hi in ((0, 1), (1, 4), (4, 9), (9, 16)):
        D[lo:hi, lo:hi] = np.linalg.lstsq(Yr[:, lo:hi], Y[:, lo:hi], rcond=None)[0]
    return D


# ---- rotations ----
def random_rotation(seed):
    q = np.random.default_rng(seed).standard_normal(4)
    return so.rotation_matrix(q[None])[0]


def axis_angle(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def Ml(q):
    a, b, c, d = q
    return np.array([[a, b, -c, d], [-b, a, d, c], [c, -d, a, b], [-d, -c, -b, a]], np.float64).T   # the literals are the columns


def Mr(q):
    p, q_, r, s = q
    return np.array([[p, q_, -r, -s], [-q_, p, s, -r], [r, -s, p, -q_], [s, r, q_, p]], np.float64).T


# ---- what a model's raw parameters stand for ----
def f64(raw, k):
    return np.asarray(raw[k], np.float64)


def rebuild4(raw):
    """[P,4,4]: R4^T S^2 R4 of raw rot_4d parameters (exp, F.normalize in float64)."""
    return so.sigma4(np.exp(f64(raw, "_scaling")), np.exp(f64(raw, "_scaling_t")).reshape(-1), f64(raw, "_rotation"), f64(raw, "_rotation_r"), 1.0)


def rebuild3(raw):
    """([P,3,3], [P]): R S^2 R^T and the temporal VARIANCE exp(_scaling_t) of raw parameters without rot_4d."""
    var_t = np.exp(f64(raw, "_scaling_t")).reshape(-1) if raw.get("_scaling_t") is not None else None
    return so.sigma3(np.exp(f64(raw, "_scaling")), f64(raw, "_rotation"), 1.0), var_t


def transformed_means(raw, R, T, s, a, b):
    """(xyz', t', bound_xyz, bound_t): float64 values and the 4 eps32 (sum_j |s R_ij| |x_j| + |T_i|) error bars: per term at most
    the roundings of R, s, the product, two sums, the product with s and the sum with T -- 7 half-ulps = 3.5 eps32."""
    x = f64(raw, "_xyz")
    sR = s * np.asarray(R, np.float64)
    xyz = x @ sR.T + np.asarray(T, np.float64)
    bound = 4 * EPS32 * (np.abs(x) @ np.abs(sR).T + np.abs(np.asarray(T, np.float64)))
    t = f64(raw, "_t").reshape(-1)
    return xyz, a * t + b, bound, 4 * EPS32 * (abs(a) * np.abs(t) + abs(b))


def transformed_cov4(raw, R, s, a):
    A = np.zeros((4, 4))
    A[:3, :3] = s * np.asarray(R, np.float64)
    A[3, 3] = a
    return A @ rebuild4(raw) @ A.T


def transformed_cov3(raw, R, s, a):
    S3, var_t = rebuild3(raw)
    sR = s * np.asarray(R, np.float64)
    return sR @ S3 @ sR.T, (None if var_t is None else a * a * var_t)


def rel_fro(got, want):
    """per Gaussian |got - want|_F / |want|_F"""
    return np.sqrt(((got - want) ** 2).sum((1, 2))) / np.sqrt((want ** 2).sum((1, 2)))


# ---- the yardstick: float64 decompositions, rounded to fp32 storage ----
def _iso_basis():
    e = np.eye(4)
    return np.array([[Mr(e[a_]) @ Ml(e[b_]) for b_ in range(4)] for a_ in range(4)])


_ISO_BASIS = _iso_basis()


def isoclinic_factor(R4):
    """(q_l, q_r) unit with Mr(q_r) Ml(q_l) = +-R4 (R4 in SO(4)): the coefficients <Mr(e_a) Ml(e_b), R4> / 4 form q_r q_l^T."""
    K = np.einsum("abij,ij->ab", _ISO_BASIS, R4) / 4.0
    U, S, Vt = np.linalg.svd(K)
    return Vt[0], U[:, 0]


def decompose4(Sigma):
    """Raw float64 parameters {_scaling [P,3], _scaling_t [P,1], _rotation, _rotation_r [P,4]} with rebuild4(...) == Sigma."""
    P = Sigma.shape[0]
    out = {"_scaling": np.zeros((P, 3)), "_scaling_t": np.zeros((P, 1)), "_rotation": np.zeros((P, 4)), "_rotation_r": np.zeros((P, 4))}
    for i in range(P):
        lam, V = np.linalg.eigh(Sigma[i])
        m = int(np.argmax(np.abs(V[3])))
        order = [j for j in range(4) if j != m] + [m]
        R4 = V[:, order].T.copy()
        if np.linalg.det(R4) < 0:
            R4[0] = -R4[0]
        ql, qr = isoclinic_factor(R4)
        if np.abs(Mr(qr) @ Ml(ql) - R4).max() > 1e-9:
            qr = -qr
        assert np.abs(Mr(qr) @ Ml(ql) - R4).max() < 1e-9
        sc = 0.5 * np.log(np.maximum(lam[order], 1e-300))
        out["_scaling"][i], out["_scaling_t"][i, 0], out["_rotation"][i], out["_rotation_r"][i] = sc[:3], sc[3], ql, qr
    return out


def to_fp32(raw):
    return {k: (None if v is None else np.asarray(v, np.float32)) for k, v in raw.items()}


def yardstick4(Sigma):
    """(per-Gaussian relative Frobenius error of the float64 decomposition after rounding to fp32 storage, the rounded parameters)"""
    r32 = to_fp32(decompose4(Sigma))
    return rel_fro(rebuild4(r32), Sigma), r32


def quat_mul(a, b):
    """Hamilton product of (w, x, y, z) rows"""
    aw, ax, ay, az = a.T
    bw, bx, by, bz = b.T
    return np.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], axis=1)


def quat_of(R):
    """unit (w, x, y, z) of a rotation matrix, through the eigenvector of the symmetric 4x4 (Bar-Itzhack)"""
    K = np.array([[R[0, 0] - R[1, 1] - R[2, 2], R[1, 0] + R[0, 1], R[2, 0] + R[0, 2], R[2, 1] - R[1, 2]],
                  [R[1, 0] + R[0, 1], R[1, 1] - R[0, 0] - R[2, 2], R[2, 1] + R[1, 2], R[0, 2] - R[2, 0]],
                  [R[2, 0] + R[0, 2], R[2, 1] + R[1, 2], R[2, 2] - R[0, 0] - R[1, 1], R[1, 0] - R[0, 1]],
                  [R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1], R[0, 0] + R[1, 1] + R[2, 2]]]) / 3.0
    w, v = np.linalg.eigh(K)
    x, y, z, ww = v[:, -1]
    return np.array([ww, x, y, z])


def exact3(raw, R, s, a):
    """The float64 raw parameters of the transformed model without rot_4d: q' = q_R * unit(q), log scales + log s, log var_t + 2 log a."""
    q = f64(raw, "_rotation")
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    out = {"_rotation": quat_mul(np.repeat(quat_of(np.asarray(R, np.float64))[None], q.shape[0], 0), q),
           "_scaling": f64(raw, "_scaling") + np.log(s), "_scaling_t": None}
    if raw.get("_scaling_t") is not None:
        out["_scaling_t"] = f64(raw, "_scaling_t") + 2.0 * np.log(a)
    return out


def yardstick3(raw, R, s, a):
    """(error of the 3x3 covariance, error of the temporal variance or None, the rounded parameters) of exact3 rounded to fp32"""
    want, want_t = transformed_cov3(raw, R, s, a)
    r32 = to_fp32(exact3(raw, R, s, a))
    got, got_t = rebuild3(r32)
    return rel_fro(got, want), (None if want_t is None else np.abs(got_t - want_t) / want_t), r32
