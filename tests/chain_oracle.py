"""Float64 oracle of the per-Gaussian backward: what preprocess_bwd.hip and sh_bwd.hip / sh_eval.h compute for ONE Gaussian from the
scene parameters, the forward's records and the accumulator record -- plain numpy, vectorised over Gaussians, nothing taken from the
product.  It restates the reference backward (diff-gaussian-rasterization/cuda_rasterizer/backward.cu), bug-compatible with the quirks
listed at the top of preprocess_bwd.hip:

    Q1  dL_dsh[1] uses the degree-0 basis in the 4D path        (backward.cu:190)       -> sh_backward
    Q2  d cos / dt has the wrong sign                           (backward.cu:303, 384)  -> sh_backward
    Q3  the k = 2 time term overwrites the k = 1 term           (backward.cu:403)       -> sh_backward
    Q4  SH view direction from the SHIFTED mean                 (backward.cu:148-153)   -> sh_backward reads out_means3D
    Q5  the whole dL_dmean is fed back as dL_d(delta_mean)      (backward.cu:771-779)   -> cov4_conditional_backward
    Q6  no marginal-opacity backward for gaussian_dim 4 without rot_4d (backward.cu:913-921)
    Q7  cov12 read as Sigma[3][k], Sigma[k][3] in the forward   (backward.cu:735)       -> cov4_conditional_backward
        (Sigma = M^T M is symmetric term by term, so Q7 changes no number: tests/test_chain_oracle_host.py says so with an assert)

``analytic_sh`` switches Q1-Q3 to the analytic gradient of the forward (fdgs_scene.analytic_sh_grad).

The accumulator record of a Gaussian, as the comment in preprocess_bwd.hip lays it out ([P,12] here; words 12..15 are the SH
backward's hand-over, an OUTPUT of this oracle): words 0-2 colour, 3 depth carrier, 4-5 flow, 6-10 the moments Mx, My, Mxx, Myy, Mxy
(pixel sums of q d^n, q = G dL/dalpha, d = mean2D - pixel), 11 opacity.

Matrices are kept as the kernels and GLM keep them: ``c[..., column, row]``; ``mul(A, B)`` is the matrix product A B in that layout.
Constants written with an ``f`` suffix in the kernels are their fp32 values here; everything else is float64.

``plant``: evaluate with ONE deliberately wrong term (PLANTS) -- tests/test_chain_oracle_host.py shows that the comparison flags each.
"""
import numpy as np


def f32(x):
    return float(np.float32(x))


SH_C0 = f32(0.28209479177387814)
SH_C1 = f32(0.4886025119029199)
SH_C2 = [f32(v) for v in (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)]
SH_C3 = [f32(v) for v in (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
                          1.445305721320277, -0.5900435899266435)]
REF_PI = 3.14159265   # auxiliary.h:20, a double
LOWPASS = f32(0.3)
CLAMP = f32(1.3)
EPS7 = f32(0.0000001)

PLANTS = ("half", "q7", "clamp", "quat_sign", "q1", "sh_c3", "sigmoid2")
OUTPUTS = ("sh_words", "stage", "dL_dsh", "dL_dmean2D", "dL_dcolor", "dL_dflows", "dL_dcov3D", "dL_dmean3D", "dL_dopacity", "dL_dts",
           "dL_dscale", "dL_dscale_t", "dL_drot", "dL_drot_r")


def mul(A, B):
    """(A B) in c[column][row] layout: R.c[j][i] = sum_k A.c[k][i] B.c[j][k] (glm/detail/type_mat3x3.inl:486, type_mat4x4.inl:630)."""
    return np.einsum("...ki,...jk->...ji", A, B)


def tr(A):
    return np.swapaxes(A, -1, -2)


def cols(rows):
    """c[..., j, i] from nested lists l[j][i] of [P] arrays."""
    return np.stack([np.stack(c, axis=-1) for c in rows], axis=-2)


def _f64(x):
    return None if x is None else np.asarray(x, np.float64)


# ---------------------------------------------------------------------------------------------------------------------------------
# SH / 4D-SH backward: computeColorFromSH backward.cu:20-139, computeColorFromSH_4D backward.cu:144-481 (sh_eval.h: sh_tables,
# ShBwdEval::begin / block / finish, sh_grad_basis0, sh_time_factor(_dt); sh_bwd.hip: which rows and words are written)
# ---------------------------------------------------------------------------------------------------------------------------------
def sh_tables(deg, x, y, z, c3):
    """Basis values l[k] and their x / y / z derivatives (forward.cu:87-131, backward.cu:172-263); zero where the reference has no term."""
    P = x.shape[0]
    l, dX, dY, dZ = (np.zeros((P, 16)) for _ in range(4))
    l[:, 0] = SH_C0
    if deg > 0:
        l[:, 1], l[:, 2], l[:, 3] = -SH_C1 * y, SH_C1 * z, -SH_C1 * x
        dY[:, 1], dZ[:, 2], dX[:, 3] = -SH_C1, SH_C1, -SH_C1
    if deg > 1:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        C = SH_C2
        l[:, 4], l[:, 5], l[:, 6], l[:, 7], l[:, 8] = C[0] * xy, C[1] * yz, C[2] * (2 * zz - xx - yy), C[3] * xz, C[4] * (xx - yy)
        dX[:, 4], dY[:, 4] = C[0] * y, C[0] * x
        dY[:, 5], dZ[:, 5] = C[1] * z, C[1] * y
        dX[:, 6], dY[:, 6], dZ[:, 6] = -2 * C[2] * x, -2 * C[2] * y, 4 * C[2] * z
        dX[:, 7], dZ[:, 7] = C[3] * z, C[3] * x
        dX[:, 8], dY[:, 8] = 2 * C[4] * x, -2 * C[4] * y
    if deg > 2:
        C = c3
        l[:, 9] = C[0] * y * (3 * xx - yy)
        l[:, 10] = C[1] * xy * z
        l[:, 11] = C[2] * y * (4 * zz - xx - yy)
        l[:, 12] = C[3] * z * (2 * zz - 3 * xx - 3 * yy)
        l[:, 13] = C[4] * x * (4 * zz - xx - yy)
        l[:, 14] = C[5] * z * (xx - yy)
        l[:, 15] = C[6] * x * (xx - 3 * yy)
        dX[:, 9], dY[:, 9] = C[0] * y * 6 * x, C[0] * (3 * xx - 3 * yy)
        dX[:, 10], dY[:, 10], dZ[:, 10] = C[1] * yz, C[1] * xz, C[1] * xy
        dX[:, 11], dY[:, 11], dZ[:, 11] = -C[2] * y * 2 * x, C[2] * (4 * zz - xx - 3 * yy), C[2] * y * 8 * z
        dX[:, 12], dY[:, 12], dZ[:, 12] = -C[3] * z * 6 * x, -C[3] * z * 6 * y, C[3] * (6 * zz - 3 * xx - 3 * yy)
        dX[:, 13], dY[:, 13], dZ[:, 13] = C[4] * (4 * zz - 3 * xx - yy), -C[4] * x * 2 * y, C[4] * x * 8 * z
        dX[:, 14], dY[:, 14], dZ[:, 14] = C[5] * z * 2 * x, -C[5] * z * 2 * y, C[5] * (xx - yy)
        dX[:, 15], dY[:, 15] = C[6] * (3 * xx - 3 * yy), -C[6] * x * 6 * y
    return l, dX, dY, dZ


def dnormvdv(v, dv):
    """Backward of v / |v| (auxiliary.h:108-118)."""
    sum2 = (v * v).sum(1)
    inv = 1.0 / np.sqrt(sum2 * sum2 * sum2)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    dx, dy, dz = dv[:, 0], dv[:, 1], dv[:, 2]
    return np.stack([((sum2 - x * x) * dx - y * x * dy - z * x * dz) * inv,
                     (-x * y * dx + (sum2 - y * y) * dy - z * y * dz) * inv,
                     (-x * z * dx - y * z * dy + (sum2 - z * z) * dz) * inv], axis=1)


def sh_plan(D, D_t, gaussian_dim, force_sh_3d):
    """(3D SH?, coefficients of block 0, blocks): time blocks only on a complete degree-3 block of the 4D path (forward.cu:133-192)."""
    sh3d = gaussian_dim == 3 or bool(force_sh_3d)
    return sh3d, min(16, (D + 1) ** 2), (1 + min(max(D_t, 0), 2)) if (not sh3d and D > 2) else 1


def sh_backward(inp, rec, acc, plant=None):
    """-> (live [P] bool, words [P,4], stage [P,8], dL_dsh [P,M,3]).  A Gaussian is live when it is visible (backward.cu:873) and a
    colour gradient is left after the clamp bits zeroed theirs (backward.cu:158-161); every output of the others is zero."""
    P, M, D = inp["P"], inp["M"], inp["D"]
    sh3d, ncoef0, nblocks = sh_plan(D, inp["D_t"], inp["gaussian_dim"], inp["force_sh_3d"])
    analytic = bool(inp.get("analytic_sh"))
    shs = _f64(inp["shs"]).reshape(P, M, 3)
    dRGB = np.where(np.asarray(rec["clamped"]).reshape(P, 3) != 0, 0.0, _f64(acc)[:, 0:3])
    live = (np.asarray(rec["radii"]) > 0) & (dRGB != 0).any(1)
    with np.errstate(all="ignore"):
        dir_orig = _f64(rec["out_means3D"]) - _f64(inp["campos"]).reshape(1, 3)   # Q4: the shifted mean
        dirn = dir_orig / np.sqrt((dir_orig * dir_orig).sum(1, keepdims=True))
        c3 = list(SH_C3)
        if plant == "sh_c3":
            c3[1] = 2.890161442640554   # two digits swapped
        l, dX, dY, dZ = sh_tables(D, dirn[:, 0], dirn[:, 1], dirn[:, 2], c3)
        dir_t = np.zeros(P) if sh3d else _f64(inp["ts"]).reshape(P) - inp["timestamp"]
        dsh = np.zeros((P, M, 3))
        g = [np.zeros((P, 3)) for _ in range(4)]   # d colour / d dir.x, .y, .z, / dt, per channel
        tk_stage = np.zeros((P, 2))
        T = inp["time_duration"]
        for blk in range(nblocks):
            nk = ncoef0 if blk == 0 else 16
            s = shs[:, 16 * blk:16 * blk + nk, :]
            if blk == 0:
                tk, dtk = np.ones(P), np.zeros(P)
                basis = l[:, :nk].copy()
                if nk > 1 and not sh3d and not analytic and plant != "q1":
                    basis[:, 1] = l[:, 0]                                    # Q1
            else:
                u = 2 * REF_PI * dir_t * blk / T
                tk = np.cos(u)
                dtk = np.sin(u) * 2 * REF_PI * blk / T                      # Q2: the reference's sign
                if analytic:
                    dtk = -dtk
                basis = tk[:, None] * l[:, :nk]
                tk_stage[:, blk - 1] = tk
            dsh[:, 16 * blk:16 * blk + nk, :] = basis[:, :, None] * dRGB[:, None, :]
            st, sx, sy, sz = ((t[:, :nk, None] * s).sum(1) for t in (l, dX, dY, dZ))
            if blk == 0:
                g[0], g[1], g[2] = sx, sy, sz
            else:
                g[0], g[1], g[2] = g[0] + tk[:, None] * sx, g[1] + tk[:, None] * sy, g[2] + tk[:, None] * sz
                g[3] = g[3] + dtk[:, None] * st if analytic else dtk[:, None] * st   # Q3: overwrite
        ddir = np.stack([(g[k] * dRGB).sum(1) for k in range(3)], axis=1)
        words = np.concatenate([dnormvdv(dir_orig, ddir), np.zeros((P, 1)) if sh3d else (g[3] * dRGB).sum(1, keepdims=True)], axis=1)
        stage = np.concatenate([dRGB, tk_stage[:, 0:1], dirn, tk_stage[:, 1:2]], axis=1)
    lv = live[:, None]
    return live, np.where(lv, words, 0.0), np.where(lv, stage, 0.0), np.where(live[:, None, None], dsh, 0.0)


# ---------------------------------------------------------------------------------------------------------------------------------
# Geometry
# ---------------------------------------------------------------------------------------------------------------------------------
def project_cov(mean, fx, fy, tanx, tany, cov3D, vm):
    """The EWA projection the backward rebuilds (backward.cu:509-537 = forward.cu:198-237; fdgs_math.h project_cov)."""
    P = mean.shape[0]
    x, y, z = mean[:, 0], mean[:, 1], mean[:, 2]
    t = np.stack([vm[0] * x + vm[4] * y + vm[8] * z + vm[12], vm[1] * x + vm[5] * y + vm[9] * z + vm[13],
                  vm[2] * x + vm[6] * y + vm[10] * z + vm[14]], axis=1)
    limx, limy = CLAMP * tanx, CLAMP * tany
    txtz, tytz = t[:, 0] / t[:, 2], t[:, 1] / t[:, 2]
    tx = np.minimum(limx, np.maximum(-limx, txtz)) * t[:, 2]
    ty = np.minimum(limy, np.maximum(-limy, tytz)) * t[:, 2]
    tz = t[:, 2]
    z0 = np.zeros(P)
    J = cols([[fx / tz, z0, -(fx * tx) / (tz * tz)], [z0, fy / tz, -(fy * ty) / (tz * tz)], [z0, z0, z0]])
    o = np.ones(P)
    W = cols([[vm[0] * o, vm[4] * o, vm[8] * o], [vm[1] * o, vm[5] * o, vm[9] * o], [vm[2] * o, vm[6] * o, vm[10] * o]])
    T = mul(W, J)
    c = cov3D
    Vrk = cols([[c[:, 0], c[:, 1], c[:, 2]], [c[:, 1], c[:, 3], c[:, 4]], [c[:, 2], c[:, 4], c[:, 5]]])
    cov = mul(mul(tr(T), tr(Vrk)), T)
    return dict(t=np.stack([tx, ty, tz], axis=1), txtz=txtz, tytz=tytz, T=T, Vrk=Vrk, W=W, a=cov[:, 0, 0], b=cov[:, 0, 1], c=cov[:, 1, 1])


def cov2d_backward(inp, mean, cov3D, g_conic, g_depth, plant=None):
    """computeCov2DCUDA, backward.cu:486-617 -> (dL_dcov3D [P,6], the view-space part of dL_dmean [P,3]), including the
    1.3 * tan_fov gradient clamps (x_grad_mul, y_grad_mul) and the depth carrier in dL_dmean2D.z (Q10)."""
    fx, fy, tanx, tany, vm = inp["focal_x"], inp["focal_y"], inp["tan_fovx"], inp["tan_fovy"], inp["viewmatrix"]
    p = project_cov(mean, fx, fy, tanx, tany, cov3D, vm)
    limx, limy = CLAMP * tanx, CLAMP * tany
    xmul = np.where((p["txtz"] < -limx) | (p["txtz"] > limx), 0.0, 1.0)
    ymul = np.where((p["tytz"] < -limy) | (p["tytz"] > limy), 0.0, 1.0)
    if plant == "clamp":
        xmul = np.ones_like(xmul)
    dcx, dcy, dcz = g_conic[:, 0], g_conic[:, 1], g_conic[:, 2]
    ca, cb, cc = p["a"] + LOWPASS, p["b"], p["c"] + LOWPASS
    denom = ca * cc - cb * cb
    d2 = 1.0 / (denom * denom + EPS7)
    dL_da = d2 * (-cc * cc * dcx + 2 * cb * cc * dcy + (denom - ca * cc) * dcz)
    dL_dc = d2 * (-ca * ca * dcz + 2 * ca * cb * dcy + (denom - ca * cc) * dcx)
    dL_db = d2 * 2 * (cb * cc * dcx - (denom + 2 * cb * cb) * dcy + ca * cb * dcz)
    T, V, W = p["T"], p["Vrk"], p["W"]
    TT = lambda i, j: T[:, i, j]   # noqa: E731
    dcov = np.stack([
        TT(0, 0) * TT(0, 0) * dL_da + TT(0, 0) * TT(1, 0) * dL_db + TT(1, 0) * TT(1, 0) * dL_dc,
        2 * TT(0, 0) * TT(0, 1) * dL_da + (TT(0, 0) * TT(1, 1) + TT(0, 1) * TT(1, 0)) * dL_db + 2 * TT(1, 0) * TT(1, 1) * dL_dc,
        2 * TT(0, 0) * TT(0, 2) * dL_da + (TT(0, 0) * TT(1, 2) + TT(0, 2) * TT(1, 0)) * dL_db + 2 * TT(1, 0) * TT(1, 2) * dL_dc,
        TT(0, 1) * TT(0, 1) * dL_da + TT(0, 1) * TT(1, 1) * dL_db + TT(1, 1) * TT(1, 1) * dL_dc,
        2 * TT(0, 2) * TT(0, 1) * dL_da + (TT(0, 1) * TT(1, 2) + TT(0, 2) * TT(1, 1)) * dL_db + 2 * TT(1, 1) * TT(1, 2) * dL_dc,
        TT(0, 2) * TT(0, 2) * dL_da + TT(0, 2) * TT(1, 2) * dL_db + TT(1, 2) * TT(1, 2) * dL_dc], axis=1)
    # dL_dT[r][j] = 2 (T[r] . Vrk[j]) dL_d(a|c) + (T[1-r] . Vrk[j]) dL_db   (backward.cu:569-580)
    TV = np.einsum("prk,pjk->prj", T[:, 0:2, :], V)
    dT0 = 2 * TV[:, 0, :] * dL_da[:, None] + TV[:, 1, :] * dL_db[:, None]
    dT1 = 2 * TV[:, 1, :] * dL_dc[:, None] + TV[:, 0, :] * dL_db[:, None]
    dJ00 = (W[:, 0, :] * dT0).sum(1)
    dJ02 = (W[:, 2, :] * dT0).sum(1)
    dJ11 = (W[:, 1, :] * dT1).sum(1)
    dJ12 = (W[:, 2, :] * dT1).sum(1)
    t = p["t"]
    tz = 1.0 / t[:, 2]
    tz2, tz3 = tz * tz, tz * tz * tz
    dtx = xmul * -fx * tz2 * dJ02
    dty = ymul * -fy * tz2 * dJ12
    dtz = -fx * tz2 * dJ00 - fy * tz2 * dJ11 + (2 * fx * t[:, 0]) * tz3 * dJ02 + (2 * fy * t[:, 1]) * tz3 * dJ12
    vz = dtz + g_depth
    dmean = np.stack([vm[0] * dtx + vm[1] * dty + vm[2] * vz, vm[4] * dtx + vm[5] * dty + vm[6] * vz,
                      vm[8] * dtx + vm[9] * dty + vm[10] * vz], axis=1)   # transformVec4x3Transpose, auxiliary.h:90-98
    return dcov, dmean


def projection_backward(inp, mean, gx, gy):
    """The projection term of preprocessCUDA's backward, backward.cu:877-894."""
    pj = inp["projmatrix"]
    x, y, z = mean[:, 0], mean[:, 1], mean[:, 2]
    w = pj[3] * x + pj[7] * y + pj[11] * z + pj[15]
    m_w = 1.0 / (w + EPS7)
    mul1 = (pj[0] * x + pj[4] * y + pj[8] * z + pj[12]) * m_w * m_w
    mul2 = (pj[1] * x + pj[5] * y + pj[9] * z + pj[13]) * m_w * m_w
    return np.stack([(pj[0] * m_w - pj[3] * mul1) * gx + (pj[1] * m_w - pj[3] * mul2) * gy,
                     (pj[4] * m_w - pj[7] * mul1) * gx + (pj[5] * m_w - pj[7] * mul2) * gy,
                     (pj[8] * m_w - pj[11] * mul1) * gx + (pj[9] * m_w - pj[11] * mul2) * gy], axis=1)


def sym_split(d, plant=None):
    """The symmetric dL_dSigma of the six upper-triangle gradients: off-diagonal halves split (backward.cu:645-649)."""
    h = 0.5
    h01 = 1.0 if plant == "half" else 0.5
    return cols([[d[:, 0], h01 * d[:, 1], h * d[:, 2]], [h * d[:, 1], d[:, 3], h * d[:, 4]], [h * d[:, 2], h * d[:, 4], d[:, 5]]])


def quat_to_R(q):
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return cols([[1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)],
                 [2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)],
                 [2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)]])   # forward.cu:251-262


def cov3_backward(sc, mod, q, dcov, plant=None):
    """computeCov3D backward, backward.cu:621-684 -> (dL_dscale [P,3], dL_drot [P,4]) of the normalised quaternion."""
    scl = mod * sc
    R = quat_to_R(q)
    Mm = R * scl[:, None, :]                    # mul(S, R): row i of every column times scl[i]
    dSig = sym_split(dcov, plant)
    dM = mul(2.0 * Mm, dSig)
    Rt, dMt = tr(R), tr(dM)
    dscale = (Rt * dMt).sum(2)
    dMt = dMt * scl[:, :, None]
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    DD = lambda i, j: dMt[:, i, j]   # noqa: E731
    sgn = -1.0 if plant == "quat_sign" else 1.0
    drot = np.stack([
        sgn * 2 * z * (DD(0, 1) - DD(1, 0)) + 2 * y * (DD(2, 0) - DD(0, 2)) + 2 * x * (DD(1, 2) - DD(2, 1)),
        2 * y * (DD(1, 0) + DD(0, 1)) + 2 * z * (DD(2, 0) + DD(0, 2)) + 2 * r * (DD(1, 2) - DD(2, 1)) - 4 * x * (DD(2, 2) + DD(1, 1)),
        2 * x * (DD(1, 0) + DD(0, 1)) + 2 * r * (DD(2, 0) - DD(0, 2)) + 2 * z * (DD(1, 2) + DD(2, 1)) - 4 * y * (DD(2, 2) + DD(0, 0)),
        2 * r * (DD(0, 1) - DD(1, 0)) + 2 * x * (DD(2, 0) + DD(0, 2)) + 2 * y * (DD(1, 2) + DD(2, 1)) - 4 * z * (DD(1, 1) + DD(0, 0))], axis=1)
    return dscale, drot


def cov4_conditional_backward(inp, sc, sct, q, qr, opac, dt, dcov, dmean, g_opacity, plant=None):
    """computeCov3D_conditional backward, backward.cu:689-834: the conditional covariance, the mean shift (Q5), the marginal-opacity
    chain over the prefiltered variance; -> dict, every entry zero where the marginal is not above 0.05."""
    mod, pv = inp["scale_modifier"], inp["prefilter_var"]
    P = sc.shape[0]
    scl = mod * np.concatenate([sc, sct[:, None]], axis=1)
    a, b, c, d = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    p_, q_, r_, s_ = qr[:, 0], qr[:, 1], qr[:, 2], qr[:, 3]
    Ml = cols([[a, b, -c, d], [-b, a, d, c], [c, -d, a, b], [-d, -c, -b, a]])          # forward.cu:315-320
    Mr = cols([[p_, q_, -r_, -s_], [-q_, p_, s_, -r_], [r_, -s_, p_, -q_], [s_, r_, q_, p_]])
    R = mul(Mr, Ml)
    Mm = R * scl[:, None, :]
    Sigma = mul(tr(Mm), Mm)
    cov_t = Sigma[:, 3, 3]
    cov_t_pre = pv + cov_t if pv > 0.0 else cov_t
    marg = np.exp(-0.5 * dt * dt / cov_t_pre)
    ok = marg > 0.05
    c12 = Sigma[:, 0:3, 3] if plant == "q7" else Sigma[:, 3, 0:3]                      # Q7
    d12 = np.stack([-(dcov[:, 0] * c12[:, 0] + dcov[:, 1] * c12[:, 1] * 0.5 + dcov[:, 2] * c12[:, 2] * 0.5),
                    -(dcov[:, 1] * c12[:, 0] * 0.5 + dcov[:, 3] * c12[:, 1] + dcov[:, 4] * c12[:, 2] * 0.5),
                    -(dcov[:, 2] * c12[:, 0] * 0.5 + dcov[:, 4] * c12[:, 1] * 0.5 + dcov[:, 5] * c12[:, 2])], axis=1) * 2.0 / cov_t[:, None]
    dcovt = (c12[:, 0] * c12[:, 0] * dcov[:, 0] + c12[:, 0] * c12[:, 1] * dcov[:, 1] + c12[:, 0] * c12[:, 2] * dcov[:, 2]
             + c12[:, 1] * c12[:, 1] * dcov[:, 3] + c12[:, 1] * c12[:, 2] * dcov[:, 4] + c12[:, 2] * c12[:, 2] * dcov[:, 5]) / (cov_t * cov_t)
    dL_dmarg = g_opacity * opac
    g_op = g_opacity * marg
    dcovt = dcovt + marg * dt * dt / 2 / (cov_t_pre * cov_t_pre) * dL_dmarg
    dL_dt = dL_dmarg * (marg * dt / cov_t_pre)
    d12 = d12 + dmean / cov_t[:, None] * dt[:, None]                                    # Q5
    ddot = (dmean * c12).sum(1)
    dcovt = dcovt + -ddot / (cov_t * cov_t) * dt
    dL_dt = dL_dt + -ddot / cov_t
    d11 = sym_split(dcov, plant)
    dSig = np.zeros((P, 4, 4))
    dSig[:, 0:3, 0:3] = d11
    dSig[:, 0:3, 3] = 0.5 * d12
    dSig[:, 3, 0:3] = 0.5 * d12
    dSig[:, 3, 3] = dcovt
    dM = mul(2.0 * Mm, dSig)
    Rt, dMt = tr(R), tr(dM)
    ds = (Rt * dMt).sum(2)
    dMt = dMt * scl[:, :, None]
    A = mul(dMt, Mr)
    B = mul(Ml, dMt)
    sgn = -1.0 if plant == "quat_sign" else 1.0
    drot = np.stack([A[:, 0, 0] + A[:, 1, 1] + A[:, 2, 2] + A[:, 3, 3], sgn * -A[:, 0, 1] + A[:, 1, 0] - A[:, 2, 3] + A[:, 3, 2],
                     A[:, 0, 2] - A[:, 1, 3] - A[:, 2, 0] + A[:, 3, 1], -A[:, 0, 3] - A[:, 1, 2] + A[:, 2, 1] + A[:, 3, 0]], axis=1)
    drot_r = np.stack([B[:, 0, 0] + B[:, 1, 1] + B[:, 2, 2] + B[:, 3, 3], -B[:, 0, 1] + B[:, 1, 0] + B[:, 2, 3] - B[:, 3, 2],
                       B[:, 0, 2] + B[:, 1, 3] - B[:, 2, 0] - B[:, 3, 1], B[:, 0, 3] - B[:, 1, 2] + B[:, 2, 1] - B[:, 3, 0]], axis=1)
    k = ok[:, None]
    return dict(ok=ok, g_opacity=np.where(ok, g_op, g_opacity), dts=np.where(ok, dL_dt, 0.0), dscale=np.where(k, ds[:, 0:3], 0.0),
                dscale_t=np.where(ok, ds[:, 3], 0.0), drot=np.where(k, drot, 0.0), drot_r=np.where(k, drot_r, 0.0))


def normalize(v):
    """F.normalize (scene/gaussian_model.py:191-197): v / max(|v|, 1e-12) -> (q, 1 / that)."""
    inv = 1.0 / np.maximum(np.sqrt((v * v).sum(1)), f32(1e-12))
    return v * inv[:, None], inv


def normalize_backward(q, inv, g):
    return (g - q * (q * g).sum(1, keepdims=True)) * inv[:, None]


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def chain(inp, rec, acc, plant=None):
    """The per-Gaussian backward in float64.

    ``inp``: P, D, D_t, M, W, H; shs [P,M,3] or None (colors_precomp: no SH); opacities [P]; ts, scales, scales_t, rotations,
    rotations_r, cov3D_precomp or None; viewmatrix, projmatrix [16] (as stored: transposed), campos [3]; tan_fovx, tan_fovy, timestamp,
    time_duration, scale_modifier, prefilter_var; rot_4d, gaussian_dim, force_sh_3d, raw, analytic_sh.  Every float is the fp32 value
    the kernels receive.
    ``rec``: the forward's records radii [P], out_means3D [P,3], cov3D [P,6], conic_opacity [P,4] (conic xx, xy, yy, effective
    opacity), clamped [P,3].   ``acc``: the accumulator records [P,12].
    Returns OUTPUTS by name (float64): what ONE view's backward computes (overwrite mode); ``accumulate`` applies the modes."""
    P = inp["P"]
    inp = dict(inp)
    for k in ("viewmatrix", "projmatrix", "campos"):
        inp[k] = _f64(inp[k]).reshape(-1)
    inp["focal_x"] = inp["W"] / (2.0 * inp["tan_fovx"])   # rasterizer_impl.cu:424-425
    inp["focal_y"] = inp["H"] / (2.0 * inp["tan_fovy"])
    acc = _f64(acc)
    vis = np.asarray(rec["radii"]) > 0
    out = {}
    if inp.get("shs") is not None and inp["M"] > 0:
        _, words, stage, dsh = sh_backward(inp, rec, acc, plant)
    else:
        words, stage, dsh = np.zeros((P, 4)), np.zeros((P, 8)), np.zeros((P, 0, 3))
    out["sh_words"], out["stage"], out["dL_dsh"] = words, stage, dsh

    with np.errstate(all="ignore"):
        co = _f64(rec["conic_opacity"])
        cA, cB, cC, o_eff = co[:, 0], co[:, 1], co[:, 2], co[:, 3]
        Mx, My, Mxx, Myy, Mxy = (acc[:, k] for k in (6, 7, 8, 9, 10))
        # moments -> dL_dmean2D, dL_dconic (backward.cu:1107-1133 summed over the pixels)
        gx = -o_eff * (0.5 * inp["W"]) * (cA * Mx + cB * My)
        gy = -o_eff * (0.5 * inp["H"]) * (cB * Mx + cC * My)
        g_conic = np.stack([-0.5 * o_eff * Mxx, -0.5 * o_eff * Mxy, -0.5 * o_eff * Myy], axis=1)
        mean = _f64(rec["out_means3D"])
        cov3D = _f64(inp["cov3D_precomp"] if inp.get("cov3D_precomp") is not None else rec["cov3D"])
        dcov, dmean = cov2d_backward(inp, mean, cov3D, g_conic, acc[:, 3], plant)
        dmean = dmean + projection_backward(inp, mean, gx, gy)
        dts = np.zeros(P)
        if inp.get("shs") is not None and inp["M"] > 0:
            dmean = dmean + words[:, 0:3]
            dts = dts + words[:, 3]
        g_op = acc[:, 11].copy()
        dscale, dscale_t, drot, drot_r = np.zeros((P, 3)), np.zeros(P), np.zeros((P, 4)), np.zeros((P, 4))
        raw = bool(inp.get("raw"))
        if inp.get("scales") is not None:
            sc, q = _f64(inp["scales"]), _f64(inp["rotations"])
            inv_nq = np.ones(P)
            if raw:
                sc = np.exp(sc)
                q, inv_nq = normalize(q)
            if inp["rot_4d"]:
                sct, qr, opac = _f64(inp["scales_t"]).reshape(P), _f64(inp["rotations_r"]), _f64(inp["opacities"]).reshape(P)
                inv_nqr = np.ones(P)
                if raw:
                    sct = np.exp(sct)
                    qr, inv_nqr = normalize(qr)
                    opac = sigmoid(opac)
                dt = inp["timestamp"] - _f64(inp["ts"]).reshape(P)
                r4 = cov4_conditional_backward(inp, sc, sct, q, qr, opac, dt, dcov, dmean, g_op, plant)
                g_op = np.where(vis, r4["g_opacity"], g_op)
                dts = dts + r4["dts"]
                dscale, dscale_t, drot, drot_r = r4["dscale"], r4["dscale_t"], r4["drot"], r4["drot_r"]
                if raw:
                    dscale_t = dscale_t * sct
                    drot_r = normalize_backward(qr, inv_nqr, drot_r)
            else:
                dscale, drot = cov3_backward(sc, inp["scale_modifier"], q, dcov, plant)   # Q6: nothing else for gaussian_dim 4
            if raw:
                dscale = dscale * sc
                drot = normalize_backward(q, inv_nq, drot)
        if raw:
            o = sigmoid(_f64(inp["opacities"]).reshape(P))
            g_op = g_op * (o * (1.0 - o))
            if plant == "sigmoid2":
                g_op = g_op * (o * (1.0 - o))
    v1, zero = vis[:, None], 0.0
    out["dL_dmean2D"] = np.stack([np.where(vis, gx, zero), np.where(vis, gy, zero), acc[:, 3]], axis=1)
    out["dL_dcolor"], out["dL_dflows"] = acc[:, 0:3].copy(), acc[:, 4:6].copy()
    out["dL_dcov3D"] = np.where(v1, dcov, zero)
    out["dL_dmean3D"] = np.where(v1, dmean, zero)
    out["dL_dopacity"] = g_op
    out["dL_dts"] = np.where(vis, dts, zero)
    out["dL_dscale"], out["dL_dscale_t"] = np.where(v1, dscale, zero), np.where(vis, dscale_t, zero)
    out["dL_drot"], out["dL_drot_r"] = np.where(v1, drot, zero), np.where(v1, drot_r, zero)
    out["dL_dconic"] = np.where(v1, g_conic, zero)   # not an output of the kernels: the host test's finite-difference check reads it
    return out


PARAM_GRADS = ("dL_dopacity", "dL_dmean3D", "dL_dts", "dL_dscale", "dL_dscale_t", "dL_drot", "dL_drot_r")


def accumulate(view, prefill, radii):
    """``accumulate`` mode, stated as fp32 addition onto a given prefill: the parameter gradients (PARAM_GRADS) of a visible Gaussian
    are prefill + this view's (each addend an fp32 number, the sum rounded to fp32 by the kernel); nothing is added for a culled one."""
    vis = np.asarray(radii) > 0
    out = dict(view)
    for k in PARAM_GRADS:
        pf = _f64(prefill[k]).reshape(view[k].shape)
        m = vis.reshape((-1,) + (1,) * (view[k].ndim - 1))
        out[k] = pf + np.where(m, view[k], 0.0)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# Input sensitivity and the comparison
# ---------------------------------------------------------------------------------------------------------------------------------
PERTURBED_INP = ("shs", "opacities", "ts", "scales", "scales_t", "rotations", "rotations_r", "cov3D_precomp", "viewmatrix", "projmatrix",
                 "campos")
PERTURBED_REC = ("out_means3D", "cov3D", "conic_opacity")


def sensitivity(inp, rec, acc, draws=16, seed=0):
    """What one ulp on the inputs does to every output element: for ``draws`` seeded draws every fp32 input of the Gaussian
    (parameters, forward records, accumulator words, camera matrices, timestamp) is multiplied by 1 +- 2^-23 with a random sign, and
    sens_e is the largest |f64(perturbed) - f64| over the draws.  The discrete records (radii, clamp bits) are not inputs of this kind."""
    rng = np.random.default_rng(seed)
    base = chain(inp, rec, acc)
    eps = 2.0 ** -23

    def jig(a):
        a = _f64(a)
        return a * (1.0 + eps * rng.choice([-1.0, 1.0], size=a.shape))

    sens = {k: np.zeros_like(v) for k, v in base.items()}
    for _ in range(draws):
        i2, r2 = dict(inp), dict(rec)
        for k in PERTURBED_INP:
            if inp.get(k) is not None:
                i2[k] = jig(inp[k])
        i2["timestamp"] = float(jig(np.array([inp["timestamp"]]))[0])
        for k in PERTURBED_REC:
            r2[k] = jig(rec[k])
        got = chain(i2, r2, jig(acc))
        for k in sens:
            sens[k] = np.maximum(sens[k], np.abs(np.nan_to_num(got[k] - base[k], nan=np.inf)))
    return base, sens


def ulp32(x):
    """One fp32 ulp at |x| (the spacing above it; the smallest normal's for smaller values)."""
    a = np.maximum(np.abs(np.asarray(x, np.float64)), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(a)) - 23)


def core_bar(f64, sens):
    """4 ulp32 of |f64_e| + sens_e: the per-element bar before its tensor's K."""
    return 4.0 * ulp32(f64) + sens


def ratio(got, f64, sens):
    """|got - f64| / (4 ulp32 of |f64_e| + sens_e), element by element (a non-finite ``got`` counts as infinitely far)."""
    d = np.abs(np.asarray(got, np.float64).reshape(f64.shape) - f64)
    return np.nan_to_num(d, nan=np.inf) / core_bar(f64, sens)


def flagged(got, f64, sens, K):
    """The comparison the GPU test asserts with: indices of the elements beyond K * (4 ulp32 of |f64_e| + sens_e)."""
    return np.argwhere(ratio(got, f64, sens) > K)
