"""PyTorch statement, on the CPU, of ``fdgs.flow.gaussian_flow`` (csrc/flow.hip), written from its definition:

    flow_i = pix(mu_i(t_1); target camera) - pix(mu_i(t_0); source camera)

* mu_i(t): with ``rot_4d`` the conditional mean ``p + Sigma[0:3,3] / Sigma[3,3] * (t - t_i)`` of the 4D Gaussian, the covariance put
  together as scene/gaussian_model.py:34-47 does (``L = R4 diag(modifier * s)``, ``Sigma = L L^T``, ``R4`` the product of the two
  isoclinic matrices of utils/general_utils.py:113-133); otherwise the plain mean.
* pix: ``h = (mu, 1) @ full_proj_transform``, ``ndc = h.xy / (h.w + 1e-7)``, ``pix = ((ndc + 1) * (W, H) - 1) / 2`` (auxiliary.h:42-45).
* a Gaussian whose view-space z ``((mu, 1) @ world_view_transform).z <= 0.2`` at either end: flow 0, and no gradient.

``raw=True``: ``scales`` / ``scales_t`` go through exp and the quaternions through F.normalize first (the model's activations);
``raw=False``: the tensors are the activated values and enter AS PASSED -- the matrices are built from the quaternions without
normalising them again, which is what "the gradient with respect to the activated values" means (for unit quaternions the value is the
same).  dtype-generic (float64: the reference of the GPU tests; float32: how far fp32 itself is from it) and differentiable.  The
timestamps are rounded to float32 first: the kernels receive them as floats.
"""
import numpy as np
import torch


def sigma4(scales4, rot, rot_r):
    """[P,4,4] Sigma = L L^T, L = R4 diag(scales4); the quaternions enter as they are."""
    a, b, c, d = rot.unbind(-1)
    p, q, r, s = rot_r.unbind(-1)
    Ml = torch.stack([a, -b, -c, -d, b, a, -d, c, c, d, a, -b, d, -c, b, a], dim=1).view(-1, 4, 4)
    Mr = torch.stack([p, q, r, s, -q, p, -s, r, -r, s, p, -q, -s, -r, q, p], dim=1).view(-1, 4, 4)
    R = (Ml @ Mr).flip(1, 2)
    L = R * scales4.unsqueeze(1)
    return L @ L.transpose(1, 2)


def velocity(scales, scales_t, rotations, rotations_r, raw, scaling_modifier=1.0):
    """[P,3]: Sigma[0:3,3] / Sigma[3,3] (the mean moves by this per unit of time)."""
    s4 = torch.cat([scales, scales_t.reshape(-1, 1)], dim=1)
    ql, qr = rotations, rotations_r
    if raw:
        s4 = torch.exp(s4)
        ql = torch.nn.functional.normalize(ql, dim=-1)
        qr = torch.nn.functional.normalize(qr, dim=-1)
    sig = sigma4(scaling_modifier * s4, ql, qr)
    return sig[:, 0:3, 3] / sig[:, 3, 3:4]


def project(mean, view, proj, W, H):
    """(pix [P,2], view-space z [P]) of world points; ``view`` / ``proj``: world_view_transform / full_proj_transform (row-vector convention)."""
    hom = torch.cat([mean, torch.ones_like(mean[:, :1])], dim=1)
    h = hom @ proj.to(mean.dtype)
    z = (hom @ view.to(mean.dtype))[:, 2]
    ndc = h[:, 0:2] / (h[:, 3:4] + 1e-7)
    wh = torch.tensor([float(W), float(H)], dtype=mean.dtype)
    return ((ndc + 1.0) * wh - 1.0) * 0.5, z


def gaussian_flow(view0, proj0, t0, view1, proj1, t1, W, H, means3D, ts, scales, scales_t, rotations, rotations_r, *, rot_4d, raw,
                  scaling_modifier=1.0, dtype=torch.float64, details=False):
    """[P,2] flow in ``dtype``; every tensor argument may require grad (convert to ``dtype`` BEFORE the call to differentiate).
    ``details``: also the two pixel positions and the validity mask."""
    cv = lambda t: None if t is None else t.to(dtype)  # noqa: E731
    means3D = cv(means3D)
    t0, t1 = float(np.float32(t0)), float(np.float32(t1))
    m0 = m1 = means3D
    if rot_4d:
        w = velocity(cv(scales), cv(scales_t), cv(rotations), cv(rotations_r), raw, scaling_modifier)
        ti = cv(ts).reshape(-1, 1)
        m0 = means3D + w * (t0 - ti)
        m1 = means3D + w * (t1 - ti)
    pix0, z0 = project(m0, view0, proj0, W, H)
    pix1, z1 = project(m1, view1, proj1, W, H)
    ok = ~(z0 <= 0.2) & ~(z1 <= 0.2)
    flow = torch.where(ok.unsqueeze(1), pix1 - pix0, torch.zeros_like(pix0))
    return (flow, pix0, pix1, ok) if details else flow


NAMES = ("means3D", "ts", "scales", "scales_t", "rotations", "rotations_r")


def flow_with_grads(view0, proj0, t0, view1, proj1, t1, W, H, params, dL_dflows, *, rot_4d, raw, scaling_modifier=1.0, dtype=torch.float64):
    """(flow, {name: gradient}) of sum(flow * dL_dflows) with respect to the six tensors of ``params`` (a dict by NAMES), in ``dtype``."""
    leaves = {n: params[n].detach().to(dtype).clone().requires_grad_(True) for n in NAMES}
    flow = gaussian_flow(view0, proj0, t0, view1, proj1, t1, W, H, *[leaves[n] for n in NAMES], rot_4d=rot_4d, raw=raw,
                         scaling_modifier=scaling_modifier, dtype=dtype)
    (flow * dL_dflows.to(dtype)).sum().backward()
    return flow.detach(), {n: (torch.zeros_like(t) if t.grad is None else t.grad.detach()) for n, t in leaves.items()}


# ---------------------------------------------------------------------------------------------------------------------------------
# The same forward and its backward written out by hand, in numpy, vectorised over Gaussians: from the statement above and the
# formulas in the header comment of csrc/flow.hip, nothing taken from the kernel.  ``dtype`` float64: the reference of the GPU tests
# (tests/test_flow_host.py holds it to float64 autograd of ``gaussian_flow``); float32: every array is float32, so every numpy
# operation rounds to float32 -- the "float32 statement", one legal float32 evaluation, whose distance from float64 prices K
# (tests/flow_cases.py).
#
#   Sigma = L L^T, L = R diag(s), s = modifier * (scales, scale_t), R = flip(Ml Mr);  c = Sigma[0:3,3], c_t = Sigma[3,3], w = c / c_t
#   mu_j = p + w (t_j - t_i);  h_j = (mu_j, 1) proj_j;  pw = 1 / (h_w + 1e-7);  pix = ((h_xy pw + 1) (W, H) - 1) / 2
#   g_j = J_pix(mu_j)^T (-+G):  a_xy = -+G (W, H) / 2 pw,  a_w = -(a_x h_x + a_y h_y) pw,  g_j = proj[0:3, (0, 1, 3)] (a_x, a_y, a_w)
#   d p = g_0 + g_1;  d w = g_0 (t_0 - t_i) + g_1 (t_1 - t_i);  d t_i = -w . (g_0 + g_1);  d c = d w / c_t;  d c_t = -(d w . c) / c_t^2
#   dSigma: d c split in halves over [r,3] and [3,r], d c_t at [3,3];  d L = 2 dSigma L;  d s_k = sum_i dL[i,k] R[i,k] (times the
#   modifier for d scale);  d R = d L diag(s);  d(Ml Mr) = flip(d R);  d Ml = D Mr^T, d Mr = Ml^T D;  the quaternion components
#   collect their entries with the signs of the two patterns;  raw: d log-scale = d scale * scale, d v = (g - q (q . g)) / |v|.
# ---------------------------------------------------------------------------------------------------------------------------------
PLANTS = ("no_mod", "ct", "no_half", "dt_swap", "no_hw", "ts_sign", "rotr_sign", "no_proj", "no_exp", "no_inv")
RAW_PLANTS = ("no_proj", "no_exp", "no_inv")                                    # touch raw terms only
# "no_proj" (act_normalize_bwd without its q (q . g) term) changes no number: w = c / c_t is homogeneous of degree 0 in either
# quaternion (Sigma is of degree 2), so the gradient with respect to the normalised quaternion has no component along it (Euler) and
# q . g is 0 up to rounding.  It cannot be flagged by any comparison, as Q7 of the rasterizer's chain cannot; tests/test_flow_host.py
# asserts that instead.  "no_inv" (the same backward without its 1 / |v|) is the plant that stands for a wrong normalisation backward.
UNOBSERVABLE_PLANTS = ("no_proj",)
ROT4D_PLANTS = ("no_mod", "ct", "no_half", "dt_swap", "ts_sign", "rotr_sign")   # touch 4D terms only
OUTPUTS = ("flows",) + NAMES

# which quaternion component stands where in Ml / Mr of ``sigma4``, and with which sign
_IDX = ((0, 1, 2, 3), (1, 0, 3, 2), (2, 3, 0, 1), (3, 2, 1, 0))
_SGN_L = ((1, -1, -1, -1), (1, 1, -1, 1), (1, 1, 1, -1), (1, -1, 1, 1))
_SGN_R = ((1, 1, 1, 1), (-1, 1, -1, 1), (-1, 1, 1, -1), (-1, -1, 1, 1))


def _pattern(sgn):
    E = np.zeros((4, 4, 4))
    for i in range(4):
        for j in range(4):
            E[_IDX[i][j], i, j] = sgn[i][j]
    return E


E_L, E_R = _pattern(_SGN_L), _pattern(_SGN_R)


def _np(t, dt):
    return None if t is None else np.ascontiguousarray(np.asarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t, dtype=dt))


def _end(mean, view, proj, W, H, dt):
    """One end: (pix [P,2], view-space z [P], h_xy [P,2], pw [P])."""
    h = mean @ proj[0:3, :] + proj[3, :]
    z = mean @ view[0:3, 2] + view[3, 2]
    pw = dt(1.0) / (h[:, 3] + dt(1e-7))
    wh = np.array([W, H], dtype=dt)
    pix = ((h[:, 0:2] * pw[:, None] + dt(1.0)) * wh - dt(1.0)) * dt(0.5)
    return pix, z, h[:, 0:2], pw


def _end_bwd(hxy, pw, proj, W, H, G, dt, plant):
    a = G * (dt(0.5) * np.array([W, H], dtype=dt)) * pw[:, None]
    aw = -(a[:, 0] * hxy[:, 0] + a[:, 1] * hxy[:, 1]) * pw
    if plant == "no_hw":
        aw = np.zeros_like(aw)
    return a[:, 0:1] * proj[0:3, 0] + a[:, 1:2] * proj[0:3, 1] + aw[:, None] * proj[0:3, 3]


def analytic(view0, proj0, t0, view1, proj1, t1, W, H, params, dL_dflows, *, rot_4d, raw, scaling_modifier=1.0, scale=1.0,
             dtype=np.float64, plant=None):
    """-> dict: "flows" [P,2], the six gradients of sum(flows * scale * dL_dflows) by NAMES (shaped as the parameters; zero rows for a
    Gaussian behind either camera, zero tensors for what the flow does not depend on), "ok" [P] bool, "z0" / "z1" [P] the view-space
    depths and "pix0" / "pix1".  ``params``: dict by NAMES (torch tensors or arrays).  ``plant``: ONE deliberately wrong term (PLANTS)."""
    assert plant is None or plant in PLANTS, plant
    dt = np.dtype(dtype).type
    f = lambda a: _np(a, dt)   # noqa: E731
    view0, proj0, view1, proj1 = f(view0), f(proj0), f(view1), f(proj1)
    t0, t1 = dt(np.float32(t0)), dt(np.float32(t1))
    mod = dt(np.float32(scaling_modifier))
    p = f(params["means3D"])
    P = p.shape[0]
    G = f(dL_dflows).reshape(P, 2) * dt(np.float32(scale))
    shapes = {n: tuple(params[n].shape) for n in NAMES if params.get(n) is not None}
    m0 = m1 = p
    if rot_4d:
        s4 = np.concatenate([f(params["scales"]), f(params["scales_t"]).reshape(P, 1)], axis=1)
        v, vr = f(params["rotations"]), f(params["rotations_r"])
        q, qr = v, vr
        if raw:
            s4 = np.exp(s4)
            inv = dt(1.0) / np.maximum(np.sqrt((v * v).sum(1)), dt(1e-12))
            inv_r = dt(1.0) / np.maximum(np.sqrt((vr * vr).sum(1)), dt(1e-12))
            q, qr = v * inv[:, None], vr * inv_r[:, None]
        s = mod * s4
        El, Er = E_L.astype(dt), E_R.astype(dt)
        Ml, Mr = np.einsum("pk,kij->pij", q, El), np.einsum("pk,kij->pij", qr, Er)
        R = (Ml @ Mr)[:, ::-1, ::-1]
        L = R * s[:, None, :]
        Sigma = L @ np.swapaxes(L, 1, 2)
        c, ct = Sigma[:, 0:3, 3], Sigma[:, 3, 3]
        w = c / ct[:, None]
        ti = f(params["ts"]).reshape(P)
        dt0, dt1 = t0 - ti, t1 - ti
        m0, m1 = p + w * dt0[:, None], p + w * dt1[:, None]
    pix0, z0, h0, pw0 = _end(m0, view0, proj0, W, H, dt)
    pix1, z1, h1, pw1 = _end(m1, view1, proj1, W, H, dt)
    ok = ~(z0 <= dt(np.float32(0.2))) & ~(z1 <= dt(np.float32(0.2)))
    out = {"ok": ok, "z0": z0, "z1": z1, "pix0": pix0, "pix1": pix1, "flows": np.where(ok[:, None], pix1 - pix0, dt(0.0))}
    out["w"] = w if rot_4d else np.zeros_like(p)
    g0 = _end_bwd(h0, pw0, proj0, W, H, -G, dt, plant)
    g1 = _end_bwd(h1, pw1, proj1, W, H, G, dt, plant)
    gp = g0 + g1
    grads = {"means3D": gp}
    if rot_4d:
        dw = g0 * dt1[:, None] + g1 * dt0[:, None] if plant == "dt_swap" else g0 * dt0[:, None] + g1 * dt1[:, None]
        dti = -(w * gp).sum(1)
        grads["ts"] = -dti if plant == "ts_sign" else dti
        dc = dw / ct[:, None]
        dct = -(dw * c).sum(1) / (ct if plant == "ct" else ct * ct)
        half = dt(1.0 if plant == "no_half" else 0.5)
        dSig = np.zeros((P, 4, 4), dtype=dt)
        dSig[:, 0:3, 3] = half * dc
        dSig[:, 3, 0:3] = half * dc
        dSig[:, 3, 3] = dct
        dLm = dt(2.0) * (dSig @ L)
        ds = (dLm * R).sum(1)
        d4 = ds if plant == "no_mod" else mod * ds
        if raw and plant != "no_exp":
            d4 = d4 * s4
        grads["scales"], grads["scales_t"] = d4[:, 0:3], d4[:, 3]
        # d scale_t is the difference of two terms of this size, the d c and the d c_t route (they cancel where w does not depend on
        # the temporal scale): what "relative" is measured against when two float64 evaluations of it are compared
        out["scales_t_terms"] = np.where(ok, dt(2.0) * np.abs((dw * c).sum(1)) / ct * (dt(1.0) if raw else dt(1.0) / s4[:, 3]), dt(0.0))
        D = (dLm * s[:, None, :])[:, ::-1, ::-1]
        dMl, dMr = D @ np.swapaxes(Mr, 1, 2), np.swapaxes(Ml, 1, 2) @ D
        Er_b = Er
        if plant == "rotr_sign":
            Er_b = Er.copy()
            Er_b[2, 1, 3] = -Er_b[2, 1, 3]
        dq, dqr = np.einsum("pij,kij->pk", dMl, El), np.einsum("pij,kij->pk", dMr, Er_b)
        if raw:
            if plant == "no_proj":
                dq, dqr = dq * inv[:, None], dqr * inv_r[:, None]
            elif plant == "no_inv":
                dq, dqr = dq - q * (q * dq).sum(1, keepdims=True), dqr - qr * (qr * dqr).sum(1, keepdims=True)
            else:
                dq = (dq - q * (q * dq).sum(1, keepdims=True)) * inv[:, None]
                dqr = (dqr - qr * (qr * dqr).sum(1, keepdims=True)) * inv_r[:, None]
        grads["rotations"], grads["rotations_r"] = dq, dqr
    for n in NAMES:
        if n in grads:
            g = grads[n].reshape(P, -1)
            out[n] = np.where(ok[:, None], g, dt(0.0)).reshape(shapes.get(n, g.shape))
        else:
            out[n] = np.zeros(shapes.get(n, (P, {"ts": 1, "scales": 3, "scales_t": 1, "rotations": 4, "rotations_r": 4}[n])), dtype=dt)
    return out


NEAR = 0.2            # the near cull's plane (view-space z), a float32 constant of the kernels
NEAR_MARGIN = 1e-4    # every case keeps every |z / 0.2 - 1| above this, at both ends, for every perturbed draw


def assert_clear_of_the_cull(res, what=""):
    near = float(np.float32(NEAR))
    for k in ("z0", "z1"):
        gap = np.abs(np.asarray(res[k], np.float64) / near - 1.0)
        assert gap.min() > NEAR_MARGIN, "%s: Gaussian %d has %s = %.9g, within %g (relative) of the near cull" % (
            what, int(gap.argmin()), k, float(res[k][gap.argmin()]), NEAR_MARGIN)


def sensitivity(view0, proj0, t0, view1, proj1, t1, W, H, params, dL_dflows, *, rot_4d, raw, scaling_modifier=1.0, scale=1.0, draws=16,
                seed=0):
    """(float64 result of ``analytic``, sens by OUTPUTS): what one float32 ulp on the inputs does to every output element -- the
    perturbation of chain_oracle.sensitivity: for ``draws`` seeded draws every element of the six tensors and of dL_dflows is
    multiplied by 1 +- 2^-23 with a random sign; sens_e is the largest |f64(perturbed) - f64|.  The cameras and the two timestamps are
    exact float32 constants and stay.  The near cull is a discrete decision: no draw may move a Gaussian within NEAR_MARGIN of it
    (asserted), so the validity mask is the same for every draw."""
    rng = np.random.default_rng(seed)
    cam = (view0, proj0, t0, view1, proj1, t1, W, H)
    kw = dict(rot_4d=rot_4d, raw=raw, scaling_modifier=scaling_modifier, scale=scale)
    base = analytic(*cam, params, dL_dflows, **kw)
    assert_clear_of_the_cull(base, "unperturbed")
    eps = 2.0 ** -23

    def jig(a):
        a = _np(a, np.float64)
        return a * (1.0 + eps * rng.choice([-1.0, 1.0], size=a.shape))

    sens = {k: np.zeros_like(base[k]) for k in OUTPUTS}
    for d in range(draws):
        got = analytic(*cam, {n: jig(params[n]) for n in NAMES if params.get(n) is not None}, jig(dL_dflows), **kw)
        assert_clear_of_the_cull(got, "draw %d" % d)
        assert np.array_equal(got["ok"], base["ok"])
        for k in OUTPUTS:
            sens[k] = np.maximum(sens[k], np.abs(np.nan_to_num(got[k] - base[k], nan=np.inf)))
    return base, sens
