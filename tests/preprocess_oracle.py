"""Float64 oracle of the per-Gaussian FORWARD: what preprocess_fwd.hip (preprocess_fwd_kernel<0/1/2>, colour_batch_kernel) and, through
fdgs_math.h, gaussian_at_time compute for ONE Gaussian -- plain numpy, vectorised over Gaussians, nothing taken from the product.  It
restates the reference's preprocessCUDA (diff-gaussian-rasterization/cuda_rasterizer/forward.cu:355-496) with its helpers: the 4D
covariance conditioned on t, the mean shift and the temporal marginal (forward.cu:279-352), the 3D covariance with the 1-D marginal
(forward.cu:242-276, 431-437), the near cull (auxiliary.h:140-163), the EWA projection (forward.cu:198-237), ndc2Pix (auxiliary.h:42-45),
the tile rectangle (auxiliary.h:47-57) and SH / 4D SH -> RGB (forward.cu:20-195), with quirk Q4: the forward's view direction comes from
the UN-shifted input mean.

What tests/chain_oracle.py already states in float64 is imported from there, not copied: mul, tr, cols, quat_to_R, project_cov,
sh_tables, sh_plan, normalize, sigmoid and the constants with their fp32 values.  Matrices are ``c[..., column, row]`` as there.
Constants the kernels write with an ``f`` suffix are their fp32 values; everything else is float64.

``forward`` returns, per Gaussian, the float outputs (FLOATS), the discrete decisions (alive, radius, tiles, rect, clamped) and the
CONTINUOUS quantity every decision thresholds (THRESHOLDS); ``sensitivity`` adds what one ulp on the inputs does to each, and
``flags`` says which decisions an fp32 evaluation may legally take the other way.

``plant``: evaluate with ONE deliberately wrong term (PLANTS); tests/test_preprocess_oracle_host.py shows the comparison flags each.
"""
import numpy as np

import chain_oracle as co
from chain_oracle import CLAMP, EPS7, LOWPASS, REF_PI, SH_C3, cols, f32, mul, normalize, project_cov, quat_to_R, sh_plan, sh_tables, sigmoid, tr, ulp32

NEAR = f32(0.2)          # auxiliary.h:153
FLOOR = f32(0.1)         # forward.cu:449-450
TILE = 16
FLOATS = ("out_means3D", "cov3D", "pix", "conic", "opacity", "depth", "rgb")
THRESHOLDS = ("near", "marg", "det", "rad", "rgb_pre", "opa255")
PLANTS = ("lowpass_one", "lambda2", "shifted_dir", "ndc_no_minus1", "dt_sign", "k2_no_times2", "trunc_radius")
# A decision is held to float64's where its quantity is further from the threshold than FLAG_ULPS * (one fp32 step of the quantity's
# own evaluation + what one ulp on the inputs does to it): a sum of three products (the view-space z, the quotients) is within 3 ulp of
# its exact value, the marginal (an fp32 expf of a double exponent) within 2, det = cx cz - cy cy within an ulp of its products,
# 3 sqrt(lambda) within the terms listed in ``flags``; 16 leaves a factor of four over the worst of them, the margin the float bars
# take as well (preprocess_cases.MARGIN).  tests/test_preprocess_oracle_host.py holds the port, one legal fp32 evaluation, to it.
FLAG_ULPS = 16.0


def _f64(x):
    return None if x is None else np.asarray(x, np.float64)


def cov4(scl, q, qr):
    """Sigma = M^T M, M = S (M_r M_l) (forward.cu:279-332): scl [P,4] the modified scales."""
    a, b, c, d = q.T
    p_, q_, r_, s_ = qr.T
    Ml = cols([[a, b, -c, d], [-b, a, d, c], [c, -d, a, b], [-d, -c, -b, a]])
    Mr = cols([[p_, q_, -r_, -s_], [-q_, p_, s_, -r_], [r_, -s_, p_, -q_], [s_, r_, q_, p_]])
    Mm = mul(Mr, Ml) * scl[:, None, :]
    return mul(tr(Mm), Mm)


def cov3(scl, q):
    """Sigma = M^T M, M = S R (forward.cu:242-276) -> the six upper-triangle entries."""
    Mm = quat_to_R(q) * scl[:, None, :]
    S = mul(tr(Mm), Mm)
    return np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], axis=1)


def gaussian_at_time(inp, plant=None, aux=None):
    """fdgs_math.h gaussian_at_time -> (alive [P] after the temporal cull, mean [P,3], cov [P,6], opacity [P], marginal - 0.05 [P] or
    None).  Mean shift, conditional covariance and the opacity product exist only where the marginal is above 0.05."""
    P = inp["P"]
    raw = bool(inp.get("raw"))
    mean = _f64(inp["means3D"]).reshape(P, 3).copy()
    opac = _f64(inp["opacities"]).reshape(P)
    if raw:
        opac = sigmoid(opac)
    alive = np.ones(P, bool)
    marg_q = None
    mod, pv, ts_now = inp["scale_modifier"], inp["prefilter_var"], inp["timestamp"]
    if inp.get("cov3D_precomp") is not None:
        return alive, mean, _f64(inp["cov3D_precomp"]).reshape(P, 6).copy(), opac, None
    sc, q = _f64(inp["scales"]).reshape(P, 3), _f64(inp["rotations"]).reshape(P, 4)
    if raw:
        sc, q = np.exp(sc), normalize(q)[0]
    if inp["rot_4d"]:
        sct, qr = _f64(inp["scales_t"]).reshape(P), _f64(inp["rotations_r"]).reshape(P, 4)
        if raw:
            sct, qr = np.exp(sct), normalize(qr)[0]
        dt = ts_now - _f64(inp["ts"]).reshape(P)
        Sigma = cov4(mod * np.concatenate([sc, sct[:, None]], axis=1), q, qr)
        cov_t = Sigma[:, 3, 3]
        marg = np.exp(-0.5 * dt * dt / (pv + cov_t if pv > 0.0 else cov_t))
        alive = marg > 0.05
        marg_q = marg - 0.05
        c12 = Sigma[:, 0:3, 3]
        k = cov_t[:, None]
        cov = np.stack([Sigma[:, 0, 0], Sigma[:, 0, 1], Sigma[:, 0, 2], Sigma[:, 1, 1], Sigma[:, 1, 2], Sigma[:, 2, 2]], axis=1)
        cov = cov - np.stack([c12[:, 0] * c12[:, 0], c12[:, 1] * c12[:, 0], c12[:, 2] * c12[:, 0], c12[:, 1] * c12[:, 1],
                              c12[:, 2] * c12[:, 1], c12[:, 2] * c12[:, 2]], axis=1) / k
        if aux is not None:   # |Sigma_ij| + |c12_i c12_j / cov_t|: the terms the conditioning subtracts (``sensitivity``)
            full = np.stack([Sigma[:, 0, 0], Sigma[:, 0, 1], Sigma[:, 0, 2], Sigma[:, 1, 1], Sigma[:, 1, 2], Sigma[:, 2, 2]], axis=1)
            aux["cov_mag"] = np.abs(full) + np.abs(full - cov)
        shift = c12 / k * (-dt if plant == "dt_sign" else dt)[:, None]
        a1 = alive[:, None]
        return alive, np.where(a1, mean + shift, mean), np.where(a1, cov, 0.0), np.where(alive, opac * marg, opac), marg_q
    cov = cov3(mod * sc, q)
    if inp["gaussian_dim"] == 4:
        sct = _f64(inp["scales_t"]).reshape(P)
        dt = _f64(inp["ts"]).reshape(P) - ts_now          # (the other sign than above: as the reference has it; dt enters squared)
        var = (np.exp(sct) if raw else sct) * mod          # the VARIANCE is scales_t here (forward.cu:431-437)
        marg = np.exp(-0.5 * dt * dt / (pv + var if pv > 0.0 else var))
        alive = ~(marg <= 0.05)
        marg_q = marg - 0.05
        opac = np.where(alive, opac * marg, opac)
    return alive, mean, cov, opac, marg_q


def sh_colour(inp, plant=None, mean_shifted=None):
    """SH / 4D SH -> (rgb before the clamp [P,3], the sum of the |terms| of each channel [P,3]: the magnitude its rounding scales with)."""
    P, M, D = inp["P"], inp["M"], inp["D"]
    sh3d, ncoef0, nblocks = sh_plan(D, inp["D_t"], inp["gaussian_dim"], inp["force_sh_3d"])
    shs = _f64(inp["shs"]).reshape(P, M, 3)
    src = mean_shifted if plant == "shifted_dir" else _f64(inp["means3D"]).reshape(P, 3)   # Q4: the UN-shifted input mean
    d = src - _f64(inp["campos"]).reshape(1, 3)
    d = d / np.sqrt((d * d).sum(1, keepdims=True))
    l = sh_tables(D, d[:, 0], d[:, 1], d[:, 2], list(SH_C3))[0]
    c = (l[:, :ncoef0, None] * shs[:, :ncoef0, :]).sum(1)
    mag = np.abs(l[:, :ncoef0, None] * shs[:, :ncoef0, :]).sum(1)
    if nblocks > 1:
        dir_t = _f64(inp["ts"]).reshape(P) - inp["timestamp"]
        for blk in range(1, nblocks):
            k = 1 if (blk == 2 and plant == "k2_no_times2") else blk
            tk = np.cos(2 * REF_PI * dir_t * k / inp["time_duration"])
            term = tk[:, None, None] * l[:, :, None] * shs[:, 16 * blk:16 * blk + 16, :]
            c, mag = c + term.sum(1), mag + np.abs(term).sum(1)
    return c + 0.5, mag + 0.5


def _trunc(q):
    return np.trunc(q).astype(np.int64)


def rect_of(pix, r, gx, gy, shift=0.0):
    """auxiliary.h:47-57 from pix [P,2] and the integer radius; ``shift`` is added to every quotient (flags: the decision at q -+ d)."""
    qs = quotients(pix, r)
    sh = np.broadcast_to(np.asarray(shift, np.float64), qs.shape)
    t = _trunc(qs + sh)
    lim = np.array([gx, gy, gx, gy])
    return np.minimum(lim, np.maximum(0, t))


def quotients(pix, r):
    """The four quotients before truncation: (pix.x - r) / 16, (pix.y - r) / 16, (pix.x + r + 15) / 16, (pix.y + r + 15) / 16."""
    r = np.asarray(r, np.float64)
    return np.stack([(pix[:, 0] - r) / TILE, (pix[:, 1] - r) / TILE, (pix[:, 0] + r + TILE - 1) / TILE, (pix[:, 1] + r + TILE - 1) / TILE], axis=1)


def forward(inp, plant=None, jitter=None):
    """The forward in float64.  ``jitter`` (``sensitivity`` only): {"cov": +-1 [P,6], "det": +-1 [P]} -- the two differences of fp32
    intermediates that cancel by structure are moved by two ulp32 of their larger term (see ``sensitivity``).

    ``inp``: P, D, D_t, M, W, H; means3D [P,3]; shs [P,M,3] or None with colors_precomp [P,3]; opacities [P]; ts, scales, scales_t,
    rotations, rotations_r, cov3D_precomp or None; viewmatrix, projmatrix [16] (as stored: transposed), campos [3]; tan_fovx, tan_fovy,
    timestamp, time_duration, scale_modifier, prefilter_var; rot_4d, gaussian_dim, force_sh_3d, raw.  Every float is the fp32 value the
    kernels receive.
    Returns FLOATS (zero for a culled Gaussian, as the kernels store them; out_means3D and cov3D as gaussian_at_time leaves them),
    alive / radius / tiles / rect [P,4] / clamped [P,3], THRESHOLDS, ``quot`` (the rectangle quotients), ``rgb_mag`` and the stages of
    the cull: ``alive_t`` (temporal), ``alive_n`` (near)."""
    P, W, H = inp["P"], inp["W"], inp["H"]
    vm, pj = _f64(inp["viewmatrix"]).reshape(-1), _f64(inp["projmatrix"]).reshape(-1)
    fx, fy = W / (2.0 * inp["tan_fovx"]), H / (2.0 * inp["tan_fovy"])
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    out = {}
    with np.errstate(all="ignore"):
        aux = {}
        alive_t, mean, cov, opac, marg_q = gaussian_at_time(inp, plant, aux)
        if jitter is not None and aux.get("cov_mag") is not None:
            cov = cov + np.where(alive_t[:, None], jitter["cov"] * 2.0 * ulp32(aux["cov_mag"]), 0.0)
        x, y, z = mean[:, 0], mean[:, 1], mean[:, 2]
        pz = vm[2] * x + vm[6] * y + vm[10] * z + vm[14]
        alive_n = alive_t & ~(pz <= NEAR)
        hx = pj[0] * x + pj[4] * y + pj[8] * z + pj[12]
        hy = pj[1] * x + pj[5] * y + pj[9] * z + pj[13]
        hw = pj[3] * x + pj[7] * y + pj[11] * z + pj[15]
        pw = 1.0 / (hw + EPS7)
        c2 = project_cov(mean, fx, fy, inp["tan_fovx"], inp["tan_fovy"], cov, vm)
        cx, cy, cz = c2["a"] + LOWPASS, c2["b"], c2["c"] + (0.0 if plant == "lowpass_one" else LOWPASS)
        det = cx * cz - cy * cy
        if jitter is not None:
            det = det + jitter["det"] * 2.0 * ulp32(np.abs(cx * cz) + cy * cy)
        conic = np.stack([cz / det, -cy / det, cx / det], axis=1)
        mid = 0.5 * (cx + cz)
        disc = np.maximum(FLOOR, mid * mid - det)
        lam1, lam2 = mid + np.sqrt(disc), mid - np.sqrt(disc)
        lam = lam2 if plant == "lambda2" else np.maximum(lam1, lam2)
        rad = 3.0 * np.sqrt(lam)
        radius = (np.trunc(rad) if plant == "trunc_radius" else np.ceil(rad))
        radius = np.where(np.isfinite(radius), radius, 0.0).astype(np.int64)
        one = 0.0 if plant == "ndc_no_minus1" else 1.0
        pix = np.stack([((hx * pw + 1.0) * W - one) * 0.5, ((hy * pw + 1.0) * H - one) * 0.5], axis=1)
        rect = rect_of(np.nan_to_num(pix), radius, gx, gy)
        area = (rect[:, 2] - rect[:, 0]) * (rect[:, 3] - rect[:, 1])
        alive = alive_n & (det != 0.0) & (area != 0) & (radius > 0)
        if inp.get("shs") is not None and inp["M"] > 0:
            rgb_pre, rgb_mag = sh_colour(inp, plant, mean)
            clamped = rgb_pre < 0
            rgb = np.maximum(rgb_pre, 0.0)
        else:
            rgb = _f64(inp["colors_precomp"]).reshape(P, 3)
            rgb_pre, rgb_mag, clamped = None, None, np.zeros((P, 3), bool)
    a1 = alive[:, None]
    out["out_means3D"], out["cov3D"] = mean, cov
    out["pix"], out["conic"] = np.where(a1, pix, 0.0), np.where(a1, conic, 0.0)
    out["opacity"], out["depth"] = np.where(alive, opac, 0.0), np.where(alive, pz, 0.0)
    out["rgb"] = np.where(a1, rgb, 0.0)
    out["alive"], out["alive_t"], out["alive_n"] = alive, alive_t, alive_n
    out["radius"], out["tiles"] = np.where(alive, radius, 0), np.where(alive, area, 0)
    out["rect"] = np.where(a1, rect, 0)
    out["clamped"] = np.where(a1, clamped, False)
    # the continuous quantities behind the decisions, for EVERY Gaussian (a culled one's are what the cull tested)
    out["near"], out["marg"], out["det"], out["rad"] = pz - NEAR, marg_q, det, rad
    out["rgb_pre"], out["rgb_mag"], out["opa255"] = rgb_pre, rgb_mag, 255.0 * opac - 1.0
    out["quot"], out["pix_all"], out["opac_all"] = quotients(np.nan_to_num(pix), radius), pix, opac
    out["_cov_mag"] = aux.get("cov_mag")
    out["_mid"], out["_disc"], out["_lam"], out["_cxcz"] = mid, disc, lam, np.abs(cx * cz) + cy * cy
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# Input sensitivity, the flags and the comparison
# ---------------------------------------------------------------------------------------------------------------------------------
PERTURBED = ("means3D", "shs", "colors_precomp", "opacities", "ts", "scales", "scales_t", "rotations", "rotations_r", "cov3D_precomp",
             "viewmatrix", "projmatrix", "campos")
SENS_OF = FLOATS + ("near", "marg", "det", "rad", "rgb_pre", "opa255", "pix_all")


def sensitivity(inp, draws=16, seed=0):
    """What one ulp on the inputs does to every float output and every thresholded quantity, as chain_oracle.sensitivity computes it:
    for ``draws`` seeded draws every fp32 input (parameters, camera matrices, timestamp) is multiplied by 1 +- 2^-23 with a random sign;
    sens_e = the largest |f64(perturbed) - f64| over the draws.
    What no ulp on an INPUT shows is a difference of two fp32 intermediates that cancels by structure; any fp32 evaluation, the
    reference's included, carries an ulp of the larger term into the result and into everything downstream.  There are two, and every
    draw moves them as well (``forward``'s jitter), by two ulp32 of the larger term with a random sign:
      det = cx cz - cy cy, by ulps of cx cz + cy cy (a needle's conic, a splat of det ~ 0);
      cov3D of the rot_4d path = Sigma_ij - c12_i c12_j / cov_t, by ulps of |Sigma_ij| + |c12_i c12_j / cov_t| (a long temporal axis
      turned slightly into space is added by the rotation and taken out again by the conditioning).  A float output is compared where the Gaussian is alive in the base
    evaluation: the perturbed value is taken before the cull zeroes it."""
    rng = np.random.default_rng(seed)
    base = forward(inp)
    eps = 2.0 ** -23

    def jig(a):
        a = _f64(a)
        return a * (1.0 + eps * rng.choice([-1.0, 1.0], size=a.shape))

    sens = {k: np.zeros_like(base[k]) for k in SENS_OF if base.get(k) is not None}
    for _ in range(draws):
        i2 = dict(inp)
        for k in PERTURBED:
            if inp.get(k) is not None:
                i2[k] = jig(inp[k])
        i2["timestamp"] = float(jig(np.array([inp["timestamp"]]))[0])
        got = forward(i2, jitter={"cov": rng.choice([-1.0, 1.0], size=(inp["P"], 6)), "det": rng.choice([-1.0, 1.0], size=inp["P"])})
        same = got["alive"] == base["alive"]
        for k in sens:
            d = np.abs(np.nan_to_num(got[k] - base[k], nan=np.inf))
            if k in FLOATS and k not in ("out_means3D", "cov3D"):
                d = np.where(same.reshape((-1,) + (1,) * (d.ndim - 1)), d, 0.0)   # (the flip itself is a flagged decision: see flags)
            sens[k] = np.maximum(sens[k], d)
    return base, sens


def flags(inp, base, sens):
    """Which decisions an fp32 evaluation may legally take the other way: {name: bool [P] (rgb: [P,3])}, and ``geo`` = any of near,
    marg, det, rad, rect (radius, tile count and rectangle follow from one another, so a Gaussian's geometry is flagged as a whole).

    The quantity's own fp32 step: one ulp32 of |z|, of the marginal, of cx cz + cy cy (det is their difference), of 3 sqrt(lambda)
    plus what an ulp of mid^2 -- the larger term of mid^2 - det, which fp32 forms before the square root -- does to it (an isotropic
    splat's discriminant cancels, and no ulp on an INPUT shows that), of the quotient's numerator over 16, of the sum of a channel's
    |terms|, of 255 opacity."""
    P, W, H = inp["P"], inp["W"], inp["H"]
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    F = FLAG_ULPS
    fl = {}
    with np.errstate(all="ignore"):
        fl["near"] = np.abs(base["near"]) <= F * (ulp32(base["near"] + NEAR) + sens["near"])
        fl["marg"] = np.zeros(P, bool) if base["marg"] is None else np.abs(base["marg"]) <= F * (ulp32(base["marg"] + 0.05) + sens["marg"])
        fl["det"] = ~(np.abs(base["det"]) > F * (ulp32(base["_cxcz"]) + sens["det"]))
        lam, disc, mid = base["_lam"], base["_disc"], base["_mid"]
        own = ulp32(base["rad"]) + np.where(disc > FLOOR, 3.0 / (4.0 * np.sqrt(lam) * np.sqrt(disc)), 0.0) * 2.0 * ulp32(mid * mid)
        d = F * (own + sens["rad"])
        rad = base["rad"]
        fl["rad"] = ~(np.ceil(rad - d) == np.ceil(rad + d))
        pix = np.nan_to_num(base["pix_all"])
        r = np.ceil(np.nan_to_num(rad, nan=0.0, posinf=0.0))
        num = np.abs(pix).max(1) + r + TILE
        dq = F * (ulp32(num) / TILE + sens["pix_all"].max(1) / TILE)
        lo, hi = rect_of(pix, r, gx, gy, -dq[:, None]), rect_of(pix, r, gx, gy, dq[:, None])
        fl["rect"] = (lo != hi).any(1) | ~np.isfinite(base["pix_all"]).all(1)
        if base["rgb_pre"] is not None:
            fl["rgb"] = ~(np.abs(base["rgb_pre"]) > F * (ulp32(base["rgb_mag"]) + sens["rgb_pre"]))
        else:
            fl["rgb"] = np.zeros((P, 3), bool)
        fl["opa"] = np.abs(base["opa255"]) <= F * (ulp32(1.0) + sens["opa255"])
    # a stage of the cull is only a decision for the Gaussians that reach it
    fl["near"] &= base["alive_t"]
    fl["det"] &= base["alive_n"]
    fl["rad"] &= base["alive_n"]
    fl["rect"] &= base["alive_n"]
    fl["geo"] = fl["near"] | fl["marg"] | fl["det"] | fl["rad"] | fl["rect"]
    return fl


def ratio(got, f64, sens):
    return co.ratio(got, f64, sens)


def flagged_elements(got, f64, sens, K):
    """The comparison the GPU test asserts with: indices of the elements beyond K * (4 ulp32 of |f64_e| + sens_e)."""
    return co.flagged(got, f64, sens, K)
