"""Float64 numpy oracle of the blend forward and backward (csrc/blend_fwd.hip, csrc/blend_bwd.hip), with a first-order error unit next
to every output element.  No GPU, no reference code: the semantics are the ones stated at the top of the two kernels.

Inputs are what the kernels read: the 12-float records (``means2D`` [P,2], ``conic_opacity`` [P,4] = conic xx, xy, yy, opacity, ``rgb``
[P,3], ``rec_depth`` [P], ``rec_flow`` [P,2]: fp32 values, taken to float64 exactly), ``point_list``, ``ranges`` [T,2], ``bg`` [3], W, H;
the backward also the forward's ``n_contrib`` and ``final_T`` and the four upstream images.  The block cull and the queue are ignored.

Forward, per pixel, front to back:  d = mean - pixel,  power = -(A dx^2 + C dy^2) / 2 - B dx dy,  G = exp(power),  alpha = min(0.99f,
opacity G); an entry with power > 0 or alpha < 1/255 is skipped; the pixel stops, uncounted, at the first entry with T (1 - alpha) <
1e-4; else w = alpha T joins colour / depth / flow, T <- T (1 - alpha), n_contrib <- list position + 1.  colour += T bg at the end.
(The three thresholds are the fp32 constants of the kernels.)

Backward, per pixel, from list position n_contrib - 1 to the front, the same skip test (the clamp is ignored: q is built from the
unclamped G):  T <- T / (1 - alpha) starting from final_T;  the reference's seven recurrences  acc_k <- la last_k + (1 - la) acc_k  (rgb,
flow, depth, mask with c = 1);  dL/dalpha = T sum_k (c_k - acc_k) dL_k - final_T (bg . dL_rgb) / (1 - alpha);  q = G dL/dalpha; record
words: 0-2 alpha T dL_rgb, 3 alpha T dL_depth, 4-5 alpha T dL_flow, 6-11 q dx, q dy, q dx^2, q dy^2, q dx dy, q -- each summed over pixels.

THE ERROR UNIT (absolute; eps = EPS32 = 2^-24, the relative error of one fp32 rounding).  First order, from the structure alone:
  power     p1 = A dx^2 / 2, p2 = C dy^2 / 2, p3 = B dx dy.  Each product sees two roundings of dx / dy (d = mean - pixel), two multiplies and
            at most two additions on its way into the sum: |err power| <= 6 eps S, S = |p1| + |p2| + |p3|.
  G         an ABSOLUTE error of power is a RELATIVE error of G; exp itself is C_EXP = 4 eps (hardware exp2 at 1 ulp, and the product
            power * log2 e: one rounding and the rounded constant, each |power| eps <= S eps):  rel G = eps (8 S + C_EXP).
  alpha     = opacity G: rel alpha = rel G + eps.   1 - alpha: relative error alpha rel alpha / (1 - alpha) + eps.
  T         forward: T <- T (1 - alpha): rel T grows by alpha rel alpha / (1 - alpha) + 2 eps per contributor;  backward: T <- T * rcp(1 -
            alpha): by alpha rel alpha / (1 - alpha) + (C_RCP + 2) eps, C_RCP = 2 (v_rcp_f32 at 1 ulp).  final_T is an input: exact.
  forward   w = alpha T: rel alpha + rel T + eps; a channel takes c w by FMA: |c| w (rel w + eps) and eps |partial sum| per step; the fold of
            the even / odd accumulators and  + T bg: 2 eps (sum |c| w + T |bg|) and T |bg| (rel T + eps).  out_T: T rel T.
  backward  words 0-5: |term| (rel alpha + rel T + 2 eps).   The recurrences, carried as ONE pair (Mabs, ES) = (sum_k |acc_k dL_k| by the same
            recurrence on absolute values, its error):  ES <- la Labs (rel la + 3 eps) + (1 - la) ES + Mabs (la rel la + 2 eps) + eps Mabs'.
            dL/dalpha = (Cd - S) T + nTf_bg / (1 - alpha): every subtraction priced at the sum of the absolute values of its operands --
            A1 = (Cabs + Mabs) T with Cabs = sum_k |c_k dL_k|, Babs = final_T sum_i |bg_i dL_i| / (1 - alpha):
              err = T (8 eps Cabs + ES) + A1 (rel T + 3 eps) + Babs (7 eps + alpha rel alpha / (1 - alpha) + C_RCP eps) + eps (A1 + Babs).
            q = G dL/dalpha: G err + G (A1 + Babs) (rel G + eps); a moment q m (m = dx, dy, dx^2, ...): err_q |m| + G (A1 + Babs) |m| r eps,
            r = 2 for dx, dy, 4 for the squares, 0 for q itself.
  a record word = sum over its pixels of the per-pixel units + eps sum |term| depth, depth = 6 (the butterfly and the drain inside a block)
            + the number of (block, Gaussian) atomics that touch the record, in whatever order.

CLIFFS.  A pixel is flagged if an entry it examines in the forward has alpha within 1e-5 (relative) of 1/255, T (1 - alpha) within 1e-5
(relative) of 1e-4, or |power| <= 1e-6: there two correct evaluations may decide differently.
"""
import numpy as np

EPS32 = 2.0 ** -24
ALPHA_MIN = float(np.float32(1.0) / np.float32(255.0))
ALPHA_MAX = float(np.float32(0.99))
T_MIN = float(np.float32(0.0001))
CLIFF_REL = 1e-5
CLIFF_POWER = 1e-6
C_EXP = 4.0
C_RCP = 2.0
BLOCK_DEPTH = 6
PLANTS = ("swap89", "xy_as_xx", "no_bg", "cur_alpha", "row_dropped", "pair_other", "no_mask")


def _d(x):
    return np.asarray(x).astype(np.float64)


def _pixels(W, H, ranges):
    yy, xx = np.divmod(np.arange(W * H), W)
    tile = (yy // 16) * ((W + 15) // 16) + xx // 16
    rg = np.asarray(ranges).astype(np.int64)
    return xx, yy, rg[tile, 0], rg[tile, 1] - rg[tile, 0]


def _entry(rec, g, xx, yy):
    """-> dx, dy, power, S, G, opacity * G of Gaussians ``g`` at the pixels (float64)."""
    m, co = rec["m"], rec["co"]
    dx, dy = m[g, 0] - xx, m[g, 1] - yy
    p1, p2, p3 = 0.5 * co[g, 0] * dx * dx, 0.5 * co[g, 2] * dy * dy, co[g, 1] * dx * dy
    power = -(p1 + p2) - p3
    with np.errstate(over="ignore"):
        G = np.exp(power)
    return dx, dy, power, np.abs(p1) + np.abs(p2) + np.abs(p3), G, co[g, 3] * G


def _rec64(rec):
    return {"m": _d(rec["means2D"]), "co": _d(rec["conic_opacity"]),
            "ch": np.concatenate([_d(rec["rgb"]), _d(rec["rec_depth"]).reshape(-1, 1), _d(rec["rec_flow"])], axis=1)}   # r g b depth fx fy


def forward(rec, point_list, ranges, bg, W, H):
    """-> dict: out_color [3,H,W], out_flow [2,H,W], out_depth, out_T, n_contrib [H,W]; u_color, u_flow, u_depth, u_T: the units;
    flagged [H,W] bool; done_at [H,W]: list position (0-based) of the entry that stopped the pixel, -1 if none did."""
    r = _rec64(rec)
    pl = np.asarray(point_list).astype(np.int64)
    bg = _d(bg)
    xx, yy, r0, n = _pixels(W, H, ranges)
    N = W * H
    T, rT = np.ones(N), np.zeros(N)
    done, flag = np.zeros(N, bool), np.zeros(N, bool)
    last, done_at = np.zeros(N, np.int64), np.full(N, -1, np.int64)
    C, aC, uC = np.zeros((6, N)), np.zeros((6, N)), np.zeros((6, N))
    for k in range(int(n.max()) if N else 0):
        live = (k < n) & ~done
        if not live.any():
            break
        g = pl[np.where(k < n, r0 + k, 0)] if pl.size else np.zeros(N, np.int64)
        dx, dy, power, S, G, araw = _entry(r, g, xx, yy)
        alpha = np.minimum(ALPHA_MAX, araw)
        relA = EPS32 * (8.0 * S + C_EXP + 1.0)
        valid = live & ~(power > 0) & ~(alpha < ALPHA_MIN)
        testT = T * (1.0 - alpha)
        cliff = (np.abs(power) <= CLIFF_POWER) | (np.abs(araw - ALPHA_MIN) <= CLIFF_REL * ALPHA_MIN) | (valid & (np.abs(testT - T_MIN) <= CLIFF_REL * T_MIN))
        flag |= live & cliff
        low = testT < T_MIN
        contrib, fin = valid & ~low, valid & low
        done_at[fin] = k
        done |= fin
        w = alpha * T
        term = np.where(contrib, r["ch"][g].T * w, 0.0)
        uC += np.abs(term) * (relA + rT + 2.0 * EPS32) + np.where(contrib, EPS32 * aC, 0.0)
        C += term
        aC += np.abs(term)
        rT = np.where(contrib, rT + alpha * relA / (1.0 - alpha) + 2.0 * EPS32, rT)
        T = np.where(contrib, testT, T)
        last = np.where(contrib, k + 1, last)
    sh = (H, W)
    Tb = T[None, :] * np.abs(bg)[:, None]
    return {"out_color": (C[0:3] + T[None, :] * bg[:, None]).reshape(3, H, W),
            "u_color": (uC[0:3] + Tb * (rT + EPS32) + 2.0 * EPS32 * (aC[0:3] + Tb)).reshape(3, H, W),
            "out_depth": C[3].reshape(sh), "u_depth": (uC[3] + EPS32 * aC[3]).reshape(sh),
            "out_flow": C[4:6].reshape(2, H, W), "u_flow": (uC[4:6] + EPS32 * aC[4:6]).reshape(2, H, W),
            "out_T": T.reshape(sh), "u_T": (T * rT).reshape(sh), "n_contrib": last.reshape(sh), "flagged": flag.reshape(sh),
            "done_at": done_at.reshape(sh)}


def _upstream(W, H, dL_color, dL_depth, dL_alpha, dL_flow):
    """[7, N]: the upstream gradient of r g b, flow x y, depth, mask (None: zero)."""
    N = W * H
    z = lambda a, c: np.zeros((c, N)) if a is None else _d(a).reshape(c, N)   # noqa: E731
    return np.concatenate([z(dL_color, 3), z(dL_flow, 2), z(dL_depth, 1), z(dL_alpha, 1)], axis=0)


def backward(rec, point_list, ranges, bg, W, H, n_contrib, final_T, dL_color=None, dL_depth=None, dL_alpha=None, dL_flow=None, plant=None,
             plant_block=(0, 0), ignore=None):
    """-> dict: words [P,12] float64; unit [P,12] (the whole unit); usum [P,12] (its summation part, eps sum |term| depth); nblk [P]: the
    (block, Gaussian) pairs with an accepting pixel; accepted [P] bool: some pixel outside ``ignore`` ([H,W] bool) accepts it.  ``plant``: one of PLANTS (a kernel with that bug);
    ``plant_block`` = (block x, block y) of the 8x8 block the block-local plants act on."""
    r = _rec64(rec)
    P = r["m"].shape[0]
    pl = np.asarray(point_list).astype(np.int64)
    bg = _d(bg)
    xx, yy, r0, n = _pixels(W, H, ranges)
    N = W * H
    last = np.asarray(n_contrib).astype(np.int64).reshape(N)
    Tf = _d(final_T).reshape(N)
    dL = _upstream(W, H, dL_color, dL_depth, dL_alpha, dL_flow)
    if plant == "no_mask":
        dL = dL.copy()
        dL_D = dL.copy()
        dL_D[6] = 0.0
    else:
        dL_D = dL
    bgdot = (bg[:, None] * dL[0:3]).sum(0)
    nTf, Nabs = -Tf * bgdot, Tf * (np.abs(bg)[:, None] * np.abs(dL[0:3])).sum(0)
    if plant == "no_bg":
        nTf = np.zeros(N)
    blk = (yy // 8) * ((W + 7) // 8) + xx // 8
    nblocks = int(blk.max()) + 1 if N else 0
    in_pb = (xx // 8 == plant_block[0]) & (yy // 8 == plant_block[1])
    T, rT = Tf.copy(), np.zeros(N)
    acc, lastc = np.zeros((7, N)), np.zeros((7, N))
    la, rel_la, Mabs, ES, Labs = np.zeros(N), np.zeros(N), np.zeros(N), np.zeros(N), np.zeros(N)
    words, unit, sabs = np.zeros((P, 12)), np.zeros((P, 12)), np.zeros((P, 12))
    touched = np.zeros((nblocks, P), bool)
    accepted = np.zeros(P, bool)
    count = np.ones(N, bool) if ignore is None else ~np.asarray(ignore, bool).reshape(N)
    for k in range(int(last.max()) - 1 if N else -1, -1, -1):
        inl = k < last
        g = pl[np.where(inl, r0 + k, 0)]
        dx, dy, power, S, G, araw = _entry(r, g, xx, yy)
        alpha = np.minimum(ALPHA_MAX, araw)
        act = inl & ~(power > 0) & ~(alpha < ALPHA_MIN)
        if not act.any():
            continue
        relA = EPS32 * (8.0 * S + C_EXP + 1.0)
        one = 1.0 - alpha
        Tn = T / one
        rTn = rT + alpha * relA / one + (C_RCP + 2.0) * EPS32
        dch = alpha * Tn
        c = np.concatenate([r["ch"][g][:, 0:3].T, r["ch"][g][:, 4:6].T, r["ch"][g][:, 3:4].T, np.ones((1, N))], axis=0)
        f = alpha if plant == "cur_alpha" else la
        acc_n = f * lastc + (1.0 - f) * acc
        Mabs_n = la * Labs + (1.0 - la) * Mabs
        ES_n = la * Labs * (rel_la + 3.0 * EPS32) + (1.0 - la) * ES + Mabs * (la * rel_la + 2.0 * EPS32) + EPS32 * Mabs_n
        Cabs = np.abs(c * dL).sum(0)
        D = ((c - acc_n) * dL_D).sum(0)
        A1, Babs = (Cabs + Mabs_n) * Tn, Nabs / one
        dLda = D * Tn + nTf / one
        e = Tn * (8.0 * EPS32 * Cabs + ES_n) + A1 * (rTn + 3.0 * EPS32) + Babs * ((7.0 + C_RCP) * EPS32 + alpha * relA / one) + EPS32 * (A1 + Babs)
        q, Qabs = G * dLda, G * (A1 + Babs)
        eq = G * e + Qabs * relA
        t = np.empty((12, N))
        u = np.empty((12, N))
        t[0:3], t[3], t[4:6] = dch * dL[0:3], dch * dL[5], dch * dL[3:5]
        u[0:6] = np.abs(t[0:6]) * (relA + rTn + 2.0 * EPS32)
        mom = (dx, dy, dx * dx, dy * dy, dx * dx if plant == "xy_as_xx" else dx * dy, np.ones(N))
        for j, (mj, rj) in enumerate(zip(mom, (2.0, 2.0, 4.0, 4.0, 4.0, 0.0))):
            t[6 + j] = q * mj
            u[6 + j] = (eq + Qabs * rj * EPS32) * np.abs(mj)
        m = act
        if plant == "row_dropped":
            m = act & ~(in_pb & (yy % 8 == 3))
        to = g
        if plant == "pair_other":
            other = pl[np.where(inl & ((k ^ 1) < n), r0 + (k ^ 1), np.where(inl, r0 + k, 0))]
            to = np.where(in_pb, other, g)
        np.add.at(words, to[m], t[:, m].T)
        np.add.at(unit, g[act], u[:, act].T)
        np.add.at(sabs, g[act], np.abs(t[:, act]).T)
        touched[blk[act], g[act]] = True
        accepted[g[act & count]] = True
        # state
        T, rT = np.where(act, Tn, T), np.where(act, rTn, rT)
        acc = np.where(act, acc_n, acc)
        lastc = np.where(act, c, lastc)
        Mabs, ES = np.where(act, Mabs_n, Mabs), np.where(act, ES_n, ES)
        Labs = np.where(act, Cabs, Labs)
        la, rel_la = np.where(act, alpha, la), np.where(act, relA, rel_la)
    if plant == "swap89":
        words[:, [8, 9]] = words[:, [9, 8]]
    nblk = touched.sum(0)
    usum = EPS32 * sabs * (BLOCK_DEPTH + nblk)[:, None]
    return {"words": words, "unit": unit + usum, "usum": usum, "nblk": nblk, "accepted": accepted}


# ---------------------------------------------------------------------------------------------------------------------------------
# ref32: the REFERENCE's formulation in numpy float32 (one rounding per operation, no FMA): its association of power, T (1 - alpha) and
# T / (1 - alpha), its seven recurrences, a sequential fp32 sum per record word (np.add.at: one addition after the other, by list position
# from the deepest to the front and by pixel index inside a position).  One correct fp32 evaluation: it sets the constants K.
# ---------------------------------------------------------------------------------------------------------------------------------
def _entry32(rec, g, xx, yy):
    f = np.float32
    m, co = rec["means2D"].astype(f), rec["conic_opacity"].astype(f)
    dx, dy = m[g, 0] - xx.astype(f), m[g, 1] - yy.astype(f)
    power = f(-0.5) * (co[g, 0] * dx * dx + co[g, 2] * dy * dy) - co[g, 1] * dx * dy
    with np.errstate(over="ignore"):
        G = np.exp(power)
    return dx, dy, power, G, np.minimum(f(0.99), co[g, 3] * G)


def forward32(rec, point_list, ranges, bg, W, H):
    f = np.float32
    pl = np.asarray(point_list).astype(np.int64)
    bg = np.asarray(bg).astype(f)
    ch = np.concatenate([rec["rgb"], np.asarray(rec["rec_depth"]).reshape(-1, 1), rec["rec_flow"]], axis=1).astype(f)
    xx, yy, r0, n = _pixels(W, H, ranges)
    N = W * H
    T, done, last, C = np.ones(N, f), np.zeros(N, bool), np.zeros(N, np.int64), np.zeros((6, N), f)
    for k in range(int(n.max()) if N else 0):
        live = (k < n) & ~done
        if not live.any():
            break
        g = pl[np.where(k < n, r0 + k, 0)]
        dx, dy, power, G, alpha = _entry32(rec, g, xx, yy)
        valid = live & ~(power > 0) & ~(alpha < f(1.0) / f(255.0))
        testT = T * (f(1) - alpha)
        low = testT < f(0.0001)
        contrib = valid & ~low
        done |= valid & low
        C = np.where(contrib, C + ch[g].T * (alpha * T), C)
        T = np.where(contrib, testT, T)
        last = np.where(contrib, k + 1, last)
    return {"out_color": (C[0:3] + T[None, :] * bg[:, None]).reshape(3, H, W), "out_depth": C[3].reshape(H, W),
            "out_flow": C[4:6].reshape(2, H, W), "out_T": T.reshape(H, W), "n_contrib": last.reshape(H, W)}


def backward32(rec, point_list, ranges, bg, W, H, n_contrib, final_T, dL_color=None, dL_depth=None, dL_alpha=None, dL_flow=None):
    f = np.float32
    P = rec["means2D"].shape[0]
    pl = np.asarray(point_list).astype(np.int64)
    bg = np.asarray(bg).astype(f)
    chn = np.concatenate([rec["rgb"], rec["rec_flow"], np.asarray(rec["rec_depth"]).reshape(-1, 1), np.ones((P, 1))], axis=1).astype(f)
    xx, yy, r0, n = _pixels(W, H, ranges)
    N = W * H
    last = np.asarray(n_contrib).astype(np.int64).reshape(N)
    Tf = np.asarray(final_T).astype(f).reshape(N)
    dL = _upstream(W, H, dL_color, dL_depth, dL_alpha, dL_flow).astype(f)
    bgdot = np.zeros(N, f)
    for i in range(3):
        bgdot = bgdot + bg[i] * dL[i]
    T, la = Tf.copy(), np.zeros(N, f)
    acc, lastc = np.zeros((7, N), f), np.zeros((7, N), f)
    words = np.zeros((P, 12), f)
    for k in range(int(last.max()) - 1 if N else -1, -1, -1):
        inl = k < last
        g = pl[np.where(inl, r0 + k, 0)]
        dx, dy, power, G, alpha = _entry32(rec, g, xx, yy)
        act = inl & ~(power > 0) & ~(alpha < f(1.0) / f(255.0))
        if not act.any():
            continue
        Tn = T / (f(1) - alpha)
        dch = alpha * Tn
        c = chn[g].T
        dLda = np.zeros(N, f)
        acc_n = np.empty((7, N), f)
        for j in range(7):
            acc_n[j] = la * lastc[j] + (f(1) - la) * acc[j]
            dLda = dLda + (c[j] - acc_n[j]) * dL[j]
        dLda = dLda * Tn
        dLda = dLda + (-Tf / (f(1) - alpha)) * bgdot
        q = G * dLda
        t = np.stack([dch * dL[0], dch * dL[1], dch * dL[2], dch * dL[5], dch * dL[3], dch * dL[4],
                      q * dx, q * dy, q * dx * dx, q * dy * dy, q * dx * dy, q]).astype(f)
        np.add.at(words, g[act], t[:, act].T)
        T, acc, lastc, la = np.where(act, Tn, T), np.where(act, acc_n, acc), np.where(act, c, lastc), np.where(act, alpha, la)
    return words


def ratio(got, want, unit):
    """|got - want| / unit, element by element; 0 where both the difference and the unit are 0; inf for a non-finite ``got`` or a
    difference where the unit is 0."""
    d = np.nan_to_num(np.abs(np.asarray(got, np.float64).reshape(np.shape(want)) - want), nan=np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(d == 0, 0.0, d / unit)


WORD_CLASS = ("w0_2", "w0_2", "w0_2", "w3", "w4_5", "w4_5", "w6_7", "w6_7", "w8_10", "w8_10", "w8_10", "w11")
