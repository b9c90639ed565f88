"""numpy restatement of the contribution statistics (csrc/contribution.hip, fdgs_contribution) on the port oracle's forward outputs.

``walk`` takes the oracle's ``means2D``, ``conic_opacity``, ``point_list`` and ``ranges`` and walks every pixel's tile list with the
DECISIONS of ``render_fwd_pixel`` (oracle/fdgs_oracle.c: forward.cu:501-626) in the same float32 arithmetic -- the same
association of ``power``, libm's ``expf`` itself (called through ctypes: numpy's vectorised exp may differ from it in the last bit),
``min(0.99, .)``, ``T * (1 - alpha)`` -- so that the set of (pixel, entry) contributions is the oracle's own: tests/
test_contribution_oracle_host.py pins it to the oracle's n_contrib, out_T and dL_dcolor.  The weights w = alpha * T of the
contributions are then formed and accumulated in float64.  ``reduce`` turns a walk into the five outputs for any pixel-weight map.
"""
import ctypes
import ctypes.util

import numpy as np

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.expf.argtypes = [ctypes.c_float]
_libm.expf.restype = ctypes.c_float

NEAR_TIE_REL = 1e-5
F32 = np.float32


def _expf(x):
    """libm expf, element by element (float32 in, float32 out)."""
    f = _libm.expf
    return np.array([f(v) for v in x.tolist()], dtype=F32)


def walk(ref, W, H):
    """Per-pixel walk of the oracle's lists.  Returns a dict:
    pix / gid / w   -- one row per (pixel, entry) contribution, pixels in index order, entries in list order: flat pixel index,
                       Gaussian index, float64 weight
    dominant_id     -- int32 [H,W]: largest-w contributor (earliest on a tie), -1 without one
    near_tie        -- bool [H,W]: the two largest w differ by less than 1e-5 relative
    ended_early     -- bool [H,W]: an entry took T below 1e-4 and ended the pixel
    last_pos        -- uint32 [H,W]: 1-based list position of the last contributor (the oracle's n_contrib)
    sum_w           -- float64 [H,W]: sum of w
    max_contrib     -- the largest number of contributions of one pixel"""
    m2d = np.asarray(ref["means2D"], F32)
    co = np.asarray(ref["conic_opacity"], F32)
    plist = np.asarray(ref["point_list"]).astype(np.int64)
    ranges = np.asarray(ref["ranges"]).astype(np.int64)
    gx = (W + 15) // 16
    dom = np.full((H, W), -1, np.int32)
    near = np.zeros((H, W), bool)
    early = np.zeros((H, W), bool)
    last = np.zeros((H, W), np.uint32)
    sumw = np.zeros((H, W), np.float64)
    rows_pix, rows_gid, rows_w, rows_ord = [], [], [], []
    max_contrib = 0
    one, half, amin, tmin, acap = F32(1.0), F32(-0.5), F32(1.0) / F32(255.0), F32(0.0001), F32(0.99)
    for t in range(ranges.shape[0]):
        r0, r1 = ranges[t]
        tx, ty = t % gx, t // gx
        xs = np.arange(tx * 16, min(tx * 16 + 16, W))
        ys = np.arange(ty * 16, min(ty * 16 + 16, H))
        if xs.size == 0 or ys.size == 0 or r1 <= r0:
            continue
        py, px = [a.reshape(-1) for a in np.meshgrid(ys, xs, indexing="ij")]
        npix = px.size
        g = plist[r0:r1]
        n = g.size
        # forward.cu:585-586 in float32, the C expression's association: -0.5f * (A dx dx + C dy dy) - B dx dy
        dx = m2d[g, 0][:, None] - px.astype(F32)[None, :]
        dy = m2d[g, 1][:, None] - py.astype(F32)[None, :]
        A, B, Cc, op = (co[g, k][:, None] for k in range(4))
        power = half * (A * dx * dx + Cc * dy * dy) - B * dx * dy
        assert power.dtype == F32 and float(op.max()) <= 1.0
        # alpha >= 1/255 needs exp(power) >= 1 / (255 opacity) >= 1 / 255, i.e. power >= -5.55: below -6 the entry is rejected for sure
        cand = (power <= 0.0) & (power >= -6.0)
        alpha = np.zeros_like(power)
        alpha[cand] = np.minimum(acap, (np.broadcast_to(op, power.shape)[cand] * _expf(power[cand])).astype(F32))
        T = np.ones(npix, F32)
        done = np.zeros(npix, bool)
        best = np.zeros(npix, np.float64)
        second = np.zeros(npix, np.float64)
        best_id = np.full(npix, -1, np.int32)
        lastc = np.zeros(npix, np.uint32)
        s = np.zeros(npix, np.float64)
        count = np.zeros(npix, np.int64)
        for k in range(n):
            a = alpha[k]
            valid = ~done & cand[k] & ~(a < amin)
            if not valid.any():
                continue
            test_T = (T * (one - a)).astype(F32)
            low = test_T < tmin
            ends = valid & low
            early[py[ends], px[ends]] = True
            done |= ends
            c = valid & ~low
            if not c.any():
                continue
            idx = np.nonzero(c)[0]
            w = a[idx].astype(np.float64) * T[idx].astype(np.float64)
            T[idx] = test_T[idx]
            lastc[idx] = k + 1
            s[idx] += w
            count[idx] += 1
            better = w > best[idx]
            second[idx] = np.where(better, best[idx], np.maximum(second[idx], w))
            best_id[idx] = np.where(better, np.int32(g[k]), best_id[idx])
            best[idx] = np.where(better, w, best[idx])
            rows_pix.append((py[idx] * W + px[idx]).astype(np.int64))
            rows_gid.append(np.full(idx.size, g[k], np.int64))
            rows_w.append(w)
            rows_ord.append(np.full(idx.size, k, np.int64))
        dom[py, px] = best_id
        near[py, px] = (second > 0.0) & ((best - second) < NEAR_TIE_REL * best)
        last[py, px] = lastc
        sumw[py, px] = s
        max_contrib = max(max_contrib, int(count.max()))
    if rows_pix:
        pix, gid, w, order = (np.concatenate(r) for r in (rows_pix, rows_gid, rows_w, rows_ord))
        o = np.lexsort((order, pix))
        pix, gid, w = pix[o], gid[o], w[o]
    else:
        pix, gid, w = np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float64)
    return {"pix": pix, "gid": gid, "w": w, "dominant_id": dom, "near_tie": near, "ended_early": early, "last_pos": last, "sum_w": sumw,
            "max_contrib": max_contrib, "W": W, "H": H}


def reduce(wk, P, pix_weight=None):
    """The five outputs of fdgs_contribution for one view from a ``walk``: weight_sum / weight_max (float64 [P]), hits / dominant
    (int64 [P]), dominant_id (int32 [H,W]).  ``pix_weight`` [H,W] or None: a pixel with weight <= 0 is skipped entirely."""
    H, W = wk["H"], wk["W"]
    pw = np.ones(H * W, np.float64) if pix_weight is None else np.asarray(pix_weight, np.float32).astype(np.float64).reshape(-1)
    live = pw > 0.0
    sel = live[wk["pix"]]
    pix, gid, w = wk["pix"][sel], wk["gid"][sel], wk["w"][sel]
    weight_sum = np.zeros(P, np.float64)
    weight_max = np.zeros(P, np.float64)
    hits = np.zeros(P, np.int64)
    np.add.at(weight_sum, gid, pw[pix] * w)
    np.maximum.at(weight_max, gid, w)
    np.add.at(hits, gid, 1)
    dom = np.where(live.reshape(H, W), wk["dominant_id"], -1).astype(np.int32)
    dominant = np.bincount(dom[dom >= 0].astype(np.int64), minlength=P).astype(np.int64)
    return {"weight_sum": weight_sum, "weight_max": weight_max, "hits": hits, "dominant": dominant, "dominant_id": dom}


def contribution_oracle(ref, P, W, H, pix_weight=None):
    """The five outputs plus ``near_tie`` (bool [H,W]) for the oracle forward ``ref``."""
    wk = walk(ref, W, H)
    out = reduce(wk, P, pix_weight)
    out["near_tie"] = wk["near_tie"]
    return out
