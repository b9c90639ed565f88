"""numpy restatement of the feature blend and its adjoint (csrc/features.hip, fdgs_feature_blend / fdgs_feature_blend_backward) on a
walk of the port oracle's lists (tests/contribution_oracle.py: ``walk`` returns one row (pix, gid, w) per contribution, the
decisions the oracle's own, w = alpha * T in float64).  tests/test_feature_oracle_host.py pins both functions to the oracle's colour
image and colour gradient."""
import numpy as np


def forward(wk, F):
    """float64 [C,H,W]: out[c, pixel] = sum over the pixel's contributions of w * F[gid, c].  ``F``: [P,C] (or [P])."""
    F = np.asarray(F, np.float64)
    if F.ndim == 1:
        F = F[:, None]
    H, W = wk["H"], wk["W"]
    out = np.zeros((H * W, F.shape[1]), np.float64)
    np.add.at(out, wk["pix"], wk["w"][:, None] * F[wk["gid"]])
    return np.ascontiguousarray(out.T).reshape(F.shape[1], H, W)


def backward(wk, g, P):
    """float64 [P,C]: dF[gid, c] = sum over the pixels gid contributes to of w * g[c, pixel].  ``g``: [C,H,W]."""
    g = np.asarray(g, np.float64)
    Cn = g.shape[0]
    gp = g.reshape(Cn, -1).T   # [pixel, C]
    d = np.zeros((P, Cn), np.float64)
    np.add.at(d, wk["gid"], wk["w"][:, None] * gp[wk["pix"]])
    return d
