"""float64 statement of csrc/exposure.hip (include/fdgs_exposure.h): the affine colour transform, its backward, the per-row Adam and
the ridge fit.  The yardstick of tests/test_exposure_host.py, tests/test_gpu_exposure.py and tests/test_gpu_pipeline_exposure.py.

Images are [3, H, W]; a row is 12 numbers A = [M | o], A[4 i + j] = M[i][j], A[4 i + 3] = o[i]."""
import numpy as np

IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float64)


def split(row):
    A = np.asarray(row, np.float64).reshape(3, 4)
    return A[:, :3], A[:, 3]


def apply(image, row):
    """out[i] = sum_j M[i][j] c[j] + o[i]."""
    M, o = split(row)
    c = np.asarray(image, np.float64)
    return np.einsum("ij,jhw->ihw", M, c) + o[:, None, None]


def apply_magnitude(image, row):
    """sum_j |M[i][j]| |c[j]| + |o[i]| per element: what the float32 kernel's rounding errors scale with."""
    M, o = split(row)
    return np.einsum("ij,jhw->ihw", np.abs(M), np.abs(np.asarray(image, np.float64))) + np.abs(o)[:, None, None]


def backward(g_out, image, row):
    """(d L / d image = M^T g', d L / d A [12]) from g' = d L / d out and the uncorrected image."""
    M, _o = split(row)
    g = np.asarray(g_out, np.float64)
    c = np.asarray(image, np.float64)
    g_image = np.einsum("ij,ihw->jhw", M, g)
    c1 = np.concatenate([c, np.ones_like(c[:1])])
    dA = np.einsum("ihw,jhw->ij", g, c1).reshape(12)
    return g_image, dA


def backward_magnitudes(g_out, image, row):
    """(sum_i |M[i][j]| |g'[i]| per element, sum over the pixels of |g'[i]| |(r, g, b, 1)[j]| [12])."""
    M, _o = split(row)
    g = np.abs(np.asarray(g_out, np.float64))
    c = np.abs(np.asarray(image, np.float64))
    c1 = np.concatenate([c, np.ones_like(c[:1])])
    return np.einsum("ij,ihw->jhw", np.abs(M), g), np.einsum("ihw,jhw->ij", g, c1).reshape(12)


def adam(table, exp_avg, exp_avg_sq, steps, indices, slots, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-15):
    """One step of the rows ``indices`` names (one index per view; slots [B, 12] the views' gradients): a row's gradient is the sum
    of its views' slots in view order, its own count advances by one, torch.optim.Adam's formula with that count.  Returns new
    (table, exp_avg, exp_avg_sq, steps); rows not named are returned as they came."""
    p, m, v = (np.array(a, np.float64) for a in (table, exp_avg, exp_avg_sq))
    t = np.array(steps, np.int64)
    slots = np.asarray(slots, np.float64)
    for row in dict.fromkeys(int(i) for i in indices):
        g = np.zeros(12)
        for b, i in enumerate(indices):
            if int(i) == row:
                g = g + slots[b]
        t[row] += 1
        m[row] = beta1 * m[row] + (1.0 - beta1) * g
        v[row] = beta2 * v[row] + (1.0 - beta2) * g * g
        bc1, bc2 = 1.0 - beta1 ** int(t[row]), 1.0 - beta2 ** int(t[row])
        p[row] = p[row] - lr / bc1 * (m[row] / (np.sqrt(v[row]) / np.sqrt(bc2) + eps))
    return p, m, v, t


def fit_moments(image, gt, clamp=True):
    """(M [4, 4] = sum [c; 1][c; 1]^T, N [3, 4] = sum gt [c; 1]^T, n) of a render against its ground truth."""
    c = np.asarray(image, np.float64).reshape(3, -1)
    if clamp:
        c = np.clip(c, 0.0, 1.0)
    t = np.asarray(gt, np.float64).reshape(3, -1)
    c1 = np.concatenate([c, np.ones_like(c[:1])])
    return c1 @ c1.T, t @ c1.T, c.shape[1]


def fit_affine(image, gt, ridge=1e-6, clamp=True, return_cond=False):
    """A = (N / n + ridge [I | 0]) (M / n + ridge I)^-1 as a row [12]; with ``return_cond`` also cond(M / n + ridge I)."""
    M, N, n = fit_moments(image, gt, clamp)
    lhs = M / n + ridge * np.eye(4)
    rhs = N / n + ridge * np.eye(3, 4)
    A = (rhs @ np.linalg.inv(lhs)).reshape(12)
    return (A, float(np.linalg.cond(lhs))) if return_cond else A


def psnr(image, gt):
    """The mean over channels of 20 log10(1 / sqrt(mse_c)) of the image clamped to [0, 1] (fdgs.metrics)."""
    c = np.clip(np.asarray(image, np.float64), 0.0, 1.0).reshape(3, -1)
    mse = ((c - np.asarray(gt, np.float64).reshape(3, -1)) ** 2).mean(axis=1)
    return float(np.mean(20.0 * np.log10(1.0 / np.sqrt(mse))))
