"""float64 / Python-int restatement of csrc/mcmc.hip (include/fdgs_mcmc.h): the yardstick of tests/test_mcmc_host.py and
tests/test_gpu_mcmc.py.

* sampling: 24-bit integer weights, exact prefix sums, Philox4x32-10 draws (tests/seed_oracle.py), u = (r64 * total) >> 64 in Python
  ints, the first prefix above u.
* ``new_opacity_and_ratio``: o' = 1 - (1 - o)^(1/N) and D as the literal double sum of the definition, in float64;
  ``exact_D`` is the same sum in rational arithmetic with 50-digit roots (the host test holds the one to the other).
* ``covariance`` / ``noise_delta``: Sigma from raw parameters and Sigma xi g(o) scale, float64.
* ``regularizer``: the three terms and their gradients, float64.
"""
import decimal
import math
from fractions import Fraction

import numpy as np

import seed_oracle

WEIGHT_ONE = 1 << 24
MAX_N = 51
O_MIN, O_MAX = 0.005, 1.0 - 2.0 ** -23
STREAM_RELOCATE, STREAM_GROW, STREAM_NOISE = 0, 1, 2


def sigmoid(x):
    x = np.asarray(x, np.float64)
    return 1.0 / (1.0 + np.exp(-x))


# ---- sampling ----
def weights_f64(opacity_raw, min_opacity=0.005):
    """rint(o 2^24) with o in float64 (the kernel's float32 sigmoid may differ by a unit or two), 0 for dead rows."""
    o = sigmoid(opacity_raw).reshape(-1)
    return np.where(o > np.float64(np.float32(min_opacity)), np.rint(o * WEIGHT_ONE), 0).astype(np.uint64)


def prefix_of(wq):
    return np.cumsum(np.asarray(wq, np.uint64), dtype=np.uint64)


def philox_words(n, seed, stream_id, call):
    counter = np.zeros((n, 4), np.uint32)
    counter[:, 0] = np.arange(n, dtype=np.uint32)
    counter[:, 1] = np.uint32(stream_id)
    counter[:, 2] = np.uint32(call & 0xFFFFFFFF)
    counter[:, 3] = np.uint32((call >> 32) & 0xFFFFFFFF)
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint32)
    return seed_oracle.philox4x32_10(counter, key[None, :])


def select(prefix, u):
    """The smallest i with prefix[i] > u (Python ints)."""
    lo, hi = 0, len(prefix) - 1
    while lo < hi:
        mid = (lo + hi) // 2
        if int(prefix[mid]) > u:
            hi = mid
        else:
            lo = mid + 1
    return lo


def draw(prefix, n, seed, stream_id, call):
    """(source int64 [n], counts int64 [P], words uint32 [n, 4]) from the prefix sums, all integer."""
    prefix = [int(v) for v in prefix]
    total = prefix[-1]
    words = philox_words(n, seed, stream_id, call)
    source, counts = np.zeros(n, np.int64), np.zeros(len(prefix), np.int64)
    for j in range(n):
        r64 = (int(words[j, 0]) << 32) | int(words[j, 1])
        u = (r64 * total) >> 64
        assert 0 <= u < total
        source[j] = select(prefix, u)
        counts[source[j]] += 1
    return source, counts, words


# ---- N copies of one Gaussian ----
def multiplicity(n_drawn):
    return np.minimum(np.asarray(n_drawn) + 1, MAX_N)


def new_opacity_and_ratio(o, N):
    """(o', D, o / D) in float64, D as the definition's double sum."""
    o, N = float(o), int(N)
    if N == 1:
        return o, o, 1.0
    op = -math.expm1(math.log1p(-o) / N)
    D = 0.0
    for i in range(1, N + 1):
        for k in range(i):
            D += math.comb(i - 1, k) * (-1.0) ** k * op ** (k + 1) / math.sqrt(k + 1)
    return op, D, o / D


def exact_D(o, N, digits=50):
    """(o', D) as decimal.Decimal: the N-th root and the square roots to ``digits`` digits, the binomial sum in exact rationals of
    those."""
    ctx = decimal.Context(prec=digits + 10)
    od = decimal.Decimal(o)                                    # the float64's exact value
    one = decimal.Decimal(1)
    root = ctx.power(ctx.subtract(one, od), ctx.divide(one, decimal.Decimal(N)))
    op = Fraction(ctx.subtract(one, root))
    total = Fraction(0)
    inv_sqrt = [Fraction(ctx.divide(one, ctx.sqrt(decimal.Decimal(k + 1)))) for k in range(N)]
    for i in range(1, N + 1):
        for k in range(i):
            total += math.comb(i - 1, k) * (-1) ** k * op ** (k + 1) * inv_sqrt[k]
    return op, total


def updated(opacity_raw, scaling_raw, N):
    """Activated new opacity (clamped) and scales of one Gaussian with raw float32 parameters that stands for N copies."""
    o = float(sigmoid(np.float64(opacity_raw)))
    op, _D, ratio = new_opacity_and_ratio(o, N)
    return min(max(op, O_MIN), O_MAX), np.exp(np.asarray(scaling_raw, np.float64)) * ratio


# ---- the noise step ----
def _normalize(q):
    return q / np.maximum(np.sqrt((q * q).sum(-1, keepdims=True)), 1e-12)


def rotation3(q):
    w, x, y, z = _normalize(np.asarray(q, np.float64)).T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], axis=1).reshape(-1, 3, 3)


def rotation4(ql, qr):
    """R4 = M_r M_l in the kernels' column-major reading (csrc/fdgs_math.h build_Ml_Mr), here as row-major numpy: A[row][col]."""
    a, b, c, d = _normalize(np.asarray(ql, np.float64)).T
    p, q, r, s = _normalize(np.asarray(qr, np.float64)).T
    # l[j][i], m[j][i] are COLUMN j, row i
    lcols = np.stack([np.stack([a, b, -c, d], 1), np.stack([-b, a, d, c], 1), np.stack([c, -d, a, b], 1), np.stack([-d, -c, -b, a], 1)], 1)
    mcols = np.stack([np.stack([p, q, -r, -s], 1), np.stack([-q, p, s, -r], 1), np.stack([r, -s, p, -q], 1), np.stack([s, r, q, p], 1)], 1)
    L, Mr = lcols.transpose(0, 2, 1), mcols.transpose(0, 2, 1)      # row-major matrices
    return Mr @ L


def covariance(model):
    """Sigma [P, d, d] (d = 3, or 4 with gaussian_dim == 4) in float64 from a dict of raw float32 arrays + gaussian_dim / rot_4d."""
    s = np.exp(np.asarray(model["_scaling"], np.float64))
    if model["rot_4d"]:
        s4 = np.concatenate([s, np.exp(np.asarray(model["_scaling_t"], np.float64)).reshape(-1, 1)], 1)
        M = s4[:, :, None] * rotation4(model["_rotation"], model["_rotation_r"])      # M = S R
        return M.transpose(0, 2, 1) @ M
    # the 3D path: R as the kernels build it (quat_to_R: column-major c[col][row], i.e. the transpose of rotation3), M = S R
    R = rotation3(model["_rotation"]).transpose(0, 2, 1)
    M = s[:, :, None] * R
    S3 = M.transpose(0, 2, 1) @ M
    if model["gaussian_dim"] == 3:
        return S3
    out = np.zeros((len(s), 4, 4))
    out[:, :3, :3] = S3
    out[:, 3, 3] = np.exp(np.asarray(model["_scaling_t"], np.float64)).reshape(-1) ** 2
    return out


def gate(o):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-100.0 * ((1.0 - o) - 0.995)))


def noise_delta(model, xi, scale):
    """delta [P, d] = Sigma xi g(o) scale in float64; xi [P, >= d]."""
    S = covariance(model)
    d = S.shape[1]
    o = sigmoid(model["_opacity"]).reshape(-1)
    return np.einsum("pij,pj->pi", S, np.asarray(xi, np.float64)[:, :d]) * (gate(o) * float(scale))[:, None]


def box_muller(words):
    """xi float64 [n, 4] from Philox words: u = ((w >> 8) + 1) 2^-24 in (0, 1]."""
    u = ((words >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    r0, r1 = np.sqrt(-2.0 * np.log(u[:, 0])), np.sqrt(-2.0 * np.log(u[:, 2]))
    a0, a1 = 2.0 * np.pi * u[:, 1], 2.0 * np.pi * u[:, 3]
    return np.stack([r0 * np.cos(a0), r0 * np.sin(a0), r1 * np.cos(a1), r1 * np.sin(a1)], 1)


# ---- the regularisers ----
def regularizer(opacity_raw, scaling_raw, scaling_t_raw, lam_o, lam_s, lam_st):
    """((L_o, L_s, L_st), g_opacity [P], g_scaling [P, 3], g_scaling_t [P]) in float64; the lambdas as the float32 the kernel gets."""
    lam_o, lam_s, lam_st = (float(np.float32(v)) for v in (lam_o, lam_s, lam_st))
    o = sigmoid(opacity_raw).reshape(-1)
    P = len(o)
    s = np.exp(np.asarray(scaling_raw, np.float64)).reshape(P, 3)
    st = np.exp(np.asarray(scaling_t_raw, np.float64)).reshape(P)
    x = np.asarray(opacity_raw, np.float64).reshape(-1)
    e = np.exp(-np.abs(x))
    dsig = e / (1.0 + e) ** 2
    terms = (lam_o / P * o.sum(), lam_s / (3 * P) * s.sum(), lam_st / P * st.sum() if lam_st > 0 else 0.0)
    return terms, lam_o / P * dsig, lam_s / (3 * P) * s, (lam_st / P * st if lam_st > 0 else np.zeros(P))
