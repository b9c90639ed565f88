"""TEST INFRASTRUCTURE -- float64 statement (numpy) of one step of csrc/adam.hip, and per-element error bars for the fp32 kernel.

``step``   torch.optim.Adam arithmetic (no amsgrad, no weight decay) with a per-element learning rate from a segment table:

    m' = b1 m + (1 - b1) g;  v' = b2 v + (1 - b2) g^2;  p' = p - lr / (1 - b1^t) * m' / (sqrt(v') / sqrt(1 - b2^t) + eps)

Segment semantics (adam.hip, seg_lr): a segment (begin, end, lr, lr_head, period, head) covers the elements [begin, end)
clipped to [0, n); with period > 0 the elements whose phase (i - begin) mod period is below ``head`` take ``lr_head`` -- the
phase counts from ``begin`` itself, which may be negative; an element in no segment has lr = 0 (its moments still update);
an element in several segments takes the rate of the LAST one in the table.

The betas, eps and the rates enter as the float32 values the kernel receives, widened to float64; the bias corrections
1 - b^t are computed in double from the step, as the launcher computes them.  What is left between this and the kernel is the
kernel's own fp32 arithmetic, which ``bounds`` bars.  tests/test_adam_oracle_host.py pins ``step`` to torch.optim.Adam (float64).

``bounds``   |kernel - step| per element for ONE step from a given fp32 state, derived from the operations of adam_update
(csrc/fdgs_common.h) and of the launcher, not from observation.  The library is built without any fast-math flag
(csrc/build.sh) and hipcc's default is correctly rounded fp32 division and square root, so every operation below is the exact
result rounded once: fl(x) = x (1 + d), |d| <= u = 2^-24, as long as x is a normal fp32 number (the callers assert that their
inputs keep it so).  Hatted values are the kernel's, plain ones the exact ones; E_x bounds |x^ - x|.

    launcher   ib^ = fl(1 / bc1), k^ = fl(1 / sqrt(bc2))  (both from doubles: one rounding each);  K = 1 / sqrt(bc2)
               l^ = fl(lr * ib^)                          |l^ - L| <= (2u + u^2) |L| = E_L,      L = lr / bc1
    m          a^ = fl(c1 g), c1 = fl(1 - b1)             |a^ - c1 g| <= u |c1 g| (+ |c1 - (1 - b1)| |g| where 1 - b1 is not an fp32 number)
               m^ = fl(b1 m + a^)           (one fma)     E_m = E_a + u (|m'| + E_a)            -- half an ulp of (1-b1) g, half an ulp of the result
    v          t^ = fl(fl(c2 g) g)                        |t^ - c2 g^2| <= (2u + u^2) |c2 g^2| = E_t (+ the c2 term as above)
               v^ = fl(b2 v + t^)           (one fma)     E_v = E_t + u (v' + E_t)              -- two roundings of (1-b2) g g, half an ulp of the result
    sqrt       s^ = fl(sqrt(v^))                          |sqrt(v^) - sqrt(v')| <= E_v / (sqrt(v') + sqrt(max(v' - E_v, 0))) = e
                                                          E_s = e + u (sqrt(v') + e)
    denom      d^ = fl(s^ k^ + eps)         (one fma)     |s^ k^ - s K| <= E_s K (1 + u) + s u K = e
                                                          E_d = e + u (D + e),                   D = s K + eps
    quotient   q^ = fl(m^ / d^)                           |m^ / d^ - m' / D| <= (E_m + |q| E_d) / (D - E_d) = e,   q = m' / D
                                                          E_q = e + u (|q| + e)
    p          p^ = fl(p - l^ q^)           (one fma)     |l^ q^ - L q| <= E_L (|q| + E_q) + |L| E_q = e
                                                          E_p = e + u (|p'| + e)                 -- half an ulp of p', plus the update's error

(v' = 0 only where v = g = 0, and then E_v = 0: the square root is exact there.)  u is taken as 2^-24 (1 + 2^-20): the 2^-20
covers the rounding of this float64 evaluation itself.  The bars are multiplied by ``SAFETY``; how that factor was chosen from
the ratios observed on the GPU is recorded in BASELINE.md next to NOISE_K.
"""
import numpy as np

F32, F64 = np.float32, np.float64
U = 2.0 ** -24 * (1.0 + 2.0 ** -20)
SAFETY = 2.0   # observed on the GPU with 1.0: at most 1.000 of the derived bound; 2 puts that at half the bar


def _w(x):
    """the float32 value the kernel receives, widened"""
    return F64(F32(x))


def lr_table(n, segments):
    """Per-element learning rate [n] (float64 holding float32 values).  ``segments``: (begin, end, lr, lr_head, period, head)."""
    lr = np.zeros(n, F64)
    for begin, end, rate, rate_head, period, head in segments:
        lo, hi = max(int(begin), 0), min(int(end), n)
        if lo >= hi:
            continue
        idx = np.arange(lo, hi, dtype=np.int64)
        val = np.full(idx.shape, _w(rate))
        if period > 0:
            val[(idx - int(begin)) % int(period) < int(head)] = _w(rate_head)
        lr[lo:hi] = val
    return lr


def _exact(p, g, m, v, lr, b1, b2, eps, step):
    b1, b2, eps = _w(b1), _w(b2), _w(eps)
    step = np.asarray(step, F64)
    p, g, m, v = (np.asarray(x, F64) for x in (p, g, m, v))
    bc1, bc2 = 1.0 - np.power(b1, step), 1.0 - np.power(b2, step)
    m2 = b1 * m + (1.0 - b1) * g
    v2 = b2 * v + (1.0 - b2) * g * g
    K = 1.0 / np.sqrt(bc2)
    s = np.sqrt(v2)
    D = s * K + eps
    q = m2 / D
    L = lr / bc1
    return dict(p=p - L * q, m=m2, v=v2, s=s, K=K, D=D, q=q, L=L, b1=b1, b2=b2)


def step(p, g, m, v, segments, b1, b2, eps, step):
    """One Adam step in float64: returns (p', m', v').  The arrays are [..., n]; ``step`` is the 1-based step count, a scalar or an
    array that broadcasts against them (one row per step)."""
    n = np.asarray(p).shape[-1]
    x = _exact(p, g, m, v, lr_table(n, segments), b1, b2, eps, step)
    return x["p"], x["m"], x["v"]


def bounds(p, g, m, v, segments, b1, b2, eps, step):
    """Error bars (E_p, E_m, E_v) for the fp32 kernel's step from the fp32 state (p, m, v) with gradient g: see the module docstring."""
    n = np.asarray(p).shape[-1]
    x = _exact(p, g, m, v, lr_table(n, segments), b1, b2, eps, step)
    g = np.abs(np.asarray(g, F64))
    u = U
    c1 = F64(F32(1.0) - F32(b1))   # what the kernel multiplies g by, against the exact 1 - b1
    c2 = F64(F32(1.0) - F32(b2))
    a = np.abs((1.0 - x["b1"]) * g)
    E_a = u * a + abs(c1 - (1.0 - x["b1"])) * g * (1 + u)
    E_m = E_a + u * (np.abs(x["m"]) + E_a)
    t = np.abs((1.0 - x["b2"]) * g * g)
    E_t = (2 * u + u * u) * t + abs(c2 - (1.0 - x["b2"])) * g * g * (1 + u) ** 2
    E_v = E_t + u * (x["v"] + E_t)
    s, K, D, q, L = x["s"], x["K"], x["D"], np.abs(x["q"]), np.abs(x["L"])
    low = np.sqrt(np.maximum(x["v"] - E_v, 0.0))
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(E_v > 0, E_v / (s + low), 0.0)
    E_s = e + u * (s + e)
    e = E_s * K * (1 + u) + s * u * K
    E_d = e + u * (D + e)
    e = (E_m + q * E_d) / (D - E_d)
    E_q = e + u * (q + e)
    E_L = (2 * u + u * u) * L
    e = E_L * (q + E_q) + L * E_q
    E_p = e + u * (np.abs(x["p"]) + e)
    return SAFETY * E_p, SAFETY * E_m, SAFETY * E_v


def ratios(got, want, bars):
    """max |got - want| / bar per tensor; an element whose bar is 0 must be met exactly (ratio inf otherwise)."""
    out = []
    for a, b, e in zip(got, want, bars):
        err = np.abs(np.asarray(a, F64) - b)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(e > 0, err / e, np.where(err == 0, 0.0, np.inf))
        out.append(float(r.max()) if r.size else 0.0)
    return out
