"""The float64 Adam statement the GPU tests hold csrc/adam.hip to (tests/adam_oracle.py) against torch.optim.Adam on float64 CPU
tensors, and the properties of its error bars that need no GPU."""
import numpy as np
import torch

import adam_oracle as ao

B1, B2, EPS = 0.9, 0.999, 1e-15
# (begin, end, lr, lr_head, period, head): DC heads with periods 1, 2, 3 and 21, a negative begin, a gap [300, 310), an overlap
# [395, 420) (the later segment wins), an end beyond n
N = 613
TABLE = [(-40, 50, 1.6e-4, 2.5e-3, 21, 3), (50, 51, 5e-2, 5e-2, 0, 0), (51, 120, 5e-3, 1e-3, 1, 1), (120, 211, 1.25e-4, 2.5e-3, 2, 1),
         (211, 300, 1e-3, 7e-3, 3, 2), (310, 420, 3e-4, 9e-3, 21, 3), (395, 500, 2e-3, 2e-3, 0, 0), (500, N + 9, 1.25e-4, 2.5e-3, 21, 3)]


def _lr_by_hand(n, table):
    """seg_lr of adam.hip, one element at a time"""
    lr = np.zeros(n)
    for i in range(n):
        for b, e, rate, rate_head, period, head in table:
            if b <= i < e:
                lr[i] = np.float32(rate)
                if period > 0 and (i - b) % period < head:
                    lr[i] = np.float32(rate_head)
    return lr


def test_lr_table_matches_the_per_element_search():
    lr = ao.lr_table(N, TABLE)
    np.testing.assert_array_equal(lr, _lr_by_hand(N, TABLE))
    assert (lr[300:310] == 0).all() and lr[0] == np.float32(1.6e-4) and lr[2] == np.float32(2.5e-3)   # phase of element 0: 40 mod 21 = 19
    assert (lr[395:420] == np.float32(2e-3)).all() and lr[N - 1] in (np.float32(1.25e-4), np.float32(2.5e-3))


def test_oracle_step_is_torch_adam_in_float64():
    """Six steps, one torch parameter group per distinct rate: parameters and both moments to 1e-12 relative.  (exp_avg is a sum of
    two terms of either sign -- torch forms it as a lerp -- so its 1e-12 is relative to the terms, not to what is left of them.)"""
    rng = np.random.default_rng(0)
    lr = _lr_by_hand(N, TABLE)
    f = lambda x: float(np.float32(x))   # noqa: E731
    p0 = rng.standard_normal(N).astype(np.float32).astype(np.float64)
    groups, views = [], []
    for val in sorted(set(lr.tolist())):
        idx = np.nonzero(lr == val)[0]
        q = torch.from_numpy(p0[idx]).clone().requires_grad_(True)
        groups.append({"params": [q], "lr": val})
        views.append((idx, q))
    assert len(groups) >= 10 and any(grp["lr"] == 0.0 for grp in groups)
    opt = torch.optim.Adam(groups, lr=0.0, betas=(f(B1), f(B2)), eps=f(EPS))
    p, m, v = p0.copy(), np.zeros(N), np.zeros(N)
    for t in range(1, 7):
        g = (rng.standard_normal(N) * 10.0 ** rng.integers(-6, 1, N)).astype(np.float32).astype(np.float64)
        g[::7] = 0.0
        m_prev = m
        p, m, v = ao.step(p, g, m, v, TABLE, B1, B2, EPS, t)
        for idx, q in views:
            q.grad = torch.from_numpy(g[idx]).clone()
        opt.step()
        tp, tm, tv = np.empty(N), np.empty(N), np.empty(N)
        for idx, q in views:
            st = opt.state[q]
            tp[idx], tm[idx], tv[idx] = q.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()
        np.testing.assert_allclose(p, tp, rtol=1e-12, atol=0)
        np.testing.assert_allclose(v, tv, rtol=1e-12, atol=0)
        terms = np.abs(f(B1) * m_prev) + np.abs((1 - f(B1)) * g)
        assert (np.abs(m - tm) <= 1e-12 * terms).all()
    fed = np.ones(N, bool)
    fed[::7] = False
    assert np.abs(p - p0)[(lr > 0) & fed].min() > 0 and (p == p0)[(lr == 0) | ~fed].all()


def test_step_broadcasts_over_a_history_of_steps():
    rng = np.random.default_rng(1)
    T, n = 5, 9
    p, g, m, v = (rng.standard_normal((T, n)) for _ in range(4))
    v = v * v
    steps = np.arange(1, T + 1)[:, None]
    rows = ao.step(p, g, m, v, TABLE, B1, B2, EPS, steps)
    for t in range(T):
        one = ao.step(p[t], g[t], m[t], v[t], TABLE, B1, B2, EPS, t + 1)
        for a, b in zip(rows, one):
            np.testing.assert_array_equal(a[t], b)


def test_bounds_hold_for_a_float32_evaluation_in_numpy():
    """adam_update restated operation by operation in numpy float32 (fma = one rounding of the float64 product and sum: exact
    enough here, a float32 product has 48 bits) stays inside the bars, a step with one term off by 1e-6 relative does not, and
    the bars of an untouched element (m = v = g = 0) are zero for the moments and half an ulp for p."""
    rng = np.random.default_rng(2)
    n, t = 4001, 3
    f32 = np.float32
    g = (10.0 ** rng.uniform(-15, 0, n) * rng.choice([-1.0, 1.0], n)).astype(f32)
    m = (10.0 ** rng.uniform(-16, -2, n) * rng.choice([-1.0, 1.0], n)).astype(f32)
    v = (10.0 ** rng.uniform(-30, -4, n)).astype(f32)
    p = rng.standard_normal(n).astype(f32)
    g[::5] = 0
    m[::3] = 0
    v[::4] = 0
    seg = [(0, n, 1e-3, 5e-2, 21, 3)]
    lr = ao.lr_table(n, seg)
    b1, b2, eps = f32(B1), f32(B2), f32(EPS)
    fma = lambda a, b, c: (a.astype(np.float64) * np.float64(b) + c).astype(f32)   # noqa: E731
    ib, k = f32(1.0 / (1.0 - float(b1) ** t)), f32(1.0 / np.sqrt(1.0 - float(b2) ** t))
    m2 = fma(m, b1, ((f32(1) - b1) * g).astype(np.float64))
    v2 = fma(v, b2, (((f32(1) - b2) * g) * g).astype(np.float64))
    d = fma(np.sqrt(v2), k, np.float64(eps))
    p2 = fma(-(lr.astype(f32) * ib), (m2 / d), p.astype(np.float64))
    want = ao.step(p, g, m, v, seg, B1, B2, EPS, t)
    bars = ao.bounds(p, g, m, v, seg, B1, B2, EPS, t)
    r = ao.ratios((p2, m2, v2), want, bars)
    assert max(r) <= 1.0, r
    assert min(r) > 0.2, r     # ... and the bars are not slack by orders of magnitude
    for i, wrong in enumerate((p + (p2 - p) * f32(1 + 1e-5), m2 * f32(1 + 1e-6), v2 * f32(1 + 1e-6))):
        got = [p2, m2, v2]
        got[i] = wrong
        assert ao.ratios(got, want, bars)[i] > 2.0
    z = np.zeros(3, f32)
    ep, em, ev = ao.bounds(np.ones(3, f32), z, z, z, seg, B1, B2, EPS, 1)
    assert (em == 0).all() and (ev == 0).all() and (ep <= 2.0 ** -24 * 1.001 * ao.SAFETY).all()
