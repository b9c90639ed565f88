"""CPU: the float64 yardstick of the MCMC densification (tests/mcmc_oracle.py) against exact arithmetic, the integer sampler's edges,
and the companion header's symbols."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import mcmc_oracle as mo
from fdgs import mcmc      # the yardstick below is this module's: without it there is nothing to hold to it

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPACITIES = (0.005, 0.01, 0.1, 0.5, 0.9, 0.99, 1.0 - 2.0 ** -23)
COPIES = (1, 2, 3, 10, 51)


@pytest.mark.parametrize("N", COPIES)
@pytest.mark.parametrize("o", OPACITIES)
def test_oracle_D_against_exact_rational_arithmetic(o, N):
    """The float64 double sum of the definition within 1e-9 relative of the same sum over exact rationals (50-digit roots): the
    alternating binomial sum loses at most that, so the float64 oracle may judge the kernel at 1e-6."""
    op, D, ratio = mo.new_opacity_and_ratio(o, N)
    op_exact, D_exact = mo.exact_D(o, N)
    err_op = abs(Fraction(op) - op_exact) / op_exact
    err_D = abs(Fraction(D) - D_exact) / D_exact
    print("o=%.9g N=%d  o'=%.17g D=%.17g  rel err o' %.2e D %.2e" % (o, N, op, D, float(err_op), float(err_D)))
    assert D_exact > 0 and float(err_op) <= 1e-9 and float(err_D) <= 1e-9
    assert abs(Fraction(ratio) - Fraction(o) / D_exact) / (Fraction(o) / D_exact) <= Fraction(1, 10 ** 9)


@pytest.mark.parametrize("o", OPACITIES)
def test_one_copy_changes_nothing(o):
    op, D, ratio = mo.new_opacity_and_ratio(o, 1)
    assert op == o and D == o and ratio == 1.0
    assert (mo.STREAM_RELOCATE, mo.STREAM_GROW, mo.STREAM_NOISE) == (mcmc.STREAM_RELOCATE, mcmc.STREAM_GROW, mcmc.STREAM_NOISE)
    assert mo.multiplicity(0) == 1 and mo.multiplicity(1) == 2 and mo.multiplicity(50) == 51 and mo.multiplicity(1000) == 51


def test_sampler_never_selects_a_zero_weight_row():
    rng = np.random.default_rng(3)
    for P in (1, 2, 7, 64, 300):
        w = rng.integers(1, 1 << 24, P).astype(np.uint64)
        w[rng.random(P) < 0.6] = 0
        if not w.any():
            w[P // 2] = 5
        prefix = mo.prefix_of(w)
        total = int(prefix[-1])
        # every boundary of every live row's interval, and the u of real draws
        us = {0, total - 1}
        for i in np.flatnonzero(w):
            us |= {int(prefix[i]) - 1, int(prefix[i]) - int(w[i])}
        for u in sorted(us):
            i = mo.select(prefix, u)
            assert w[i] > 0 and int(prefix[i]) - int(w[i]) <= u < int(prefix[i])
        source, counts, _ = mo.draw(prefix, 200, seed=9, stream_id=1, call=2 ** 33 + 5)
        assert (w[source] > 0).all() and counts.sum() == 200 and (counts[w == 0] == 0).all()


def test_sampler_selects_the_first_and_the_last_live_row_at_the_ends():
    w = np.array([0, 0, 3, 0, 1 << 24, 0, 1, 0, 0], np.uint64)
    prefix = mo.prefix_of(w)
    total = int(prefix[-1])
    assert mo.select(prefix, 0) == 2 and mo.select(prefix, 2) == 2 and mo.select(prefix, 3) == 4
    assert mo.select(prefix, total - 1) == 6 and mo.select(prefix, total - 2) == 4
    # u = (r64 * total) >> 64 spans exactly [0, total)
    assert (0 * total) >> 64 == 0 and ((2 ** 64 - 1) * total) >> 64 == total - 1


def test_weights_are_opacity_in_units_of_2_to_the_minus_24():
    raw = np.float32([-20.0, -5.3, -5.2, 0.0, 5.0, 30.0])
    w = mo.weights_f64(raw, 0.005)
    assert w[0] == 0 and w[1] == 0 and w[2] > 0 and w[3] == 1 << 23 and w[5] == 1 << 24
    assert mo.prefix_of(w)[-1] == w.sum()


def _declared_symbols():
    with open(os.path.join(ROOT, "include", "fdgs_mcmc.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return sorted(set(re.findall(r"\b(fdgs_[a-z_0-9]+)\s*\(", text)))


def test_library_exports_every_symbol_of_the_mcmc_header():
    from fdgs import _capi, _mcmc_capi
    names = _declared_symbols()
    assert len(names) == 9 and all(n.startswith("fdgs_mcmc_") for n in names)
    assert sorted(_mcmc_capi.EXPORTED) == names
    for n in names:
        assert hasattr(_capi.lib, n), "libfdgs.so does not export %s" % n
        restype, argtypes = _mcmc_capi.SIGNATURES[n]
        fn = getattr(_mcmc_capi.lib, n)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), n
    assert not set(names) & set(_capi.EXPORTED) and _mcmc_capi.lib is _capi.lib and _mcmc_capi.call is _capi.call
    assert _mcmc_capi.MCMC_MAX_MULTIPLICITY == mo.MAX_N and 1 << _mcmc_capi.MCMC_WEIGHT_BITS == mo.WEIGHT_ONE


_N = None
_REJECTED = [
    ("fdgs_mcmc_weights", (0, _N, 0.005, _N, _N, _N, _N, _N), "fdgs_mcmc_weights: P=0"),
    ("fdgs_mcmc_weights", (8, _N, 0.005, _N, _N, _N, _N, _N), "fdgs_mcmc_weights: opacity_raw"),
    ("fdgs_mcmc_draw", (8, -1, _N, 0, 0, 0, _N, _N, _N, _N), "fdgs_mcmc_draw: P=8"),
    ("fdgs_mcmc_draw", (8, 4, _N, 0, 0, 0, _N, _N, _N, _N), "fdgs_mcmc_draw: prefix"),
    ("fdgs_mcmc_copy_rows", (0, _N, 8, 1, _N, _N, _N, _N), "fdgs_mcmc_copy_rows: num_segments=0"),
    ("fdgs_mcmc_zero_rows", (17, _N, 8, 1, _N, _N, _N, _N), "fdgs_mcmc_zero_rows: num_segments=17"),
    ("fdgs_mcmc_update", (4, 5, _N, _N, _N, _N, _N, _N, _N), "fdgs_mcmc_update: gaussian_dim=5"),
    ("fdgs_mcmc_update", (4, 3, _N, _N, _N, _N, _N, _N, _N), "fdgs_mcmc_update: rows"),
    ("fdgs_mcmc_noise", (4, 3, 1) + (_N,) * 7 + (1.0, _N, 0, 0, 0, _N, _N, _N), "fdgs_mcmc_noise: rot_4d needs gaussian_dim == 4"),
    ("fdgs_mcmc_noise", (4, 4, 1) + (_N,) * 7 + (1.0, _N, 0, 0, 0, _N, _N, _N), "fdgs_mcmc_noise: xyz"),
    ("fdgs_mcmc_regularize", (0,) + (_N,) * 3 + (0.01, 0.01, 0.0) + (_N,) * 6, "fdgs_mcmc_regularize: P=0"),
    ("fdgs_mcmc_regularize", (8,) + (_N,) * 3 + (0.01, 0.01, 0.0) + (_N,) * 6, "fdgs_mcmc_regularize: opacity_raw"),
]


@pytest.mark.parametrize("row", range(len(_REJECTED)), ids=lambda i: "%s-%d" % (_REJECTED[i][0], i))
def test_mcmc_entry_points_reject_bad_arguments_before_any_launch(row):
    from fdgs import _capi, _mcmc_capi
    name, args, text = _REJECTED[row]
    assert getattr(_mcmc_capi.lib, name)(*args) == 1
    assert text in _capi.last_error(), _capi.last_error()


def test_row_functions_check_their_segment_table():
    from fdgs import _capi, _mcmc_capi
    rows = _mcmc_capi.host_ints([3, 0, 4])
    assert _mcmc_capi.lib.fdgs_mcmc_copy_rows(3, rows, 8, 0, None, None, None, None) == 1 and "row_floats[1]=0" in _capi.last_error()
    good = _mcmc_capi.host_ints([3, 1, 4])
    assert _mcmc_capi.lib.fdgs_mcmc_copy_rows(3, good, 8, 0, None, None, None, None) == 0      # n == 0: nothing to do, nothing launched
    assert _mcmc_capi.lib.fdgs_mcmc_zero_rows(3, good, 8, 2, None, None, None, None) == 1 and "NULL" in _capi.last_error()
    assert _mcmc_capi.lib.fdgs_mcmc_weights_scratch_bytes(1) == 256 and _mcmc_capi.lib.fdgs_mcmc_weights_scratch_bytes(257 * 256) % 256 == 0
    assert _mcmc_capi.lib.fdgs_mcmc_regularize_num_partials(256) == 3 and _mcmc_capi.lib.fdgs_mcmc_regularize_num_partials(257) == 6


def test_strategy_counts_calls_and_resumes(monkeypatch):
    """The call counter moves once per kernel call that draws, and a state dict carries seed and counter (no GPU: the functions
    underneath are stubbed)."""
    seen = []
    monkeypatch.setattr(mcmc, "relocate", lambda m, o, seed, call, mn: seen.append(("relocate", seed, call)) or
                        {"dead": 1, "relocated": 1, "sources": 1, "drew": True})
    monkeypatch.setattr(mcmc, "grow", lambda m, o, cap, seed, call, mn: seen.append(("grow", seed, call)) or
                        {"P_old": 10, "P_new": 10, "added": 0, "sources": 0, "drew": False})
    monkeypatch.setattr(mcmc, "noise_step", lambda m, lr, nlr, seed, call, xi=None: seen.append(("noise", seed, call, lr * nlr)))
    s = mcmc.MCMCStrategy(object(), None, cap=10, seed=77)
    s.refine()
    s.after_step(1e-4)
    s.after_step(1e-4, xi=object())     # injected normals: nothing drawn
    s.after_step(1e-4)
    assert seen == [("relocate", 77, 0), ("grow", 77, 1), ("noise", 77, 1, 50.0), ("noise", 77, 2, 50.0), ("noise", 77, 2, 50.0)]
    assert s.state_dict() == {"seed": 77, "call": 3}
    t = mcmc.MCMCStrategy(object(), None, cap=10)
    t.load_state_dict(s.state_dict())
    assert (t.seed, t.call) == (77, 3)
    assert mcmc.grown_size(1000, 5000) == 1050 and mcmc.grown_size(1000, 1020) == 1020 and mcmc.grown_size(1000, 1000) == 1000
    assert mcmc.grown_size(1000, 900) == 1000 and mcmc.grown_size(19, 100) == 19 and mcmc.grown_size(20, 100) == 21
    with pytest.raises(ValueError):
        mcmc.MCMCStrategy(object(), None, cap=0)
