"""CPU: the binding of include/fdgs_seed.h, the argument errors of its entry points, and the numpy restatements of tests/seed_oracle.py
themselves (Philox4x32-10 against the algorithm's published known-answer vectors)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import seed_cases
import seed_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Random123's kat_vectors for philox4x32 with 10 rounds: counter, key, result
KAT = [
    ((0x00000000,) * 4, (0x00000000,) * 2, (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def test_philox_known_answers():
    for counter, key, want in KAT:
        got = so.philox4x32_10(np.array([counter], np.uint32), np.array([key], np.uint32))[0]
        assert tuple(int(x) for x in got) == want
    w, u = so.draws(1000, 0x9E3779B97F4A7C15, 3)
    assert w.shape == (1000, 4) and u.dtype == np.float32 and u.min() >= 0.0 and u.max() < 1.0
    assert len(np.unique(w)) == 4000 and abs(float(u.mean()) - 0.5) < 0.02
    one = so.philox4x32_10(np.array([[7, 3, 0, 0]], np.uint32), np.array([[0x7F4A7C15, 0x9E3779B9]], np.uint32))[0]
    assert np.array_equal(one, w[7])                      # the counter and key layout draws() documents


def test_signature_table_matches_the_library_and_the_header():
    from fdgs import _capi, _seed_capi
    with open(os.path.join(ROOT, "include", "fdgs_seed.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(fdgs_[a-z_0-9]+)\s*\(", text)))
    assert declared == sorted(_seed_capi.EXPORTED) and len(declared) == 4
    for name, (restype, argtypes) in _seed_capi.SIGNATURES.items():
        fn = getattr(_capi.lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, text, flags=re.S)
        assert m and len([a for a in m.group(1).split(",") if a.strip()]) == len(argtypes), name
    assert _seed_capi.lib is _capi.lib and _seed_capi.call is _capi.call
    # the pinned table of include/fdgs.h did not grow
    assert len(_capi.EXPORTED) == 95 and not set(_capi.EXPORTED) & set(_seed_capi.EXPORTED)
    assert _capi.lib.fdgs_version() == _capi.FDGS_VERSION == 502
    with open(os.path.join(ROOT, "include", "fdgs_seed.h")) as f:
        head = f.read()
    assert int(re.search(r"#define FDGS_SEED_AXIS_CELLS (\d+)", head).group(1)) == _seed_capi.SEED_AXIS_CELLS == 1 << _seed_capi.SEED_AXIS_BITS
    with open(os.path.join(ROOT, "4d-gaussian-splatting_amd", "csrc", "build.sh")) as f:
        sh = f.read()
    assert re.search(r"for src in [^;]*\bseed\b[^;]*; do", sh) and '[seed]="-ffp-contract=off"' in sh


def test_scratch_size():
    from fdgs import _seed_capi
    lib = _seed_capi.lib
    a, b = lib.fdgs_seed_thin_scratch_bytes(1000), lib.fdgs_seed_thin_scratch_bytes(2_000_000)
    assert 0 < lib.fdgs_seed_thin_scratch_bytes(0) <= a < b and a % 256 == 0 and b % 256 == 0
    assert 24 * 2_000_000 <= b < 26 * 2_000_000           # six words per point, the sort's histograms, one count per workgroup


_N = None
_F4 = (C.c_float * 4)(0.0, 0.0, 0.0, 0.0)
_ONE4 = (C.c_float * 4)(1.0, 1.0, 1.0, 1.0)
_NAN4 = (C.c_float * 4)(0.0, float("nan"), 0.0, 0.0)
_F6 = (C.c_float * 6)()
_X = 256   # a non-NULL placeholder, never dereferenced on the host
_REJECTED = [
    ("fdgs_seed_thin", (-1, _N, _N, _N, _F4, _ONE4, 0, 0) + (_N,) * 9, "N=-1"),
    ("fdgs_seed_thin", (1 << 28, _N, _N, _N, _F4, _ONE4, 0, 0) + (_N,) * 9, "2^28"),
    ("fdgs_seed_thin", (4, _X, _N, _N, _F4, _ONE4, 0, -1) + (_N,) * 9, "capacity"),
    ("fdgs_seed_thin", (4, _X, _N, _N, _N, _ONE4, 0, 4) + (_N,) * 9, "must not be NULL"),
    ("fdgs_seed_thin", (4, _X, _N, _N, _F4, _F4, 1, 0) + (_N,) * 6 + (_X, _X, _N), "inv_cell[0]"),
    ("fdgs_seed_thin", (4, _X, _N, _N, _NAN4, _ONE4, 1, 0) + (_N,) * 6 + (_X, _X, _N), "origin[1]"),
    ("fdgs_seed_thin", (4, _N, _N, _N, _F4, _ONE4, 1, 0) + (_N,) * 6 + (_X, _X, _N), "xyz / scratch"),
    ("fdgs_seed_thin", (4, _X, _N, _N, _F4, _ONE4, 0, 4) + (_N,) * 6 + (_X, _X, _N), "an output is NULL"),
    ("fdgs_seed_random", (-1, 0, 0, 0, _F6, _N, _N, _N, _N), "N=-1"),
    ("fdgs_seed_random", (4, 0, 0, 3, _F6, _X, _N, _N, _N), "unknown shape 3"),
    ("fdgs_seed_random", (4, 0, 0, 0, _N, _X, _N, _N, _N), "params"),
    ("fdgs_seed_random", (4, 0, 0, 0, _F6, _N, _N, _N, _N), "out must not be NULL"),
    ("fdgs_seed_init", (-1, 16, 4, _N, _N, _N, _N, 0.0, 0.0, _N, _N), "bad sizes"),
    ("fdgs_seed_init", (4, 0, 4, _X, _X, _X, _X, 0.0, 0.0, _X, _N), "bad sizes"),
    ("fdgs_seed_init", (4, 16, 5, _X, _X, _X, _X, 0.0, 0.0, _X, _N), "gaussian_dim=5"),
    ("fdgs_seed_init", (40_000_000, 48, 4, _X, _X, _X, _X, 0.0, 0.0, _X, _N), "2^31"),
    ("fdgs_seed_init", (4, 16, 4, _X, _X, _N, _X, 0.0, 0.0, _X, _N), "t must not be NULL"),
    ("fdgs_seed_init", (4, 16, 3, _X, _N, _N, _X, 0.0, 0.0, _X, _N), "xyz / rgb / dist2 / flat"),
]


@pytest.mark.parametrize("row", range(len(_REJECTED)), ids=lambda i: "%s-%d" % (_REJECTED[i][0], i))
def test_argument_errors_carry_their_own_message(row):
    """Everything here is turned away before anything touches the GPU, through the library's one error path."""
    from fdgs import _capi, _seed_capi
    name, args, text = _REJECTED[row]
    assert getattr(_seed_capi.lib, name)(*args) == 1
    err = _capi.last_error()
    print(name, "->", err)
    assert err.startswith(name + ":") and text in err


def test_restatement_of_the_thinning_on_a_worked_example():
    """Two cells by hand: keys, order, first members and the sequential float32 means."""
    xyz = np.array([[0.9, 0.1, 0.1], [0.0, 0.0, 0.0], [1.0, 0.2, 0.3], [0.4, 0.4, 0.4], [0.1, 0.2, 0.3]], np.float32)
    rgb = np.arange(15, dtype=np.float32).reshape(5, 3) / 16
    origin, inv = so.grid_of(xyz, None, 0.5, None)
    r = so.thin(xyz, rgb, None, origin, inv)
    assert origin.tolist() == [0.0, 0.0, 0.0, 0.0] and inv[0] == 2.0
    assert r["key"].tolist() == [0, 1 << 48, 2 << 48]       # x cells 0, 1, 2 (a point ON the face x = 1.0 belongs to the cell above)
    assert r["count"].tolist() == [3, 1, 1] and r["first"].tolist() == [1, 0, 2]
    assert [m.tolist() for m in r["members"]] == [[1, 3, 4], [0], [2]]
    want = ((xyz[1] + xyz[3]) + xyz[4]) / np.float32(3)
    assert np.abs(r["xyz"][0] - want).max() <= 2.0 ** -24 and np.array_equal(r["xyz"][1], xyz[0])
    t = np.array([0.0, 0.0, 0.0, 1.0, 0.0], np.float32)
    r = so.thin(xyz, rgb, t, *so.grid_of(xyz, t, 0.5, 0.5))
    assert r["key"].tolist() == [0, 2, 1 << 48, 2 << 48] and r["count"].tolist() == [2, 1, 1, 1]


def test_every_thinning_case_meets_the_sequential_sum_bound_in_the_restatement():
    """The GPU test holds the kernel to these bits; here the restatement itself is held to the float64 mean on the same clouds."""
    for name, (xyz, rgb, t, cell, cell_t) in seed_cases.cases().items():
        r = so.thin(xyz, rgb, t, *so.grid_of(xyz, t, cell, cell_t))
        assert int(r["count"].sum()) == len(xyz)
        for k, idx in enumerate(r["members"]):
            for nm, col in (("xyz", xyz), ("rgb", rgb), ("t", t[:, None])):
                mean, bound = so.mean_bound(col, idx)
                assert (np.abs(np.atleast_1d(r[nm][k]).astype(np.float64) - mean) <= bound).all(), (name, nm, len(idx))


def test_init_restatement():
    d2 = np.array([0.0, 1e-9, 1e-7, 4.0, 1e6], np.float32)
    z = np.zeros((5, 3), np.float32)
    r = so.init_f32(z, z + np.float32(0.5), np.zeros(5, np.float32), d2, 4, 4, (0.0, 10.0))
    assert np.abs(r["_scaling"][:, 0].astype(np.float64) - so.scaling_f64(d2)).max() < 1e-6
    assert r["_scaling"][0, 0] == r["_scaling"][1, 0] == r["_scaling"][2, 0] and abs(r["_scaling"][3, 0] - np.log(2.0)) < 1e-7
    assert abs(float(r["_opacity"][0, 0]) - np.log(0.1 / 0.9)) < 1e-6 and abs(float(r["_scaling_t"][0, 0]) - np.log(np.sqrt(2.0))) < 1e-7
    assert not r["_features"].any() and r["_rotation"][:, 0].all() and not r["_rotation"][:, 1:].any()
    from fdgs.seed import init_constants
    assert tuple(np.float32(v) for v in init_constants((0.0, 10.0))) == tuple(so.init_constants((0.0, 10.0)))
