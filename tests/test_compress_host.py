"""CPU: the k-means oracle's monotonicity, the CompressedModel file format, the CPU-tensor errors of fdgs.compress and the host-side
argument checks of its five C entry points (nothing is launched here)."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import compress_oracle as co


def test_oracle_lloyd_iterations_never_increase_the_objective():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((400, 9)).astype(np.float32)
    for w in (None, rng.uniform(0.0, 2.0, 400) * (rng.uniform(size=400) > 0.2)):
        c = x[rng.permutation(400)[:17]].astype(np.float64)
        index, _ = co.assign(x, c)
        last = co.objective(x, c, index, w)
        for _ in range(6):
            c, counts, _ws = co.update(x, index, c, w)
            assert int(counts.sum()) == 400
            mid = co.objective(x, c, index, w)      # the means minimise the objective for a fixed assignment ...
            index, _ = co.assign(x, c)
            now = co.objective(x, c, index, w)      # ... and the nearest centroid for fixed means
            assert mid <= last * (1 + 1e-12) and now <= mid * (1 + 1e-12)
            last = now


def test_oracle_quantise_round_trip_and_ties():
    x = np.array([[0.0, 5.0], [1.0, 5.0], [0.5, 5.0], [0.25, 5.0]], np.float32)
    lo, hi = x.min(0), x.max(0)
    for bits in (8, 16):
        step, inv = co.ranges(lo, hi, bits)
        assert step[1] == 0 and inv[1] == 0            # a constant column
        q = co.quantize(x, lo, inv, bits)
        qmax = (1 << bits) - 1
        assert q[0, 0] == 0 and q[1, 0] == qmax and (q[:, 1] == 0).all()
        back = co.dequantize(q, lo, step)
        assert back[0, 0] == 0.0 and (back[:, 1] == 5.0).all()
        assert np.abs(back - x).max() <= 0.5 * step[0] * (1 + 1e-3)
    # duplicate codebook rows: the lowest index wins
    c = np.array([[0.0, 0.0], [1.0, 1.0], [0.0, 0.0], [1.0, 1.0]], np.float32)
    index, _ = co.assign(np.array([[0.1, 0.0], [0.9, 1.0]], np.float32), c)
    assert index.tolist() == [0, 1]


def _hand_built():
    from fdgs.compress import SEGMENTS, CompressedModel
    rng = np.random.default_rng(11)
    P, M, K = 37, 4, 5
    bits = {"_xyz": 32, "_t": 16, "_scaling": 16, "_scaling_t": 16, "_opacity": 8, "dc": 16, "_rotation": 8, "_rotation_r": 8}
    tensors, lo, step = {}, {}, {}
    for name, cols in SEGMENTS:
        b = bits[name]
        if b == 32:
            tensors[name] = torch.from_numpy(rng.standard_normal((P, cols)).astype(np.float32))
        else:
            tensors[name] = torch.from_numpy(rng.integers(0, 1 << b, (P, cols)).astype(np.uint8 if b == 8 else np.uint16))
            lo[name] = [float(np.float32(v)) for v in rng.standard_normal(cols)]
            step[name] = [float(np.float32(v)) for v in rng.uniform(1e-4, 1e-2, cols)]
    tensors["sh_codebook"] = torch.from_numpy(rng.standard_normal((K, 3 * (M - 1))).astype(np.float32))
    tensors["sh_index"] = torch.from_numpy(rng.integers(0, K, P).astype(np.uint16))
    meta = {"format": 1, "P": P, "M": M, "codebook_size": K, "max_sh_degree": 1, "max_sh_degree_t": 0, "active_sh_degree": 1,
            "active_sh_degree_t": 0, "time_duration": [0.0, 1.5], "gaussian_dim": 4, "rot_4d": True, "force_sh_3d": True,
            "prefilter_var": -1.0, "bits": bits, "lo": lo, "step": step}
    return CompressedModel(tensors, meta)


def test_save_load_round_trip_bit_for_bit(tmp_path):
    from fdgs import compress
    cm = _hand_built()
    path = str(tmp_path / "model.npz")
    compress.save(path, cm)
    back = compress.load(path)
    assert back.meta == cm.meta and json.dumps(back.meta, sort_keys=True) == json.dumps(cm.meta, sort_keys=True)
    assert set(back.tensors) == set(cm.tensors)
    for k, t in cm.tensors.items():
        b = back.tensors[k]
        assert b.dtype == t.dtype and tuple(b.shape) == tuple(t.shape), k
        assert t.numpy().tobytes() == b.numpy().tobytes(), k
    with np.load(path) as z:
        payload = sum(z[k].nbytes for k in z.files)
    assert compress.nbytes(cm) == payload == compress.nbytes(back)
    # 37 B of columns + a 2-byte index per Gaussian, the codebook, the metadata text
    P = cm.meta["P"]
    assert payload == P * (12 + 2 + 6 + 2 + 1 + 6 + 4 + 4 + 2) + 5 * 9 * 4 + len(json.dumps(cm.meta, sort_keys=True).encode())
    # the oracle decodes a hand-built model into a bucket of the right size, the float32 segment bit for bit
    flat = co.decode_model({k: t.numpy() for k, t in back.tensors.items()}, back.meta)
    assert flat.dtype == np.float32 and flat.size == P * (17 + 3 * cm.meta["M"])
    assert flat[:3 * P].tobytes() == cm.tensors["_xyz"].numpy().tobytes()


def test_cpu_tensors_raise():
    from fdgs import compress, synth
    from fdgs.train_host import GaussianParams
    x, c = torch.zeros(8, 3), torch.zeros(2, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        compress.kmeans(x, 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        compress.assign(x, c)
    with pytest.raises(RuntimeError, match="no CPU path"):
        compress.update(x, torch.zeros(8, dtype=torch.int32), c)
    with pytest.raises(RuntimeError, match="no CPU path"):
        compress.quantize_columns(x, [0, 0, 0], [1, 1, 1], 8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        compress.decode_into(torch.zeros(24), 8, 3, 32, x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        compress.decompress(_hand_built(), "cpu")
    scene = synth.make_scene(synth.SceneConfig("cpu", 16, 32, 32, 1, 0, 0.03, 1.0, True, 4, True), seed=1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        compress.compress(GaussianParams(scene, "cpu"))


def test_bad_arguments_are_rejected_on_the_host():
    """FDGS_ERR_INVALID_ARG (1) with a message, before any HIP call: the pointers below are never dereferenced."""
    from fdgs import _capi
    lib = _capi.lib
    p = C.c_void_p(0x1000)   # a non-NULL value that must never be read
    assert {"fdgs_kmeans_assign", "fdgs_kmeans_update", "fdgs_kmeans_scratch_bytes", "fdgs_quantize_columns", "fdgs_compact_decode"} <= set(_capi.EXPORTED)
    for N, K, D, word in ((10, 0, 4, "K"), (10, 4, 193, "D"), (10, 65537, 4, "K"), (10, 4, 0, "D"), (0, 4, 4, "N")):
        assert lib.fdgs_kmeans_assign(N, K, D, p, p, p, None, p, None) == 1
        assert "fdgs_kmeans_assign" in _capi.last_error() and word + " must" in _capi.last_error()
        assert lib.fdgs_kmeans_update(N, K, D, p, p, None, p, None, p, None) == 1
        assert "fdgs_kmeans_update" in _capi.last_error() and word + " must" in _capi.last_error()
    for args in ((None, p, p, None, p), (p, None, p, None, p), (p, p, None, None, p), (p, p, p, None, None)):
        assert lib.fdgs_kmeans_assign(10, 4, 4, *args, None) == 1 and "NULL" in _capi.last_error()
    for args in ((None, p, None, p, None, p), (p, None, None, p, None, p), (p, p, None, None, None, p), (p, p, None, p, None, None)):
        assert lib.fdgs_kmeans_update(10, 4, 4, *args, None) == 1 and "NULL" in _capi.last_error()
    assert lib.fdgs_quantize_columns(10, 3, p, p, p, 1000, p, None) == 1 and "qmax" in _capi.last_error()
    assert lib.fdgs_quantize_columns(10, 0, p, p, p, 255, p, None) == 1
    for args in ((None, p, p, 255, p), (p, None, p, 255, p), (p, p, None, 65535, p), (p, p, p, 255, None)):
        assert lib.fdgs_quantize_columns(10, 3, *args, None) == 1 and "NULL" in _capi.last_error()
    assert lib.fdgs_compact_decode(10, 3, 12, p, p, p, 0, None, None, 0, p, None) == 1 and "bits" in _capi.last_error()
    assert lib.fdgs_compact_decode(10, 0, 8, None, None, None, 0, None, None, 0, p, None) == 1
    assert lib.fdgs_compact_decode(10, 3, 8, p, p, p, 9, p, p, 0, p, None) == 1 and "K >= 1" in _capi.last_error()
    for args in ((None, p, p, 0, None, None, 0, p), (p, None, p, 0, None, None, 0, p), (p, p, None, 0, None, None, 0, p),
                 (p, p, p, 0, None, None, 0, None), (p, p, p, 9, None, None, 0, p)):
        assert lib.fdgs_compact_decode(10, 3, 8, *args, None) == 1 and "NULL" in _capi.last_error()
    # scratch sizes: room for the norms, two key and two value buffers, the histograms and the segment table
    s1, s2 = lib.fdgs_kmeans_scratch_bytes(1000, 16), lib.fdgs_kmeans_scratch_bytes(300000, 4096)
    assert 0 < s1 < s2 and s1 % 256 == 0 and s2 >= 16 * 300000 + 12 * 4096


def test_python_argument_errors():
    from fdgs import compress
    assert compress.DEFAULT_BITS == {"_xyz": 32, "_t": 16, "_scaling": 16, "_scaling_t": 16, "_opacity": 8, "dc": 16, "_rotation": 8,
                                     "_rotation_r": 8}
    step, inv = compress.column_ranges(np.array([0.0, 2.0], np.float32), np.array([1.0, 2.0], np.float32), 8)
    assert step.dtype == inv.dtype == np.float32
    assert step[0] == np.float32(1.0) / np.float32(255) and inv[0] == np.float32(255) and step[1] == 0 and inv[1] == 0
    s2, i2 = co.ranges(np.array([0.0, 2.0], np.float32), np.array([1.0, 2.0], np.float32), 8)
    assert step.tobytes() == s2.tobytes() and inv.tobytes() == i2.tobytes()
