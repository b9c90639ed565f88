"""GPU: fdgs.compress (csrc/compress.hip) against the numpy restatement tests/compress_oracle.py -- the MFMA assignment exactly where
the data decides it and at a per-row error bar where it does not, the reproducible update at a per-component bar, Lloyd iterations that
do not lose ground, quantise / decode bit for bit, and whole models through compress / decompress / the file."""
import functools

import numpy as np
import pytest
import torch

import compress_oracle as co

pytestmark = pytest.mark.gpu

U = co.U
DEV = "cuda:0"

# (N, D, K), a thinned cross product of D in {1, 9, 45, 141, 192}, K in {1, 2, 31, 257, 4096}, N in {1, 63, 257, 3001}: every value of
# each, N < K, K below / at / across the 64-column tile and the 32-column half of it, every D bucket of the kernel (16, 48, 96, 144, 192).
# D = 1 goes with K <= 2 only: N(0,1) centroids on a line are not separated beyond that.
CASES = [(1, 1, 1), (63, 1, 2), (3001, 9, 1), (257, 9, 31), (63, 9, 257), (3001, 45, 257), (257, 45, 4096), (63, 141, 31), (257, 141, 2),
         (3001, 192, 257), (1, 192, 4096), (257, 192, 1), (3001, 141, 4096)]
EVEN_K = [c for c in CASES if c[2] % 2 == 0]
# rows and centroids on a line: where near-ties do occur (only the general test takes them)
GENERAL_CASES = CASES + [(3001, 1, 257), (3001, 1, 4096)]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def gpu(a):
    return torch.from_numpy(np.array(a)).to(DEV)   # (a copy: the cached cases are read-only)


@functools.lru_cache(maxsize=None)
def data(N, D, K, kind):
    """(x, c, oracle index, oracle distances) of one case, computed once.  separated: rows = a centroid + 1e-3 N(0,1); duplicate: the
    same with every centroid stored twice (k and k + K/2); general: rows N(0,1)."""
    rng = np.random.default_rng(1000 * N + 10 * D + K + {"separated": 1, "duplicate": 2, "general": 3}[kind])
    if kind == "duplicate":
        half = rng.standard_normal((K // 2, D)).astype(np.float32)
        c = np.concatenate([half, half])
    else:
        c = rng.standard_normal((K, D)).astype(np.float32)
    if kind == "general":
        x = rng.standard_normal((N, D)).astype(np.float32)
    else:
        x = (c[rng.integers(0, K, N)] + np.float32(1e-3) * rng.standard_normal((N, D)).astype(np.float32)).astype(np.float32)
    index, d = co.assign(x, c)
    for a in (x, c, index, d):
        a.setflags(write=False)
    return x, c, index, d


def gpu_assign(x, c, want_dist=False):
    from fdgs import compress
    index, dist = compress.assign(gpu(x), gpu(c), want_dist=want_dist)
    torch.cuda.synchronize()
    return index.cpu().numpy(), None if dist is None else dist.cpu().numpy()


@pytest.mark.parametrize("N,D,K", CASES)
def test_assign_well_separated_equals_the_oracle(N, D, K):
    x, c, ref, d = data(N, D, K, "separated")
    index, dist = gpu_assign(x, c, want_dist=True)
    assert index.dtype == np.int32 and index.shape == (N,)
    assert np.array_equal(index, ref), "rows %s differ" % np.nonzero(index != ref)[0][:8]
    # the optional output: the winner's squared distance, a D-term float32 sum
    win = d[np.arange(N), ref]
    assert np.all(np.abs(dist - win) <= 4 * (D + 4) * U * np.maximum(win, 1e-30) + 1e-12)


@pytest.mark.parametrize("N,D,K", EVEN_K)
def test_assign_duplicate_rows_go_to_the_lower_copy(N, D, K):
    x, c, ref, _d = data(N, D, K, "duplicate")
    index, _ = gpu_assign(x, c)
    assert int(index.max()) < K // 2 and int(index.min()) >= 0
    assert np.array_equal(index, ref)
    # ... and with rows that sit near no centroid
    xg = data(N, D, K, "general")[0]
    index, _ = gpu_assign(xg, c)
    assert int(index.max()) < K // 2 and int(index.min()) >= 0


@pytest.mark.parametrize("N,D,K", GENERAL_CASES)
def test_assign_general_is_within_the_rounding_bar_of_the_minimum(N, D, K):
    x, c, _ref, d = data(N, D, K, "general")
    index, _ = gpu_assign(x, c)
    assert int(index.min()) >= 0 and int(index.max()) < K
    excess = d[np.arange(N), index] - d.min(axis=1)
    bar = co.assign_bar(x, c)
    worst = int(np.argmax(excess - bar))
    print("assign (%d, %d, %d): largest excess %.3e at a bar of %.3e; %d rows differ from the float64 argmin" % (
        N, D, K, excess[worst], bar[worst], int((index != _ref).sum())))
    assert np.all(excess <= bar), "row %d: %.3e above the minimum, bar %.3e" % (worst, excess[worst], bar[worst])


UPDATE_CASES = [(1, 1, 1), (63, 9, 257), (257, 45, 31), (3001, 141, 257), (3001, 192, 1), (3001, 9, 4096)]


@pytest.mark.parametrize("weighted", (False, True))
@pytest.mark.parametrize("N,D,K", UPDATE_CASES)
def test_update_matches_float64_and_is_reproducible(N, D, K, weighted):
    from fdgs import compress
    rng = np.random.default_rng(7 * N + D + K + int(weighted))
    x = rng.standard_normal((N, D)).astype(np.float32)
    old = rng.standard_normal((K, D)).astype(np.float32)
    index = rng.integers(0, K, N).astype(np.int32)
    if K > 2:
        index[index == 1] = 0          # an empty cluster even where N >> K
    w = None
    if weighted:
        w = rng.uniform(0.0, 3.0, N).astype(np.float32)
        w[rng.uniform(size=N) < 0.2] = 0.0
        w[index == K - 1] = 0.0        # a cluster whose rows weigh nothing
    ref, counts_ref, wsum = co.update(x, index, old, w)
    xd, idx_d, wd = gpu(x), gpu(index), None if w is None else gpu(w)
    runs = []
    for _ in range(2):
        c = gpu(old)
        counts = compress.update(xd, idx_d, c, weights=wd)
        torch.cuda.synchronize()
        runs.append((c.cpu().numpy(), counts.cpu().numpy()))
    (c1, n1), (c2, n2) = runs
    assert np.array_equal(bits(c1), bits(c2)) and np.array_equal(n1, n2)
    assert np.array_equal(n1, counts_ref)
    kept = wsum <= 0
    assert kept.any() or K == 1
    assert np.array_equal(bits(c1[kept]), bits(old[kept]))
    colmax = np.zeros((K, D))
    np.maximum.at(colmax, index, np.abs(x.astype(np.float64)))
    bar = 2.0 * (counts_ref[:, None] + 4) * U * colmax
    live = ~kept
    err = np.abs(c1.astype(np.float64) - ref)
    assert np.all(err[live] <= bar[live]), "largest error / bar: %.3f" % float((err[live] / np.maximum(bar[live], 1e-300)).max())


def test_kmeans_does_not_lose_ground_and_is_deterministic():
    from fdgs import compress
    N, D, K = 3001, 45, 257
    rng = np.random.default_rng(21)
    centres = rng.standard_normal((40, D)).astype(np.float32)
    x = (centres[rng.integers(0, 40, N)] + np.float32(0.3) * rng.standard_normal((N, D)).astype(np.float32)).astype(np.float32)
    w = rng.uniform(0.0, 2.0, N).astype(np.float32)
    w[::7] = 0.0
    init = x[rng.permutation(N)[:K]].copy()
    xd = gpu(x)
    for weights in (None, w):
        wd = None if weights is None else gpu(weights)
        c0, i0 = compress.kmeans(xd, K, iters=0, weights=wd, init=gpu(init))
        assert np.array_equal(bits(c0.cpu().numpy()), bits(init))            # iters = 0 returns init unchanged
        pairs = [(c0.cpu().numpy(), i0.cpu().numpy())]
        for t in range(1, 6):
            c, i = compress.kmeans(xd, K, iters=t, weights=wd, init=gpu(init))
            pairs.append((c.cpu().numpy(), i.cpu().numpy()))
        objs = [co.objective(x, c, i, weights) for c, i in pairs]
        print("objective over iterations:", ["%.6e" % o for o in objs])
        for t in range(5):
            bar = co.assign_bar(x, pairs[t + 1][0])
            slack = float(bar.sum() if weights is None else (bar * weights.astype(np.float64)).sum())
            assert objs[t + 1] <= objs[t] + slack, (t, objs[t], objs[t + 1], slack)
        assert objs[5] < 0.9 * objs[0]    # (it does make progress on clustered data)
    # seeded initialisation: two calls agree bit for bit; N < K cycles the rows
    a = compress.kmeans(xd, K, iters=3, seed=5)
    b = compress.kmeans(xd, K, iters=3, seed=5)
    assert np.array_equal(bits(a[0].cpu().numpy()), bits(b[0].cpu().numpy())) and torch.equal(a[1], b[1])
    other = compress.kmeans(xd, K, iters=3, seed=6)
    assert not torch.equal(a[0], other[0])
    small, idx = compress.kmeans(xd[:5], 12, iters=0, seed=1)
    assert tuple(small.shape) == (12, D) and torch.equal(small[:5], small[5:10]) and int(idx.max()) < 5


@pytest.mark.parametrize("nbits", (8, 16))
@pytest.mark.parametrize("P", (1, 63, 1025))
@pytest.mark.parametrize("C", (1, 3, 4))
def test_quantise_and_decode_bit_for_bit(C, P, nbits):
    from fdgs import compress
    rng = np.random.default_rng(100 * C + P + nbits)
    x = (rng.standard_normal((P, C)) * [3.0, 0.01, 50.0, 1.0][:C] + [0.5, -2.0, 100.0, 0.0][:C]).astype(np.float32)
    constant = C > 1 or P == 63                          # a constant last column (hi == lo); with C == 1 it is the only one
    if constant:
        x[:, C - 1] = np.float32(-1.25)
    lo, hi = x.min(0), x.max(0)                          # the ends are values of the data: they must come back as 0 and qmax
    step, inv = co.ranges(lo, hi, nbits)
    qmax = (1 << nbits) - 1
    q_ref = co.quantize(x, lo, inv, nbits)
    back_ref = co.dequantize(q_ref, lo, step)
    q = compress.quantize_columns(gpu(x), lo, inv, nbits)
    out = torch.empty(P * C, dtype=torch.float32, device=DEV)
    compress.decode_into(out, P, C, nbits, q, lo, step)
    torch.cuda.synchronize()
    q_np = q.cpu().numpy().view(np.uint8 if nbits == 8 else np.uint16)
    back = out.cpu().numpy().reshape(P, C)
    assert np.array_equal(q_np, q_ref)
    assert np.array_equal(bits(back), bits(back_ref))
    for col in range(C):
        if hi[col] > lo[col]:
            assert q_np[np.argmin(x[:, col]), col] == 0 and q_np[np.argmax(x[:, col]), col] == qmax
    if constant or P == 1:
        assert step[C - 1] == 0 and np.array_equal(bits(back[:, C - 1]), bits(x[:, C - 1]))
    bar = step.astype(np.float64) * (0.5 + 4 * qmax * U) + 2 * U * np.maximum(np.abs(lo), np.abs(hi)).astype(np.float64)
    err = np.abs(back.astype(np.float64) - x.astype(np.float64))
    assert np.all(err <= bar[None, :]), "largest error / bar: %.4f" % float((err / np.maximum(bar[None, :], 1e-300)).max())
    # 32 bits: the floats themselves
    out32 = torch.empty(P * C, dtype=torch.float32, device=DEV)
    compress.decode_into(out32, P, C, 32, gpu(x))
    assert np.array_equal(bits(out32.cpu().numpy().reshape(P, C)), bits(x))


W = H = 64
MODELS = {"dim3": (3, False, 16), "dim4_norot": (4, False, 33), "rot_4d": (4, True, 48)}


@functools.lru_cache(maxsize=None)
def model_of(kind, P=1500, distinct=0):
    """(scene, model): a fdgs.synth geometry with M coefficients per Gaussian of random values (from_raw: M = 33 is no product of
    degrees, which makes 3 (M - 1) = 96 the edge of a kernel bucket and 3 M no multiple of 4); ``distinct``: that many different
    non-DC rows in all."""
    from fdgs import synth
    from fdgs.train_host import GaussianParams
    dim, rot_4d, M = MODELS[kind]
    D, D_t = (3, 0) if dim == 3 else (3, 1)
    cfg = synth.SceneConfig(kind, P, W, H, D, D_t, 0.05, 1.0, rot_4d, dim, False)
    scene = synth.make_scene(cfg, seed=4, bg=(0.1, 0.2, 0.3), pose="rig1", alloc=(3, 2) if M == 48 else None, timestamp_frac=0.4)
    base = GaussianParams(scene, DEV)
    rng = np.random.default_rng(M)
    feats = (0.3 * rng.standard_normal((P, M, 3))).astype(np.float32)
    if distinct:
        rows = (0.3 * rng.standard_normal((distinct, M - 1, 3))).astype(np.float32)
        feats[:, 1:, :] = rows[np.arange(P) % distinct]
    tensors = {k: v.detach() for k, v in base.params.items()}
    tensors["_features"] = torch.from_numpy(feats)
    model = GaussianParams.from_raw(tensors, DEV, max_sh_degree=base.max_sh_degree, max_sh_degree_t=base.max_sh_degree_t,
                                    active_sh_degree=base.active_sh_degree, active_sh_degree_t=base.active_sh_degree_t,
                                    time_duration=base.time_duration, rot_4d=rot_4d, gaussian_dim=dim, force_sh_3d=False)
    return scene, model


def render_image(scene, model):
    from fdgs.fused import render_raw
    from fdgs.train_host import PipelineFlags, SyntheticCamera
    with torch.no_grad():
        out = render_raw(SyntheticCamera(scene, DEV), model, PipelineFlags(), scene["bg"].to(DEV))
    torch.cuda.synchronize()
    return out["render"].cpu().numpy()


@pytest.mark.parametrize("codebook_size", (256, None))
@pytest.mark.parametrize("kind", sorted(MODELS))
def test_decompress_equals_the_oracle_decode(kind, codebook_size):
    from fdgs import compress
    _scene, model = model_of(kind)
    cm = compress.compress(model, codebook_size=codebook_size, iters=2)
    M = MODELS[kind][2]
    assert cm.meta["P"] == model.P and cm.meta["M"] == M and cm.meta["gaussian_dim"] == MODELS[kind][0] and cm.meta["rot_4d"] == MODELS[kind][1]
    assert all(not t.is_cuda for t in cm.tensors.values())
    assert cm.tensors["_opacity"].dtype == torch.uint8 and cm.tensors["_t"].dtype == torch.uint16 and cm.tensors["_xyz"].dtype == torch.float32
    if codebook_size:
        assert tuple(cm.tensors["sh_codebook"].shape) == (256, 3 * (M - 1)) and cm.tensors["sh_index"].dtype == torch.uint16
    else:
        assert tuple(cm.tensors["sh_rest"].shape) == (model.P, 3 * (M - 1))
    back = compress.decompress(cm, DEV)
    torch.cuda.synchronize()
    ref = co.decode_model({k: t.numpy() for k, t in cm.tensors.items()}, cm.meta)
    assert back.P == model.P and back.M == M and back.flat.numel() == ref.size
    assert np.array_equal(bits(back.flat.detach().cpu().numpy()), bits(ref))
    assert (back.rot_4d, back.gaussian_dim, back.active_sh_degree, back.active_sh_degree_t) == (
        model.rot_4d, model.gaussian_dim, model.active_sh_degree, model.active_sh_degree_t)
    # 32-bit positions survive untouched; unit quaternions come back within a quantisation step per component
    assert torch.equal(back._xyz.detach(), model._xyz.detach())
    q = torch.nn.functional.normalize(model._rotation.detach())
    assert float((back._rotation.detach() - q).abs().max()) <= 0.5 * (2.0 / 255.0) * (1 + 1e-3)


def test_non_finite_parameters_raise():
    from fdgs import compress
    from fdgs.train_host import GaussianParams
    _scene, model = model_of("dim3")
    bad = GaussianParams.from_raw({k: v.detach().clone() for k, v in model.params.items()}, DEV, max_sh_degree=3)
    with torch.no_grad():
        bad._scaling[3, 1] = float("nan")
    with pytest.raises(ValueError, match="non-finite"):
        compress.compress(bad, codebook_size=16, iters=0)


def test_lossless_corner():
    """bits all 32, the codebook = the model's own 64 distinct rows, no iteration: the model comes back bit for bit."""
    from fdgs import compress
    from fdgs.gaussian_renderer import render
    from fdgs.slice import time_slice
    from fdgs.train_host import PipelineFlags, SyntheticCamera
    scene, model = model_of("rot_4d", distinct=64)
    rows = model._features.detach()[:64, 1:, :].reshape(64, -1).contiguous()
    assert torch.unique(rows, dim=0).shape[0] == 64
    cm = compress.compress(model, codebook_size=64, iters=0, init=rows, bits={k: 32 for k in compress.DEFAULT_BITS})
    assert np.array_equal(bits(cm.tensors["sh_codebook"].numpy()), bits(rows.cpu().numpy()))
    back = compress.decompress(cm, DEV)
    torch.cuda.synchronize()
    assert np.array_equal(bits(back.flat.detach().cpu().numpy()), bits(model.flat.detach().cpu().numpy()))
    assert np.array_equal(bits(render_image(scene, back)), bits(render_image(scene, model)))
    # ... and it is a model like any other: render() and time_slice take it
    cam, bg = SyntheticCamera(scene, DEV), scene["bg"].to(DEV)
    with torch.no_grad():
        a, b = render(cam, back, PipelineFlags(), bg)["render"], render(cam, model, PipelineFlags(), bg)["render"]
    assert torch.equal(a, b)
    assert time_slice(back, scene["timestamp"]).n == time_slice(model, scene["timestamp"]).n


def test_through_the_file(tmp_path):
    """Default settings on a rot_4d model.  39 bytes per Gaussian plus the codebook (256 x 141 x 4 = 144 KB) plus the metadata text stay
    below an eighth of 644 P only for P > 3600, so this model has 6000 Gaussians (the other tests' 1500 cannot meet that count)."""
    from fdgs import compress
    scene, model = model_of("rot_4d", P=6000)
    cm = compress.compress(model, codebook_size=256)
    path = str(tmp_path / "m.npz")
    compress.save(path, cm)
    direct = compress.decompress(cm, DEV)
    loaded = compress.decompress(compress.load(path), DEV)
    torch.cuda.synchronize()
    assert torch.equal(direct.flat.detach(), loaded.flat.detach())
    img_d, img_l = render_image(scene, direct), render_image(scene, loaded)
    assert np.array_equal(bits(img_d), bits(img_l))
    size, full = compress.nbytes(cm), 4 * model.P * model.floats_per_gaussian()
    print("compressed %d B, float32 %d B: 1 / %.2f" % (size, full, full / size))
    assert model.floats_per_gaussian() == 161 and size < full / 8
    with np.load(path) as z:
        assert sum(z[k].nbytes for k in z.files) == size
    # lossy, but the same scene: the report (not a bar) of how far the render moved
    mse = float(((img_d - render_image(scene, model)) ** 2).mean())
    print("PSNR of the decompressed render against the original: %.2f dB" % (10 * np.log10(1.0 / max(mse, 1e-30))))
