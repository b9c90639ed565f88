"""GPU: the k-NN query (fdgs.knn.knn), the rigid / motion regularisers (fdgs.loss.rigid_motion_loss and the C entries
fdgs_rigid_motion_forward / _backward) and the opacity-mask loss (fdgs.loss.opa_mask_loss, fdgs_opa_mask_loss) against the CPU
oracle (tests/regularizer_oracle.py), and a reference-style training loop with them.

The bar of the rigid / motion gradients is regularizer_oracle.grad_bar:  |hip - ref64| <= K * max(e32, 4 eps32 max|ref64|)  per
tensor, where e32 = max|float32 statement - float64 statement| of that tensor on that input and K is measured (BASELINE.md,
"Regulariser gradients").  It has no floor and is relative to the tensor's own size.  The bar these tests had before,
err <= 1e-4 * max(1.0, max|ref|), was blind: both losses are means over P, so every gradient is O(1 / P) and lay at or below the
floor of 1e-4.  max|reference gradient| of (g_rigid, g_motion) = (1, 0.5) on the models of test_rigid_motion_vs_float64_oracle:

    case (P, clones, k)   _scaling   _scaling_t   _rotation   _rotation_r
    700, 0, 20            3.3e-8     4.3e-8       1.6e-4      1.4e-4
    3000, 0, 8            2.4e-8     2.6e-8       6.8e-5      5.9e-5
    2000, 400, 20         1.7e-8     2.5e-8       5.1e-5      5.0e-5

A kernel writing zeros into d_scaling and d_scaling_t passed every case, one writing zeros into d_rotation and d_rotation_r three
of four, and so did a missing / k, a dropped reverse-neighbour term or a wrong sign on dSig[3][3].  tests/regularizer_cases.py
holds the inputs (with the rigid term alive: asserted there) and tests/test_regularizer_oracle_host.py proves on the CPU that the
bar accepts the float32 statement and rejects those wrong gradients."""
import numpy as np
import pytest
import torch

from util import synth
import regularizer_cases as rc
import regularizer_oracle as ro

pytestmark = pytest.mark.gpu
SC = synth.SceneConfig


def _pts(P, seed, kind):
    rng = np.random.default_rng(seed)
    if kind == "gauss":
        return (rng.standard_normal((P, 3)) * np.array([3.0, 1.0, 0.2])).astype(np.float32)
    if kind == "shifted":
        return (rng.random((P, 3)) + np.array([50.0, -20.0, 7.0])).astype(np.float32)
    if kind == "dups":
        base = rng.standard_normal((max(P // 3, 1), 3)).astype(np.float32)
        return base[rng.integers(0, base.shape[0], P)]
    raise ValueError(kind)


def _check_rows(got_i, got_d, want_i, want_d):
    np.testing.assert_array_equal(got_d.view(np.uint32), want_d.view(np.uint32))
    np.testing.assert_array_equal(got_i, want_i)


@pytest.mark.parametrize("k", [1, 3, 8, 20, 32, 64])
@pytest.mark.parametrize("P,kind", [(1, "gauss"), (5, "gauss"), (19, "gauss"), (20, "gauss"), (21, "gauss"), (1025, "shifted"),
                                    (4097, "dups"), (20000, "gauss")])
def test_knn_exact_vs_oracle(P, kind, k, gpu_device):
    """b = 2, queries != sources (their own set, of another size): d2 bit-exact, indices exact under the (d2, index) rule,
    slots beyond the sources padded with (1e10, 0)."""
    from fdgs.knn import knn
    n = max(1, P // 2 + 3)
    src = np.stack([_pts(P, 11 * P + b, kind) for b in range(2)])
    x = np.stack([_pts(n, 13 * P + b, kind) for b in range(2)])
    if kind == "dups":
        x[:, : n // 2] = src[:, : n // 2]          # queries sitting on (duplicated) sources: ties at d2 = 0
    idx, d2 = knn(torch.from_numpy(x).to(gpu_device), torch.from_numpy(src).to(gpu_device), k)
    assert idx.dtype == torch.int64 and d2.dtype == torch.float32 and tuple(idx.shape) == (2, n, k)
    idx, d2 = idx.cpu().numpy(), d2.cpu().numpy()
    rows = np.arange(n) if n <= 5000 else np.random.default_rng(P + k).choice(n, 1500, replace=False)
    for b in range(2):
        wi, wd = ro.knn(x[b], src[b], k, rows=rows)
        _check_rows(idx[b][rows], d2[b][rows], wi, wd)
    if P < k:
        assert (d2[:, :, P:] == 1e10).all() and (idx[:, :, P:] == 0).all()


def test_knn_self_query_and_transpose(gpu_device):
    from fdgs.knn import knn
    pts = torch.from_numpy(_pts(3000, 5, "dups")).to(gpu_device)[None]
    idx, d2 = knn(pts, pts, 20)
    assert (d2[..., 0] == 0).all()
    idx_t, d2_t = knn(pts.transpose(1, 2), pts.transpose(1, 2), 20, transpose=True)
    assert torch.equal(idx, idx_t) and torch.equal(d2, d2_t)
    wi, wd = ro.knn(pts[0].cpu().numpy(), pts[0].cpu().numpy(), 20)
    _check_rows(idx[0].cpu().numpy(), d2[0].cpu().numpy(), wi, wd)


def test_knn_at_c3_size_sampled_rows(gpu_device):
    """The C3 means (300 k), k = 20: 2000 sampled rows against brute force over all of them."""
    from fdgs.knn import knn
    scene = synth.make_scene(synth.CONFIGS["C3"], seed=0)
    pts = scene["means3D"].float().contiguous()
    idx, d2 = knn(pts.to(gpu_device)[None], pts.to(gpu_device)[None], 20)
    rows = np.random.default_rng(3).choice(pts.shape[0], 2000, replace=False)
    wi, wd = ro.knn(pts.numpy(), pts.numpy(), 20, rows=rows, chunk=50)
    _check_rows(idx[0].cpu().numpy()[rows], d2[0].cpu().numpy()[rows], wi, wd)


def test_knn_refuses_what_it_does_not_do(gpu_device):
    from fdgs.knn import knn
    x = torch.zeros(1, 10, 3, device=gpu_device)
    with pytest.raises(ValueError, match="k <= 64"):
        knn(x, x, 65)
    with pytest.raises(ValueError, match="k <= 64"):
        knn(x, x, 0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        knn(x.cpu(), x.cpu(), 3)


# ---- rigid + motion ----

def _model(dev, P, seed, dup=0):
    from fdgs import train_host
    cfg = SC("reg", P, 96, 64, 1, 1, 0.05, 10.0, True, 4, False)
    scene = synth.make_scene(cfg, seed=seed)
    m = train_host.ReferenceStyleModel(scene, dev)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        m._rotation.mul_((0.5 + 1.5 * torch.rand(P, 1, generator=g)).to(dev))
        m._rotation_r.mul_((0.5 + 1.5 * torch.rand(P, 1, generator=g)).to(dev))
        m._scaling_t.add_((torch.randn(P, 1, generator=g) * 0.3).to(dev))
        if dup:   # densification clones: exact copies of the first `dup` Gaussians appended
            for n in ("_xyz", "_scaling", "_scaling_t", "_rotation", "_rotation_r", "_t"):
                t = getattr(m, n)
                setattr(m, n, torch.nn.Parameter(torch.cat([t, t[:dup]]).contiguous()))
    return m


NAMES4 = ro.NAMES4
WORST = {}    # (tensor, case) -> err / unit of the bar, printed by test_worst_ratios_are_reported


def _hold(tag, bars, got):
    """Prints every tensor's err / unit (K is 4 x the worst of them) and then holds it to its bar."""
    for n, bar in bars.items():
        ratio = bar.ratio(got[n])
        WORST[(n, tag)] = max(WORST.get((n, tag), 0.0), ratio)
        print("%-28s %-12s max|ref| %.2e e32 %.2e err %.2e err/unit %.2f (K %g)" % (tag, n, bar.ref_max, bar.e32, bar.err(got[n]), ratio,
                                                                                    ro.GRAD_BAR_K[n]))
    for n, bar in bars.items():
        assert torch.isfinite(got[n]).all(), (tag, n)
        assert bar.accepts(got[n]), (tag, n, bar.err(got[n]), bar.bar, bar.ref_max)


def _loss_close(got, want):
    assert got == 0 if want == 0 else abs(got - want) <= 1e-5 * abs(want), (got, want)


def _kernel_run(m, k, g_rigid=1.0, g_motion=0.5):
    from fdgs.loss import rigid_motion_loss
    for n in NAMES4:
        getattr(m, n).grad = None
    lr, lm = rigid_motion_loss(m, k)
    (g_rigid * lr + g_motion * lm).backward()
    return float(lr.detach()), float(lm.detach()), {n: getattr(m, n).grad.detach().cpu().clone() for n in NAMES4}


def _oracle_run(m, k, g_rigid=1.0, g_motion=0.5):
    """(L_rigid, L_motion) in float64 and the bars of the four gradients, on the k-NN table the GPU query returns."""
    from fdgs.knn import knn
    idx, d2 = knn(m._xyz.detach()[None], m._xyz.detach()[None], k)
    params = {n: getattr(m, n).detach().cpu() for n in NAMES4 + ("_t",)}
    idx, d2 = idx[0].cpu(), d2[0].cpu()
    wr, wm, _ = ro.rigid_motion_with_grads(params, idx, d2, torch.float64, g_rigid, g_motion)
    return wr, wm, ro.grad_bar(params, idx, d2, g_rigid, g_motion)


@pytest.mark.parametrize("P,dup,k", [(700, 0, 20), (3000, 0, 8), (2000, 400, 20), (300_000, 0, 20)], ids=["small", "k8", "clones", "C3"])
def test_rigid_motion_vs_float64_oracle(P, dup, k, gpu_device):
    m = _model(gpu_device, P, seed=P + dup, dup=dup)
    lr, lm, g = _kernel_run(m, k)
    wr, wm, bars = _oracle_run(m, k)
    assert abs(lr - wr) <= 1e-5 * abs(wr) and abs(lm - wm) <= 1e-5 * abs(wm), (lr, wr, lm, wm)
    _hold("synth-P%d-dup%d-k%d" % (P, dup, k), bars, g)


def test_rigid_motion_gradient_is_bit_reproducible(gpu_device):
    m = _model(gpu_device, 20000, seed=9, dup=3000)
    a = _kernel_run(m, 20)
    b = _kernel_run(m, 20)
    assert a[0] == b[0] and a[1] == b[1]
    for n in NAMES4:
        assert torch.equal(a[2][n], b[2][n]), n


def test_rigid_motion_on_the_flat_bucket_model(gpu_device):
    """GaussianParams: the gradients land in the flat gradient bucket's slices (the reference attribute names)."""
    from fdgs import train_host
    from fdgs.loss import rigid_motion_loss
    scene = synth.make_scene(SC("reg", 1500, 96, 64, 1, 1, 0.05, 10.0, True, 4, False), seed=2)
    gp = train_host.GaussianParams(scene, gpu_device)
    gp.zero_grad()
    lr, lm = rigid_motion_loss(gp)
    (lr + lm).backward()
    wr, wm, bars = _oracle_run(gp, 20, 1.0, 1.0)
    assert abs(float(lr) - wr) <= 1e-5 * abs(wr)
    got = {n: gp.flat_grad[gp.offsets[n][0]:gp.offsets[n][1]].view(bars[n].ref.shape).cpu() for n in NAMES4}
    _hold("flat-bucket-P1500-k20", bars, got)


def test_rigid_motion_refuses_a_model_without_rot_4d(gpu_device):
    from fdgs import train_host
    from fdgs.loss import rigid_motion_loss
    scene = synth.make_scene(SC("norot", 500, 96, 64, 1, 0, 0.05, 1.0, False, 4, True), seed=1)
    with pytest.raises(ValueError, match="rot_4d"):
        rigid_motion_loss(train_host.ReferenceStyleModel(scene, gpu_device))


# ---- the shared cases (tests/regularizer_cases.py) against grad_bar ----

class _Pc:
    """The reference model's attribute names on a case's tensors (what rigid_motion_loss asks of its argument)."""
    rot_4d, gaussian_dim = True, 4

    def __init__(self, case, dev):
        for n in rc.NAMES:
            setattr(self, n, case.params[n].to(dev).clone().requires_grad_(n in NAMES4))

    get_xyz = property(lambda s: s._xyz)
    get_t = property(lambda s: s._t)


class _CRun:
    """One case through the C entries.  ``carve(name, shape)`` hands out the buffers (default: fresh tensors), ``outs`` the four
    gradient buffers [P + spare, c] to ADD into (default: zeros)."""

    def __init__(self, case, dev, carve=None):
        from fdgs import _capi
        self.capi, self.case, self.dev, self.P, self.k = _capi, case, dev, case.P, case.k
        carve = carve or (lambda name, shape: torch.empty(shape, dtype=torch.float32, device=dev))
        self.carve = carve
        self.ins = []
        for n in NAMES4 + ("_t",):
            buf = carve(n, tuple(case.params[n].shape))
            buf.copy_(case.params[n])
            self.ins.append(buf)
        self.idx, self.d2 = case.idx.to(dev).contiguous(), case.d2.to(dev).contiguous()
        self.vel = carve("velocity", (self.P, 3))
        self.losses = torch.empty(2, dtype=torch.float32, device=dev)
        self.scratch = torch.empty(_capi.lib.fdgs_rigid_motion_scratch_bytes(self.P, self.k), dtype=torch.uint8, device=dev)

    def forward(self):
        c = self.capi
        with torch.cuda.device(self.dev):
            rc_ = c.lib.fdgs_rigid_motion_forward(self.P, self.k, *[t.data_ptr() for t in self.ins], self.idx.data_ptr(), self.d2.data_ptr(),
                                                  self.vel.data_ptr(), self.losses.data_ptr(), self.scratch.data_ptr(),
                                                  c.current_stream_handle(self.dev))
        c._check(rc_, "fdgs_rigid_motion_forward")
        lo = self.losses.cpu()
        return float(lo[0]), float(lo[1]), self.vel.cpu().clone()

    def zeros(self, spare=0, fill=None):
        outs = []
        for n in NAMES4:
            buf = self.carve("d" + n, (self.P + spare, self.case.params[n].shape[1]))
            buf.zero_() if fill is None else buf.copy_(fill[n])
            outs.append(buf)
        return outs

    def backward(self, g, scale=1.0, outs=None):
        c = self.capi
        outs = self.zeros() if outs is None else outs
        gl = torch.tensor(g, dtype=torch.float32, device=self.dev)
        with torch.cuda.device(self.dev):
            rc_ = c.lib.fdgs_rigid_motion_backward(self.P, self.k, *[t.data_ptr() for t in self.ins], self.idx.data_ptr(), self.d2.data_ptr(),
                                                   self.vel.data_ptr(), gl.data_ptr(), scale, *[o.data_ptr() for o in outs],
                                                   self.scratch.data_ptr(), c.current_stream_handle(self.dev))
        c._check(rc_, "fdgs_rigid_motion_backward")
        torch.cuda.synchronize()
        return {n: o.cpu().clone() for n, o in zip(NAMES4, outs)}


def _wanted(case, w):
    wr, wm, _ = ro.rigid_motion_with_grads(case.params, case.idx, case.d2, torch.float64, w[0], w[1], case.mask)
    return wr, wm, ro.grad_bar(case.params, case.idx, case.d2, w[0], w[1], case.mask)


def _zero_case_is_zero(case, lr, lm, g):
    if case.zero:   # the reference's initial state: v = 0 for every Gaussian, through the nrm > 0 guard and 0 / ct
        assert lr == 0 and lm == 0 and all(torch.isfinite(t).all() and float(t.abs().max()) == 0 for t in g.values())
    if not case.rigid:
        assert lr == 0


@pytest.mark.parametrize("w", rc.WEIGHTS, ids=lambda w: "r%g-m%g" % w)
@pytest.mark.parametrize("spec", rc.MODEL_SPECS, ids=rc.spec_id)
def test_model_cases_hold_the_gradient_bar(spec, w, gpu_device):
    """Every model case through fdgs.loss.rigid_motion_loss: P in {1, 2, 5, 20, 21, 255, 256, 257, 1024, 1025} (P <= k: empty
    slots of (1e10, 0); a workgroup boundary; a power of two), clones, the initial state, late t, thin time extents."""
    from fdgs.knn import knn
    case = rc.case_of(spec)
    m = _Pc(case, gpu_device)
    idx, d2 = knn(m._xyz.detach()[None], m._xyz.detach()[None], case.k)
    assert torch.equal(idx[0].cpu(), case.idx) and torch.equal(d2[0].cpu(), case.d2), "the k-NN query differs from its oracle"
    lr, lm, g = _kernel_run(m, case.k, *w)
    wr, wm, bars = _wanted(case, w)
    _loss_close(lr, wr)
    _loss_close(lm, wm)
    _zero_case_is_zero(case, lr, lm, g)
    _hold("%s r%g m%g" % (case.name, w[0], w[1]), bars, g)


@pytest.mark.parametrize("w", rc.WEIGHTS, ids=lambda w: "r%g-m%g" % w)
@pytest.mark.parametrize("spec", rc.TABLE_SPECS, ids=rc.spec_id)
def test_crafted_tables_hold_the_gradient_bar(spec, w, gpu_device):
    """Tables no k-NN query returns, through the C entries: one Gaussian that is everybody's neighbour (a reverse segment of P * k
    entries), a neighbour twice in a row, self entries only, entries outside [0, P) (-1, P, P + 7, 2^40: bucket P of the sort, which
    at P = 256 and 1024 needs one key bit more than P - 1), rows in descending order."""
    case = rc.case_of(spec)
    run = _CRun(case, gpu_device)
    lr, lm, _v = run.forward()
    g = run.backward(w)
    wr, wm, bars = _wanted(case, w)
    _loss_close(lr, wr)
    _loss_close(lm, wm)
    _zero_case_is_zero(case, lr, lm, g)
    _hold("%s r%g m%g" % (case.name, w[0], w[1]), bars, g)


@pytest.mark.parametrize("spec", rc.MODEL_SPECS + rc.TABLE_SPECS, ids=rc.spec_id)
def test_velocity_output_vs_float64(spec, gpu_device):
    case = rc.case_of(spec)
    _lr, _lm, v = _CRun(case, gpu_device).forward()
    bar = ro.velocity_bar(case.params)
    if case.zero:
        assert float(v.abs().max()) == 0
    _hold(case.name, {"velocity": bar}, {"velocity": v})


def _ulp(x):
    """The spacing of float32 at |x| (the smallest normal's below it)."""
    x = x.abs().clamp_min(float(np.finfo(np.float32).tiny))
    return torch.ldexp(torch.ones_like(x), torch.frexp(x).exponent - 24)


@pytest.mark.parametrize("spec", [("compact", 257, 20), ("foreign", 256, 8)], ids=rc.spec_id)
def test_c_entry_scale_argument(spec, gpu_device):
    """scale = 0.37 gives 0.37 x the scale = 1 gradients, element by element to 2 ulp of the element (the kernel multiplies the
    finished gradient by scale; scaling the upstream weights first, as it did, moved every later rounding: up to 14708 ulp of an
    element that is a cancelling sum, 5 ulp of the tensor's largest entry)."""
    run = _CRun(rc.case_of(spec), gpu_device)
    run.forward()
    one = run.backward((0.7, 0.3), 1.0)
    got = run.backward((0.7, 0.3), 0.37)
    for n in NAMES4:
        want = one[n] * torch.tensor(0.37, dtype=torch.float32)
        off = float(((got[n] - want).abs() / _ulp(want)).max())
        print("scale 0.37 %-12s worst gap %.2f ulp of the element" % (n, off))
        assert float(want.abs().max()) > 0 and off <= 2, (n, off)


@pytest.mark.parametrize("spec", [("compact", 255, 8), ("compact", 256, 8), ("compact", 257, 20), ("hub", 1024, 8)], ids=rc.spec_id)
def test_c_entry_adds_into_its_buffers_and_leaves_guard_rows(spec, gpu_device):
    """Gradient buffers pre-filled with a pattern come back as pattern + gradient (one float32 addition per element), and the 3 rows
    after the last Gaussian are untouched."""
    case = rc.case_of(spec)
    run = _CRun(case, gpu_device)
    run.forward()
    plain = run.backward((0.7, 0.3))
    gen = torch.Generator().manual_seed(5)
    fill = {n: (torch.rand(case.P + 3, case.params[n].shape[1], generator=gen) - 0.5) * 0.1 for n in NAMES4}
    got = run.backward((0.7, 0.3), outs=run.zeros(spare=3, fill=fill))
    for n in NAMES4:
        assert torch.equal(got[n][:case.P], fill[n][:case.P] + plain[n]), n
        assert torch.equal(got[n][case.P:], fill[n][case.P:]), n


@pytest.mark.parametrize("spec", [("compact", 257, 20), ("foreign", 1024, 8)], ids=rc.spec_id)
def test_c_entry_on_unaligned_slices_of_a_flat_bucket(spec, gpu_device):
    """Every float buffer a slice of one flat bucket that starts 4, 8 or 12 bytes past a 16-byte boundary: the same bits as on
    aligned tensors."""
    case = rc.case_of(spec)
    ref = _CRun(case, gpu_device)
    want_f = ref.forward()
    want_g = ref.backward((0.7, 0.3))
    flat = torch.zeros(64 * case.P + 256, dtype=torch.float32, device=gpu_device)
    assert flat.data_ptr() % 16 == 0
    state = {"at": 0, "n": 0}

    def carve(_name, shape):
        numel = int(np.prod(shape))
        at = state["at"] + (4 - state["at"] % 4) % 4 + 1 + state["n"] % 3      # 1, 2, 3 floats past a 16-byte boundary in turn
        state["at"], state["n"] = at + numel, state["n"] + 1
        out = flat[at:at + numel].view(shape)
        assert out.data_ptr() % 16 != 0
        return out
    run = _CRun(case, gpu_device, carve=carve)
    got_f = run.forward()
    got_g = run.backward((0.7, 0.3))
    assert got_f[0] == want_f[0] and got_f[1] == want_f[1] and torch.equal(got_f[2], want_f[2])
    for n in NAMES4:
        assert torch.equal(got_g[n], want_g[n]), n


@pytest.mark.parametrize("spec", [("hub", 1024, 8), ("foreign", 1024, 20)], ids=rc.spec_id)
def test_crafted_tables_are_bit_reproducible(spec, gpu_device):
    runs = []
    for _ in range(2):
        run = _CRun(rc.case_of(spec), gpu_device)
        runs.append((run.forward(), run.backward((0.7, 0.3))))
    assert runs[0][0][:2] == runs[1][0][:2] and torch.equal(runs[0][0][2], runs[1][0][2])
    for n in NAMES4:
        assert torch.equal(runs[0][1][n], runs[1][1][n]), n


# ---- opacity mask ----

def test_opa_mask_value_and_gradient_vs_oracle(gpu_device):
    from fdgs.loss import opa_mask_loss
    H, W = 97, 131
    gen = torch.Generator().manual_seed(4)
    alpha = torch.rand(1, H, W, generator=gen)
    flat = alpha.view(-1)
    flat[:6] = torch.tensor([1e-6, 1 - 1e-6, 0.0, 1.0, 1e-7, 1 - 1e-7])   # at and beyond both clamp bounds
    mask = (torch.rand(1, H, W, generator=gen) > 0.4).float()
    mask.view(-1)[:6] = 0.0    # sky = 1 there: the clamp decides the gradient
    a = alpha.to(gpu_device).requires_grad_(True)
    val = opa_mask_loss(a, mask.to(gpu_device))
    (3.0 * val).backward()
    ar = alpha.double().requires_grad_(True)
    want = ro.opa_mask(ar, mask.double(), bounds=ro.OPA_BOUNDS_F32)
    (3.0 * want).backward()
    assert abs(float(val) - float(want)) <= 1e-5 * abs(float(want))
    g = a.grad.cpu().double()
    torch.testing.assert_close(g, ar.grad, rtol=1e-5, atol=1e-12)
    # torch.clamp passes the gradient AT both float32 bounds and blocks it beyond them
    assert (g.view(-1)[:2] > 0).all() and (g.view(-1)[2:6] == 0).all(), g.view(-1)[:6]


def _opa_call(dev, H, W, a, alpha_is_T, mask, up, scale, grad, accumulate):
    from fdgs import _capi
    parts = torch.empty(max(1, _capi.lib.fdgs_opa_mask_num_partials(H, W)), dtype=torch.float32, device=dev)
    out = torch.empty(1, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rc_ = _capi.lib.fdgs_opa_mask_loss(H, W, a.data_ptr(), alpha_is_T, mask.data_ptr(), None if up is None else up.data_ptr(), scale,
                                           None if grad is None else grad.data_ptr(), accumulate, parts.data_ptr(), out.data_ptr(),
                                           _capi.current_stream_handle(dev))
    _capi._check(rc_, "fdgs_opa_mask_loss")
    torch.cuda.synchronize()
    return float(out.cpu()[0])


@pytest.mark.parametrize("alpha_is_T", [0, 1])
@pytest.mark.parametrize("H,W", [(1, 1), (1, 255), (16, 16), (1, 257), (97, 131)])
def test_opa_mask_c_entry_arguments(H, W, alpha_is_T, gpu_device):
    """fdgs_opa_mask_loss directly, with the arguments StepPipeline passes: the transmittance T in place of alpha (the clamp-edge
    values placed in T), a device upstream scalar times scale = 0.3, accumulate = 1 onto a pattern, grad = NULL for the value only.
    rtol 1e-5 against the float64 statement, exact zeros beyond the clamp bounds."""
    dev, HW = gpu_device, H * W
    gen = torch.Generator().manual_seed(HW + alpha_is_T)
    a = torch.rand(HW, generator=gen)
    # at and beyond both clamp bounds.  Not at H W = 1: log(1 - o) of o = 1e-6 alone is lost to the rounding of 1 - o in any float32
    # statement (torch's included), and would be the whole value there
    edge = torch.tensor([1e-6, 1 - 1e-6, 0.0, 1.0, 1e-7, 1 - 1e-7, -0.5, 1.5] if HW >= 8 else [])
    a[:edge.numel()] = edge
    mask = (torch.rand(HW, generator=gen) > 0.4).float()
    mask[:edge.numel()] = 0.0     # sky = 1 there: the clamp decides the gradient
    given = (1 - a) if alpha_is_T else a                 # float32: what the kernel is handed
    alpha = (1 - given) if alpha_is_T else given         # float32, as the kernel computes it: 1.f - T
    up = torch.tensor([1.7], dtype=torch.float32)
    ar = alpha.double().requires_grad_(True)
    want = ro.opa_mask(ar, mask.double(), bounds=ro.OPA_BOUNDS_F32)
    (0.3 * float(up[0]) * want).backward()
    lo, hi = ro.OPA_BOUNDS_F32
    beyond = (alpha.double() < lo) | (alpha.double() > hi)
    assert (ar.grad[beyond] == 0).all() and (ar.grad[~beyond & (mask == 0)] > 0).all() and int(beyond.sum()) == (6 if HW >= 8 else 0)
    d_given, d_mask, d_up = given.to(dev), mask.to(dev), up.to(dev)
    # value only
    val = _opa_call(dev, H, W, d_given, alpha_is_T, d_mask, None, 1.0, None, 0)
    assert abs(val - float(want)) <= 1e-5 * abs(float(want)), (val, float(want))
    # written
    g = torch.full((HW + 3,), 7.0, dtype=torch.float32, device=dev)
    val2 = _opa_call(dev, H, W, d_given, alpha_is_T, d_mask, d_up, 0.3, g, 0)
    assert val2 == val
    g = g.cpu()
    torch.testing.assert_close(g[:HW].double(), ar.grad, rtol=1e-5, atol=0)
    assert (g[:HW][beyond] == 0).all() and (g[HW:] == 7.0).all()
    # added onto a pattern: one float32 addition per element
    pattern = (torch.rand(HW + 3, generator=gen) - 0.5) * 0.01
    acc = pattern.to(dev)
    _opa_call(dev, H, W, d_given, alpha_is_T, d_mask, d_up, 0.3, acc, 1)
    acc = acc.cpu()
    assert torch.equal(acc[:HW], pattern[:HW] + g[:HW]) and torch.equal(acc[HW:], pattern[HW:])
    assert torch.equal(acc[:HW][beyond], pattern[:HW][beyond])


def test_render_with_opa_mask_matches_the_torch_expression(gpu_device):
    """render()'s alpha -> opa_mask_loss gives the parameter gradients of the reference's torch expression (blend AUX path)."""
    from fdgs import train_host
    from fdgs.gaussian_renderer import render
    from fdgs.loss import opa_mask_loss
    scene = synth.make_scene(SC("opa", 4000, 160, 112, 2, 1, 0.03, 10.0, True, 4, False), seed=6)
    model = train_host.ReferenceStyleModel(scene, gpu_device)
    cam = train_host.SyntheticCamera(scene, gpu_device, timestamp=0.4 * scene["time_duration"])
    bg = torch.tensor([0.1, 0.2, 0.3], device=gpu_device)
    mask = (torch.rand(1, scene["H"], scene["W"], generator=torch.Generator().manual_seed(1)) > 0.5).float().to(gpu_device)
    names = ("_xyz", "_opacity", "_scaling", "_rotation", "_t", "_scaling_t", "_rotation_r")
    grads = {}
    for which in ("fdgs", "torch"):
        for n in names:
            getattr(model, n).grad = None
        pkg = render(cam, model, train_host.PipelineFlags(), bg)
        loss = opa_mask_loss(pkg["alpha"], mask) if which == "fdgs" else ro.opa_mask(pkg["alpha"], mask)
        loss.backward()
        grads[which] = {n: getattr(model, n).grad.detach().clone() for n in names}
    for n in names:
        ref = grads["torch"][n]
        err = float((grads["fdgs"][n] - ref).abs().max())
        assert err <= 1e-4 * max(1.0, float(ref.abs().max())), (n, err)


def test_reference_loop_with_the_regularisers(gpu_device):
    """ReferenceStyleModel + render() + fdgs.optim.Adam + the fused terms against torch.optim.Adam + the torch oracle terms."""
    from fdgs import train_host
    from fdgs.gaussian_renderer import render
    from fdgs.knn import knn
    from fdgs.loss import opa_mask_loss, rigid_motion_loss
    cfg = SC("loop", 5000, 160, 112, 2, 1, 0.03, 10.0, True, 4, False)
    scene = synth.make_scene(cfg, seed=8)
    gen = torch.Generator().manual_seed(2)
    gts = [torch.rand(3, cfg.H, cfg.W, generator=gen).to(gpu_device) for _ in range(2)]
    masks = [(torch.rand(1, cfg.H, cfg.W, generator=gen) > 0.5).float().to(gpu_device) for _ in range(2)]
    bg = torch.tensor([0.1, 0.2, 0.3], device=gpu_device)
    final, losses, first = {}, {}, {}
    for which in ("fdgs", "torch"):
        model = train_host.ReferenceStyleModel(scene, gpu_device, optimizer=which)
        for g in model.optimizer.param_groups:
            g["lr"] = 1e-3
        cams = [train_host.SyntheticCamera(scene, gpu_device, timestamp=(b + 0.5) / 2 * scene["time_duration"]) for b in range(2)]
        hist = []
        for step in range(3):
            model.optimizer.zero_grad(set_to_none=True)
            for b in range(2):
                pkg = render(cams[b], model, train_host.PipelineFlags(), bg)
                loss = (pkg["render"] - gts[b]).abs().mean()
                if which == "fdgs":
                    lo = opa_mask_loss(pkg["alpha"], masks[b])
                    lr, lm = rigid_motion_loss(model, 20)
                else:
                    lo = ro.opa_mask(pkg["alpha"], masks[b])
                    idx, d2 = knn(model.get_xyz.detach()[None], model.get_xyz.detach()[None], 20)
                    v = ro.velocity(model._scaling, model._scaling_t, model._rotation, model._rotation_r, model._t, torch.float32)
                    lr, lm = ro.rigid(v, idx[0], d2[0]), ro.motion(v)
                loss = loss + 0.5 * lo + 1.0 * lr + 0.1 * lm
                (loss / 2).backward()
                hist.append(float(loss))
            if step == 0:
                first[which] = {n: getattr(model, n).grad.detach().clone() for n in ("_scaling", "_rotation", "_scaling_t", "_rotation_r")}
            model.optimizer.step()
        losses[which] = hist
        final[which] = {n: getattr(model, n).detach().clone() for n in ("_xyz", "_scaling", "_rotation", "_scaling_t", "_rotation_r")}
    np.testing.assert_allclose(losses["fdgs"], losses["torch"], rtol=2e-5)
    for n, ref in first["torch"].items():
        err = float((first["fdgs"][n] - ref).abs().max())
        assert err <= 1e-4 * max(1.0, float(ref.abs().max())), (n, err)
    # Adam divides by sqrt(v): where a gradient is ~0 an ulp of difference can move that element by up to lr per step, so the
    # parameters are held to the project's bar on all but 0.1 % of their elements and to Adam's bounded step (3 steps x lr) everywhere
    for n, ref in final["torch"].items():
        d = (final["fdgs"][n] - ref).abs()
        bar = 1e-4 * max(1.0, float(ref.abs().max()))
        assert float((d > bar).float().mean()) <= 1e-3 and float(d.max()) <= 3 * 1e-3 * 1.01, (n, float(d.max()))


def test_worst_ratios_are_reported():
    """Not a check of its own: prints, per tensor, the worst err / unit the tests above observed and the case it came from
    (regularizer_oracle.GRAD_BAR_K is 4 x the worst, rounded up to a power of two, at least 8: BASELINE.md, "Regulariser gradients")."""
    for n in NAMES4 + ("velocity",):
        seen = sorted(((v, tag) for (name, tag), v in WORST.items() if name == n), reverse=True)
        for v, tag in seen[:3]:
            print("worst ratio %-12s %.3f  %s  (K %g)" % (n, v, tag, ro.GRAD_BAR_K[n]))
