"""GPU: all three implementations of the photometric loss in csrc/ssim.hip -- the forward + backward pair, the one-kernel form
(``ssim_options["fused"]``) and the reduction of the per-tile partial sums -- on the inputs and shapes where they can go wrong.

Tests 1, 2 and 5 compare EACH path directly with the float64 evaluation of the reference's statement (tests/loss_cases.py), never
path against path, at an error bar that follows the conditioning of the input: 4 x the float32 reference's own error on the case,
floored by the same figure on noise of the same shape (derivation in loss_cases; the bar never looks at a kernel's output).  Every
comparison is a maximum over all C*H*W elements.  Test 3 checks that every output element is written and nothing around it; test 4
the reduction kernel alone, against a float64 sum, with partial counts on both sides of its 8192-per-trip loop."""
import pytest
import torch

import loss_cases as lc

pytestmark = pytest.mark.gpu

UP = 0.37          # upstream scalar d(total)/d(loss): not 1; the gradient and its bar scale by it
PATHS = [False, True]
PATH_IDS = ["pair", "fused"]


def _run(img, gt, lam, fused, dev, up=UP):
    """(loss value, gradient on the CPU as float64, num_partials) of one path through fdgs.loss.l1_ssim_grad + l1_ssim_loss."""
    from fdgs import loss as fl
    upstream = torch.full((1,), up, dtype=torch.float32, device=dev)
    fl.ssim_options["fused"] = fused
    try:
        g, handle = fl.l1_ssim_grad(img.to(dev), gt.to(dev), lam, upstream)
        val = fl.l1_ssim_loss(handle)
        torch.cuda.synchronize()
    finally:
        fl.ssim_options["fused"] = False
    return float(val), g.cpu().double(), handle[1]


def _check(c, val, g, tag, up=UP):
    """Value and gradient of a path against ref64 at the case's bars; prints the observed error and the bar."""
    err_v = abs(val - c.loss64)
    err_g = float((g.reshape(c.grad64.shape) - up * c.grad64).abs().max())
    print("%-15s %-13s lam %.1f %-5s | value err %.2e (bar %.2e) | gradient err %.2e (bar %.2e = %.2f of it; ref32 %.2e; max|g| %.2e)"
          % (c.name, "x".join(map(str, c.shape)), c.lam, tag, err_v, c.bar_v, err_g, up * c.bar_g, err_g / (up * c.bar_g), up * c.err_g, up * c.grad_max))
    assert torch.isfinite(g).all()
    assert err_v <= c.bar_v, (err_v, c.bar_v)
    assert err_g <= up * c.bar_g, (err_g, up * c.bar_g)


# ---- 1. input classes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", PATHS, ids=PATH_IDS)
@pytest.mark.parametrize("lam", [0.2, 1.0])
@pytest.mark.parametrize("shape", [(3, 48, 70), (3, 97, 131)], ids=["3x48x70", "3x97x131"])
@pytest.mark.parametrize("name", list(lc.CLASSES))
def test_input_classes_against_float64(name, shape, lam, fused, gpu_device):
    """Every input class of loss_cases on both paths: noise, a smooth pair, a white-background scene near convergence (flat bright
    regions, img ~ gt: sigma12 = E[xy] - mu1 mu2 cancels against C2 = 9e-4), two constants 1e-3 apart, img == gt, all black, an unclamped
    render.  Where img == gt the true gradient is 0: the bar is the noise floor of the shape, and with lambda = 0 -- the L1 term alone,
    whose sign(0) is 0 -- the gradient is +0 bit for bit."""
    c = lc.case(name, shape, lam)
    val, g, _ = _run(c.img, c.gt, lam, fused, gpu_device)
    _check(c, val, g, PATH_IDS[fused])
    if name in ("identical", "black"):
        assert abs(c.loss64) <= 1e-12
        val0, g0, _ = _run(c.img, c.gt, 0.0, fused, gpu_device)
        assert val0 == 0.0
        assert not g0.float().view(torch.int32).any(), "lambda = 0 on img == gt: the L1 part of the gradient is not exactly absent"


# ---- 2. shapes -----------------------------------------------------------------------------------------------------------------
SHAPES = lc.EDGE_SHAPES      # shape -> number of 32 x 32 tiles


@pytest.mark.parametrize("fused", PATHS, ids=PATH_IDS)
@pytest.mark.parametrize("shape", list(SHAPES), ids=["x".join(map(str, s)) for s in SHAPES])
def test_shapes_against_float64(shape, fused, gpu_device):
    """Noise at lambda = 0.2 on the smallest shapes that exercise each mechanism (SHAPES above), both paths, same bars.  The tile
    totals of SHAPES are C * ceil(H / 32) * ceil(W / 32) -- (1,32,225): 1*1*8 = 8; (1,32,257): 1*1*9 = 9; (3,33,33): 3*2*2 = 12;
    (1,33,97): 1*2*4 = 8; (2,64,129): 2*2*5 = 20; (3,95,97): 3*3*4 = 36 -- and fdgs_l1_ssim_num_partials must return them."""
    from fdgs import _capi
    assert _capi.lib.fdgs_l1_ssim_num_partials(*shape) == SHAPES[shape]
    c = lc.case("noise", shape, 0.2)
    val, g, nparts = _run(c.img, c.gt, 0.2, fused, gpu_device)
    assert nparts == SHAPES[shape]
    _check(c, val, g, PATH_IDS[fused])


# ---- 3. every element written, nothing else touched ----------------------------------------------------------------------------
GUARD = 4096
NAN_BITS = 0x7FC00ABC      # a quiet NaN with a payload: what an untouched float of a buffer holds


class _Guarded:
    """A buffer [GUARD | n | GUARD] of floats, all NaN_BITS; ``ptr``: the address of the middle slice."""

    def __init__(self, n, dev):
        self.n = n
        self.bits = torch.full((n + 2 * GUARD,), NAN_BITS, dtype=torch.int32, device=dev)
        self.ptr = self.bits[GUARD:].data_ptr()

    def check(self, what):
        body = self.bits[GUARD:GUARD + self.n].view(torch.float32)
        unwritten = int((self.bits[GUARD:GUARD + self.n] == NAN_BITS).sum())
        assert unwritten == 0, "%s: %d of %d elements were never written" % (what, unwritten, self.n)
        assert torch.isfinite(body).all(), what + ": non-finite output"
        for side, guard in (("below", self.bits[:GUARD]), ("above", self.bits[GUARD + self.n:])):
            touched = (guard != NAN_BITS).nonzero().flatten()
            assert touched.numel() == 0, "%s: %d floats %s the output were written (first at guard offset %d)" % (what, touched.numel(), side, int(touched[0]))
        return body


@pytest.mark.parametrize("fused", PATHS, ids=PATH_IDS)
@pytest.mark.parametrize("shape", [(3, 5, 6), (3, 33, 31), (1, 32, 257)], ids=["3x5x6", "3x33x31", "1x32x257"])
def test_every_output_element_is_written_and_nothing_else(shape, fused, gpu_device):
    """The C ABI directly, every output -- gradient, the three derivative maps of the pair, both partial arrays -- a slice of a larger
    buffer pre-filled with NaN, 4096 floats of guard on both sides: afterwards every element of the slices is finite (torch.empty hides an
    unwritten slot) and every guard float still holds its bit pattern (... and a store past the end).  One shape of each group of test 2."""
    from fdgs import _capi
    dev = gpu_device
    C, H, W = shape
    c = lc.case("noise", shape, 0.2)
    img, gt = c.img.to(dev).contiguous(), c.gt.to(dev).contiguous()
    up = torch.full((1,), UP, dtype=torch.float32, device=dev)
    n, nparts = C * H * W, SHAPES[shape]
    grad, pl1, pss = _Guarded(n, dev), _Guarded(nparts, dev), _Guarded(nparts, dev)
    maps = [] if fused else [_Guarded(n, dev) for _ in range(3)]
    with torch.cuda.device(dev):
        st = _capi.current_stream_handle(dev)
        if fused:
            rc = _capi.lib.fdgs_l1_ssim_value_and_grad(img.data_ptr(), gt.data_ptr(), C, H, W, up.data_ptr(), 0.2, grad.ptr, pl1.ptr, pss.ptr, st)
            assert rc == 0
        else:
            rc = _capi.lib.fdgs_l1_ssim_forward(img.data_ptr(), gt.data_ptr(), C, H, W, maps[0].ptr, maps[1].ptr, maps[2].ptr, pl1.ptr, pss.ptr, st)
            assert rc == 0
            rc = _capi.lib.fdgs_l1_ssim_backward(img.data_ptr(), gt.data_ptr(), C, H, W, maps[0].ptr, maps[1].ptr, maps[2].ptr, up.data_ptr(), 0.2, grad.ptr, st)
            assert rc == 0
        torch.cuda.synchronize()
    for i, m in enumerate(maps):
        m.check("derivative map %d" % i)
    g = grad.check("gradient")
    l1, ss = pl1.check("partial_l1"), pss.check("partial_ssim")
    # ... and what was written is the loss: the partial sums and the gradient against ref64
    val = 0.8 * float(l1.double().sum()) / n + 0.2 * (1.0 - float(ss.double().sum()) / n)
    assert abs(val - c.loss64) <= c.bar_v, (val, c.loss64)
    assert float((g.cpu().double().reshape(shape) - UP * c.grad64).abs().max()) <= UP * c.bar_g


# ---- 4. the reduction of the partial sums on its own ---------------------------------------------------------------------------
U = 2.0 ** -24       # unit roundoff of float32
FINISH_CHW = (4, 2048, 2048)     # n = 2^24: inv_n = 2^-24 and the products by it are exact


def _finish_bars(nparts, p64, lam32):
    """(value, bar) for out[1] / out[2] / out[0] from the float64 sums of a [2, nparts] array of partials.  A partial passes through at
    most 7 additions of its thread's tree of 8, one per trip of the 8192-wide loop, 6 of the wave's shuffle tree and 16 over the waves:
    |err| <= that count x 2^-24 x sum|p| x inv_n, plus one rounding of the product by inv_n; the loss adds the roundings of 1 - lambda,
    1 - ssim, two products and a sum."""
    inv_n = 1.0 / (FINISH_CHW[0] * FINISH_CHW[1] * FINISH_CHW[2])
    adds = 7 + -(-nparts // 8192) + 6 + 16
    l1, ss = float(p64[0].sum()) * inv_n, float(p64[1].sum()) * inv_n
    b_l1 = adds * U * float(p64[0].abs().sum()) * inv_n + U * abs(l1)
    b_ss = adds * U * float(p64[1].abs().sum()) * inv_n + U * abs(ss)
    a, b = (1.0 - lam32) * l1, lam32 * (1.0 - ss)
    b_loss = (1.0 - lam32) * b_l1 + lam32 * b_ss + 3.0 * U * (abs(a) + abs(b))
    return (a + b, b_loss), (l1, b_l1), (ss, b_ss)


@pytest.mark.parametrize("nparts", [1, 63, 1024, 8191, 8192, 8193, 16320, 20001])
def test_finish_kernel_against_a_float64_sum(nparts, gpu_device):
    """fdgs_l1_ssim_loss and fdgs_l1_ssim_loss_batch on synthetic positive partials (the kernel does not look at image data): counts
    below, at and above one trip of the 8 x 1024 loop (the largest image the suite runs has 4128 partials; 2704 x 2028 has 16320), a
    wave and a thread's tree partly filled; 64 floats of 1e30 behind each array must not enter the sum (they would, through an index
    past the end); the rows of the batch call are bit-identical to the single calls."""
    from fdgs import _capi
    dev = gpu_device
    C, H, W = FINISH_CHW
    lam = 0.2
    lam32 = float(torch.tensor(lam, dtype=torch.float32))
    V, TAIL = 3, 64
    g = torch.Generator().manual_seed(100 + nparts)
    # [views, 2, nparts]: |x - y| sums up to 50 and ssim sums up to 900 per tile, like tiles of 1024 pixels
    parts = torch.rand(V, 2, nparts, generator=g) * torch.tensor([50.0, 900.0])[None, :, None] + 1e-3
    assert float(parts.min()) > 0.0
    with torch.cuda.device(dev):
        st = _capi.current_stream_handle(dev)
        singles = []
        for v in range(V):
            res = []
            for tail in (1e30, 0.0):       # the same call with the poison behind the arrays and without it
                a = torch.full((2, nparts + TAIL), tail, dtype=torch.float32, device=dev)
                a[:, :nparts] = parts[v].to(dev)
                out = torch.full((3,), float("nan"), dtype=torch.float32, device=dev)
                rc = _capi.lib.fdgs_l1_ssim_loss(a[0].data_ptr(), a[1].data_ptr(), nparts, C, H, W, lam, out.data_ptr(), st)
                assert rc == 0
                torch.cuda.synchronize()
                res.append(out.cpu())
            assert torch.equal(res[0], res[1]), "the sum read past num_partials: %s against %s" % (res[0], res[1])
            singles.append(res[0])
            wants = _finish_bars(nparts, parts[v].double(), lam32)
            for k, (want, bar) in enumerate(wants):
                err = abs(float(res[0][k].double()) - want)
                print("nparts %5d view %d out[%d] = %.9g, float64 %.9g, err %.2e (bar %.2e)" % (nparts, v, k, float(res[0][k]), want, err, bar))
                assert err <= bar, (k, err, bar)
        # the batch call: [V, 2, nparts] contiguous, the poison behind the last view
        buf = torch.full((V * 2 * nparts + TAIL,), 1e30, dtype=torch.float32, device=dev)
        buf[:V * 2 * nparts] = parts.reshape(-1).to(dev)
        outs = torch.full((V + 1, 3), float("nan"), dtype=torch.float32, device=dev)
        rc = _capi.lib.fdgs_l1_ssim_loss_batch(buf.data_ptr(), V, nparts, C, H, W, lam, outs.data_ptr(), st)
        assert rc == 0
        torch.cuda.synchronize()
    outs = outs.cpu()
    for v in range(V):
        assert torch.equal(outs[v], singles[v]), (v, outs[v], singles[v])
    assert torch.isnan(outs[V]).all()      # a row per view, none behind them
    assert len({float(s[0]) for s in singles}) == V


# ---- 5. layouts the Python entry points accept ---------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", PATHS, ids=PATH_IDS)
@pytest.mark.parametrize("layout", ["batch_of_one", "permuted", "float64"])
def test_layouts_of_the_python_entry_points(layout, fused, gpu_device):
    """fused_l1_ssim (autograd; always the pair) and l1_ssim_grad (both paths) on a [1, 3, H, W] image, on a non-contiguous one (a
    permute of [H, W, 3]) and on a float64 one (the entry points call .contiguous() and .float()), at 3x33x31 against the same ref64 and bars."""
    from fdgs import loss as fl
    dev = gpu_device
    c = lc.case("smooth", (3, 33, 31), 0.2)

    def lay(t):
        t = t.to(dev)
        if layout == "batch_of_one":
            return t[None].contiguous()
        if layout == "permuted":
            p = t.permute(1, 2, 0).contiguous().permute(2, 0, 1)
            assert not p.is_contiguous()
            return p
        return t.double()
    img, gt = lay(c.img), lay(c.gt)
    upstream = torch.full((1,), UP, dtype=torch.float32, device=dev)
    fl.ssim_options["fused"] = fused
    try:
        g, handle = fl.l1_ssim_grad(img, gt, 0.2, upstream)
        val = float(fl.l1_ssim_loss(handle))
    finally:
        fl.ssim_options["fused"] = False
    assert g.numel() == c.grad64.numel() and tuple(g.shape[-3:]) == c.shape
    _check(c, val, g.cpu().double(), layout + "/" + PATH_IDS[fused])
    if not fused:
        x = img.clone().requires_grad_(True)
        out = fl.fused_l1_ssim(x, gt, 0.2)
        (out * UP).backward()
        assert x.grad.shape == x.shape and x.grad.dtype == x.dtype
        _check(c, out.item(), x.grad.cpu().double(), layout + "/autograd")
