"""The SSIM loss on the GPU: gsasr_ssim_loss (k_ssim_stats, k_ssim_grad, k_ssim_reduce), gsasr_amd.ssim_loss, and `ssim_weight`
of generate_2D_gaussian_splatting_loss / _batch_loss.

Oracle and bar are those of tests/test_ssim_loss.py: the float64 restatement of the maths on the CPU, and for every input
`4 * e32 + 1e-6 * scale`, e32 being the error of the fp32 torch expression against the same oracle on the same input (scale: |L|
for a loss, the gradient's max-abs for a gradient).  Every check prints the ratio it measured before it asserts.

Shapes: 11 x 11 (one valid pixel), 12 x 27, 37 x 53 (straddles the 32 x 32 tiles in both directions, odd pitch), 75 x 107 and
43 x 139 (3 x 4 and 2 x 5 tiles of the valid map: interior tiles, a second tile row), and a batch of three, (11, 16), (24, 40),
(17, 11), padded to [3, 3, 24, 40] with a target of 29 rows and a gradient of 26; at the end of the entry-point tests, pictures and
canvases with more partials than the reduce kernel has lanes and batches of 2 to 64 samples (every split of its 16 waves).
Inputs: uniform noise, a sinusoid, a near-flat picture, and one with two flat levels 0.7 apart (tests/test_ssim_loss.py).
profiles/ssim_loss_geometry.txt keeps the figures of one run.

End to end the fused call is compared with what a user composes today on the same GPU: the plain step / batch image, the fp32 torch
expression of L1 + SSIM and autograd; the gs_parameters gradients under the project's own bars (tests/test_fused_loss_gpu.py)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)
from test_fused_loss_gpu import check_param_grads, conditioned_target, forced_backward, torch_loss  # noqa: E402
from test_ssim_loss import BATCH_SIZES, KINDS, SHAPES, bar, fp32_error, make_input  # noqa: E402

pytestmark = pytest.mark.gpu
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the MI355X box)"
    return torch.device("cuda:0")


_REFS = {}


def reference(kind, shape, weight=0.8):
    """(x, y, L, gradient, e32 of L, e32 of the gradient) of one single-sample input: computed once, shared, never written"""
    key = (kind, shape, weight)
    if key not in _REFS:
        x, y = make_input(kind, *shape)
        _REFS[key] = (x, y) + fp32_error(x, y, weight)
    return _REFS[key]


def batch_reference(kind, weight=0.8):
    """the batch of three: padded x [3,3,24,40] and y [3,3,29,40] with NaN outside every sample, and per sample (L_b, d L / d x_b,
    e32 of both) with the 1 / B of the batch mean in the gradient"""
    key = ("batch", kind, weight)
    if key not in _REFS:
        B = len(BATCH_SIZES)
        x, y, per = torch.full((B, 3, 24, 40), NAN), torch.full((B, 3, 29, 40), NAN), []
        for b, (h, w) in enumerate(BATCH_SIZES):
            xb, yb = make_input(kind, h, w, seed=b + 1)
            x[b, :, :h, :w], y[b, :, :h, :w] = xb, yb
            per.append(fp32_error(xb, yb, weight, B))
        _REFS[key] = (x, y, per)
    return _REFS[key]


def check(got, want, e32, scale, what):
    err = abs(got - want) if np.isscalar(got) else float((got.double().cpu() - want).abs().max())
    print(f"{what}: error {err:.3e}, e32 {e32:.3e}, ratio to e32 {err / max(e32, 1e-30):.2f}, bar {bar(e32, scale):.3e}")
    assert err <= bar(e32, scale), (what, err, e32, scale)


def own_pixels_mask(rows, hwc):
    m = torch.zeros(len(BATCH_SIZES), 3, rows, 40, dtype=torch.bool)
    for b, (h, w) in enumerate(BATCH_SIZES):
        m[b, :, :h, :w] = True
    return m.permute(0, 2, 3, 1).contiguous() if hwc else m


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_entry_point_single_sample(shape, kind, dev):
    from gsasr_amd import _cabi
    x, y, L, g64, e_loss, e_grad = reference(kind, shape)
    xd, yd = x.to(dev), y.to(dev)
    gmax = float(g64.abs().max())
    loss, grad = _cabi.ssim_loss(xd, yd, None, 0.8)
    assert tuple(loss.shape) == (2,) and float(loss[0]) == float(loss[1])
    check(float(loss[0]), L, e_loss, abs(L), f"{kind} {shape} loss")
    check(grad, g64, e_grad, gmax, f"{kind} {shape} planar gradient")
    _, hwc = _cabi.ssim_loss(xd, yd, None, 0.8, hwc=True)
    assert tuple(hwc.shape) == shape + (3,)
    check(hwc.permute(2, 0, 1), g64, e_grad, gmax, f"{kind} {shape} interleaved gradient")
    # the value alone, and a second call: the same bits
    only, none = _cabi.ssim_loss(xd, yd, None, 0.8, want_grad=False)
    again, grad2 = _cabi.ssim_loss(xd, yd, None, 0.8)
    assert none is None and torch.equal(bits(only), bits(loss)) and torch.equal(bits(again), bits(loss))
    assert torch.equal(bits(grad2), bits(grad))
    # accumulate: buffer + the stored result, to one rounding
    for layout, stored in ((False, grad), (True, hwc)):
        buf = torch.randn(stored.shape, generator=torch.Generator().manual_seed(5)).to(dev) * gmax
        acc = buf.clone()
        _cabi.ssim_loss(xd, yd, None, 0.8, grad=acc, hwc=layout, accumulate=True)
        slack = 1.2e-7 * (buf.abs() + stored.abs())
        assert bool(((acc - (buf + stored)).abs() <= slack).all()), (kind, shape, layout)


@pytest.mark.parametrize("hwc", [False, True], ids=["planar", "interleaved"])
@pytest.mark.parametrize("kind", KINDS)
def test_entry_point_padded_batch_never_touches_the_padding(kind, hwc, dev):
    """image, target and gradient padding hold NaN: the losses are finite and right per sample, the gradient is right on every
    sample's own pixels, and its padding is NaN bit for bit after a store and after an accumulate."""
    from gsasr_amd import _cabi
    x, y, per = batch_reference(kind)
    B, grows = len(BATCH_SIZES), 26
    xd, yd = x.to(dev), y.to(dev)
    own = own_pixels_mask(grows, hwc).to(dev)
    shape = (B, grows, 40, 3) if hwc else (B, 3, grows, 40)
    grad = torch.full(shape, NAN, device=dev)
    before = bits(grad)
    loss, _ = _cabi.ssim_loss(xd, yd, BATCH_SIZES, 0.8, grad=grad, hwc=hwc)
    assert tuple(loss.shape) == (1 + B,) and bool(torch.isfinite(loss).all())
    total = sum(p[0] for p in per) / B
    check(float(loss[0]), total, sum(p[2] for p in per) / B, abs(total), f"{kind} batch loss")
    assert bool(torch.isfinite(grad[own]).all()) and torch.equal(bits(grad)[~own.cpu()], before[~own.cpu()])
    planar = grad.permute(0, 3, 1, 2) if hwc else grad
    for b, (h, w) in enumerate(BATCH_SIZES):
        L, g64, e_loss, e_grad = per[b]
        check(float(loss[1 + b]), L, e_loss, abs(L), f"{kind} sample {b} loss")
        check(planar[b, :, :h, :w], g64, e_grad, float(g64.abs().max()), f"{kind} sample {b} gradient")
    buf = torch.where(own, torch.randn(shape, generator=torch.Generator().manual_seed(6)).to(dev) * 1e-3, torch.full(shape, NAN, device=dev))
    acc = buf.clone()
    again, _ = _cabi.ssim_loss(xd, yd, BATCH_SIZES, 0.8, grad=acc, hwc=hwc, accumulate=True)
    assert torch.equal(bits(again), bits(loss))
    assert torch.equal(bits(acc)[~own.cpu()], bits(buf)[~own.cpu()])
    assert bool(((acc[own] - (buf[own] + grad[own])).abs() <= 1.2e-7 * (buf[own].abs() + grad[own].abs())).all())


def test_ssim_loss_autograd_with_an_upstream_scalar(dev):
    from gsasr_amd import ssim_loss
    x, y, per = batch_reference("noise", 0.6)
    B = len(BATCH_SIZES)
    xd = torch.nan_to_num(x).to(dev).requires_grad_(True)          # (autograd hands the padding's zero gradient on: no NaN in the leaf)
    value = ssim_loss(xd, torch.nan_to_num(y).to(dev), 0.6, BATCH_SIZES)
    assert value.dim() == 0 and value.requires_grad
    (2.5 * value).backward()
    for b, (h, w) in enumerate(BATCH_SIZES):
        L, g64, _, e_grad = per[b]
        check(xd.grad[b, :, :h, :w], 2.5 * g64, 2.5 * e_grad, 2.5 * float(g64.abs().max()), f"2.5 x sample {b} gradient")
        assert not xd.grad[b, :, h:].any() and not xd.grad[b, :, :, w:].any()      # the padding's gradient is zero
    total = sum(p[0] for p in per) / B
    check(float(value.detach()), total, sum(p[2] for p in per) / B, abs(total), "batch loss")
    # a single image, no gradient asked for
    x1, y1, L1, _, e1, _ = reference("smooth", (37, 53), 0.6)
    with torch.no_grad():
        check(float(ssim_loss(x1.to(dev), y1.to(dev), 0.6)), L1, e1, abs(L1), "single image under no_grad")
    with pytest.raises(ValueError, match="require grad"):
        ssim_loss(xd, y.to(dev).requires_grad_(True), 0.6, BATCH_SIZES)


# ---- end to end: ssim_weight of the fused loss against the composed path of today -----------------------------------------
SCALE = 2.0
WINDOWS = [(0, 2, 11, 13), (5, 7, 16, 30), (3, 0, 12, 11)]


def composed(img_of, p, targets, hw, ssim_weight):
    """the plain image(s) + the fp32 torch expression of L1 + SSIM + autograd, on the GPU"""
    from gsasr_amd import ssim as ssim_mod
    q = p.detach().clone().requires_grad_(True)
    out = img_of(q)
    if out.dim() == 3:
        out, targets = out[None], targets[None]
    pix = [torch_loss(out[b, :, :h, :w], targets[b, :, :h, :w], "l1", 1.0, 1e-12, "mean") for b, (h, w) in enumerate(hw)]
    ssm = [ssim_mod.ssim_torch(out[b, :, :h, :w], targets[b, :, :h, :w], ssim_weight) for b, (h, w) in enumerate(hw)]
    l_pix, l_ssim = sum(pix) / len(hw), sum(ssm) / len(hw)
    (l_pix + l_ssim).backward()
    return l_pix.detach(), l_ssim.detach(), q.grad, out.detach()


def check_terms(got_pix, got_ssim, total, want_pix, image, targets, hw, ssim_weight, what):
    """l_pix under the fused pixel loss' own bar (2e-5 relative); l_ssim under the SSIM bar against the float64 oracle on the image
    the call returned; the total is their fp32 sum"""
    if image.dim() == 3:
        image, targets = image[None], targets[None]
    assert abs(float(got_pix) - float(want_pix)) <= 2e-5 * abs(float(want_pix)), what
    refs = [fp32_error(image[b, :, :h, :w].cpu(), targets[b, :, :h, :w].cpu(), ssim_weight) for b, (h, w) in enumerate(hw)]
    L = sum(r[0] for r in refs) / len(hw)
    check(float(got_ssim), L, sum(r[2] for r in refs) / len(hw), abs(L), what + " l_ssim")
    assert abs(float(total) - (float(got_pix) + float(got_ssim))) <= 2.4e-7 * abs(float(total)), what


def same_value(a, b):
    """two renderings of one image add their terms in the order the plan binned them: the loss value's own bar, 2e-5 relative"""
    return abs(float(a.detach()) - float(b.detach())) <= 2e-5 * abs(float(b.detach()))


@pytest.mark.parametrize("kernel", ["gaussian", "tile", "home"])
def test_fused_single_image_and_window(kernel, dev):
    from gsasr_amd import gaussian_splatting as gsp, synthetic
    H, W = 24, 40
    p = synthetic.gs_parameters(12, 20, seed=31).to(dev).requires_grad_(True)
    with forced_backward(kernel):
        for window in (None, (5, 7, 16, 30)):
            hw = [(H, W) if window is None else window[2:]]
            img_of = (lambda q: gsp.generate_2D_gaussian_splatting_step((H, W), q, SCALE, (SCALE, SCALE), dmax=0.3)) if window is None else \
                (lambda q: gsp.generate_2D_gaussian_splatting_view((H, W), q, SCALE, (SCALE, SCALE), window, dmax=0.3))
            with torch.no_grad():
                t = conditioned_target(img_of(p), 13)
            want_pix, want_ssim, want_g, _ = composed(img_of, p, t, hw, 0.5)
            p.grad = None
            value, image, (l_pix, l_ssim) = gsp.generate_2D_gaussian_splatting_loss(
                (H, W), p, SCALE, (SCALE, SCALE), t, loss="l1", window=window, dmax=0.3, return_image=True, ssim_weight=0.5, return_terms=True)
            assert value.dim() == 0 and value.requires_grad and not l_pix.requires_grad and not l_ssim.requires_grad
            value.backward()
            what = f"{kernel} window={window}"
            check_terms(l_pix, l_ssim, value.detach(), want_pix, image, t, hw, 0.5, what)
            check_param_grads(p.grad, want_g, p, what)
            with torch.no_grad():       # a forward-only plan: the value alone
                quiet = gsp.generate_2D_gaussian_splatting_loss((H, W), p, SCALE, (SCALE, SCALE), t, loss="l1", window=window, dmax=0.3,
                                                                ssim_weight=0.5)
            assert not quiet.requires_grad and same_value(quiet, value)
            plain = gsp.generate_2D_gaussian_splatting_loss((H, W), p, SCALE, (SCALE, SCALE), t, loss="l1", window=window, dmax=0.3)
            assert same_value(plain, l_pix)         # ssim_weight = 0: the call of before, and the same pixel term
    gsp.deferred_asserts.flush()


@pytest.mark.parametrize("kernel", ["gaussian", "tile", "home"])
def test_fused_batch_and_batched_windows(kernel, dev):
    from gsasr_amd import gaussian_splatting as gsp, synthetic
    B = len(BATCH_SIZES)
    p = torch.stack([synthetic.gs_parameters(12, 20, seed=40 + b) for b in range(B)]).to(dev).requires_grad_(True)
    scales, sms = [SCALE] * B, [(SCALE, SCALE)] * B
    with forced_backward(kernel):
        for windows in (None, WINDOWS):
            hw = BATCH_SIZES if windows is None else [w[2:] for w in windows]
            img_of = lambda q: gsp.generate_2D_gaussian_splatting_batch(BATCH_SIZES, q, scales, sms, windows=windows, dmax=0.3)  # noqa: E731
            with torch.no_grad():
                t = conditioned_target(img_of(p), 17)
            if windows is None:     # the padded ground truth: more rows than the tallest sample
                t = torch.cat([t, torch.full((B, 3, 5, t.shape[3]), NAN, device=dev)], 2)
            want_pix, want_ssim, want_g, _ = composed(img_of, p, t, hw, 0.5)
            p.grad = None
            value, per, images, (l_pix, l_ssim) = gsp.generate_2D_gaussian_splatting_batch_loss(
                BATCH_SIZES, p, scales, sms, t, loss="l1", windows=windows, dmax=0.3, return_per_sample=True, return_images=True,
                ssim_weight=0.5, return_terms=True)
            assert value.dim() == 0 and value.requires_grad and tuple(per.shape) == (B,) and not per.requires_grad
            value.backward()
            what = f"{kernel} batch windows={windows is not None}"
            check_terms(l_pix, l_ssim, value.detach(), want_pix, images, t, hw, 0.5, what)
            assert abs(float(per.mean()) - float(value.detach())) <= 1e-6 * abs(float(value.detach()))
            check_param_grads(p.grad, want_g, p, what)
            with torch.no_grad():
                quiet = gsp.generate_2D_gaussian_splatting_batch_loss(BATCH_SIZES, p, scales, sms, t, loss="l1", windows=windows, dmax=0.3,
                                                                      ssim_weight=0.5)
            assert not quiet.requires_grad and same_value(quiet, value)
    gsp.deferred_asserts.flush()


def test_fused_per_sample_path_and_argument_errors(dev):
    """a batch of one goes through the single-sample call: the same rules; and the errors come before any launch"""
    from gsasr_amd import gaussian_splatting as gsp, synthetic
    B = len(BATCH_SIZES)
    p = torch.stack([synthetic.gs_parameters(12, 20, seed=50 + b) for b in range(B)]).to(dev).requires_grad_(True)
    scales, sms = [SCALE] * B, [(SCALE, SCALE)] * B
    t = torch.rand(B, 3, 24, 40, device=dev)
    kw = dict(loss="l1", ssim_weight=0.5, return_terms=True, return_per_sample=True)
    fused, per_f, _ = gsp.generate_2D_gaussian_splatting_batch_loss(BATCH_SIZES, p, scales, sms, t, dmax=0.3, **kw)
    loop, per_l, (pix_l, ssm_l) = gsp.generate_2D_gaussian_splatting_batch_loss(BATCH_SIZES[1:2], p[1:2], scales[1:2], sms[1:2], t[1:2], dmax=0.3, **kw)
    assert loop.requires_grad and abs(float(per_l[0]) - float(per_f[1])) <= 2e-5 * abs(float(per_f[1]))     # B = 1: the per-sample path
    assert abs(float(pix_l) + float(ssm_l) - float(loop.detach())) <= 2.4e-7 * abs(float(loop.detach()))
    with pytest.raises(ValueError, match="smaller than"):
        gsp.generate_2D_gaussian_splatting_batch_loss(BATCH_SIZES, p, scales, sms, t, windows=[(0, 0, 11, 11), (0, 0, 10, 30), (0, 0, 11, 11)],
                                                      ssim_weight=0.5)
    with pytest.raises(ValueError, match="reduction"):
        gsp.generate_2D_gaussian_splatting_loss((24, 40), p[0], SCALE, (SCALE, SCALE), t[0], reduction="sum", ssim_weight=0.5)


# ---- more than 2 x 2 tiles, more than 16 samples, more than one trip of the reduce loops -----------------------------------
# Until here every picture was at most 37 x 53 (a valid map of 27 x 43: no tile of k_ssim_stats with ty0 > 0, none with a
# neighbour on all four sides), every canvas one tile, every batch three samples (wps = 4).  SHAPES now holds 75 x 107 (3 x 4
# tiles of the map, interior ones in both kernels) and 43 x 139 (a second tile row of ONE map row), so the tests above run them
# with every kind, "two-level" included.  Below: what the shapes alone do not reach.
def canvas_reference(B, cycle, rows, w, trows, weight=0.8):
    """a canvas of B samples whose sizes cycle through `cycle`, kinds through KINDS and seeds through 0..4: x [B,3,rows,w] and y
    [B,3,trows,w] with NaN outside every sample, and per sample (L_b, d L / d x_b, e32 of both) with the 1 / B of the batch mean
    in the gradient.  One float64 reference per distinct (kind, size, seed, B), shared through _REFS."""
    sizes = [cycle[b % len(cycle)] for b in range(B)]
    x, y, per = torch.full((B, 3, rows, w), NAN), torch.full((B, 3, trows, w), NAN), []
    for b, (h, ww) in enumerate(sizes):
        kind, seed = KINDS[b % len(KINDS)], b % 5
        xb, yb = make_input(kind, h, ww, seed=seed)
        x[b, :, :h, :ww], y[b, :, :h, :ww] = xb, yb
        key = ("sample", kind, (h, ww), seed, weight, B)
        if key not in _REFS:
            _REFS[key] = fp32_error(xb, yb, weight, B)
        per.append(_REFS[key])
    return sizes, x, y, per


def check_canvas(B, sizes, x, y, per, grows, hwc, dev, what):
    """the checks of test_entry_point_padded_batch_never_touches_the_padding on any canvas"""
    from gsasr_amd import _cabi
    rows, w = x.shape[2], x.shape[3]
    xd, yd = x.to(dev), y.to(dev)
    own = torch.zeros(B, 3, grows, w, dtype=torch.bool)
    for b, (h, ww) in enumerate(sizes):
        own[b, :, :h, :ww] = True
    own = (own.permute(0, 2, 3, 1).contiguous() if hwc else own).to(dev)
    shape = (B, grows, w, 3) if hwc else (B, 3, grows, w)
    grad = torch.full(shape, NAN, device=dev)
    before = bits(grad)
    loss, _ = _cabi.ssim_loss(xd, yd, sizes, 0.8, grad=grad, hwc=hwc)
    assert tuple(loss.shape) == (1 + B,) and bool(torch.isfinite(loss).all()), what
    total = sum(p[0] for p in per) / B
    check(float(loss[0]), total, sum(p[2] for p in per) / B, abs(total), f"{what} loss")
    # ... and loss[0] is the mean of the per-sample values the call itself returned, formed in double and rounded once
    assert abs(float(loss[0]) - float(loss[1:].double().mean())) <= 1.2e-7 * abs(total), what
    assert bool(torch.isfinite(grad[own]).all()) and torch.equal(bits(grad)[~own.cpu()], before[~own.cpu()]), what
    planar = grad.permute(0, 3, 1, 2) if hwc else grad
    for b, (h, ww) in enumerate(sizes):
        L, g64, e_loss, e_grad = per[b]
        check(float(loss[1 + b]), L, e_loss, abs(L), f"{what} sample {b} {KINDS[b % len(KINDS)]} {h}x{ww} loss")
        check(planar[b, :, :h, :ww], g64, e_grad, float(g64.abs().max()), f"{what} sample {b} {KINDS[b % len(KINDS)]} {h}x{ww} gradient")
    buf = torch.where(own, torch.randn(shape, generator=torch.Generator().manual_seed(6)).to(dev) * 1e-3, torch.full(shape, NAN, device=dev))
    acc = buf.clone()
    again, _ = _cabi.ssim_loss(xd, yd, sizes, 0.8, grad=acc, hwc=hwc, accumulate=True)
    assert torch.equal(bits(again), bits(loss)), what
    assert torch.equal(bits(acc)[~own.cpu()], bits(buf)[~own.cpu()]), what
    assert bool(((acc[own] - (buf[own] + grad[own])).abs() <= 1.2e-7 * (buf[own].abs() + grad[own].abs())).all()), what


def test_reduce_second_trip_of_the_lane_loop_one_sample(dev):
    """618 x 586: a valid map of 19 x 18 tiles, 3 * 342 = 1026 partials for the 1024 lanes of wps = 16 -- two lanes of
    k_ssim_reduce take a second trip; and tiles that are interior many times over"""
    from gsasr_amd import _cabi
    shape = (618, 586)
    x, y, L, g64, e_loss, e_grad = reference("smooth", shape)
    assert 3 * ((shape[0] - 10 + 31) // 32) * ((shape[1] - 10 + 31) // 32) == 1026
    loss, grad = _cabi.ssim_loss(x.to(dev), y.to(dev), None, 0.8)
    check(float(loss[0]), L, e_loss, abs(L), f"smooth {shape} loss")
    check(grad, g64, e_grad, float(g64.abs().max()), f"smooth {shape} planar gradient")
    only, _ = _cabi.ssim_loss(x.to(dev), y.to(dev), None, 0.8, want_grad=False)
    assert torch.equal(bits(only), bits(loss))


NINE = [(170, 170), (11, 11), (43, 160), (75, 107), (160, 43)]


def test_reduce_second_trip_of_the_lane_loop_one_wave_per_sample(dev):
    """nine samples in [9,3,170,170]: wps = 1, and 3 * 25 = 75 partials per sample for the 64 lanes of its one wave"""
    sizes, x, y, per = canvas_reference(9, NINE, 170, 170, 170)
    assert 3 * ((170 - 10 + 31) // 32) ** 2 == 75
    check_canvas(9, sizes, x, y, per, 170, False, dev, "nine in 170x170")


RAGGED = [(75, 107), (11, 11), (11, 107), (75, 11), (43, 80), (33, 65)]


@pytest.mark.parametrize("hwc", [False, True], ids=["planar", "interleaved"])
@pytest.mark.parametrize("B", [2, 5, 9, 17, 64])
def test_every_wave_split_of_the_reduce_and_padding_tiles(B, hwc, dev):
    """B = 2, 5, 9, 17, 64 in a [B,3,75,107] canvas (3 x 4 tiles; a target of 80 rows, a gradient of 78): wps = 8, 2, 1, 1, 1, and
    from B = 17 on the second to fourth trip of `b += 16 / wps`.  Most samples leave whole tiles of the canvas to the padding
    (the zero partial of k_ssim_stats, the early return of k_ssim_grad); image, target and gradient hold NaN there."""
    sizes, x, y, per = canvas_reference(B, RAGGED, 75, 107, 80)
    check_canvas(B, sizes, x, y, per, 78, hwc, dev, f"B={B}")
