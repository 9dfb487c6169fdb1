"""The scratch areas of the ops around the rasterizer at exactly their declared size, between guards, on garbage.

The companion of tests/test_workspace_bounds_gpu.py (which holds the plan, step and sample workspaces, and through the step
entry points the scratch of gsasr_step_forward_loss): the `*_scratch_bytes` functions of the fused pixel loss, the SSIM loss, the
validation metrics and the six window-attention families.  Every scratch is the middle of a `GuardedBytes` (tests/wsguard.py) of
exactly the bytes the sizing function returns, starts from 0xFF bytes, from zeros and from seeded random bytes, and the op is held
to the float64 restatement and the bar of its own test module:

  fused pixel loss   tests/test_fused_loss_gpu.py::check_store: the loss within 1e-5 of loss_f64 on the stored image, the gradient
                     within 1e-6 of the fp32 expression's max-abs, the stored image within IMG_ATOL of the oracle
  SSIM loss          tests/test_ssim_loss_gpu.py::check (4 e32 + 1e-6 scale against tests/test_ssim_loss.py's float64 maths)
  metrics            tests/test_metrics_gpu.py::check (BAR_PSNR_RGB, BAR_PSNR_Y, BAR_SSIM against tests/test_metrics.py)
  window attention   tests/test_window_attention.py::held (4 e + 1e-6 scale) against the float64 torch expression, e from the
                     yardsticks of test_window_attention_gpu / _rope_gpu / _bf16_gpu / _masked_gpu / _masked_bf16_gpu

Across the three fills the results agree BIT FOR BIT where include/gsasr_splat.h says two calls give the same bits: the fused loss
on one plan ("two calls on one plan give the same bits": held wherever the forward repeats its pixels bit for bit, which the
search kernels do not where Gaussians overlap -- see check_loss), the SSIM loss and its gradient ("two calls give the same bits"), the
metrics ("two calls on the same inputs give the same bits"), the attention's out, g_q, g_k, g_v and the rotary g_angles ("written
once ... two calls give the same bits"); g_table is the exception the header names ("its last bits may differ between two calls"):
the bar alone.

The descriptors of these ops carry a scratch POINTER and no size, so the C ABI cannot refuse a scratch that is one byte short;
the ctypes wrappers can, and do (a RuntimeError, nothing written).  The attention sizes are never 0 (256 bytes at the least): a
backward that needs no scratch gets those 256 bytes and must leave them alone.

gsasr_resize_scratch_bytes and gsasr_batch_scratch_bytes are held by tests/test_imresize_wide_gpu.py and
tests/test_make_batch_gpu.py, which run the same fills.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from test_workspace_bounds_gpu import IMG_ATOL, F, _t, lr_scene, order_bar, padded, px_scene
from wsguard import FILLS, GuardedBytes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the MI355X box)"
    return torch.device("cuda:0")


def slack_of(guards):
    n = guards[0].n
    return n - 1 - max(a.highest_written(b) for a in guards for b in guards if a.fill != b.fill)


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32) if t.dtype == torch.float32 else t


def short_scratch_is_refused(call, g, drop):
    """`call(scratch)` with `drop` bytes less than the op needs: the wrapper raises and nothing is written"""
    before = g.buf.clone()
    with pytest.raises(RuntimeError, match="scratch"):
        call(g.mid[:g.n - drop])
    torch.cuda.synchronize()
    assert torch.equal(g.buf, before)


def guard_that_starts_early_reports(run, n, dev, fill="zero", early=256):
    """`run(scratch)` on n bytes of which the helper believes the last `early` to be guard: it must report them changed"""
    g = GuardedBytes(n - early, dev, fill, seed=9)
    run(g.span(n))
    torch.cuda.synchronize()
    c = g.intact()
    assert not c and n - early <= c.first <= c.last <= n - 1, repr(c)
    return c


# ---- gsasr_loss_scratch_bytes / gsasr_splat_forward_loss -----------------------------------------------------------------------
# forward kernels the loss can run behind AT THESE SIZES (the one-wave-per-sub-tile search, the list tile forms and the dense
# default of tests/test_u8_output_gpu.py's KERNELS need thousands of sub-tiles or tiles: images of 512 px and more):
# name -> (dense, forward flag, list_cap); dense = one record per four pixels (NaN records pad the list: a dense plan is a
# matter of the count), which selects the record-pair kernels
LOSS_KERNELS = {
    "narrow-search": (False, "FWD_NARROW", -1),
    "narrow-lists": (False, "FWD_NARROW", 64),
    "wide-search": (False, "FWD_WIDE", -1),
    "wide-lists": (False, "FWD_WIDE", 64),
    "split-pairs": (True, "FWD_NARROW", -1),
    "lists-pairs": (True, "FWD_NARROW", 64),
}
LOSS_SIZES = [(50, 70), (130, 34)]         # h x w: multiples of neither 8 nor 16 in either direction
LOSS_CANVAS = [(50, 70), (34, 50), (20, 66)]
LOSS_DMAX = 0.2


def sep_dmax(side=70):
    """boxes of at most 5 px each way on grids of up to `side` pixels; centres 12 px apart: one term per pixel"""
    return 10.0 / (side - 1)


def sep_scene(h, w, seed):
    """Gaussians of 1 - 1.5 px std on a 12-px lattice (jittered by half a pixel): under sep_dmax() their boxes do not overlap"""
    rng = np.random.default_rng(seed)
    cy, cx = np.meshgrid(np.arange(6.0, h - 1, 12.0), np.arange(6.0, w - 1, 12.0), indexing="ij")
    n = cy.size
    return px_scene(h, w, cx.ravel() + rng.uniform(-0.5, 0.5, n), cy.ravel() + rng.uniform(-0.5, 0.5, n), rng.uniform(1.0, 1.5, (n, 2)),
                    seed, colour=(0.2, 0.8))


def loss_scene(h, w, dense, seed, separated=False):
    smp = sep_scene(h, w, seed) if separated else lr_scene(h, w, seed)
    return padded(smp, (h * w + 3) // 4 + 8) if dense else smp


def loss_reference(stored, target, kind, weight, eps, c):
    """test_fused_loss_gpu.check_store's yardsticks on the stored image: (loss_f64's value, the fp32 gradient expression)"""
    from test_fused_loss import loss_f64
    from test_fused_loss_gpu import torch_grad
    ref, _ = loss_f64(stored.cpu().numpy(), target.cpu().numpy(), kind, weight, eps, "mean")
    return ref, torch_grad(stored, target, kind, c, eps)


def check_loss(plan, flag, sizes, refs, dev, what, exact):
    """every kind of loss on `plan` with the scratch between guards, three fills: values against check_store's bars, the image
    against the oracle, bits equal across the fills; returns the scratch size and slack"""
    from gsasr_amd import _cabi
    from test_fused_loss_gpu import coef
    d = plan.dims
    B = max(int(d.batch), 1)
    n = int(_cabi.lib().gsasr_loss_scratch_bytes(ctypes.byref(d)))
    assert n > 0 and n % 4 == 0
    rows = d.slot if B > 1 else d.h
    target = torch.rand(B, 3, rows + 2, d.w, generator=torch.Generator().manual_seed(d.h + d.w)).to(dev)      # (taller than needed)
    if B == 1:
        target = target[0, :, :rows].contiguous()
    worst = dict(loss=0.0, grad=0.0, image=0.0)
    guards_all, same_pixels = [], 0
    for kind in ("mse", "charbonnier"):
        weight, eps = 0.75, 1e-6
        guards, results = [], []
        for fill in FILLS:
            g = GuardedBytes(n, dev, fill, seed=len(what))
            loss, grad, img = _cabi.forward_loss(plan, target, _cabi.LOSS_KINDS[kind], 0, weight, eps, chw=True, grad_chw=True,
                                                 want_image=True, flags=flag, scratch=g.mid.view(torch.float32))
            torch.cuda.synchronize()
            g.check(f"{what} {kind}/{fill}")
            guards.append(g)
            results.append((loss, grad, img))
            img = img.reshape(B, 3, rows, d.w)
            grad = grad.reshape(B, 3, rows, d.w)
            tgt = target.reshape(B, 3, -1, d.w)
            total = 0.0
            for b, (h, w) in enumerate(sizes):
                got = img[b, :, :h, :w]
                err = float(np.abs(got.permute(1, 2, 0).cpu().numpy().astype(np.float64) - refs[b]).max())
                worst["image"] = max(worst["image"], err)
                assert err <= IMG_ATOL, (what, kind, fill, b, err)
                ref, want = loss_reference(got, tgt[b, :, :h, :w], kind, weight, eps, coef(weight, h, w, B))
                rel = abs(float(loss[1 + b]) - ref) / ref
                gerr = float((grad[b, :, :h, :w] - want).abs().max()) / float(want.abs().max())
                worst["loss"], worst["grad"] = max(worst["loss"], rel), max(worst["grad"], gerr)
                assert rel <= 1e-5 and gerr <= 1e-6, (what, kind, fill, b, rel, gerr)
                total += ref / B
            assert abs(float(loss[0]) - total) <= 1e-5 * total, (what, kind, fill)
        own = torch.zeros(B, 3, rows, d.w, dtype=torch.bool)
        for b, (h, w) in enumerate(sizes):
            own[b, :, :h, :w] = True
        own = own.reshape(results[0][1].shape)
        for other in results[1:]:
            # One plan: the partials are added in a fixed order, so the same pixels give the same bits of loss and gradient.  The
            # pixels themselves are not always the same bits where Gaussians overlap: a pixel's terms are added in an order that
            # follows wave timing (tests/test_view_gpu.py) -- measured here on narrow-search, wide-search and, on the canvas,
            # split-pairs.  Then everything agrees to the bar for sums in another order; the scenes of separated Gaussians
            # (`exact`) always take the first branch
            if torch.equal(bits(other[2]), bits(results[0][2])):
                same_pixels += 1
                assert torch.equal(bits(other[0]), bits(results[0][0])), (what, kind, "loss")
                assert torch.equal(bits(other[1])[own], bits(results[0][1])[own]), (what, kind, "gradient")
            else:
                for x, y, name in zip(other, results[0], ("loss", "gradient", "image")):
                    x, y = (x[own], y[own]) if name == "gradient" else (x, y)
                    err = float((x - y).abs().max())
                    assert err <= order_bar(y.cpu().numpy()), (what, kind, name, err)
        guards_all.append(guards)
    slack = min(slack_of(g) for g in guards_all)
    print(f"{what}: the same pixel bits as the first fill in {same_pixels} of 4 repeated calls")
    # `exact`: Gaussians whose boxes do not overlap, one term per pixel -- every kernel repeats its pixels, so every repeated call
    # went through the bit-for-bit branch above: the fixed-order reduction is exact
    assert same_pixels == 4 or not exact, f"{what}: only {same_pixels} of 4 repeated calls gave the same pixels"
    print(f"{what}: loss scratch n = {n}, slack = {slack}; loss rel err {worst['loss']:.3e} (bar 1e-5), gradient {worst['grad']:.3e} of "
          f"max-abs (bar 1e-6), image max|err| {worst['image']:.3e} (bar {IMG_ATOL:.0e})")
    g = GuardedBytes(n, dev, "seeded")
    short_scratch_is_refused(lambda s: _cabi.forward_loss(plan, target, 1, 0, 0.75, 1e-6, chw=True, grad_chw=True, flags=flag,
                                                           scratch=s.view(torch.float32)), g, 4)
    return n, slack


@functools.lru_cache(maxsize=None)
def loss_oracle(h, w, seed, separated=False):
    from oracle import gs_oracle
    smp = sep_scene(h, w, seed) if separated else lr_scene(h, w, seed)
    ref = gs_oracle.forward_f64(smp.sig, smp.xy, smp.col, h, w, sep_dmax(max(h, w, 70)) if separated else LOSS_DMAX)
    assert float(np.abs(ref).max()) > 0.1
    return ref


@pytest.mark.parametrize("size", LOSS_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", list(LOSS_KERNELS))
def test_loss_scratch_single_image(name, size, dev):
    from gsasr_amd import _cabi
    dense, fwd, cap = LOSS_KERNELS[name]
    h, w = size
    smp = loss_scene(h, w, dense, 70)
    plan = _cabi.plan(_t(smp.sig, dev), _t(smp.xy, dev), _t(smp.col, dev), h, w, LOSS_DMAX, flags=F(fwd), list_cap=cap)
    assert _cabi.forward_subtile_width(plan, F(fwd)) == (16 if fwd == "FWD_WIDE" else 8)
    n, slack = check_loss(plan, F(fwd), [(h, w)], [loss_oracle(h, w, 70)], dev, f"loss {name} {h}x{w}", False)
    # ... and the same kernel on Gaussians that do not overlap: the same bits from every call
    sep = loss_scene(h, w, dense, 71, separated=True)
    sep_plan = _cabi.plan(_t(sep.sig, dev), _t(sep.xy, dev), _t(sep.col, dev), h, w, sep_dmax(max(h, w, 70)), flags=F(fwd), list_cap=cap)
    assert _cabi.forward_subtile_width(sep_plan, F(fwd)) == (16 if fwd == "FWD_WIDE" else 8)
    check_loss(sep_plan, F(fwd), [(h, w)], [loss_oracle(h, w, 71, True)], dev, f"loss {name} {h}x{w} separated", True)
    if name == "narrow-search" and size == LOSS_SIZES[0]:      # can this file fail?  the last partial is written: a guard that
        run = lambda s: _cabi.forward_loss(plan, torch.zeros(3, h, w, device=dev), 1, 0, 1.0, 1e-6, chw=True, flags=F(fwd),      # noqa: E731
                                           scratch=s.view(torch.float32))
        early = 4 * ((slack + 4) // 4 + 1)                      # starts inside the written part must report it
        print(f"loss {name}: a guard {early} bytes early: {guard_that_starts_early_reports(run, n, dev, early=early)!r}")


@pytest.mark.parametrize("name", ["narrow-search", "narrow-lists", "split-pairs"])
def test_loss_scratch_canvas_of_three(name, dev):
    from gsasr_amd import _cabi
    dense, fwd, cap = LOSS_KERNELS[name]
    smps = [lr_scene(h, w, 80 + b) for b, (h, w) in enumerate(LOSS_CANVAS)]
    n_per = max(max(s.sig.shape[0] for s in smps), max((h * w + 3) // 4 + 8 for h, w in LOSS_CANVAS) if dense else 0)
    smps = [padded(s, n_per) for s in smps]
    inputs = [_t(np.concatenate([getattr(s, k) for s in smps]), dev) for k in ("sig", "xy", "col")]
    plan = _cabi.plan(*inputs, 0, 0, LOSS_DMAX, flags=F(fwd), list_cap=cap, sizes=LOSS_CANVAS)
    refs = [loss_oracle(h, w, 80 + b) for b, (h, w) in enumerate(LOSS_CANVAS)]
    check_loss(plan, F(fwd), LOSS_CANVAS, refs, dev, f"loss {name} canvas of 3", False)
    seps = [padded(sep_scene(h, w, 90 + b), n_per) for b, (h, w) in enumerate(LOSS_CANVAS)]
    inputs = [_t(np.concatenate([getattr(s, k) for s in seps]), dev) for k in ("sig", "xy", "col")]
    sep_plan = _cabi.plan(*inputs, 0, 0, sep_dmax(), flags=F(fwd), list_cap=cap, sizes=LOSS_CANVAS)
    refs = [loss_oracle(h, w, 90 + b, True) for b, (h, w) in enumerate(LOSS_CANVAS)]
    check_loss(sep_plan, F(fwd), LOSS_CANVAS, refs, dev, f"loss {name} canvas of 3 separated", True)


# ---- gsasr_ssim_scratch_bytes / gsasr_ssim_loss --------------------------------------------------------------------------------
def ssim_size(B, rows, w, sizes, trows, want_grad, hwc):
    from gsasr_amd import _cabi
    d = _cabi.make_ssim(B, rows, w, sizes, trows, 0, 0.8, _cabi.SSIM_GRAD_HWC if hwc else 0)
    d.grad_img = 256 if want_grad else None          # (only looked at)
    d.img = d.target = 256
    n = int(_cabi.lib().gsasr_ssim_scratch_bytes(ctypes.byref(d)))
    assert n > 0 and n % 4 == 0
    return n


SSIM_FORMS = [(False, False), (True, False), (True, True)]       # (gradient wanted, GSASR_SSIM_GRAD_HWC)
SSIM_IDS = ["value", "planar-gradient", "interleaved-gradient"]


@pytest.mark.parametrize("want_grad,hwc", SSIM_FORMS, ids=SSIM_IDS)
@pytest.mark.parametrize("shape", [(11, 11), (43, 75)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_ssim_scratch_single_sample(shape, want_grad, hwc, dev):
    from gsasr_amd import _cabi
    from test_ssim_loss_gpu import check, reference
    kind = "smooth"
    x, y, L, g64, e_loss, e_grad = reference(kind, shape)
    xd, yd = x.to(dev), y.to(dev)
    n = ssim_size(1, shape[0], shape[1], None, shape[0], want_grad, hwc)
    guards, results = [], []
    for fill in FILLS:
        g = GuardedBytes(n, dev, fill, seed=shape[1])
        loss, grad = _cabi.ssim_loss(xd, yd, None, 0.8, want_grad=want_grad, hwc=hwc, scratch=g.mid.view(torch.float32))
        torch.cuda.synchronize()
        g.check(f"ssim {shape} {fill}")
        guards.append(g)
        check(float(loss[0]), L, e_loss, abs(L), f"ssim {shape} {fill} loss")
        if want_grad:
            check(grad.permute(2, 0, 1) if hwc else grad, g64, e_grad, float(g64.abs().max()), f"ssim {shape} {fill} gradient")
        results.append((loss, grad))
    for loss, grad in results[1:]:
        assert torch.equal(bits(loss), bits(results[0][0])) and (grad is None or torch.equal(bits(grad), bits(results[0][1])))
    slack = slack_of(guards)
    print(f"ssim {shape} gradient={want_grad} hwc={hwc}: scratch n = {n}, slack = {slack}")
    short_scratch_is_refused(lambda s: _cabi.ssim_loss(xd, yd, None, 0.8, want_grad=want_grad, hwc=hwc, scratch=s.view(torch.float32)),
                             GuardedBytes(n, dev, "seeded"), 4)
    if want_grad and not hwc and shape == (43, 75):       # the derivative maps are the last region: written to the end
        run = lambda s: _cabi.ssim_loss(xd, yd, None, 0.8, scratch=s.view(torch.float32))      # noqa: E731
        early = 4 * ((slack + 4) // 4 + 1)
        print(f"ssim {shape}: a guard {early} bytes early: {guard_that_starts_early_reports(run, n, dev, early=early)!r}")


@pytest.mark.parametrize("want_grad,hwc", SSIM_FORMS, ids=SSIM_IDS)
def test_ssim_scratch_padded_batch(want_grad, hwc, dev):
    """the batch of three of tests/test_ssim_loss_gpu.py: unequal sample_hw, NaN in every padding, a taller target"""
    from gsasr_amd import _cabi
    from test_ssim_loss import BATCH_SIZES
    from test_ssim_loss_gpu import batch_reference, check
    x, y, per = batch_reference("noise")
    B = len(BATCH_SIZES)
    xd, yd = x.to(dev), y.to(dev)
    n = ssim_size(B, 24, 40, BATCH_SIZES, 29, want_grad, hwc)
    guards, results = [], []
    for fill in FILLS:
        g = GuardedBytes(n, dev, fill, seed=B)
        loss, grad = _cabi.ssim_loss(xd, yd, BATCH_SIZES, 0.8, want_grad=want_grad, hwc=hwc, scratch=g.mid.view(torch.float32))
        torch.cuda.synchronize()
        g.check(f"ssim batch {fill}")
        guards.append(g)
        planar = None if grad is None else grad.permute(0, 3, 1, 2) if hwc else grad
        for b, (h, w) in enumerate(BATCH_SIZES):
            L, g64, e_loss, e_grad = per[b]
            check(float(loss[1 + b]), L, e_loss, abs(L), f"ssim batch {fill} sample {b} loss")
            if want_grad:
                check(planar[b, :, :h, :w], g64, e_grad, float(g64.abs().max()), f"ssim batch {fill} sample {b} gradient")
        results.append((loss, None if planar is None else torch.stack([planar[b, :, :11, :11] for b in range(B)])))
    for loss, grad in results[1:]:
        assert torch.equal(bits(loss), bits(results[0][0])) and (grad is None or torch.equal(bits(grad), bits(results[0][1])))
    print(f"ssim batch of 3 gradient={want_grad} hwc={hwc}: scratch n = {n}, slack = {slack_of(guards)}")
    short_scratch_is_refused(lambda s: _cabi.ssim_loss(xd, yd, BATCH_SIZES, 0.8, want_grad=want_grad, hwc=hwc, scratch=s.view(torch.float32)),
                             GuardedBytes(n, dev, "seeded"), 4)


# ---- gsasr_metrics_scratch_bytes / gsasr_image_metrics -------------------------------------------------------------------------
def metrics_size(B, h, w, sizes, cb, y):
    from gsasr_amd import _cabi
    d = _cabi.make_metrics(B, h, w, sizes, cb, _cabi.METRIC_PSNR | _cabi.METRIC_SSIM | (_cabi.METRIC_Y if y else 0))
    n = int(_cabi.lib().gsasr_metrics_scratch_bytes(ctypes.byref(d)))
    assert n > 0 and n % 8 == 0
    return n


@pytest.mark.parametrize("y", [False, True], ids=["rgb", "y"])
@pytest.mark.parametrize("shape,cb", [((19, 19), 4), ((45, 77), 0)], ids=["19x19-crop4", "45x77"])
def test_metrics_scratch_single_picture(shape, cb, y, dev):
    from gsasr_amd import _cabi
    from test_metrics import make_pair
    from test_metrics_gpu import check
    img, ref = make_pair(*shape, seed=2)
    ti, tr = torch.from_numpy(img).to(dev), torch.from_numpy(ref).to(dev)
    n = metrics_size(1, shape[0], shape[1], None, cb, y)
    guards, results = [], []
    for fill in FILLS:
        g = GuardedBytes(n, dev, fill, seed=shape[0])
        got = _cabi.image_metrics(ti, tr, None, cb, y, True, scratch=g.mid)
        torch.cuda.synchronize()
        g.check(f"metrics {shape} {fill}")
        guards.append(g)
        check(got[0].cpu(), img, ref, cb, y, True, f"metrics {shape} cb={cb} y={y} {fill}")
        results.append(got.cpu())
    assert all(torch.equal(r.view(torch.int64), results[0].view(torch.int64)) for r in results[1:])
    slack = slack_of(guards)
    print(f"metrics {shape} cb={cb} y={y}: scratch n = {n}, slack = {slack}")
    short_scratch_is_refused(lambda s: _cabi.image_metrics(ti, tr, None, cb, y, True, scratch=s), GuardedBytes(n, dev, "seeded"), 1)


@pytest.mark.parametrize("y", [False, True], ids=["rgb", "y"])
def test_metrics_scratch_padded_batch(y, dev):
    """the batch of three of tests/test_metrics_gpu.py: unequal sample_hw in a padded [3, 64, 80, 3]"""
    from gsasr_amd import _cabi
    from test_metrics import make_pair
    from test_metrics_gpu import check
    sizes, cb = [(33, 45), (64, 64), (21, 80)], 3
    cimg, cref = np.full((3, 64, 80, 3), 255, np.uint8), np.zeros((3, 64, 80, 3), np.uint8)
    for b, (h, w) in enumerate(sizes):
        cimg[b, :h, :w], cref[b, :h, :w] = make_pair(h, w, seed=6 + b)
    ti, tr = torch.from_numpy(cimg).to(dev), torch.from_numpy(cref).to(dev)
    n = metrics_size(3, 64, 80, sizes, cb, y)
    guards, results = [], []
    for fill in FILLS:
        g = GuardedBytes(n, dev, fill, seed=5)
        got = _cabi.image_metrics(ti, tr, sizes, cb, y, False, scratch=g.mid)
        torch.cuda.synchronize()
        g.check(f"metrics batch {fill}")
        guards.append(g)
        for b, (h, w) in enumerate(sizes):
            check(got[b].cpu(), cimg[b, :h, :w], cref[b, :h, :w], cb, y, False, f"metrics batch sample {b} y={y} {fill}")
        results.append(got.cpu())
    assert all(torch.equal(r.view(torch.int64), results[0].view(torch.int64)) for r in results[1:])
    print(f"metrics batch of 3 y={y}: scratch n = {n}, slack = {slack_of(guards)}")
    short_scratch_is_refused(lambda s: _cabi.image_metrics(ti, tr, sizes, cb, y, False, scratch=s), GuardedBytes(n, dev, "seeded"), 1)


# ---- window attention: the six *_scratch_bytes families ------------------------------------------------------------------------
BF = torch.bfloat16
BIASED = [(3, 9, 9, 2, 5), (258, 5, 7, 2, 4)]              # W, nq, nk, H, d: 3 window slots; past one slot of 256
ROPE = [(3, 9, 9, 2, 6), (258, 5, 7, 1, 4)]                # one slice of windows (no scratch need); 33 slices
MASKED = [(4, 9, 9, 2, 5, 2), (258, 9, 9, 2, 5, 3)]        # ..., mask windows
MIN_SCRATCH = 256


def attention_case(family, shape):
    """-> (acts (q, k, v), side (table or angles), index or None, mask or None, wgt, want[5] float64, e[5], bf16)"""
    bf16 = family.endswith("bf16")
    kind = family.split("-")[0]
    if kind == "masked":
        if bf16:
            import test_window_attention_masked_bf16_gpu as m
            (acts, table, index, mask, wgt), want, e = m.yardsticks(shape)
        else:
            import test_window_attention_masked_gpu as m
            (q, k, v, table, index, mask, wgt), want, e = m.yardsticks(shape)
            acts = (q, k, v)
        return acts, table, index, mask, wgt, want, e, bf16
    if bf16:
        import test_window_attention_bf16_gpu as m
        (acts, side, tail, wgt), want, e = m.yardsticks(kind, shape, "extra rows" if kind == "rope" else "plain")
        return acts, side, (tail[0] if tail else None), None, wgt, want, e, bf16
    if kind == "biased":
        import test_window_attention_gpu as m
        (q, k, v, side, index, wgt), want, e = m.yardsticks(shape)
    else:
        import test_window_attention_rope_gpu as m
        (q, k, v, side, wgt), want, e = m.yardsticks(shape, "extra rows")
        index = None
    return (q, k, v), side, index, None, wgt, want, e, bf16


def attention_size(family, acts, side, mask, need_side, bf16):
    """the family's `*_scratch_bytes` for the backward of this case (`need_side`: g_table / g_angles wanted)"""
    from gsasr_amd import _cabi
    kind = family.split("-")[0]
    W, nq, C = acts[0].shape
    nk = acts[1].shape[1]
    if kind == "rope":
        H = side.shape[0]
        d = _cabi.make_window_attn_rope(W, H, nq, nk, C // H, side.shape[1], (C // H) ** -0.5, bf16)
        d.g_angles = 256 if need_side else None
        d.g_q = d.g_k = 256
        fn = _cabi._ATTN_FNS[True, bf16]["scratch_bytes"]
    else:
        H = side.shape[1]
        if kind == "masked":
            d = _cabi.make_window_attn_masked(W, H, nq, nk, C // H, side.shape[0], (C // H) ** -0.5, bf16, mask_windows=mask.shape[0])
            fn = _cabi._MASKED_FNS[bf16]["scratch_bytes"]
        else:
            d = _cabi.make_window_attn(W, H, nq, nk, C // H, side.shape[0], (C // H) ** -0.5, bf16)
            fn = _cabi._ATTN_FNS[False, bf16]["scratch_bytes"]
        d.g_table = 256 if need_side else None
    n = int(getattr(_cabi.lib(), fn)(ctypes.byref(d)))
    assert n >= MIN_SCRATCH, (family, n, _cabi.lib().gsasr_last_error())
    return n


def attention_run(family, case, need_side, scratch, dev):
    """forward + backward through the ctypes wrappers with the backward's scratch = `scratch` -> [out, g_q, g_k, g_v, g_side]"""
    from gsasr_amd import _cabi
    acts, side, index, mask, wgt, _, _, bf16 = case
    kind = family.split("-")[0]
    dt = BF if bf16 else torch.float32
    q, k, v = (t.to(dev, dt).contiguous() for t in acts)
    side_d, go = side.to(dev).contiguous(), wgt.to(dev, dt).contiguous()
    scale = float((q.shape[2] // (side.shape[0] if kind == "rope" else side.shape[1])) ** -0.5)
    need = (True, True, True, need_side)
    if kind == "rope":
        out, stats, cossin = _cabi.window_attn_rope_forward(q, k, v, side_d, scale)
        g = _cabi.window_attn_rope_backward(q, k, v, side_d, scale, out, stats, cossin, go, need=need, scratch=scratch)
    elif kind == "masked":
        idx, msk = index.to(dev, torch.int32).contiguous(), mask.to(dev).contiguous()
        out, stats = _cabi.window_attn_masked_forward(q, k, v, side_d, idx, msk, scale)
        g = _cabi.window_attn_masked_backward(q, k, v, side_d, idx, msk, scale, out, stats, go, need=need, scratch=scratch)
    else:
        idx = index.to(dev, torch.int32).contiguous()
        out, stats = _cabi.window_attn_forward(q, k, v, side_d, idx, scale)
        g = _cabi.window_attn_backward(q, k, v, side_d, idx, scale, out, stats, go, need=need, scratch=scratch)
    return [out, *g]


ATTENTION = [(f"{kind}{suffix}", shape) for kind, shapes in (("biased", BIASED), ("rope", ROPE), ("masked", MASKED))
             for suffix in ("", "-bf16") for shape in shapes]


@pytest.mark.parametrize("need_side", [True, False], ids=["side-gradient", "no-side-gradient"])
@pytest.mark.parametrize("family,shape", ATTENTION, ids=[f"{f}-{'x'.join(map(str, s))}" for f, s in ATTENTION])
def test_attention_scratch(family, shape, need_side, dev):
    """`need_side`: g_table (the biased and masked families: partial table columns per window slot) / g_angles (the rotary
    families: partial angle gradients per slice of windows, past one slice) is wanted"""
    from test_window_attention import held
    case = attention_case(family, shape)
    acts, side, _, mask, _, want, e, bf16 = case
    kind = family.split("-")[0]
    n = attention_size(family, acts, side, mask, need_side, bf16)
    slices = (shape[0] + max((shape[0] + 63) // 64, 8) - 1) // max((shape[0] + 63) // 64, 8)
    needed = need_side and (kind != "rope" or slices > 1)
    if not needed:
        assert n == MIN_SCRATCH, (family, shape, n)        # nothing to keep: the minimum, which the call must not touch
    else:
        assert n > MIN_SCRATCH
    names = ("out", "g_q", "g_k", "g_v", "g_angles" if kind == "rope" else "g_table")
    guards, results = [], []
    for fill in FILLS:
        g = GuardedBytes(n, dev, fill, seed=shape[0])
        got = attention_run(family, case, need_side, g.mid, dev)
        torch.cuda.synchronize()
        g.check(f"{family} {shape} {fill}")
        guards.append(g)
        ok = True
        for name, x, w, err in zip(names, got, want, e):
            if x is not None:
                ok &= held(f"{family} {shape} {fill} {name}", x, w, err)
        assert ok
        if not needed:
            assert not g.written().any(), f"{family} {shape}: a backward without scratch need wrote its scratch"
        results.append(got)
    for other in results[1:]:
        for name, x, y in zip(names, other, results[0]):
            if x is not None and name != "g_table":      # (g_table: "its last bits may differ between two calls")
                assert torch.equal(bits(x), bits(y)), (family, shape, name)
    slack = slack_of(guards) if needed else n
    print(f"{family} {shape} side gradient={need_side}: scratch n = {n}, slack = {slack}")
    short_scratch_is_refused(lambda s: attention_run(family, case, need_side, s, dev), GuardedBytes(n, dev, "seeded"), 1)


def test_attention_scratch_of_a_large_table(dev):
    """above 4096 table rows the table's sums are kept in double in the scratch, "zeroed by the call" (include/gsasr_splat.h):
    from garbage that is the whole point"""
    import test_window_attention_gpu as m
    from gsasr_amd import attention as att
    from test_window_attention import held
    q, k, v, _, index, wgt = m.make_case((2, 9, 9, 2, 5))
    table = 0.5 * torch.randn(5000, 2, generator=torch.Generator().manual_seed(1))
    index = index * 290
    want = m.evaluate(att.window_attention_torch, q, k, v, table, index, wgt, dtype=torch.float64)
    f32 = m.evaluate(att.window_attention_torch, q, k, v, table, index, wgt)
    e = [float((a.double() - b).abs().max()) for a, b in zip(f32, want)]
    case = ((q, k, v), table, index, None, wgt, want, e, False)
    n = attention_size("biased", (q, k, v), table, None, True, False)
    assert n >= 5000 * 2 * 8
    guards = []
    for fill in FILLS:
        g = GuardedBytes(n, dev, fill, seed=1)
        got = attention_run("biased", case, True, g.mid, dev)
        torch.cuda.synchronize()
        g.check(f"large table {fill}")
        guards.append(g)
        assert all([held(f"T 5000 {fill} {name}", x, w, err) for name, x, w, err in zip(m.NAMES, got, want, e)])
        used = torch.zeros(5000, dtype=torch.bool)
        used[index.flatten()] = True
        assert bool((got[4].cpu()[~used] == 0).all())
    print(f"biased, 5000 table rows: scratch n = {n}, slack = {slack_of(guards)}")
    short_scratch_is_refused(lambda s: attention_run("biased", case, True, s, dev), GuardedBytes(n, dev, "seeded"), 1)
