"""How much there is of what the kernels index by: canvases of 17 to 64 samples (GSASR_MAX_BATCH = 64), and pixels whose row or
column index has bit 14 set (the plan packs window bounds into 15-bit fields: `c0 | test<<15 | c1<<16`, `r0 | spans<<15 | r1<<16`).

Until here the largest canvas held to the oracle had 3 samples, the largest held to anything 16; the tallest image was 8192 rows,
the widest 4200 columns, the tallest canvas 16 x 192 rows.  An inference canvas of 64 tiles of 480 px is 31 744 rows.

References and bars are the suite's own: oracle.gs_oracle.forward_f64 / backward_f64 behind oracle.host_ref.prologue, the image
within IMG_ATOL (1e-4 absolute), gradients within GRAD_RTOL (2e-4 of the tensor's max-abs), as test_batched_step_against_oracle
holds a batch of three; the fused loss within 2e-5 relative of the float64 loss of the image the call returned; 8-bit bytes equal
to `quantise` of the float canvas of the same plan.  Every oracle result is computed once per (sample, size, op) and shared.

Nothing here is large: a canvas of 64 samples of about 50 x 50 px, and images of 32767 x 24 (0.8 Mpx).  Every check prints the
worst error it measured next to its bar (profiles/large_batch_parity.txt keeps the figures of one run)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import gradbars  # noqa: E402
from test_fused_loss import loss_f64  # noqa: E402
from test_fused_loss_gpu import check_param_grads, conditioned_target, forced_backward, unfused_batch  # noqa: E402
from test_hip_parity import GRAD_RTOL, IMG_ATOL, _batch_case, _relmax  # noqa: E402
from test_ssim_loss_gpu import WINDOWS, check_terms, composed  # noqa: E402
from test_u8_output_gpu import TAU, quantise, raw_parameters, separated  # noqa: E402

pytestmark = pytest.mark.gpu
KERNELS = ["gaussian", "tile", "home"]
LR, SEED, DMAX = (12, 10), 120, 0.25
RAGGED = [(48, 40), (36, 52), (61, 33), (20, 64), (33, 47)]        # heights no multiple of 16, widths all different
ROOMY = [(48, 40), (36, 52), (61, 37), (21, 64), (33, 47)]         # ... and every window of WINDOWS fits every one of these


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the MI355X box)"
    return torch.device("cuda:0")


def cycle(sizes, B):
    return [sizes[b % len(sizes)] for b in range(B)]


# ---- the oracle, once per sample ------------------------------------------------------------------------------------------
_REFS = {}


def sample_reference(b, size, bounded, window=None):
    """sample b (seed SEED + b, as `_batch_case` makes it) on its own h x w grid: (float64 image [h,w,3] -- of the window if
    one is given --, the weight [h,w,3] of the scalar that is differentiated, zero outside the window, and d / d raw parameters
    [N,9] through the float64 prologue + backward_f64).  Computed once, shared, never written."""
    key = (b, size, bounded, window)
    if key not in _REFS:
        from gsasr_amd import synthetic
        from oracle import gs_oracle, host_ref
        h, w = size
        p = synthetic.gs_parameters(LR[0], LR[1], seed=SEED + b)
        sm = torch.tensor([h / LR[0]] * 2)
        sig, xy, col, _ = host_ref.prologue(p, (h, w), sm, dmax=DMAX, dmax_mode="fix")
        dmax = DMAX if bounded else None
        ref = gs_oracle.forward_f64(sig.numpy(), xy.numpy(), col.numpy(), h, w, dmax)
        wgt = synthetic.grad_image(h, w, 140 + b)
        if window is not None:
            y0, x0, wh, ww = window
            mask = torch.zeros(h, w, 1)
            mask[y0:y0 + wh, x0:x0 + ww] = 1.0
            wgt, ref = wgt * mask, ref[y0:y0 + wh, x0:x0 + ww]
        pr = p.clone().double().requires_grad_(True)
        s2, x2, c2, _ = host_ref.prologue(pr, (h, w), sm.double(), dmax=DMAX, dmax_mode="fix")
        g = gs_oracle.backward_f64(sig.numpy(), xy.numpy(), col.numpy(), wgt.numpy(), dmax)
        torch.autograd.backward([s2, x2, c2], [torch.from_numpy(a) for a in g])
        _REFS[key] = (ref, wgt, pr.grad.numpy())
    return _REFS[key]


_DEVICE_TRUTH = {}


def device_frame_truth(b, p_b, size, sm_b, wgt, dmax, window):
    """The float64 truth of d sum(wgt * image) / d raw parameters for the per-ELEMENT bars: backward_f64 at the kernel frame that
    THIS device's fp32 torch makes of the parameters (the reference's own host code, gsp._activate + _to_kernel_frame, which the
    fused prologue equals bit for bit: test_fused_prologue_matches_unfused_torch_path), then the float64 chain rule of
    oracle/host_ref.py.  `sample_reference` takes the frame of the CPU's fp32 torch; the two differ by an ulp in some centres, and at
    the scales here (x1.67 up: standard deviations from 0.3 px) a Gaussian's d / d mean is a cancelling sum over a few pixels that
    an ulp of its centre moves by 1e-3 of itself (tools/fuzz_host.py) -- measured on sample 13 of the batched windows, row 105
    (0.72 px, rho -0.90): 8.6e-4 for one ulp of the centre's y, the same 1.9e-3 off the CPU frame's truth in all three kernels.
    That is the conditioning of the input, which the tensor-level bar never saw and an element's own bar does."""
    key = (b, size, dmax, window)
    if key not in _DEVICE_TRUTH:
        from gsasr_amd import gaussian_splatting as gsp
        from oracle import gs_oracle, host_ref
        frame = gsp._to_kernel_frame(*gsp._activate(p_b.detach()), size, 1.2 / sm_b[0])[:3]
        g = gs_oracle.backward_f64(*(t.cpu().numpy() for t in frame), wgt, dmax)
        pr = p_b.detach().cpu().double().requires_grad_(True)
        s2, x2, c2, _ = host_ref.prologue(pr, size, sm_b.detach().cpu().double(), dmax=DMAX, dmax_mode="fix")
        torch.autograd.backward([s2, x2, c2], [torch.from_numpy(a) for a in g])
        _DEVICE_TRUTH[key] = pr.grad.numpy()
    return _DEVICE_TRUTH[key]


def render_and_check(dev, sizes, bounded, which=None, windows=None, what=""):
    """the construction of test_batched_step_against_oracle on a canvas of len(sizes) samples: image, padding and raw-parameter
    gradient of sum(out * wgt) of every sample in `which` (default: all) against its own single-image oracle"""
    from gsasr_amd import gaussian_splatting as gsp
    B = len(sizes)
    which = range(B) if which is None else which
    p, scales, sms = _batch_case(dev, sizes, LR, SEED)
    pa = p.clone().requires_grad_(True)
    kw = dict(if_dmax=True, dmax_mode="fix", dmax=DMAX) if bounded else dict(if_dmax=False)
    out = gsp.generate_2D_gaussian_splatting_batch(sizes, pa, scales, sms, windows=windows, **kw)
    own = sizes if windows is None else [wn[2:] for wn in windows]
    assert tuple(out.shape) == (B, 3, max(h for h, _ in own), max(w for _, w in own))
    refs = [sample_reference(b, sizes[b], bounded, None if windows is None else windows[b]) for b in range(B)]
    loss = 0.0
    for b, (h, w) in enumerate(own):        # every sample takes part in the scalar, so no gradient is zero by construction
        wgt = refs[b][1] if windows is None else refs[b][1][windows[b][0]:windows[b][0] + h, windows[b][1]:windows[b][1] + w]
        loss = loss + (out[b, :, :h, :w] * wgt.permute(2, 0, 1).to(dev)).sum()
    loss.backward()
    got, grad = out.detach().cpu(), pa.grad.cpu().numpy()
    worst_img = worst_grad = 0.0
    for b in which:
        h, w = own[b]
        ref, _, gref = refs[b]
        e_img = float(np.abs(got[b, :, :h, :w].permute(1, 2, 0).numpy() - ref).max())
        pad = got[b].clone()
        pad[:, :h, :w] = 0
        assert float(pad.abs().max()) == 0.0, (what, b)
        e_grad = _relmax(grad[b], gref)
        worst_img, worst_grad = max(worst_img, e_img), max(worst_grad, e_grad)
        assert e_img <= IMG_ATOL, (what, b, e_img)
        assert e_grad <= GRAD_RTOL, (what, b, e_grad)
        # every column to its own bar (tests/gradbars.py); 120 rows a sample, at most one of them outside its scope (seed 169 has one)
        truth = device_frame_truth(b, p[b], sizes[b], sms[b], refs[b][1].numpy(), DMAX if bounded else None,
                                   None if windows is None else windows[b])
        gradbars.check_raw(grad[b], truth, p[b], 0.99, f"{what} B={B} sample {b}")
    print(f"{what}: B={B}, samples checked {len(list(which))}, image max|err| {worst_img:.3e} (bar {IMG_ATOL:.0e}), "
          f"gradient max rel err {worst_grad:.3e} (bar {GRAD_RTOL:.0e})")


# ---- A. canvases of 17, 33 and 64 samples ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("B,bounded", [(17, True), (33, True), (64, True), (64, False)],
                         ids=["B17-dmax0.25", "B33-dmax0.25", "B64-dmax0.25", "B64-unbounded"])
def test_ragged_canvas_against_the_oracle(B, bounded, kernel, dev):
    with forced_backward(kernel):
        render_and_check(dev, cycle(RAGGED, B), bounded, what=f"ragged {kernel} {'bounded' if bounded else 'unbounded'}")


@pytest.mark.parametrize("kernel", KERNELS)
def test_uniform_canvas_of_64_against_the_oracle(kernel, dev):
    """all samples 48 x 40: the geometry is arithmetic on P.geo_h, no k_batch_geo runs"""
    with forced_backward(kernel):
        render_and_check(dev, [(48, 40)] * 64, True, which=(0, 15, 16, 17, 47, 63), what=f"uniform {kernel}")


@pytest.mark.parametrize("kernel", KERNELS)
def test_batched_windows_of_33_against_the_oracle(kernel, dev):
    """one window per sample (k_batch_views entries 16..32 are read): each equals the same rectangle of the sample's own
    single-image oracle render; the gradient is that of a weight that is zero outside the window"""
    B = 33
    with forced_backward(kernel):
        render_and_check(dev, cycle(ROOMY, B), True, windows=cycle(WINDOWS, B), what=f"windows {kernel}")


def levelled_target(v, seed):
    """`conditioned_target` (t = v + s u, |u| >= 1e-2) pushed a further 0.01 * b away from sample b's image on the side it is
    already on: no |v - t| below 1e-2, and every sample's mean |v - t| differs from its neighbours' by 0.01 -- a loss dealt to
    the wrong sample, or a sample the reduce skipped, is off by percents"""
    t = conditioned_target(v, seed)
    level = 0.01 * torch.arange(v.shape[0], device=v.device, dtype=v.dtype).view(-1, 1, 1, 1)
    return (t + level * torch.sign(t - v)).contiguous()


@pytest.mark.parametrize("kind", ["l1", "mse"])
@pytest.mark.parametrize("B", [17, 64])
def test_fused_loss_of_17_and_64(B, kind, dev):
    """k_loss_reduce deals samples to waves with `b += 16 / wps`: its second to fourth trip, and wps = 1"""
    from gsasr_amd import gaussian_splatting as gsp
    sizes = cycle(RAGGED, B)
    p, scales, sms = _batch_case(dev, sizes, LR, SEED)
    kw = dict(dmax=DMAX)
    with torch.no_grad():
        t = levelled_target(gsp.generate_2D_gaussian_splatting_batch(sizes, p, scales, sms, **kw), 21)
    _, _, want_g, _ = unfused_batch(p, sizes, scales, sms, t, kind, 1.0, 1e-12, "mean", None, kw)
    pa = p.clone().requires_grad_(True)
    value, per, images = gsp.generate_2D_gaussian_splatting_batch_loss(sizes, pa, scales, sms, t, loss=kind, return_per_sample=True,
                                                                       return_images=True, **kw)
    assert value.dim() == 0 and value.requires_grad and tuple(per.shape) == (B,)
    value.backward()
    img, tgt, refs, worst = images.cpu().numpy(), t.cpu().numpy(), [], 0.0
    for b, (h, w) in enumerate(sizes):
        ref, _ = loss_f64(img[b, :, :h, :w], tgt[b, :, :h, :w], kind, 1.0, 1e-12, "mean")
        refs.append(ref)
        rel = abs(float(per[b]) - ref) / ref
        worst = max(worst, rel)
        assert rel <= 2e-5, (b, float(per[b]), ref)
    assert min(abs(a - b) for i, a in enumerate(refs) for b in refs[i + 1:]) > 1e-3 * max(refs)      # no two samples alike
    mean = float(np.mean(refs))
    print(f"fused {kind} B={B}: per-sample loss max rel err {worst:.3e}, total rel err {abs(float(value.detach()) - mean) / mean:.3e} (bar 2e-5)")
    assert abs(float(value.detach()) - mean) <= 2e-5 * mean
    check_param_grads(pa.grad, want_g, p, f"fused {kind} B={B}")
    gsp.deferred_asserts.flush()


def test_fused_loss_with_ssim_of_17(dev):
    """L1 + SSIM in one call at B = 17: k_ssim_reduce and k_loss_reduce both with wps = 1 and a second trip over the samples"""
    from gsasr_amd import gaussian_splatting as gsp
    B = 17
    sizes = cycle(RAGGED, B)
    p, scales, sms = _batch_case(dev, sizes, LR, SEED)
    img_of = lambda q: gsp.generate_2D_gaussian_splatting_batch(sizes, q, scales, sms, dmax=DMAX)      # noqa: E731
    with torch.no_grad():
        t = levelled_target(img_of(p), 22)
    want_pix, _, want_g, _ = composed(img_of, p, t, sizes, 0.5)
    pa = p.clone().requires_grad_(True)
    value, per, images, (l_pix, l_ssim) = gsp.generate_2D_gaussian_splatting_batch_loss(
        sizes, pa, scales, sms, t, loss="l1", dmax=DMAX, return_per_sample=True, return_images=True, ssim_weight=0.5, return_terms=True)
    value.backward()
    check_terms(l_pix, l_ssim, value.detach(), want_pix, images, t, sizes, 0.5, "fused l1 + ssim B=17")
    assert abs(float(per.mean()) - float(value.detach())) <= 1e-6 * abs(float(value.detach()))
    check_param_grads(pa.grad, want_g, p, "fused l1 + ssim B=17")
    gsp.deferred_asserts.flush()


U8_SIZES = [(128, 128), (64, 192), (131, 70), (192, 77), (70, 140)]


@pytest.mark.parametrize("dmax_on", [True, False], ids=["bounded", "unbounded"])
def test_u8_canvas_of_64_is_exact(dmax_on, dev):
    """64 samples of `separated` Gaussians (one term per pixel: the forward is bit-stable) in one canvas: the bytes of every
    sample -- 0, 16, 31, 32 and 63 among them -- are `quantise` of the float canvas of the same plan, zero beyond the sample"""
    from gsasr_amd import _cabi
    B, n_per = 64, 8
    sizes = cycle(U8_SIZES, B)
    parts = [separated(h, w, n_per, seed=300 + b) for b, (h, w) in enumerate(sizes)]
    assert all(q[0].shape[0] == n_per for q in parts)
    sig, xy, col = (torch.cat([q[k] for q in parts]).to(dev) for k in range(3))
    d = _cabi.make_batch_dims(n_per, sizes, 192, 192, 40.0 / 191 if dmax_on else None, cutoff=TAU, flags=_cabi.FLAG_FORWARD_ONLY)
    L = _cabi.lib()
    nbytes = L.gsasr_splat_workspace_bytes(ctypes.byref(d))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _cabi.check(L.gsasr_splat_plan(sig.data_ptr(), xy.data_ptr(), col.data_ptr(), ctypes.byref(d), ws.data_ptr(), nbytes,
                                   torch.cuda.current_stream(dev).cuda_stream), "gsasr_splat_plan")
    plan = _cabi.Plan(d, ws, dev)
    assert d.batch == B and d.slot == 192 and d.w == 192
    img = torch.full((B * d.slot, d.w, 3), float("nan"), device=dev)
    _cabi.forward(plan, img, overwrite=True)
    img = img.reshape(B, d.slot, d.w, 3)
    assert bool(torch.isfinite(img).all())
    for crop, bgr in ((None, False), ((192 - 21, 192 - 37), True)):
        rows, cols = crop or (192, 192)
        want = quantise(img[:, :rows, :cols])
        got = _cabi.forward_u8(plan, crop=crop, bgr=bgr).cpu().numpy()
        if bgr:
            want = want[..., ::-1]
        for b, (h, w) in enumerate(sizes):
            assert np.array_equal(got[b], want[b]), (b, crop, int((got[b] != want[b]).sum()))
            assert got[b, :h, :w].max() == 255 and not got[b, h:].any() and not got[b, :, w:].any(), b


STEP_U8_SIZES = [(96, 192), (192, 96), (100, 110), (192, 192), (110, 200)]


def test_u8_step_canvas_of_64_is_exact(dev):
    """the same through the batched 8-bit step entry point (raw parameters: prologue + plan + 8-bit forward in one call), on
    `raw_parameters` -- the raw form of `separated`; the float forward on the plan the call left behind gives the canvas"""
    from gsasr_amd import _cabi
    B, scale = 64, 8.0
    sizes = cycle(STEP_U8_SIZES, B)
    p = torch.stack([raw_parameters(h, w, scale, 8, seed=400 + b) for b, (h, w) in enumerate(sizes)]).to(dev)
    steps = torch.full((B,), 1.2 / scale, device=dev)
    got, plan = _cabi.batch_forward_u8(p, steps, sizes, 40.0 / 199)
    d = plan.dims
    assert d.batch == B and d.slot == 192 and d.w == 200 and tuple(got.shape) == (B, 192, 200, 3)
    img = torch.full((B * d.slot, d.w, 3), float("nan"), device=dev)
    _cabi.forward(plan, img, overwrite=True)
    want = quantise(img.reshape(B, d.slot, d.w, 3))
    got = got.cpu().numpy()
    for b, (h, w) in enumerate(sizes):
        assert np.array_equal(got[b], want[b]), (b, int((got[b] != want[b]).sum()))
        assert got[b, :h, :w].any() and not got[b, h:].any() and not got[b, :, w:].any(), b


# ---- B. rows and columns with bit 14 set ----------------------------------------------------------------------------------
def longest_side():
    """the largest h and w `dims_ok` admits (gsasr_amd/csrc/splat_common.h), taken from the code"""
    m = re.search(r"d->h <= (\d+) && d->w <= (\d+)", open(os.path.join(ROOT, "gsasr_amd", "csrc", "splat_common.h")).read())
    assert m and m.group(1) == m.group(2)
    return int(m.group(1))


SHORT = 24
KERNEL_FLAGS = {"gaussian": "FLAG_BWD_GAUSSIAN", "tile": "FLAG_BWD_TILE", "home": "FLAG_BWD_HOME"}


def long_gaussians(L, tall, seed=7):
    """kernel-frame Gaussians of an image of L x 24 (`tall`) or 24 x L pixels: 350 of the size of an LR pixel on a x4 grid
    (std 0.7 .. 3.3 px) in three clusters along the long axis -- centres at 60..140, at 16384 +- 40 (windows that start below
    2^14 and end above it) and at L - 48 .. L + 4 (windows clipped at the last index, centres past it) -- and three of the large
    class, std 50 px (an extent of 300 px), centred at 16384.  Along the short axis every other small Gaussian sits exactly on a
    pixel centre: a dmax box of +- 20 px along the long axis is +- 0.014 px along the short one, and those are the ones it keeps."""
    rng = np.random.RandomState(seed)
    along = np.concatenate([rng.uniform(60, 140, 100), rng.uniform(16384 - 40, 16384 + 40, 150), rng.uniform(L - 48, L + 4, 100),
                            16384 + np.array([-3.0, 0.0, 2.5])])
    n = along.size
    across = rng.uniform(-1, SHORT, n)
    across[:350:2] = np.rint(np.clip(across[:350:2], 0, SHORT - 1))
    across[350:] = (5, 12, 19)
    std_along = np.concatenate([(0.2 + 0.8 * rng.uniform(size=350)) * 4 / 1.2, [50.0, 50.0, 50.0]])
    std_across = np.concatenate([(0.2 + 0.8 * rng.uniform(size=350)) * 4 / 1.2, [3.0, 4.0, 3.0]])
    rho = np.concatenate([rng.uniform(-0.8, 0.8, 350), [-0.3, 0.0, 0.3]])
    col = np.concatenate([rng.uniform(0.05, 0.6, (350, 3)), np.full((3, 3), 0.3)])
    H, W = (L, SHORT) if tall else (SHORT, L)
    x_px, y_px, sx_px, sy_px = (across, along, std_across, std_along) if tall else (along, across, std_along, std_across)
    # pixel X sits at 2 X / (W - 1) - 1: the expression of the kernels' and the oracle's pixel tables, rounded to fp32 once
    xy = np.stack([2.0 * x_px / (W - 1) - 1.0, 2.0 * y_px / (H - 1) - 1.0], 1).astype(np.float32)
    sig = np.stack([sx_px * 2.0 / (W - 1), sy_px * 2.0 / (H - 1), rho], 1).astype(np.float32)
    return sig, xy, col.astype(np.float32), H, W


def long_bands(L):
    """(the three bands that hold the clusters, two bands between them that no Gaussian reaches)"""
    return ((0, 256), (16256, 16512), (L - 256, L)), ((8000, 8256), (24000, 24256))


_LONG = {}


def long_reference(tall, bounded):
    """the oracle on the three bands along the long axis -- for the wide image the WHOLE image --, and the gradients of
    sum(img * wgt) with wgt uniform noise on the three bands and zero elsewhere (the sum of the bands' gradients)"""
    key = (tall, bounded)
    if key not in _LONG:
        from oracle import gs_oracle
        L = longest_side()
        sig, xy, col, H, W = long_gaussians(L, tall)
        dmax = 40.0 / (L - 1) if bounded else None
        live, _ = long_bands(L)
        wgt = np.zeros((H, W, 3), np.float32)
        rng = np.random.RandomState(11)
        for a, b in live:
            if tall:
                wgt[a:b] = rng.uniform(size=(b - a, W, 3))
            else:
                wgt[:, a:b] = rng.uniform(size=(H, b - a, 3))
        if tall:
            img = {r: gs_oracle.forward_f64(sig, xy, col, H, W, dmax, rows=r) for r in live}
            grads = [gs_oracle.backward_f64(sig, xy, col, wgt[a:b], dmax, h=H, rows=(a, b)) for a, b in live]
            grads = tuple(sum(g[k] for g in grads) for k in range(3))
        else:
            img = gs_oracle.forward_f64(sig, xy, col, H, W, dmax)
            grads = gs_oracle.backward_f64(sig, xy, col, wgt, dmax)
        _LONG[key] = (sig, xy, col, H, W, dmax, wgt, img, grads)
    return _LONG[key]


@pytest.mark.parametrize("bounded", [True, False], ids=["box40px", "unbounded"])
@pytest.mark.parametrize("tall", [True, False], ids=["tall", "wide"])
def test_longest_image_against_the_oracle(tall, bounded, dev):
    """32767 x 24 and 24 x 32767: the forward and each of the three backward kernels where window bounds need all 15 bits"""
    from gsasr_amd import _cabi
    L = longest_side()
    assert L == 32767
    sig, xy, col, H, W, dmax, wgt, ref, gref = long_reference(tall, bounded)
    live, empty = long_bands(L)
    a, b, c = (torch.from_numpy(t).to(dev) for t in (sig, xy, col))
    gw = torch.from_numpy(wgt).to(dev)
    for kernel in KERNELS:
        plan = _cabi.plan(a, b, c, H, W, dmax, flags=getattr(_cabi, KERNEL_FLAGS[kernel]))
        img = torch.full((H, W, 3), float("nan"), device=dev)
        _cabi.forward(plan, img, overwrite=True)
        got = img.cpu().numpy()
        assert np.isfinite(got).all()
        if tall:
            e_img = max(float(np.abs(got[r0:r1] - ref[(r0, r1)]).max()) for r0, r1 in live)
            assert all(float(np.abs(ref[r]).max()) > 0.3 for r in live)        # (every cluster shows, under the box as well)
            for r0, r1 in empty:
                assert not got[r0:r1].any(), (kernel, r0)
        else:
            e_img = float(np.abs(got - ref).max())
            assert all(float(np.abs(ref[:, r0:r1]).max()) > 0.3 for r0, r1 in live)
            for r0, r1 in empty:
                assert not got[:, r0:r1].any(), (kernel, r0)
        g = [torch.empty_like(t) for t in (a, b, c)]
        _cabi.backward(plan, a, b, c, gw, *g, overwrite=True)
        rels = [_relmax(t.cpu().numpy(), want) for t, want in zip(g, gref)]
        print(f"{'tall' if tall else 'wide'} {H}x{W} {'box 40 px' if bounded else 'unbounded'} {kernel}: image max|err| {e_img:.3e} "
              f"(bar {IMG_ATOL:.0e}), gradient max rel err sigmas {rels[0]:.3e} coords {rels[1]:.3e} colors {rels[2]:.3e} (bar {GRAD_RTOL:.0e})")
        assert e_img <= IMG_ATOL, (kernel, e_img)
        assert max(rels) <= GRAD_RTOL, (kernel, rels)
        # (element bar only: every other small Gaussian sits on a pixel centre of the only line across that its box keeps, so the
        # truth's d / d sigma across the short axis is zero but for 3e-5 -- against 1e4 along the long one, in the same rows)
        gradbars.check_kernel(g, gref, sig, 0.0, f"longest image tall={tall} bounded={bounded} {kernel}", column_bar=False)


@pytest.mark.parametrize("rows", [(16300, 16460), (-100, None)], ids=["across_2^14", "last_100_rows"])
def test_row_band_of_the_tallest_image(rows, dev):
    """a band that starts below row 2^14 and ends above it, and the last 100 rows, through HipBackend.forward / backward as
    test_unsorted_random_gaussians_large_n does"""
    from gsasr_amd.shard import HipBackend
    from oracle import gs_oracle
    L = longest_side()
    sig, xy, col, H, W = long_gaussians(L, True)
    rows = (rows[0] % H, rows[1] or H)
    a, b, c = (torch.from_numpy(t).to(dev) for t in (sig, xy, col))
    gw = np.random.RandomState(12).uniform(size=(rows[1] - rows[0], W, 3)).astype(np.float32)
    for dmax in (40.0 / (L - 1), None):
        ref = gs_oracle.forward_f64(sig, xy, col, H, W, dmax, rows=rows)
        gref = gs_oracle.backward_f64(sig, xy, col, gw, dmax, h=H, rows=rows)
        assert float(np.abs(ref).max()) > 0.3
        slab, st = HipBackend.forward(a, b, c, H, W, dmax, rows)
        assert tuple(slab.shape) == (rows[1] - rows[0], W, 3)
        e_img = float(np.abs(slab.cpu().numpy() - ref).max())
        g3 = HipBackend.backward(st, a, b, c, torch.from_numpy(gw).to(dev))
        rels = [_relmax(t.cpu().numpy(), want) for t, want in zip(g3, gref)]
        print(f"tall rows {rows} dmax {dmax}: image max|err| {e_img:.3e} (bar {IMG_ATOL:.0e}), gradient max rel err {max(rels):.3e} "
              f"(bar {GRAD_RTOL:.0e})")
        assert e_img <= IMG_ATOL and max(rels) <= GRAD_RTOL, (dmax, e_img, rels)
        gradbars.check_kernel(g3, gref, sig, 0.0, f"tall rows {rows} dmax {dmax}")


def test_tallest_canvas(dev):
    """23 slots of 1424 rows = 32 752 canvas rows, the largest multiple of 16 below 2^15; samples of 1424 - k x 24, k = 0..15,
    240 Gaussians each in the first and the last 40 rows.  Every sample equals its own single-image call within 2e-6 (the bar
    of test_batched_step_equals_per_sample_steps); samples 0, 11 and 22 the oracle, in their gradients as well."""
    from gsasr_amd import gaussian_splatting as gsp
    from oracle import gs_oracle, host_ref
    B, slot, n, scale = 23, 1424, 240, 4.0
    assert B * slot == 32752 and gsp.max_canvas_batch(slot) == B
    sizes = [(slot - b % 16, SHORT) for b in range(B)]
    g = torch.Generator().manual_seed(9)
    p = 0.5 * torch.randn(B, n, 9, generator=g)
    p[:, :, 7] = torch.rand(B, n, generator=g)
    for b, (h, _) in enumerate(sizes):
        edge = torch.rand(n, generator=g) * 40.0 / h
        p[b, :, 8] = torch.where(torch.arange(n) % 2 == 0, edge, 1.0 - edge)
    scales, sms = [scale] * B, [torch.tensor([scale, scale], device=dev) for _ in range(B)]
    wgt = torch.zeros(B, 3, slot, SHORT)
    noise = torch.rand(B, 3, slot, SHORT, generator=g)
    for b, (h, _) in enumerate(sizes):
        wgt[b, :, :64], wgt[b, :, h - 64:h] = noise[b, :, :64], noise[b, :, h - 64:h]
    pa = p.to(dev).requires_grad_(True)
    kw = dict(if_dmax=True, dmax_mode="fix", dmax=DMAX)
    out = gsp.generate_2D_gaussian_splatting_batch(sizes, pa, scales, sms, **kw)
    assert tuple(out.shape) == (B, 3, slot, SHORT)
    (out * wgt.to(dev)).sum().backward()
    worst = 0.0
    with torch.no_grad():
        for b, (h, w) in enumerate(sizes):
            one = gsp.generate_2D_gaussian_splatting_step((h, w), pa[b], scale, sms[b], **kw)
            worst = max(worst, float((out[b, :, :h, :w] - one).abs().max()))
            assert not out[b, :, h:].any(), b
    assert worst <= 2e-6, worst
    got, grad = out.detach().cpu(), pa.grad.cpu().numpy()
    for b in (0, 11, 22):
        h, w = sizes[b]
        sig, xy, col, dmax = host_ref.prologue(p[b], (h, w), torch.tensor([scale, scale]), dmax=DMAX, dmax_mode="fix")
        ref = gs_oracle.forward_f64(sig.numpy(), xy.numpy(), col.numpy(), h, w, dmax)
        e_img = float(np.abs(got[b, :, :h, :w].permute(1, 2, 0).numpy() - ref).max())
        assert float(np.abs(ref[:48]).max()) > 0.3 and float(np.abs(ref[h - 48:]).max()) > 0.3
        pr = p[b].clone().double().requires_grad_(True)
        s2, x2, c2, _ = host_ref.prologue(pr, (h, w), torch.tensor([scale, scale]).double(), dmax=DMAX, dmax_mode="fix")
        gref = gs_oracle.backward_f64(sig.numpy(), xy.numpy(), col.numpy(), wgt[b, :, :h].permute(1, 2, 0).contiguous().numpy(), dmax)
        torch.autograd.backward([s2, x2, c2], [torch.from_numpy(a) for a in gref])
        e_grad = _relmax(grad[b], pr.grad.numpy())
        print(f"tallest canvas sample {b} ({h}x{w}, canvas rows {b * slot}..{b * slot + h - 1}): against its own call {worst:.3e} "
              f"(all samples, bar 2e-6), image max|err| {e_img:.3e} (bar {IMG_ATOL:.0e}), gradient max rel err {e_grad:.3e} (bar {GRAD_RTOL:.0e})")
        assert e_img <= IMG_ATOL, (b, e_img)
        assert e_grad <= GRAD_RTOL, (b, e_grad)
        truth = device_frame_truth(b, pa[b], (h, w), sms[b], wgt[b, :, :h].permute(1, 2, 0).contiguous().numpy(), dmax, None)
        gradbars.check_raw(grad[b], truth, p[b], 1.0, f"tallest canvas sample {b}")
