"""The SSIM loss (gsasr_ssim_loss; gsasr_amd.ssim_loss; `ssim_weight` of generate_2D_gaussian_splatting_loss / _batch_loss):
what can be checked without a GPU -- the ABI surface, the argument checks of the header (they come before anything is enqueued),
the Python argument errors, and the torch expression the CPU path and the per-sample fallbacks use.
tests/test_ssim_loss_gpu.py has the kernels.

The oracle `ssim_f64` restates `pytorch_msssim.ssim` with the defaults `SSIMLoss` uses (basicsr/losses/basic_loss.py:256-264) in
float64 from the formula: a depthwise conv2d with the 11 x 11 outer-product window, autograd for the gradient.  The reference's
other statement of the quantity, basicsr/metrics/psnr_ssim.py:201-231 (a 2-D window, 255-scaled constants, one channel at a time),
is `ssim_metric_f64`; the two agree in float64.

The bar of every fp32 result (`bar`): its error against the float64 oracle may be 4 x the error of the fp32 torch expression on
the same input plus 1e-6 of the quantity's scale -- the cancellation in g*(x^2) - mu^2 depends on the input, a separable 11 + 11
sum rounds differently from a 121-term one but no worse, and the floor covers about 16 fp32 roundings."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gsasr_amd import _cabi
from gsasr_amd import gaussian_splatting as gsp
from gsasr_amd import ssim as ssim_mod
from gsasr_amd import ssim_loss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(11, 11), (12, 27), (37, 53), (75, 107), (43, 139)]      # the last two: valid maps of 3 x 4 and 2 x 5 tiles of 32 x 32
BATCH_SIZES = [(11, 16), (24, 40), (17, 11)]      # padded to [3, 3, 24, 40], the target to 29 rows
KINDS = ("noise", "smooth", "flat", "two-level")


def window_f64():
    g = torch.exp(-(torch.arange(11, dtype=torch.float64) - 5) ** 2 / (2 * 1.5 ** 2))
    return g / g.sum()


def ssim_map_f64(x, y):
    """[3,h,w] float64 -> the SSIM map [3,h-10,w-10]: the maths of the issue / of pytorch_msssim with its defaults"""
    g = window_f64()
    k = torch.outer(g, g)[None, None].expand(3, 1, 11, 11)
    blur = lambda t: F.conv2d(t[None], k, groups=3)[0]      # noqa: E731
    mu1, mu2 = blur(x), blur(y)
    s1, s2, s12 = blur(x * x) - mu1 * mu1, blur(y * y) - mu2 * mu2, blur(x * y) - mu1 * mu2
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    return (2 * mu1 * mu2 + c1) / (mu1 ** 2 + mu2 ** 2 + c1) * (2 * s12 + c2) / (s1 + s2 + c2)


def ssim_f64(x, y, weight=1.0, batch=1):
    """(L_b, d (L_b / batch) / d x) in float64 for one sample"""
    x = x.detach().double().clone().requires_grad_(True)
    value = weight * (1.0 - ssim_map_f64(x, y.detach().double()).mean())
    (value / batch).backward()
    return float(value.detach()), x.grad


def ssim_metric_f64(x, y):
    """psnr_ssim.py:201-231 (_ssim per channel on [0, 255] images, cropped to the valid region, averaged) in float64"""
    c1, c2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    g = window_f64()
    k = torch.outer(g, g)[None, None]
    vals = []
    for ch in range(3):
        a, b = 255.0 * x[ch][None, None].double(), 255.0 * y[ch][None, None].double()
        mu1, mu2 = F.conv2d(a, k), F.conv2d(b, k)
        s1, s2, s12 = F.conv2d(a * a, k) - mu1 ** 2, F.conv2d(b * b, k) - mu2 ** 2, F.conv2d(a * b, k) - mu1 * mu2
        vals.append((((2 * mu1 * mu2 + c1) * (2 * s12 + c2)) / ((mu1 ** 2 + mu2 ** 2 + c1) * (s1 + s2 + c2))).mean())
    return float(torch.stack(vals).mean())


def make_input(kind, h, w, seed=0):
    """(x, y) fp32 [3,h,w] of the kinds the bars were measured on: uniform noise; a smooth sinusoid + 2 % noise; near-flat
    0.7 + 0.1 % noise; two flat levels, 0.15 left of column w // 2 and 0.85 from it on (the sample's centre pixel is on the bright
    side, so half the picture is 0.7 away from it), + 0.1 % noise"""
    g = torch.Generator().manual_seed(1000 * seed + 10 * h + w)
    if kind == "noise":
        return torch.rand(3, h, w, generator=g), torch.rand(3, h, w, generator=g)
    if kind == "smooth":
        yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
        base = torch.stack([0.5 + 0.4 * torch.sin(0.21 * xx + 0.13 * yy + c) for c in range(3)])
        return (base + 0.02 * torch.randn(3, h, w, generator=g)).clamp(0, 1), (base + 0.02 * torch.randn(3, h, w, generator=g)).clamp(0, 1)
    if kind == "two-level":
        level = torch.where(torch.arange(w) < w // 2, 0.15, 0.85).expand(3, h, w)
        return level + 0.001 * torch.randn(3, h, w, generator=g), level + 0.001 * torch.randn(3, h, w, generator=g)
    return 0.7 + 0.001 * torch.randn(3, h, w, generator=g), 0.7 + 0.001 * torch.randn(3, h, w, generator=g)


def fp32_error(x, y, weight=1.0, batch=1):
    """(L_b and gradient of the float64 oracle, e32 of the loss, e32 of the gradient as max-abs): the fp32 torch expression of
    gsasr_amd/ssim.py against the oracle, on the CPU"""
    want, want_g = ssim_f64(x, y, weight, batch)
    q = x.detach().float().clone().requires_grad_(True)
    v = ssim_mod.ssim_torch(q, y.float(), weight)
    (v / batch).backward()
    return want, want_g, abs(float(v.detach()) - want), float((q.grad.double() - want_g).abs().max())


def bar(e32, scale):
    return 4.0 * e32 + 1e-6 * scale


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES + [(48, 48)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_torch_expression_against_the_oracle(shape, kind):
    x, y = make_input(kind, *shape)
    # in float64 the separable expression IS the oracle, to rounding
    want, want_g = ssim_f64(x, y, 0.8)
    q = x.double().requires_grad_(True)
    v = ssim_mod.ssim_torch(q, y.double(), 0.8)
    v.backward()
    assert abs(float(v.detach()) - want) <= 1e-12 * max(1.0, abs(want))
    assert float((q.grad - want_g).abs().max()) <= 1e-11 * float(want_g.abs().max())
    # in fp32: the level the issue measured (noise ~2e-6, smooth ~1e-4, near-flat ~6e-4 of the gradient's max-abs), with room
    _, g64, e_loss, e_grad = fp32_error(x, y, 0.8)
    rel = e_grad / float(g64.abs().max())
    print(f"{kind} {shape}: e32 loss {e_loss:.3e}, gradient {rel:.3e} of max-abs")
    # (two-level: each half is a near-flat picture and cancels like one, so it is held to the near-flat level)
    assert rel <= {"noise": 2e-5, "smooth": 2e-3, "flat": 2e-2, "two-level": 2e-2}[kind] and e_loss <= 1e-4


def test_the_two_restatements_of_the_reference_agree():
    for kind in KINDS:
        x, y = make_input(kind, 37, 53, seed=1)
        assert abs(float(ssim_map_f64(x.double(), y.double()).mean()) - ssim_metric_f64(x, y)) <= 1e-12


def test_window_constants():
    g = ssim_mod.window(torch.float64)
    assert float((g - window_f64()).abs().max()) <= 1e-16 and abs(float(g.sum()) - 1.0) <= 1e-15
    assert torch.equal(ssim_mod.window(torch.float32), window_f64().float())
    # ... and the six distinct taps of the kernels are those values
    src = open(os.path.join(ROOT, "gsasr_amd", "csrc", "splat_ssim.hip")).read()
    taps = [float(v) for v in re.findall(r"(\d\.\d+e-0\d)f", src[src.index("ss_g(int j)"):src.index("struct SsimArgs")])]
    assert len(taps) == 6 and np.array_equal(np.float32(taps), window_f64().float().numpy()[5:])


def test_identical_images_have_zero_loss():
    x, _ = make_input("noise", 24, 31)
    assert abs(float(ssim_loss(x, x.clone()))) <= 1e-6
    assert abs(float(ssim_loss(x.double(), x.double().clone()))) <= 1e-14


def test_batch_averaging_sizes_and_taller_target():
    B, (H, W) = len(BATCH_SIZES), (24, 40)
    g = torch.Generator().manual_seed(3)
    x = torch.rand(B, 3, H, W, generator=g).requires_grad_(True)
    y = torch.rand(B, 3, 29, W, generator=g)
    total, per = ssim_loss(x, y, 0.6, BATCH_SIZES, return_per_sample=True)
    assert total.dim() == 0 and tuple(per.shape) == (B,) and not per.requires_grad
    want = [ssim_f64(x[b, :, :h, :w], y[b, :, :h, :w], 0.6, B) for b, (h, w) in enumerate(BATCH_SIZES)]
    assert np.allclose(per.numpy(), [v for v, _ in want], rtol=1e-5, atol=1e-6)
    assert abs(float(total.detach()) - sum(v for v, _ in want) / B) <= 1e-5
    total.backward()
    for b, (h, w) in enumerate(BATCH_SIZES):
        assert float((x.grad[b, :, :h, :w] - want[b][1]).abs().max()) <= 1e-4 * float(want[b][1].abs().max())
        assert not x.grad[b, :, h:].any() and not x.grad[b, :, :, w:].any()         # the padding takes no part
    # default sizes: every sample whole; a single image is a batch of one
    full = ssim_loss(x.detach(), y[:, :, :H])
    assert abs(float(full) - np.mean([ssim_f64(x[b], y[b, :, :H])[0] for b in range(B)])) <= 1e-5
    assert float(ssim_loss(x[1].detach(), y[1])) == pytest.approx(ssim_f64(x[1], y[1, :, :H])[0], abs=1e-5)


def test_python_argument_errors():
    x, y = torch.rand(2, 3, 24, 20), torch.rand(2, 3, 24, 20)
    with pytest.raises(ValueError, match="require grad"):
        ssim_loss(x, y.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="smaller than"):
        ssim_loss(x, y, sizes=[(24, 20), (10, 20)])
    with pytest.raises(ValueError, match="smaller than"):
        ssim_loss(torch.rand(3, 24, 10), torch.rand(3, 24, 10))
    with pytest.raises(ValueError, match="larger"):
        ssim_loss(x, y, sizes=[(24, 20), (25, 20)])
    with pytest.raises(ValueError, match="one \\(h, w\\)"):
        ssim_loss(x, y, sizes=[(24, 20)])
    with pytest.raises(ValueError, match="shape"):
        ssim_loss(x, torch.rand(2, 3, 24, 21))
    with pytest.raises(ValueError, match="shape"):
        ssim_loss(torch.rand(2, 1, 24, 20), torch.rand(2, 1, 24, 20))
    with pytest.raises(ValueError, match="rows"):
        ssim_loss(x, torch.rand(2, 3, 23, 20))
    with pytest.raises(ValueError, match="floating"):
        ssim_loss(x, (y * 255).to(torch.uint8))


# ---- the C ABI ------------------------------------------------------------------------------------------------------------
SSIM_SYMBOLS = ("gsasr_ssim_scratch_bytes", "gsasr_ssim_loss")
HOST = (ctypes.c_float * 64)()
PTR = ctypes.cast(HOST, ctypes.c_void_p).value      # a host stand-in for every pointer: never dereferenced


def test_header_bindings_and_library_agree_on_the_ssim_entry_points():
    hdr = open(os.path.join(ROOT, "include", "gsasr_splat.h")).read()
    assert re.search(r"typedef struct gsasr_ssim \{[^}]*int batch, rows, w;[^}]*int target_rows;[^}]*int grad_rows;[^}]*"
                     r"const int \*sample_hw;[^}]*float weight;[^}]*unsigned flags;[^}]*const float \*img, \*target;[^}]*"
                     r"float \*grad_img;[^}]*float \*loss;[^}]*void \*scratch;[^}]*\} gsasr_ssim;", hdr)
    assert re.search(r"#define GSASR_SSIM_GRAD_HWC 1u\b", hdr) and re.search(r"#define GSASR_SSIM_ACCUMULATE 2u\b", hdr)
    assert (_cabi.SSIM_GRAD_HWC, _cabi.SSIM_ACCUMULATE) == (1, 2)
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(gsasr_[a-z_0-9]+)\s*\(", code))
    L = ctypes.CDLL(_cabi.LIB_PATH)
    for name in SSIM_SYMBOLS:
        assert name in declared and name in _cabi.EXPORTS and hasattr(L, name), name
    assert declared == set(_cabi.EXPORTS), declared ^ set(_cabi.EXPORTS)
    # additive: the version and every existing struct stay
    assert _cabi.lib().gsasr_abi_version() == 7 and "#define GSASR_SPLAT_ABI_VERSION 7" in hdr
    assert ctypes.sizeof(_cabi.Dims) == 64 and ctypes.sizeof(_cabi.View) == 16 and ctypes.sizeof(_cabi.Loss) == 64
    assert ctypes.sizeof(_cabi.Ssim) == 80


def descriptor(sizes=None, batch=1, rows=24, w=40, **kw):
    d = _cabi.make_ssim(batch, rows, w, sizes, kw.pop("target_rows", 0), kw.pop("grad_rows", 0), 1.0, kw.pop("flags", 0))
    f = dict(img=PTR, target=PTR, grad_img=PTR, loss=PTR, scratch=PTR)
    f.update(kw)
    for k, v in f.items():
        setattr(d, k, v)
    return d


BAD = {
    "null img": lambda: descriptor(img=None),
    "null target": lambda: descriptor(target=None),
    "null loss": lambda: descriptor(loss=None),
    "null scratch": lambda: descriptor(scratch=None),
    "sample 10 rows": lambda: descriptor([(10, 40)]),
    "sample 10 columns": lambda: descriptor([(24, 40), (24, 10)], batch=2),
    "image 10 columns": lambda: descriptor(w=10),
    "sample taller than rows": lambda: descriptor([(25, 40)]),
    "sample wider than w": lambda: descriptor([(24, 41)]),
    "target_rows below a sample's height": lambda: descriptor([(24, 40), (11, 11)], batch=2, target_rows=23),
    "grad_rows below a sample's height": lambda: descriptor([(11, 11), (24, 40)], batch=2, grad_rows=23),
    "unknown flag": lambda: descriptor(flags=4),
    "batch 0": lambda: descriptor(batch=0),
    "batch 65": lambda: descriptor(batch=65),
}


@pytest.mark.parametrize("case", sorted(BAD), ids=lambda c: c.replace(" ", "_").replace("'", ""))
def test_illegal_arguments_are_refused_before_anything_is_enqueued(case):
    L = _cabi.lib()
    d = BAD[case]()
    assert L.gsasr_ssim_loss(ctypes.byref(d), None) == -1 and L.gsasr_last_error(), case      # GSASR_ERR_ARG, with a message
    if not case.startswith("null"):
        assert L.gsasr_ssim_scratch_bytes(ctypes.byref(d)) == 0
    assert L.gsasr_ssim_loss(None, None) == -1 and L.gsasr_ssim_scratch_bytes(None) == 0


def test_scratch_bytes():
    L = _cabi.lib()
    for d in (descriptor(), descriptor(BATCH_SIZES, batch=3, target_rows=29), descriptor(batch=16, rows=192, w=192)):
        n = L.gsasr_ssim_scratch_bytes(ctypes.byref(d))
        tiles = 3 * d.batch * ((d.rows - 10 + 31) // 32) * ((d.w - 10 + 31) // 32)
        assert n % 4 == 0 and n >= 4 * tiles + 36 * d.batch * d.rows * d.w        # partials + three derivative maps per channel
        d.grad_img = None                                                           # value only: the partials alone
        m = L.gsasr_ssim_scratch_bytes(ctypes.byref(d))
        assert 4 * tiles <= m < 4 * tiles + 256 and m == n - 36 * d.batch * d.rows * d.w


# ---- ssim_weight of the fused pixel loss, CPU path -----------------------------------------------------------------------
def parameters(n=96, seed=5, batch=None):
    g = torch.Generator().manual_seed(seed)
    shape = (n, 9) if batch is None else (batch, n, 9)
    p = 0.5 * torch.randn(*shape, generator=g)
    p[..., 7:9] = torch.rand(*shape[:-1], 2, generator=g)
    return p


def test_ssim_weight_argument_errors():
    p, t = parameters(), torch.rand(3, 24, 20)
    with pytest.raises(ValueError, match="reduction"):
        gsp.generate_2D_gaussian_splatting_loss((24, 20), p, 2.0, [2.0, 2.0], t, reduction="sum", ssim_weight=0.5)
    with pytest.raises(ValueError, match="smaller than"):
        gsp.generate_2D_gaussian_splatting_loss((24, 20), p, 2.0, [2.0, 2.0], t[:, :10, :12], window=(2, 3, 10, 12), ssim_weight=0.5)
    with pytest.raises(ValueError, match="smaller than"):
        gsp.generate_2D_gaussian_splatting_loss((24, 10), p, 2.0, [2.0, 2.0], t[:, :, :10], ssim_weight=0.5)
    pb, sizes = parameters(batch=2), [(24, 20), (10, 13)]
    bargs = (sizes, pb, [2.0, 2.0], [[2.0, 2.0]] * 2, torch.rand(2, 3, 24, 20))
    with pytest.raises(ValueError, match="smaller than"):
        gsp.generate_2D_gaussian_splatting_batch_loss(*bargs, ssim_weight=0.5)
    with pytest.raises(ValueError, match="reduction"):
        gsp.generate_2D_gaussian_splatting_batch_loss(*bargs, reduction="sum", ssim_weight=0.5)
    # the same calls without the SSIM term are legal
    assert gsp.generate_2D_gaussian_splatting_batch_loss(*bargs).dim() == 0


def test_ssim_weight_zero_changes_nothing_on_the_cpu_path():
    H, W = 24, 20
    p, t = parameters(seed=7), torch.rand(3, H, W, generator=torch.Generator().manual_seed(8))
    args = ((H, W), p, 2.0, [2.0, 2.0], t)
    for kw in (dict(loss="l1"), dict(loss="mse", reduction="sum", loss_weight=0.7), dict(loss="charbonnier", window=(3, 5, 12, 11))):
        tt = t if "window" not in kw else t[:, 3:15, 5:16]
        a = (args[:4] + (tt,))
        plain = gsp.generate_2D_gaussian_splatting_loss(*a, **kw)
        assert torch.equal(plain, gsp.generate_2D_gaussian_splatting_loss(*a, ssim_weight=0.0, **kw))
        value, (l_pix, l_ssim) = gsp.generate_2D_gaussian_splatting_loss(*a, return_terms=True, **kw)
        assert torch.equal(value, plain) and torch.equal(l_pix, plain) and float(l_ssim) == 0.0
        value, image, terms = gsp.generate_2D_gaussian_splatting_loss(*a, return_image=True, return_terms=True, **kw)
        assert torch.equal(value, plain) and image.shape[0] == 3 and len(terms) == 2


@pytest.mark.parametrize("window", [None, (3, 5, 12, 11)], ids=["image", "window"])
def test_ssim_weight_single_image_is_pixel_loss_plus_ssim(window):
    H, W = 24, 20
    p = parameters(seed=7).requires_grad_(True)
    plain = gsp.generate_2D_gaussian_splatting_step((H, W), p, 2.0, [2.0, 2.0], cuda_rendering=False)
    if window is not None:
        plain = plain[:, 3:15, 5:16]
    t = torch.rand(plain.shape, generator=torch.Generator().manual_seed(8))
    value, image, (l_pix, l_ssim) = gsp.generate_2D_gaussian_splatting_loss((H, W), p, 2.0, [2.0, 2.0], t, loss="l1", loss_weight=0.7,
                                                                           window=window, return_image=True, ssim_weight=0.5,
                                                                           return_terms=True)
    assert torch.equal(image, plain.detach()) and not l_pix.requires_grad and not l_ssim.requires_grad and l_pix.dim() == l_ssim.dim() == 0
    want_pix = gsp._pixel_loss(plain, t, "l1", 0.7, 1e-12, "mean")
    want_ssim = ssim_mod.ssim_torch(plain, t, 0.5)
    assert torch.equal(l_pix, want_pix.detach()) and torch.equal(l_ssim, want_ssim.detach())
    assert torch.equal(value.detach(), (want_pix + want_ssim).detach())
    assert abs(float(l_ssim) - ssim_f64(plain, t, 0.5)[0]) <= 1e-5
    value.backward()
    got = p.grad.clone()
    p.grad = None
    (want_pix + want_ssim).backward()
    assert float((got - p.grad).abs().max()) <= 1e-6 * float(p.grad.abs().max())


def test_ssim_weight_batch_on_the_per_sample_path():
    sizes = [(24, 20), (17, 13), (11, 20)]
    B = len(sizes)
    p = parameters(n=64, seed=9, batch=B).requires_grad_(True)
    padded = torch.rand(B, 3, 27, 20, generator=torch.Generator().manual_seed(10))
    scales, sms = [2.0] * B, [[2.0, 2.0]] * B
    total, per, images, (l_pix, l_ssim) = gsp.generate_2D_gaussian_splatting_batch_loss(
        sizes, p, scales, sms, padded, loss="mse", loss_weight=1.3, return_per_sample=True, return_images=True, ssim_weight=0.5,
        return_terms=True)
    assert total.dim() == 0 and tuple(per.shape) == (B,) and tuple(images.shape) == (B, 3, 24, 20)
    pix, ssm = [], []
    for b, (h, w) in enumerate(sizes):
        out = gsp.generate_2D_gaussian_splatting_step(sizes[b], p[b], 2.0, [2.0, 2.0], cuda_rendering=False).detach()
        pix.append(float(gsp._pixel_loss(out, padded[b, :, :h, :w], "mse", 1.3, 1e-12, "mean")))
        ssm.append(ssim_f64(out, padded[b, :, :h, :w], 0.5)[0])
    assert np.allclose(per.numpy(), np.add(pix, ssm), rtol=2e-5)
    assert abs(float(l_pix) - np.mean(pix)) <= 2e-5 * np.mean(pix) and abs(float(l_ssim) - np.mean(ssm)) <= 2e-5
    assert abs(float(total.detach()) - np.mean(pix) - np.mean(ssm)) <= 2e-5
    total.backward()
    assert bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0
    # windows: patches [B,3,hmax,wmax]; without the terms the return is what it was
    wins = [(2, 3, 12, 12), (0, 0, 17, 13), (0, 4, 11, 16)]
    patches = torch.rand(B, 3, 17, 16, generator=torch.Generator().manual_seed(11))
    got = gsp.generate_2D_gaussian_splatting_batch_loss(sizes, p.detach(), scales, sms, patches, windows=wins, ssim_weight=0.5)
    want = 0.0
    for b, (y0, x0, h, w) in enumerate(wins):
        out = gsp.generate_2D_gaussian_splatting_step(sizes[b], p[b].detach(), 2.0, [2.0, 2.0], cuda_rendering=False)[:, y0:y0 + h, x0:x0 + w]
        want += float(gsp._pixel_loss(out, patches[b, :, :h, :w], "l1", 1.0, 1e-12, "mean")) + ssim_f64(out, patches[b, :, :h, :w], 0.5)[0]
    assert got.dim() == 0 and abs(float(got) - want / B) <= 2e-5
