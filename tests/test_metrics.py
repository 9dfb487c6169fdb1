"""Validation metrics of an 8-bit picture (gsasr_image_metrics; gsasr_amd.metrics): what can be checked without a GPU -- the
float64 restatement of the reference the GPU tests measure against, pinned three ways; the CPU path of the public functions
against it; the ABI surface and the argument checks of the header (they come before anything is enqueued).
tests/test_metrics_gpu.py has the kernels.

The restatement (`psnr_f64`, `ssim_f64`, `to_y_f64`) is written from basicsr/metrics/psnr_ssim.py:12-48 (calculate_psnr),
85-128 (calculate_ssim), 170-198 (_ssim), basicsr/metrics/metric_util.py:32-45 (to_y_channel) and
basicsr/utils/color_util.py:38-68 (bgr2ycbcr) with NumPy alone: cv2.filter2D with the 11 x 11 window cut to [5:-5, 5:-5] is a
direct 2-D "valid" correlation with outer(g, g), and cv2.getGaussianKernel(11, 1.5) is exp(-(i - 5)^2 / (2 * 1.5^2)) normalised.

Bars of everything that is not float64 end to end (the Y mode, whose values pass through float32 twice, and the kernels):
    RGB PSNR  1e-9 relative      (the sum of squares is an exact integer)
    Y PSNR    5e-4 dB            (a Y off by one fp32 ulp, at most 3e-5 with both pictures, moves mse by at most 2 dY / rms: 6e-5
                                  relative at rms >= 1, 2.6e-4 dB -- `make_pair` keeps rms >= 1 and the tests assert it)
    SSIM      5e-6 absolute      (a tenth of half a unit of the fourth decimal the validation log prints)"""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from gsasr_amd import _cabi
from gsasr_amd import gaussian_splatting as gsp
from gsasr_amd import metrics as M
from gsasr_amd import ssim as ssim_mod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR_PSNR_RGB, BAR_PSNR_Y, BAR_SSIM = 1e-9, 5e-4, 5e-6
C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2          # psnr_ssim.py:183-184


# ---- the restatement ------------------------------------------------------------------------------------------------------
def window_f64():
    """psnr_ssim.py:185-186: cv2.getGaussianKernel(11, 1.5) and its outer product"""
    g = np.exp(-((np.arange(11, dtype=np.float64) - 5.0) ** 2) / (2.0 * 1.5 ** 2))
    g /= g.sum()
    return np.outer(g, g)


def to_y_f64(img, bgr=True):
    """metric_util.py:32-45 on a uint8 [h,w,C] picture -> float32 [h,w,1] in [0, 255] (the caller widens it, as
    psnr_ssim.py:42-43 / 122-123 do).  The reference's pictures are BGR; an RGB picture is the reference on its flipped bytes."""
    x = img.astype(np.float32) / np.float32(255.)                           # metric_util.py:41
    if x.ndim == 3 and x.shape[2] == 3:
        if not bgr:
            x = x[..., ::-1]
        y = np.dot(x, [24.966, 128.553, 65.481]) + 16.0                     # color_util.py:63 (float64: the weights are doubles)
        x = (y / 255.).astype(np.float32)[..., None]                        # color_util.py:67 (_convert_output_type_range), metric_util.py:44
    return x * np.float32(255.)                                            # metric_util.py:45


def _prepare(img, ref, cb, y, bgr):
    if img.ndim == 2:
        img, ref = img[..., None], ref[..., None]                           # metric_util.py:25-26
    if cb != 0:                                                             # psnr_ssim.py:34-36
        img, ref = img[cb:-cb, cb:-cb, ...], ref[cb:-cb, cb:-cb, ...]
    if y:                                                                   # psnr_ssim.py:38-40
        img, ref = to_y_f64(img, bgr), to_y_f64(ref, bgr)
    return img.astype(np.float64), ref.astype(np.float64)                   # psnr_ssim.py:42-43


def psnr_f64(img, ref, cb=0, y=False, bgr=True):
    a, b = _prepare(img, ref, cb, y, bgr)
    mse = np.mean((a - b) ** 2)                                             # psnr_ssim.py:45
    return float('inf') if mse == 0 else float(10. * np.log10(255. * 255. / mse))   # psnr_ssim.py:46-48


def ssim_channel_f64(a, b):
    """psnr_ssim.py:170-198 for one channel, float64 [h,w]"""
    win = window_f64()
    blur = lambda t: np.einsum("ijkl,kl->ij", np.lib.stride_tricks.sliding_window_view(t, (11, 11)), win)      # noqa: E731
    mu1, mu2 = blur(a), blur(b)                                             # :188-189
    s1, s2, s12 = blur(a ** 2) - mu1 ** 2, blur(b ** 2) - mu2 ** 2, blur(a * b) - mu1 * mu2         # :193-195
    return float((((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 ** 2 + mu2 ** 2 + C1) * (s1 + s2 + C2))).mean())    # :197-198


def ssim_f64(img, ref, cb=0, y=False, bgr=True):
    a, b = _prepare(img, ref, cb, y, bgr)
    return float(np.array([ssim_channel_f64(a[..., i], b[..., i]) for i in range(a.shape[2])]).mean())      # psnr_ssim.py:125-128


# ---- inputs (shared with the GPU tests) ------------------------------------------------------------------------------------
def make_pair(h, w, seed=0, noise=3.0):
    """(img, ref) uint8 [h,w,3]: ref a smooth random field plus texture, quantised; img = ref plus Gaussian noise of about
    `noise` levels, clipped and quantised -- an rms error of at least one level"""
    rng = np.random.RandomState(1000 * seed + 10 * h + w)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    field = np.zeros((h, w, 3))
    for c in range(3):
        for _ in range(4):
            fx, fy, ph, amp = rng.uniform(-0.15, 0.15), rng.uniform(-0.15, 0.15), rng.uniform(0, 2 * np.pi), rng.uniform(15, 40)
            field[..., c] += amp * np.sin(fx * xx + fy * yy + ph)
    ref = np.clip(np.rint(128.0 + field + 10.0 * rng.randn(h, w, 3)), 0, 255).astype(np.uint8)
    img = np.clip(np.rint(ref.astype(np.float64) + noise * rng.randn(h, w, 3)), 0, 255).astype(np.uint8)
    return img, ref


def rms(img, ref, cb=0, y=False, bgr=True):
    """of the values the metric is defined on: the bytes, or Y"""
    a, b = _prepare(img, ref, cb, y, bgr)
    return float(np.sqrt(np.mean((a - b) ** 2)))


# ---- the restatement, pinned ---------------------------------------------------------------------------------------------
def test_restatement_closed_forms():
    img, ref = make_pair(24, 31)
    for y in (False, True):
        assert psnr_f64(ref, ref, 0, y) == float('inf') and ssim_f64(ref, ref, 0, y) == 1.0
    # ref and ref + d without clipping: mse = d^2
    base = (ref // 2 + 20).astype(np.uint8)
    for d in (1, 7, 60):
        assert abs(psnr_f64(base + np.uint8(d), base, 2) - 20.0 * math.log10(255.0 / d)) <= 1e-12
    # two constant pictures: no variance, the luminance term alone
    for a, b in ((0, 255), (100, 103), (17, 17), (255, 254)):
        pa, pb = np.full((13, 16, 3), a, np.uint8), np.full((13, 16, 3), b, np.uint8)
        assert abs(ssim_f64(pa, pb) - (2.0 * a * b + C1) / (a * a + b * b + C1)) <= 1e-12


def test_restatement_agrees_with_ssim_map_in_float64():
    for (h, w), cb in (((24, 31), 0), ((45, 77), 4), ((11, 11), 0)):
        img, ref = make_pair(h, w, seed=1)
        a, b = _prepare(img, ref, cb, False, True)
        m = ssim_mod.ssim_map(torch.from_numpy(a / 255.0).permute(2, 0, 1), torch.from_numpy(b / 255.0).permute(2, 0, 1))
        assert tuple(m.shape) == (3, h - 2 * cb - 10, w - 2 * cb - 10)
        assert abs(float(m.mean()) - ssim_f64(img, ref, cb)) <= 1e-12
        for c in range(3):
            assert abs(float(m[c].mean()) - ssim_channel_f64(a[..., c], b[..., c])) <= 1e-12


def test_restatement_y_weights():
    white, black = np.full((2, 2, 3), 255, np.uint8), np.zeros((2, 2, 3), np.uint8)
    ulp = 1.5e-5        # of float32 at this magnitude
    assert np.abs(to_y_f64(white).astype(np.float64) - 235.0).max() <= ulp and to_y_f64(white).shape == (2, 2, 1)
    assert np.abs(to_y_f64(black).astype(np.float64) - 16.0).max() <= ulp
    # which byte is which: a pure first byte is blue in a BGR picture (weight 24.966), red in an RGB one (65.481)
    first = np.zeros((1, 1, 3), np.uint8)
    first[..., 0] = 255
    assert abs(float(to_y_f64(first, bgr=True)[0, 0, 0]) - 40.966) <= ulp and abs(float(to_y_f64(first, bgr=False)[0, 0, 0]) - 81.481) <= ulp
    # a single channel is the byte itself
    grey = np.arange(256, dtype=np.uint8).reshape(16, 16, 1)
    assert np.array_equal(to_y_f64(grey).astype(np.float64), grey.astype(np.float64))


# ---- the public functions, CPU path ---------------------------------------------------------------------------------------
def as_input(a, kind, order):
    if order == "CHW":
        a = np.ascontiguousarray(a.transpose(2, 0, 1))
    elif order == "grey":
        a = np.ascontiguousarray(a[..., 1])
    return a if kind == "numpy" else torch.from_numpy(a)


@pytest.mark.parametrize("cb", [0, 4])
@pytest.mark.parametrize("kind", ["numpy", "torch"])
@pytest.mark.parametrize("order", ["HWC", "CHW", "grey"])
def test_calculate_functions_against_the_restatement(order, kind, cb):
    img, ref = make_pair(29, 38, seed=2)
    assert rms(img, ref, cb) >= 1.0 and (order == "grey" or rms(img, ref, cb, True) >= 1.0)
    a, b = as_input(img, kind, order), as_input(ref, kind, order)
    ra, rb = (img[..., 1], ref[..., 1]) if order == "grey" else (img, ref)
    io = "CHW" if order == "CHW" else "HWC"
    p, s = M.calculate_psnr(a, b, cb, input_order=io), M.calculate_ssim(a, b, cb, input_order=io)
    assert isinstance(p, float) and isinstance(s, float)
    assert abs(p - psnr_f64(ra, rb, cb)) <= 1e-12 * psnr_f64(ra, rb, cb) and abs(s - ssim_f64(ra, rb, cb)) <= 1e-12
    py, sy = M.calculate_psnr(a, b, cb, io, test_y_channel=True), M.calculate_ssim(a, b, cb, io, test_y_channel=True)
    e_p, e_s = abs(py - psnr_f64(ra, rb, cb, True)), abs(sy - ssim_f64(ra, rb, cb, True))
    print(f"{order} {kind} cb={cb}: Y mode psnr error {e_p:.3e} dB, ssim error {e_s:.3e}")
    assert e_p <= BAR_PSNR_Y and e_s <= BAR_SSIM
    assert M.calculate_psnr(a, a, cb, io) == float('inf') and M.calculate_ssim(a, a, cb, io, test_y_channel=True) == 1.0


def test_image_metrics_cpu_single_batch_and_sizes():
    img, ref = make_pair(45, 77, seed=3)
    for y in (False, True):
        for bgr in (False, True):
            got = M.image_metrics(torch.from_numpy(img), torch.from_numpy(ref), 4, y, bgr)
            assert got.dtype == torch.float64 and tuple(got.shape) == (2,)
            want = psnr_f64(img, ref, 4, y, bgr)
            assert abs(float(got[0]) - want) <= (BAR_PSNR_Y if y else 1e-12 * want)
            assert abs(float(got[1]) - ssim_f64(img, ref, 4, y, bgr)) <= (BAR_SSIM if y else 1e-12)
    sizes = [(33, 45), (45, 77), (21, 60)]
    cimg, cref = np.full((3, 45, 77, 3), 255, np.uint8), np.zeros((3, 45, 77, 3), np.uint8)
    for b, (h, w) in enumerate(sizes):
        cimg[b, :h, :w], cref[b, :h, :w] = make_pair(h, w, seed=4 + b)
    got = M.image_metrics(torch.from_numpy(cimg), torch.from_numpy(cref), 2, sizes=sizes)
    assert tuple(got.shape) == (3, 2)
    for b, (h, w) in enumerate(sizes):
        one = M.image_metrics(torch.from_numpy(cimg[b, :h, :w]), torch.from_numpy(cref[b, :h, :w]), 2)
        assert torch.equal(got[b], one) and abs(float(one[1]) - ssim_f64(cimg[b, :h, :w], cref[b, :h, :w], 2)) <= 1e-12


def test_python_argument_errors():
    img, ref = (torch.from_numpy(a) for a in make_pair(24, 31))
    with pytest.raises(ValueError, match="Image shapes are different"):
        M.calculate_psnr(img.numpy(), ref.numpy()[:, :30], 0)
    with pytest.raises(ValueError, match="Image shapes are different"):
        M.image_metrics(img, ref[:23])
    for fn in (M.calculate_psnr, M.calculate_ssim):
        with pytest.raises(ValueError, match='Wrong input_order WHC. Supported input_orders are "HWC" and "CHW"'):
            fn(img, ref, 0, input_order="WHC")
        with pytest.raises(ValueError, match="uint8"):
            fn(img.float(), ref.float(), 0)
        with pytest.raises(ValueError, match="negative"):
            fn(img, ref, -1)
    with pytest.raises(ValueError, match="leaves no pixel"):
        M.calculate_psnr(img, ref, 12)
    with pytest.raises(ValueError, match="smaller than"):
        M.calculate_ssim(img, ref, 7)                      # 10 x 17 left
    assert M.calculate_psnr(img, ref, 7) > 0               # ... which PSNR takes
    with pytest.raises(ValueError, match="smaller than"):
        M.image_metrics(img, ref, 7)
    with pytest.raises(ValueError, match="uint8"):
        M.image_metrics(img.float(), ref)
    with pytest.raises(ValueError, match="expected"):
        M.image_metrics(img[..., :2], ref[..., :2])
    with pytest.raises(ValueError, match="one \\(h, w\\)"):
        M.image_metrics(img[None], ref[None], sizes=[(24, 31), (24, 31)])
    with pytest.raises(ValueError, match="larger"):
        M.image_metrics(img[None], ref[None], sizes=[(25, 31)])


def test_package_exports():
    import gsasr_amd
    assert gsasr_amd.image_metrics is M.image_metrics and gsasr_amd.calculate_psnr is M.calculate_psnr
    assert gsasr_amd.calculate_ssim is M.calculate_ssim


def test_fused_function_on_the_cpu_path():
    g = torch.Generator().manual_seed(5)
    p = 0.5 * torch.randn(96, 9, generator=g)
    p[..., 7:9] = torch.rand(96, 2, generator=g)
    gt = torch.from_numpy(make_pair(22, 19, seed=6)[1])
    args = ((24, 20), p, 2.0, [2.0, 2.0])
    picture, m = gsp.generate_2D_gaussian_splatting_step_uint8_metrics(*args, gt, crop_border=2, test_y_channel=True, bgr=True)
    assert torch.equal(picture, gsp.generate_2D_gaussian_splatting_step_uint8(*args, crop=(22, 19), bgr=True))
    assert torch.equal(m, M.image_metrics(picture, gt, 2, True, True)) and tuple(m.shape) == (2,)
    with pytest.raises(ValueError, match="Image shapes are different"):
        gsp.generate_2D_gaussian_splatting_step_uint8_metrics(*args, gt, crop=(22, 20))
    with pytest.raises(ValueError, match="uint8"):
        gsp.generate_2D_gaussian_splatting_step_uint8_metrics(*args, gt.float())


# ---- the C ABI ------------------------------------------------------------------------------------------------------------
METRIC_SYMBOLS = ("gsasr_metrics_scratch_bytes", "gsasr_image_metrics")
HOST = (ctypes.c_double * 64)()
PTR = ctypes.cast(HOST, ctypes.c_void_p).value      # a host stand-in for every pointer: never dereferenced


def test_header_bindings_and_library_agree_on_the_metrics_entry_points():
    hdr = open(os.path.join(ROOT, "include", "gsasr_splat.h")).read()
    assert re.search(r"typedef struct gsasr_metrics \{[^}]*int batch, h, w;[^}]*const int \*sample_hw;[^}]*const unsigned char \*img;[^}]*"
                     r"size_t img_pitch, img_stride;[^}]*const unsigned char \*ref;[^}]*size_t ref_pitch, ref_stride;[^}]*"
                     r"int crop_border;[^}]*unsigned flags;[^}]*double \*out;[^}]*void \*scratch;[^}]*\} gsasr_metrics;", hdr)
    for name, value in (("PSNR", 1), ("SSIM", 2), ("Y", 4), ("BGR", 8)):
        assert re.search(rf"#define GSASR_METRIC_{name} {value}u\b", hdr) and getattr(_cabi, "METRIC_" + name) == value
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(gsasr_[a-z_0-9]+)\s*\(", code))
    L = ctypes.CDLL(_cabi.LIB_PATH)
    for name in METRIC_SYMBOLS:
        assert name in declared and name in _cabi.EXPORTS and hasattr(L, name), name
    assert declared == set(_cabi.EXPORTS), declared ^ set(_cabi.EXPORTS)
    # additive: the version and every existing struct stay
    assert _cabi.lib().gsasr_abi_version() == 7 and "#define GSASR_SPLAT_ABI_VERSION 7" in hdr
    assert ctypes.sizeof(_cabi.Dims) == 64 and ctypes.sizeof(_cabi.Ssim) == 80 and ctypes.sizeof(_cabi.Metrics) == 96
    # the contract is stated in the header, and the new unit is part of the build
    for words in ("crop_border", "24.966", "128.553", "65.481", "(0.01 * 255)^2", "+inf", "left untouched"):
        assert words in hdr, words
    from gsasr_amd import build
    assert "splat_metrics" in build.PARTS
    assert '#include "splat_metrics.hip"' in open(os.path.join(ROOT, "gsasr_amd", "csrc", "gsasr_splat.hip")).read()


def test_window_taps_of_the_kernel():
    src = open(os.path.join(ROOT, "gsasr_amd", "csrc", "splat_metrics.hip")).read()
    taps = [float(v) for v in re.findall(r"(0\.\d{10,})", src[src.index("mt_g(int j)"):src.index("struct MetricArgs")])]
    g = window_f64()[5] / window_f64()[5].sum()
    assert len(taps) == 6 and np.abs(np.array(taps) - g[5:]).max() <= 1e-17


def descriptor(sizes=None, batch=1, h=24, w=40, cb=0, flags=3, **kw):
    d = _cabi.make_metrics(batch, h, w, sizes, cb, flags, kw.pop("img_pitch", None), None, kw.pop("ref_pitch", None), None)
    f = dict(img=PTR, ref=PTR, out=PTR, scratch=PTR)
    f.update(kw)
    for k, v in f.items():
        setattr(d, k, v)
    return d


BAD = {
    "null img": lambda: descriptor(img=None),
    "null ref": lambda: descriptor(ref=None),
    "null out": lambda: descriptor(out=None),
    "null scratch": lambda: descriptor(scratch=None),
    "img pitch below 3 w": lambda: descriptor(img_pitch=119),
    "ref pitch below 3 w": lambda: descriptor(ref_pitch=119),
    "batch 0": lambda: descriptor(batch=0),
    "batch 65": lambda: descriptor(batch=65),
    "no metric flag": lambda: descriptor(flags=4 | 8),
    "unknown flag": lambda: descriptor(flags=3 | 16),
    "negative crop_border": lambda: descriptor(cb=-1),
    "crop leaves no row": lambda: descriptor(cb=12, flags=1),
    "crop leaves no column": lambda: descriptor(h=60, w=24, cb=12, flags=1),
    "ssim with 10 rows left": lambda: descriptor(cb=7),
    "ssim with 10 columns left": lambda: descriptor(h=40, w=24, cb=7),
    "ssim on a sample of 10 rows": lambda: descriptor([(24, 40), (10, 40)], batch=2),
    "sample taller than h": lambda: descriptor([(25, 40)]),
    "sample wider than w": lambda: descriptor([(24, 41)]),
    "h above 32767": lambda: descriptor(h=32768),
    "w above 32767": lambda: descriptor(w=32768),
    "h 0": lambda: descriptor(h=0),
}


@pytest.mark.parametrize("case", sorted(BAD), ids=lambda c: c.replace(" ", "_"))
def test_illegal_arguments_are_refused_before_anything_is_enqueued(case):
    L = _cabi.lib()
    d = BAD[case]()
    assert L.gsasr_image_metrics(ctypes.byref(d), None) == -1 and L.gsasr_last_error(), case      # GSASR_ERR_ARG, with a message
    if not case.startswith("null"):
        assert L.gsasr_metrics_scratch_bytes(ctypes.byref(d)) == 0
    assert L.gsasr_image_metrics(None, None) == -1 and L.gsasr_last_error() and L.gsasr_metrics_scratch_bytes(None) == 0


def test_scratch_bytes():
    L = _cabi.lib()
    tiles = lambda n: (n + 31) // 32       # noqa: E731
    for d, nch in ((descriptor(), 3), (descriptor(cb=4, flags=1 | 4), 1), (descriptor([(33, 45), (64, 64), (21, 80)], batch=3, h=64, w=80), 3),
                   (descriptor(h=32767, w=32767, cb=100, flags=2), 3), (descriptor(cb=7, flags=1), 3)):
        n = L.gsasr_metrics_scratch_bytes(ctypes.byref(d))
        want = 16 * d.batch * nch * tiles(d.h - 2 * d.crop_border) * tiles(d.w - 2 * d.crop_border)      # two doubles per tile and channel
        assert n % 8 == 0 and want <= n < want + 256
