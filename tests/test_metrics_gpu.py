"""Validation metrics on the GPU (gsasr_image_metrics: k_metric_stats / k_metric_reduce of csrc/splat_metrics.hip) against the
float64 restatement of the reference in tests/test_metrics.py, on the same bytes.

Bars (tests/test_metrics.py derives them): RGB PSNR 1e-9 relative (the sum of squares is an exact integer); Y PSNR 5e-4 dB (the
inputs keep an rms error of at least one level, asserted); SSIM 5e-6 absolute in either mode.  Every case prints its errors.
Shapes are the smallest at which the part in question can go wrong: full and partial 32 x 32 tiles in both directions, a
one-pixel map, an error that sits only where no map tile reaches, the largest per-tile integer sums, every residue of the base
address modulo 4, a padded batch; then 4 x 5 tiles (interior ones), more items than the reduce kernel has lanes, and batches of
17 and 64 samples."""
import math
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
from test_metrics import BAR_PSNR_RGB, BAR_PSNR_Y, BAR_SSIM, C1, make_pair, psnr_f64, rms, ssim_f64      # noqa: E402

from gsasr_amd import _cabi      # noqa: E402
from gsasr_amd import gaussian_splatting as gsp      # noqa: E402
from gsasr_amd import metrics as M      # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the MI355X box)"
    return torch.device("cuda:0")


def check(got, img, ref, cb, y, bgr, what):
    """`got` = (psnr, ssim) of the kernels against the restatement on the same bytes, to the bars"""
    p, s = float(got[0]), float(got[1])
    wp, ws = psnr_f64(img, ref, cb, y, bgr), ssim_f64(img, ref, cb, y, bgr)
    e_p = 0.0 if p == wp else abs(p - wp)
    print(f"{what}: psnr {p:.9f} dB (error {e_p:.3e} dB, {e_p / abs(wp) if math.isfinite(wp) and wp else 0.0:.3e} relative), "
          f"ssim {s:.9f} (error {abs(s - ws):.3e})")
    if y:
        assert rms(img, ref, cb, True, bgr) >= 1.0
        assert e_p <= BAR_PSNR_Y, what
    else:
        assert e_p <= BAR_PSNR_RGB * abs(wp), what
    assert abs(s - ws) <= BAR_SSIM, what
    return p, s


@pytest.mark.parametrize("bgr", [False, True], ids=["rgb_bytes", "bgr_bytes"])
@pytest.mark.parametrize("y", [False, True], ids=["rgb", "y"])
@pytest.mark.parametrize("cb", [0, 4])
def test_full_and_partial_tiles(dev, cb, y, bgr):
    img, ref = make_pair(45, 77, seed=1)
    got = M.image_metrics(torch.from_numpy(img).to(dev), torch.from_numpy(ref).to(dev), cb, y, bgr)
    assert got.dtype == torch.float64 and tuple(got.shape) == (2,) and got.is_cuda
    check(got.cpu(), img, ref, cb, y, bgr, f"45x77 cb={cb} y={y} bgr={bgr}")


@pytest.mark.parametrize("shape,cb", [((19, 19), 4), ((11, 40), 0), ((40, 11), 0)], ids=["one_map_pixel", "strip_11x40", "strip_40x11"])
def test_smallest_maps(dev, shape, cb):
    img, ref = make_pair(*shape, seed=2)
    for y in (False, True):
        got = M.image_metrics(torch.from_numpy(img).to(dev), torch.from_numpy(ref).to(dev), cb, y, True)
        check(got.cpu(), img, ref, cb, y, True, f"{shape} cb={cb} y={y}")


def test_where_the_error_sits(dev):
    h, w, cb = 45, 77, 4
    _, ref = make_pair(h, w, seed=3)
    noise, _ = make_pair(h, w, seed=4)
    t = lambda a: torch.from_numpy(a).to(dev)      # noqa: E731
    # only inside the crop border: the metrics do not see it
    img = noise.copy()
    img[cb:h - cb, cb:w - cb] = ref[cb:h - cb, cb:w - cb]
    assert not np.array_equal(img, ref)
    for y in (False, True):
        got = M.image_metrics(t(img), t(ref), cb, y, True).cpu()
        assert float(got[0]) == float("inf") and float(got[1]) == 1.0
    # only in the last 10 rows / the last 10 columns of the cropped region: pixels that no tile of the valid map owns
    for name, region in (("last 10 rows", (slice(h - cb - 10, h - cb), slice(cb, w - cb))), ("last 10 columns", (slice(cb, h - cb), slice(w - cb - 10, w - cb)))):
        img = ref.copy()
        img[region] = np.clip(ref[region].astype(np.int64) + np.where(ref[region][..., 1:2] < 128, 8, -8), 0, 255).astype(np.uint8)
        for y in (False, True):
            p, _ = check(M.image_metrics(t(img), t(ref), cb, y, True).cpu(), img, ref, cb, y, True, f"{name} y={y}")
            assert math.isfinite(p)


def test_largest_tile_sums(dev):
    img, ref = np.zeros((64, 64, 3), np.uint8), np.full((64, 64, 3), 255, np.uint8)
    got = M.image_metrics(torch.from_numpy(img).to(dev), torch.from_numpy(ref).to(dev)).cpu()
    closed = C1 / (255.0 * 255.0 + C1)
    print(f"0 against 255: psnr {float(got[0])!r} dB, ssim {float(got[1])!r} (closed form {closed!r})")
    assert float(got[0]) == 0.0                             # mse = 255^2 exactly
    assert abs(float(got[1]) - closed) <= 1e-12             # double throughout: nothing here is within reach of 5e-6
    assert abs(ssim_f64(img, ref) - closed) <= 1e-12


def test_windows_and_alignment(dev):
    h, w = 40, 51
    img, ref = make_pair(h, w, seed=5)
    dense = {y: M.image_metrics(torch.from_numpy(img).to(dev), torch.from_numpy(ref).to(dev), 2, y, True) for y in (False, True)}
    check(dense[False].cpu(), img, ref, 2, False, True, "40x51 dense")
    check(dense[True].cpu(), img, ref, 2, True, True, "40x51 dense y")
    wide_ref = torch.full((45, 61, 3), 255, dtype=torch.uint8, device=dev)       # another pitch (183 bytes), another residue
    wide_ref[2:2 + h, 7:7 + w] = torch.from_numpy(ref).to(dev)
    for x0 in (0, 1, 2, 3):
        big = torch.full((50, 70, 3), 255, dtype=torch.uint8, device=dev)
        big[3:3 + h, x0:x0 + w] = torch.from_numpy(img).to(dev)
        view = big[3:3 + h, x0:x0 + w]
        assert not view.is_contiguous() and view.data_ptr() % 4 == (big.data_ptr() + 3 * 210 + 3 * x0) % 4
        for y in (False, True):
            assert torch.equal(M.image_metrics(view, torch.from_numpy(ref).to(dev), 2, y, True), dense[y]), (x0, y)
            assert torch.equal(M.image_metrics(view, wide_ref[2:2 + h, 7:7 + w], 2, y, True), dense[y]), (x0, y)


def test_batch_of_three(dev):
    sizes = [(33, 45), (64, 64), (21, 80)]
    cimg = np.full((3, 64, 80, 3), 255, np.uint8)
    cref = np.zeros((3, 64, 80, 3), np.uint8)
    for b, (h, w) in enumerate(sizes):
        cimg[b, :h, :w], cref[b, :h, :w] = make_pair(h, w, seed=6 + b)
    ti, tr = torch.from_numpy(cimg).to(dev), torch.from_numpy(cref).to(dev)
    for y in (False, True):
        got = M.image_metrics(ti, tr, 3, y, False, sizes=sizes)
        assert tuple(got.shape) == (3, 2)
        for b, (h, w) in enumerate(sizes):
            one = M.image_metrics(ti[b, :h, :w], tr[b, :h, :w], 3, y, False)
            assert torch.equal(got[b], one), (b, y)
            assert torch.equal(got[b], M.image_metrics(ti[b, :h, :w].contiguous(), tr[b, :h, :w].contiguous(), 3, y, False)), (b, y)
            check(got[b].cpu(), cimg[b, :h, :w], cref[b, :h, :w], 3, y, False, f"batch sample {b} y={y}")


# ---- more than 2 x 3 tiles, more than one trip of the reduce loop, more than 16 samples ------------------------------------
@pytest.mark.parametrize("bgr", [False, True], ids=["rgb_bytes", "bgr_bytes"])
@pytest.mark.parametrize("y", [False, True], ids=["rgb", "y"])
@pytest.mark.parametrize("cb", [0, 4])
def test_interior_tiles(dev, cb, y, bgr):
    """109 x 141: cropped by 4 it is 101 x 133, 4 x 5 tiles, of which 2 x 3 have a neighbour on every side"""
    img, ref = make_pair(109, 141, seed=20)
    got = M.image_metrics(torch.from_numpy(img).to(dev), torch.from_numpy(ref).to(dev), cb, y, bgr)
    check(got.cpu(), img, ref, cb, y, bgr, f"109x141 cb={cb} y={y} bgr={bgr}")


@pytest.mark.parametrize("shape,cb,y", [((300, 332), 4, False), ((544, 512), 0, True)], ids=["rgb_330_items", "y_272_items"])
def test_reduce_second_trip(dev, shape, cb, y):
    """k_metric_reduce adds a sample's channels x tiles with 256 lanes: 3 x 10 x 11 = 330 and 1 x 17 x 16 = 272 items"""
    hc, wc, nch = shape[0] - 2 * cb, shape[1] - 2 * cb, 1 if y else 3
    assert nch * ((hc + 31) // 32) * ((wc + 31) // 32) == (272 if y else 330)
    img, ref = make_pair(*shape, seed=21)
    got = M.image_metrics(torch.from_numpy(img).to(dev), torch.from_numpy(ref).to(dev), cb, y, True)
    check(got.cpu(), img, ref, cb, y, True, f"{shape} cb={cb} y={y}")


BIG_BATCH_SIZES = [(96, 112), (17, 17), (33, 45), (21, 112), (96, 20)]
_BIG_BATCH = {}


def big_batch(B):
    """[B,96,112,3] (3 x 4 tiles), sizes cycling; the padding holds 255 in img and 0 in ref: one leaked pixel moves PSNR by dBs"""
    if B not in _BIG_BATCH:
        sizes = [BIG_BATCH_SIZES[b % len(BIG_BATCH_SIZES)] for b in range(B)]
        cimg, cref = np.full((B, 96, 112, 3), 255, np.uint8), np.zeros((B, 96, 112, 3), np.uint8)
        for b, (h, w) in enumerate(sizes):
            cimg[b, :h, :w], cref[b, :h, :w] = make_pair(h, w, seed=30 + b)
        _BIG_BATCH[B] = (sizes, cimg, cref)
    return _BIG_BATCH[B]


@pytest.mark.parametrize("y", [False, True], ids=["rgb", "y"])
@pytest.mark.parametrize("B", [17, 64])
def test_batches_past_sixteen(dev, B, y):
    """every row of a batch of 17 and of 64 equals the single-sample call on the same view bit for bit, and is within the bars of
    the float64 restatement"""
    sizes, cimg, cref = big_batch(B)
    ti, tr = torch.from_numpy(cimg).to(dev), torch.from_numpy(cref).to(dev)
    got = M.image_metrics(ti, tr, 3, y, False, sizes=sizes)
    assert tuple(got.shape) == (B, 2)
    host = got.cpu()
    for b, (h, w) in enumerate(sizes):
        one = M.image_metrics(ti[b, :h, :w], tr[b, :h, :w], 3, y, False)
        assert torch.equal(got[b], one), (b, y)
        check(host[b], cimg[b, :h, :w], cref[b, :h, :w], 3, y, False, f"batch of {B} sample {b} y={y}")


def test_two_calls_and_one_metric_alone(dev):
    img, ref = make_pair(45, 77, seed=9)
    ti, tr = torch.from_numpy(img).to(dev), torch.from_numpy(ref).to(dev)
    for y in (False, True):
        a, b = _cabi.image_metrics(ti, tr, None, 4, y, True), _cabi.image_metrics(ti, tr, None, 4, y, True)
        assert torch.equal(a, b) and tuple(a.shape) == (1, 2)
        out = torch.full((1, 2), -7.5, dtype=torch.float64, device=dev)
        assert _cabi.image_metrics(ti, tr, None, 4, y, True, psnr=True, ssim=False, out=out) is out
        assert float(out[0, 1]) == -7.5 and float(out[0, 0]) == float(a[0, 0])
        out = torch.full((1, 2), -7.5, dtype=torch.float64, device=dev)
        _cabi.image_metrics(ti, tr, None, 4, y, True, psnr=False, ssim=True, out=out)
        assert float(out[0, 0]) == -7.5 and float(out[0, 1]) == float(a[0, 1])
    # PSNR alone has no 11 x 11 rule: a 10-row region
    got = _cabi.image_metrics(ti[:10], tr[:10], psnr=True, ssim=False)
    assert abs(float(got[0, 0]) - psnr_f64(img[:10], ref[:10])) <= BAR_PSNR_RGB * psnr_f64(img[:10], ref[:10])
    with pytest.raises(RuntimeError, match="smaller than the 11 x 11"):
        _cabi.image_metrics(ti[:10], tr[:10])
    # the innermost [w,3] must be dense, also where w == 1
    wide = torch.zeros(20, 1, 6, dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match="dense"):
        _cabi.image_metrics(wide[:, :, ::2], wide[:, :, ::2], psnr=True, ssim=False)
    with pytest.raises(RuntimeError, match="dense"):
        _cabi.image_metrics(ti[:, ::2], tr[:, ::2])


def one_channel_parameters(n_total, seed):
    """raw parameters [n_total, 9] of three wide Gaussians that each colour ONE channel (the other two raw colours are -200:
    sigmoid = 0 in fp32) among records whose alpha is sigmoid(-200) = 0.  The forward's sum over a pixel's Gaussians follows wave
    timing in general (tests/test_u8_output_gpu.py); here every channel of every pixel has one non-zero term, so two renders of
    the same parameters give the same bytes."""
    rng = np.random.RandomState(seed)
    p = np.zeros((n_total, 9), np.float32)
    p[:, 3] = -200.0
    p[:, 7:9] = rng.uniform(0, 1, (n_total, 2))
    for k, (cx, cy) in enumerate(((0.3, 0.4), (0.62, 0.5), (0.45, 0.72))):
        p[k, 0:2] = np.log(np.array([0.85, 0.7]) / (1 - np.array([0.85, 0.7]))) * rng.uniform(0.9, 1.0)
        p[k, 2] = rng.uniform(-0.4, 0.4)
        p[k, 3] = 6.0
        p[k, 4:7] = -200.0
        p[k, 4 + k] = 5.0
        p[k, 7:9] = (cx, cy)
    return torch.from_numpy(p)


def test_fused_render_and_metrics(dev):
    """300 records at 48 x 64, of which THREE Gaussians are live (`one_channel_parameters`): the bit-equality of two renders that
    this test is about needs a forward whose sums have one term, so the metrics are not run on a densely overlapped render here
    -- the dense, textured pictures of the other tests are what exercises the metric kernels."""
    H, W, n = 48, 64, 300
    p = one_channel_parameters(n, seed=11).to(dev)
    args = ((H, W), p, 8.0, [8.0, 8.0])
    plain = gsp.generate_2D_gaussian_splatting_step_uint8(*args, crop=(45, 61), bgr=True)
    assert int(plain.max()) > 200 and len(torch.unique(plain)) > 100 and all(int(plain[..., k].max()) > 200 for k in range(3))
    noisy = np.clip(np.rint(plain.cpu().numpy().astype(np.float64) + 3.0 * np.random.RandomState(12).randn(45, 61, 3)), 0, 255).astype(np.uint8)
    gt = torch.from_numpy(noisy).to(dev)
    for y in (False, True):
        picture, m = gsp.generate_2D_gaussian_splatting_step_uint8_metrics(*args, gt, crop_border=4, test_y_channel=y, bgr=True)
        assert picture.dtype == torch.uint8 and tuple(picture.shape) == (45, 61, 3) and torch.equal(picture, plain)
        assert torch.equal(m, M.image_metrics(picture, gt, 4, y, True)) and tuple(m.shape) == (2,) and m.is_cuda
        host = picture.cpu().numpy()
        check(m.cpu(), host, noisy, 4, y, True, f"fused y={y}")
        # the drop-in functions: on the host copy (the torch expression) and on the device tensors (the kernels)
        for a, b in ((host, noisy), (picture, gt)):
            check((M.calculate_psnr(a, b, 4, test_y_channel=y), M.calculate_ssim(a, b, 4, test_y_channel=y)), host, noisy, 4, y, True,
                  f"calculate_* on {'the device' if torch.is_tensor(a) else 'numpy'} y={y}")
    # grey and CHW pictures on the device are host-side reshapes in front of the same kernels
    grey_a, grey_b = picture[..., 1], gt[..., 1]
    got = (M.calculate_psnr(grey_a, grey_b, 4, test_y_channel=True), M.calculate_ssim(grey_a, grey_b, 4))
    assert abs(got[0] - psnr_f64(host[..., 1], noisy[..., 1], 4)) <= BAR_PSNR_RGB * got[0] and abs(got[1] - ssim_f64(host[..., 1], noisy[..., 1], 4)) <= BAR_SSIM
    chw = (M.calculate_psnr(picture.permute(2, 0, 1), gt.permute(2, 0, 1), 4, input_order="CHW"),
           M.calculate_ssim(picture.permute(2, 0, 1), gt.permute(2, 0, 1), 4, input_order="CHW"))
    check(chw, host, noisy, 4, False, True, "calculate_* CHW on the device")


def test_c_program_metrics(tmp_path):
    """the metrics from plain C (tests/c_abi/c_abi_metrics_check.c): built with gcc against libgsasr_splat.so, run on the GPU"""
    lib = _cabi.LIB_PATH
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc and os.path.exists(lib)
    exe = str(tmp_path / "c_abi_metrics_check")
    subprocess.check_call([cc, "-O1", "-std=c11", "-D__HIP_PLATFORM_AMD__", f"-I{rocm}/include", f"-I{ROOT}/include",
                           os.path.join(HERE, "c_abi", "c_abi_metrics_check.c"), lib, f"-L{rocm}/lib", "-lamdhip64", "-lm",
                           f"-Wl,-rpath,{os.path.dirname(lib)}", f"-Wl,-rpath,{rocm}/lib", "-o", exe])
    out = subprocess.run(["timeout", "-k", "10", "120", exe], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "C-ABI METRICS CHECK OK" in out.stdout, out.stdout + out.stderr
