"""The validation metrics of GSASR (`val.metrics`: basicsr/metrics/psnr_ssim.py `calculate_psnr` and `calculate_ssim`, called per
validation image by basicsr/models/gsasr_model.py:483-488) on the 8-bit picture the forward kernels store.

    image_metrics(img, ref, crop_border=0, test_y_channel=False, bgr=False, sizes=None)   -> float64 [2] / [B,2] = {psnr, ssim}
    calculate_psnr(img, img2, crop_border, input_order='HWC', test_y_channel=False)        -> float   (the reference's signature)
    calculate_ssim(img, img2, crop_border, input_order='HWC', test_y_channel=False)        -> float

CUDA tensors: gsasr_image_metrics (hand-written HIP, csrc/splat_metrics.hip), on the current stream, nothing read on the host.
CPU tensors and NumPy arrays: the torch float64 expression below, which is the executable statement of the contract in
include/gsasr_splat.h -- the bytes as numbers 0..255 (or the reference's Y with its two float32 roundings), the mean squared
difference over `img[cb:-cb, cb:-cb]`, and `ssim.ssim_map` on x / 255 (SSIM with data range 255 on x is SSIM with data range 1
on x / 255: both constants and every moment scale by 255^2).
"""
import math

import numpy as np
import torch

from . import ssim as _ssim

__all__ = ["image_metrics", "calculate_psnr", "calculate_ssim", "y_channel"]


def y_channel(picture: torch.Tensor, bgr: bool = False) -> torch.Tensor:
    """uint8 `[..., 3]` -> the reference's Y `[...]` in float64 (metric_util.py:32-45 `to_y_channel`, color_util.py:38-68):
    x = float32(v) / 255f; y64 = 24.966 b + 128.553 g + 65.481 r + 16.0 in double; float32(y64 / 255.0); float32(. * 255f)"""
    x = picture.to(torch.float32) / 255.0
    r, g, b = (x[..., k].double() for k in ((2, 1, 0) if bgr else (0, 1, 2)))
    y64 = b * 24.966 + g * 128.553 + r * 65.481 + 16.0
    return ((y64 / 255.0).to(torch.float32) * 255.0).double()


def _planes(picture: torch.Tensor, cb: int, y: bool, bgr: bool) -> torch.Tensor:
    """uint8 `[h,w,C]` -> float64 `[C or 1, hc, wc]`: the cropped values the metrics are defined on"""
    h, w = picture.shape[:2]
    p = picture[cb:h - cb, cb:w - cb]
    if y and p.shape[-1] == 3:
        return y_channel(p, bgr)[None]
    return p.permute(2, 0, 1).double()      # (one channel: float32(v) / 255f * 255f is v for every byte)


def _check_extent(hc: int, wc: int, cb: int, ssim: bool) -> None:
    if hc < 1 or wc < 1:
        raise ValueError(f"crop_border {cb} leaves no pixel")
    if ssim and (hc < _ssim.WIN or wc < _ssim.WIN):
        raise ValueError(f"a cropped picture of {hc} x {wc} pixels is smaller than the {_ssim.WIN} x {_ssim.WIN} SSIM window: no valid pixel")


def _metrics_torch(img: torch.Tensor, ref: torch.Tensor, cb: int, y: bool, bgr: bool, psnr: bool = True, ssim: bool = True):
    """(psnr, ssim) as Python floats of one pair of uint8 `[h,w,C]` CPU tensors (a metric not asked for: None)"""
    _check_extent(img.shape[0] - 2 * cb, img.shape[1] - 2 * cb, cb, ssim)
    a, b = _planes(img, cb, y, bgr), _planes(ref, cb, y, bgr)
    p = s = None
    if psnr:
        mse = float(((a - b) ** 2).mean())
        p = math.inf if mse == 0 else 10.0 * math.log10(255.0 * 255.0 / mse)
    if ssim:
        s = float(_ssim.ssim_map(a / 255.0, b / 255.0).mean(dim=(-2, -1)).mean())
    return p, s


def _sizes(sizes, B: int, H: int, W: int):
    if sizes is None:
        return [(H, W)] * B
    sizes = [(int(h), int(w)) for h, w in (sizes.tolist() if torch.is_tensor(sizes) else sizes)]
    if len(sizes) != B:
        raise ValueError("one (h, w) per sample")
    if any(h > H or w > W for h, w in sizes):
        raise ValueError(f"a sample is larger than the picture's {H} x {W} pixels")
    return sizes


def image_metrics(img, ref, crop_border=0, test_y_channel=False, bgr=False, sizes=None):
    """PSNR and SSIM of the 8-bit picture `img` against `ref`, as the reference's `calculate_psnr` / `calculate_ssim` define them.

    `img`, `ref`: uint8 `[h,w,3]` or `[B,H,W,3]` (`sizes`: the per-sample (h_b, w_b) of a padded batch, sample b being
    `img[b, :h_b, :w_b]`); windows of larger tensors are read in place.  `crop_border` pixels on every side take no part;
    `test_y_channel`: the metrics of the Y channel, `bgr` saying which byte is which.  Returns float64 `[2]` or `[B,2]` =
    {psnr, ssim} on the pictures' device; on CUDA tensors nothing is synchronised.  Both metrics are always computed, so a
    cropped extent under 11 pixels is a ValueError here even though PSNR alone is defined on it: `calculate_psnr`, or
    `_cabi.image_metrics(..., psnr=True, ssim=False)` on CUDA tensors, give the PSNR of such a region."""
    if not (torch.is_tensor(img) and torch.is_tensor(ref) and img.dtype == torch.uint8 and ref.dtype == torch.uint8):
        raise ValueError("img and ref must be uint8 tensors")
    if img.shape != ref.shape:
        raise ValueError(f"Image shapes are different: {tuple(img.shape)}, {tuple(ref.shape)}.")
    if img.dim() not in (3, 4) or img.shape[-1] != 3:
        raise ValueError(f"img has shape {tuple(img.shape)}, expected [h,w,3] or [B,H,W,3]")
    if img.device != ref.device:
        raise ValueError("img and ref must be on the same device")
    cb = int(crop_border)
    if cb < 0:
        raise ValueError("crop_border must not be negative")
    single = img.dim() == 3
    B, H, W = (1 if single else img.shape[0]), int(img.shape[-3]), int(img.shape[-2])
    sizes = _sizes(sizes, B, H, W)
    for h, w in sizes:
        _check_extent(h - 2 * cb, w - 2 * cb, cb, True)
    if img.is_cuda:
        from . import _cabi
        out = _cabi.image_metrics(img, ref, None if all(s == (H, W) for s in sizes) else sizes, cb, bool(test_y_channel), bool(bgr))
        return out[0] if single else out
    x, y = (img[None], ref[None]) if single else (img, ref)
    rows = [_metrics_torch(x[b, :h, :w], y[b, :h, :w], cb, bool(test_y_channel), bool(bgr)) for b, (h, w) in enumerate(sizes)]
    out = torch.tensor(rows, dtype=torch.float64)
    return out[0] if single else out


def _hwc(img, input_order):
    """the reference's reorder_image (metric_util.py:6-29) -> a uint8 `[h,w,C]` tensor, C = 1 or 3"""
    t = torch.from_numpy(np.ascontiguousarray(img)) if isinstance(img, np.ndarray) else img
    if not torch.is_tensor(t) or t.dtype != torch.uint8:
        raise ValueError("the pictures must be uint8 NumPy arrays or torch tensors (range [0, 255])")
    if t.dim() == 2:
        t = t[..., None]
    elif t.dim() != 3:
        raise ValueError(f"a picture has shape {tuple(t.shape)}, expected [h,w,3], [3,h,w] or [h,w]")
    elif input_order == 'CHW':
        t = t.permute(1, 2, 0)
    if t.shape[-1] not in (1, 3):
        raise ValueError(f"a picture has {t.shape[-1]} channels, expected 1 or 3")
    return t


def _calculate(which, img, img2, crop_border, input_order, test_y_channel):
    if tuple(img.shape) != tuple(img2.shape):
        raise ValueError(f"Image shapes are different: {tuple(img.shape)}, {tuple(img2.shape)}.")
    if input_order not in ('HWC', 'CHW'):
        raise ValueError(f'Wrong input_order {input_order}. Supported input_orders are "HWC" and "CHW"')
    a, b = _hwc(img, input_order), _hwc(img2, input_order)
    cb = int(crop_border)
    if cb < 0:
        raise ValueError("crop_border must not be negative")
    ssim = which == 1
    _check_extent(a.shape[0] - 2 * cb, a.shape[1] - 2 * cb, cb, ssim)
    if a.is_cuda or b.is_cuda:
        from . import _cabi
        b = b.to(a.device) if a.is_cuda else b
        a = a.to(b.device)
        if a.shape[-1] == 1:      # grey: one channel in RGB mode, three times (Y of one channel is the byte itself)
            a, b, test_y_channel = a.expand(-1, -1, 3).contiguous(), b.expand(-1, -1, 3).contiguous(), False
        elif a.stride()[-2:] != (3, 1):
            a, b = a.contiguous(), b.contiguous()       # (CHW: a host-side reorder)
        if b.stride()[-2:] != (3, 1):
            b = b.contiguous()
        # the reference's pictures are BGR (tensor2img(rgb2bgr=True), cv2.imread): to_y_channel is bgr2ycbcr
        out = _cabi.image_metrics(a, b, None, cb, bool(test_y_channel), True, psnr=not ssim, ssim=ssim)
        return float(out[0, which])
    return _metrics_torch(a, b, cb, bool(test_y_channel), True, psnr=not ssim, ssim=ssim)[which]


def calculate_psnr(img, img2, crop_border, input_order='HWC', test_y_channel=False, **kwargs):
    """basicsr.metrics.calculate_psnr (psnr_ssim.py:12-48) for uint8 pictures, NumPy or torch, `HWC`, `CHW` or 2-D grey, in the
    reference's BGR channel order -> float (inf for equal pictures).  CUDA tensors go through gsasr_image_metrics."""
    return _calculate(0, img, img2, crop_border, input_order, test_y_channel)


def calculate_ssim(img, img2, crop_border, input_order='HWC', test_y_channel=False, **kwargs):
    """basicsr.metrics.calculate_ssim (psnr_ssim.py:85-128) for uint8 pictures, as `calculate_psnr` -> float"""
    return _calculate(1, img, img2, crop_border, input_order, test_y_channel)
