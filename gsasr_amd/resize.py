"""MATLAB-compatible antialiased bicubic `imresize`: the degradation GSASR trains and validates against
(basicsr/utils/matlab_functions.py `imresize` / `imresize_new`, applied to every GT crop by
basicsr/data/continuous_bicubic_downsample_dataset.py:70-72), batched and differentiable.

    imresize(img, scale, antialiasing=True)                       the reference's signature; output ceil(n * scale)
    imresize_new(img, scale_h, scale_w, antialiasing=True)        ...; output round(n * scale), Python's round
    imresize_batch(imgs, sizes=None, scales=None, out_size=None, antialiasing=True)     [B,C,Hmax,Wmax] -> [B,C,out_h,out_w]

CUDA float tensors: gsasr_imresize / gsasr_imresize_backward (hand-written HIP, csrc/splat_resize.hip) as one autograd node on
the current stream.  CPU tensors and NumPy arrays: the torch expression `resize_torch` below, the executable statement of the
contract in include/gsasr_splat.h (differentiable by autograd).
"""
import math

import numpy as np
import torch

from ._amp import fp32_boundary_bwd, fp32_boundary_fwd

__all__ = ["imresize", "imresize_new", "imresize_batch", "resize_torch", "axis_taps"]


def _cubic(x: torch.Tensor) -> torch.Tensor:
    a = x.abs()
    a2, a3 = a * a, a * a * a
    return torch.where(a <= 1, 1.5 * a3 - 2.5 * a2 + 1, torch.where(a <= 2, -0.5 * a3 + 2.5 * a2 - 4 * a + 2, torch.zeros_like(a)))


def axis_taps(n: int, m: int, scale: float, antialiasing: bool = True):
    """one axis of the resize, `n` inputs -> `m` outputs: (index `[m,p]` int64 of the input each tap reads, after the single
    reflection; weight `[m,p]` float64, rows summing to 1).  ValueError where a tap with a non-zero weight lies beyond one
    reflection, or the scale is not a positive finite number."""
    scale = float(scale)
    if not (scale > 0.0 and math.isfinite(scale)):
        raise ValueError(f"scale {scale} must be a positive finite number")
    if n < 1 or m < 1:
        raise ValueError(f"{n} -> {m}: no pixel")
    shrink = scale < 1.0 and antialiasing
    kw = 4.0 / scale if shrink else 4.0
    if kw > 4.0 * 32767:
        raise ValueError(f"scale {scale}: a tap with non-zero weight lies beyond one reflection of {n} pixels")
    p = math.ceil(kw) + 2
    o = torch.arange(1, m + 1, dtype=torch.float64)
    u = o / scale + 0.5 * (1.0 - 1.0 / scale)
    left = torch.floor(u - kw / 2.0)
    k = left[:, None] + torch.arange(p, dtype=torch.float64)[None, :]         # 1-based taps
    w = scale * _cubic((u[:, None] - k) * scale) if shrink else _cubic(u[:, None] - k)
    w = w / w.sum(1, keepdim=True)
    k0 = k.long() - 1
    idx = torch.where(k0 < 0, -1 - k0, torch.where(k0 >= n, 2 * n - 1 - k0, k0))
    outside = (idx < 0) | (idx >= n)
    if bool((outside & (w != 0)).any()):
        raise ValueError(f"{n} pixels at scale {scale}: a tap with non-zero weight lies beyond one reflection of the input "
                         "(the reference's symmetric copy fails there too)")
    return idx.clamp_(0, n - 1), w


def resize_torch(img: torch.Tensor, out_hw, scales, antialiasing: bool = True) -> torch.Tensor:
    """`[..., h, w]` -> `[..., out_h, out_w]`: rows first, then columns, each a dot product over the taps, in `img`'s dtype"""
    (oh, ow), (sh, sw) = out_hw, scales
    h, w = img.shape[-2:]
    ih, wh = axis_taps(h, oh, sh, antialiasing)
    iw, ww = axis_taps(w, ow, sw, antialiasing)
    t = (img[..., ih, :] * wh.to(img.dtype)[:, :, None]).sum(-2)              # [..., oh, p, w] -> [..., oh, w]
    return (t[..., iw] * ww.to(img.dtype)).sum(-1)                            # [..., oh, ow, p] -> [..., oh, ow]


class _Resize(torch.autograd.Function):
    """`[B,C,H,W]` -> `[B,C,out_h,out_w]`; the backward is the adjoint kernel on the same descriptor"""

    @staticmethod
    @fp32_boundary_fwd
    def forward(ctx, x, sizes, scales, out_hw, antialiasing):
        from . import _cabi
        x = x if x.stride(-1) == 1 and x.stride(-2) >= x.shape[-1] else x.contiguous()
        out = torch.empty(x.shape[:2] + tuple(out_hw), dtype=torch.float32, device=x.device)
        _cabi.imresize(x, out, scales, sizes, antialiasing)
        ctx.args = (tuple(x.shape), sizes, scales, antialiasing)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    @fp32_boundary_bwd
    def backward(ctx, g):
        from . import _cabi
        shape, sizes, scales, antialiasing = ctx.args
        g = g.to(torch.float32)
        g = g if g.stride(-1) == 1 and g.stride(-2) >= g.shape[-1] and min(g.stride()) >= 0 else g.contiguous()
        # (the kernel writes the samples' own pixels only: the padding of a padded batch gets its zero gradient here)
        padded = sizes is not None and any(tuple(s) != shape[2:] for s in sizes)
        gx = (torch.zeros if padded else torch.empty)(shape, dtype=torch.float32, device=g.device)
        _cabi.imresize(gx, g, scales, sizes, antialiasing, backward=True)
        return gx, None, None, None, None


def _resize(x: torch.Tensor, sizes, scales, out_hw, antialiasing: bool) -> torch.Tensor:
    """`[B,C,H,W]` floating-point tensor, CUDA or CPU; `scales`: one (sh, sw) per sample"""
    B, C, H, W = x.shape
    sizes = [(H, W)] * B if sizes is None else sizes
    for (h, w), (sh, sw) in zip(sizes, scales):       # the argument errors as ValueError, on either device
        _check_axis(h, out_hw[0], sh, antialiasing)
        _check_axis(w, out_hw[1], sw, antialiasing)
    if x.is_cuda:
        if not (1 <= B <= 64):
            raise ValueError("the batch must hold 1..64 samples")
        full = all(tuple(s) == (H, W) for s in sizes)
        shared = all(tuple(s) == tuple(scales[0]) for s in scales)
        y = _Resize.apply(x if x.dtype == torch.float32 else x.float(), None if full else tuple(map(tuple, sizes)),
                          tuple(scales[0]) if shared else tuple(map(tuple, scales)), tuple(out_hw), bool(antialiasing))
        return y
    outs = [resize_torch(x[b, :, :h, :w], out_hw, scales[b], antialiasing) for b, (h, w) in enumerate(sizes)]
    return torch.stack(outs)


_AXIS_OK = {}


def _check_axis(n, m, s, antialiasing):
    key = (n, m, float(s), bool(antialiasing))
    if key not in _AXIS_OK:
        axis_taps(n, m, s, antialiasing)
        if len(_AXIS_OK) > 4096:
            _AXIS_OK.clear()
        _AXIS_OK[key] = True


def _single(img, scale_h, scale_w, antialiasing, size_rule):
    """the reference's accepted inputs: torch (c,h,w) or (h,w); numpy (h,w,c) or (h,w) -> the matching kind"""
    is_np = isinstance(img, np.ndarray)
    if is_np:
        t = torch.from_numpy(np.ascontiguousarray(img if img.ndim == 2 else img.transpose(2, 0, 1) if img.ndim == 3 else img)).float()
    elif torch.is_tensor(img):
        t = img if img.dtype.is_floating_point else img.float()
    else:
        raise ValueError("img must be a torch tensor (c,h,w) / (h,w) or a NumPy array (h,w,c) / (h,w)")
    if t.dim() not in (2, 3):
        raise ValueError(f"img has shape {tuple(img.shape)}, expected (c,h,w) / (h,w) as a tensor, (h,w,c) / (h,w) as an array")
    squeeze = t.dim() == 2
    t = t[None] if squeeze else t
    h, w = int(t.shape[-2]), int(t.shape[-1])
    if h < 1 or w < 1 or t.shape[0] < 1:
        raise ValueError("img has no pixel")
    out_hw = (size_rule(h * scale_h), size_rule(w * scale_w))
    if out_hw[0] < 1 or out_hw[1] < 1:
        raise ValueError(f"scale ({scale_h}, {scale_w}) leaves no pixel of {h} x {w}")
    y = _resize(t[None], None, [(float(scale_h), float(scale_w))], out_hw, bool(antialiasing))[0]
    y = y[0] if squeeze else y
    if is_np:
        y = y.numpy()
        return y if squeeze else y.transpose(1, 2, 0)
    return y


def imresize(img, scale, antialiasing=True):
    """matlab_functions.imresize: bicubic, the same scale on both axes, output `ceil(n * scale)`.  `img`: tensor `(c,h,w)` or
    `(h,w)`, or NumPy `(h,w,c)` or `(h,w)` (computed and returned in float32); the result is of the matching kind.  CUDA
    tensors run the HIP kernels and are differentiable.  ValueError where the reference's symmetric copy fails (a tap with
    non-zero weight beyond one reflection, e.g. 26 pixels at scale 1/16)."""
    return _single(img, scale, scale, antialiasing, math.ceil)


def imresize_new(img, scale_h, scale_w, antialiasing=True):
    """matlab_functions.imresize_new: as `imresize` with a scale per axis and output `round(n * scale)` (Python's round)"""
    return _single(img, scale_h, scale_w, antialiasing, round)


def imresize_batch(imgs, sizes=None, scales=None, out_size=None, antialiasing=True):
    """A padded batch `[B,C,Hmax,Wmax]` -> `[B,C,out_h,out_w]`, one call, differentiable.

    `sizes`: the per-sample (h_b, w_b) -- sample b is `imgs[b, :, :h_b, :w_b]`; the rest of its slot is never read and gets
    a zero gradient --, default every sample Hmax x Wmax.  Give `scales`, one `(scale_h, scale_w)` (or one number) per sample
    or for all, with `imresize_new`'s size rule `round(n * scale)`; or `out_size` = (out_h, out_w), the scale of sample b
    then being out / in per axis (what the dataset does with `1 / scale_modify`); or both.  All samples must arrive at one
    output size: ValueError otherwise."""
    if not (torch.is_tensor(imgs) and imgs.dtype.is_floating_point and imgs.dim() == 4):
        raise ValueError("imgs must be a floating-point tensor [B,C,H,W]")
    B, C, H, W = (int(v) for v in imgs.shape)
    if B < 1 or C < 1 or H < 1 or W < 1:
        raise ValueError("imgs has no pixel")
    if sizes is None:
        sizes = [(H, W)] * B
    else:
        sizes = [(int(h), int(w)) for h, w in (sizes.tolist() if torch.is_tensor(sizes) else sizes)]
        if len(sizes) != B:
            raise ValueError("one (h, w) per sample")
        if any(h < 1 or w < 1 or h > H or w > W for h, w in sizes):
            raise ValueError(f"a sample is empty or larger than the batch's {H} x {W} pixels")
    if scales is None and out_size is None:
        raise ValueError("give scales, out_size or both")
    if out_size is not None:
        out_size = (int(out_size[0]), int(out_size[1]))
        if out_size[0] < 1 or out_size[1] < 1:
            raise ValueError("out_size must be at least 1 x 1")
    if scales is None:
        scales = [(out_size[0] / h, out_size[1] / w) for h, w in sizes]
    else:
        scales = scales.tolist() if torch.is_tensor(scales) else scales
        if isinstance(scales, (int, float)):
            scales = [(float(scales), float(scales))] * B
        elif len(scales) == 2 and all(isinstance(v, (int, float)) for v in scales) and B != 2:
            scales = [(float(scales[0]), float(scales[1]))] * B
        else:
            scales = [(float(s), float(s)) if isinstance(s, (int, float)) else (float(s[0]), float(s[1])) for s in scales]
        if len(scales) != B:
            raise ValueError("one scale or (scale_h, scale_w) per sample")
        got = [(round(h * sh), round(w * sw)) for (h, w), (sh, sw) in zip(sizes, scales)]
        if out_size is None:
            out_size = got[0]
        if any(g != out_size for g in got):
            raise ValueError(f"the samples' rounded sizes {got} disagree with the output size {out_size}")
        if out_size[0] < 1 or out_size[1] < 1:
            raise ValueError("the scales leave no pixel")
    return _resize(imgs, sizes, scales, out_size, bool(antialiasing))
