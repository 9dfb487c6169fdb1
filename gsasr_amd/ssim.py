"""The SSIM loss of GSASR's training step (`cri_ssim` = SSIMLoss, basicsr/losses/basic_loss.py:256-264:
`loss_weight * (1 - pytorch_msssim.ssim(x, y, data_range=1, size_average=True))`, per sample, summed and divided by b:
basicsr/models/gsasr_model.py:213-242).

    ssim_loss(image, target, loss_weight=1.0, sizes=None)

CUDA tensors: gsasr_ssim_loss (hand-written HIP, csrc/splat_ssim.hip) as one autograd node.  CPU tensors: the torch
expression `ssim_torch` below -- `pytorch_msssim.ssim` with its defaults (11-tap Gaussian window of sigma 1.5 applied
separably in "valid" mode, K = (0.01, 0.03), no clamping) written out.  include/gsasr_splat.h has the formulas.
"""
import math

import torch
import torch.nn.functional as F

from ._amp import fp32_boundary_bwd, fp32_boundary_fwd

WIN = 11            # taps; a sample needs at least this many pixels in both extents
SIGMA = 1.5
C1, C2 = 0.01 ** 2, 0.03 ** 2


def window(dtype=torch.float32, device=None) -> torch.Tensor:
    """g[i] = exp(-(i - 5)^2 / (2 * 1.5^2)), normalised to sum 1 (computed in double, rounded once to `dtype`)"""
    g = [math.exp(-((i - WIN // 2) ** 2) / (2.0 * SIGMA ** 2)) for i in range(WIN)]
    s = math.fsum(g)
    return torch.tensor([v / s for v in g], dtype=torch.float64).to(dtype=dtype, device=device)


def _blur(t: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    """the window along the rows, then the columns, per channel, "valid" (pytorch_msssim's gaussian_filter)"""
    c = t.shape[1]
    t = F.conv2d(t, g.view(1, 1, WIN, 1).expand(c, 1, WIN, 1), groups=c)
    return F.conv2d(t, g.view(1, 1, 1, WIN).expand(c, 1, 1, WIN), groups=c)


def ssim_map(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """the SSIM map `[..., C, h - 10, w - 10]` of `x` against `y` (`[C,h,w]` or `[B,C,h,w]`, data range 1), in their dtype"""
    lead = x.dim() == 3
    if lead:
        x, y = x[None], y[None]
    g = window(x.dtype, x.device)
    mu1, mu2 = _blur(x, g), _blur(y, g)
    s1 = _blur(x * x, g) - mu1 * mu1
    s2 = _blur(y * y, g) - mu2 * mu2
    s12 = _blur(x * y, g) - mu1 * mu2
    m = (2 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1) * ((2 * s12 + C2) / (s1 + s2 + C2))
    return m[0] if lead else m


def ssim_torch(image: torch.Tensor, target: torch.Tensor, loss_weight: float = 1.0) -> torch.Tensor:
    """`SSIMLoss(loss_weight)(image[None], target[None])` for one sample `[3,h,w]`: the torch expression of what
    gsasr_ssim_loss computes (differentiable by autograd; CPU tensors and the per-sample paths use it)"""
    return loss_weight * (1.0 - ssim_map(image, target).mean())


def check_sizes(sizes, what="sample"):
    for h, w in sizes:
        if h < WIN or w < WIN:
            raise ValueError(f"a {what} of {h} x {w} pixels is smaller than the {WIN} x {WIN} SSIM window: no valid pixel")


class _SsimLoss(torch.autograd.Function):
    """image `[B,3,H,W]`, target `[B,3,rows,W]` -> (L, `[B]` per-sample losses); d L / d image from k_ssim_grad, kept in `ctx`"""

    @staticmethod
    @fp32_boundary_fwd
    def forward(ctx, image, target, sizes, weight, needs_grad):
        from . import _cabi
        image = image.contiguous()
        # (the kernel writes the samples' own pixels only: the padding of a padded batch gets its zero gradient here)
        padded = needs_grad and any((h, w) != tuple(image.shape[-2:]) for h, w in sizes)
        loss, grad = _cabi.ssim_loss(image, target, sizes, weight, want_grad=needs_grad, grad=torch.zeros_like(image) if padded else None)
        ctx.grad = grad
        total, per = loss[0], loss[1:]
        ctx.mark_non_differentiable(per)
        return total, per

    @staticmethod
    @torch.autograd.function.once_differentiable
    @fp32_boundary_bwd
    def backward(ctx, g_loss, *_):
        if ctx.grad is None:
            raise RuntimeError("the SSIM loss was computed without a gradient (image did not require grad)")
        return ctx.grad.mul_(g_loss.to(torch.float32)), None, None, None, None


def ssim_loss(image, target, loss_weight=1.0, sizes=None, return_per_sample=False):
    """`SSIMLoss(loss_weight)` of every sample, averaged over the batch, as ONE differentiable call (0-dim).

    `image`: `[3,H,W]` or `[B,3,H,W]`; `target`: the same, with any number of rows >= the tallest sample (the padded
    `self.gt`, read in place); `sizes`: the per-sample (h_b, w_b) of a padded batch -- sample b is `image[b, :, :h_b, :w_b]`
    --, default every sample H x W.  The gradient goes to `image` only (a target that requires grad: ValueError).  A sample
    under 11 pixels in either extent has no valid pixel: ValueError.  `return_per_sample`: also the `[B]` losses L_b
    (non-differentiable)."""
    if not (torch.is_tensor(image) and torch.is_tensor(target) and image.dtype.is_floating_point and target.dtype.is_floating_point):
        raise ValueError("image and target must be floating-point tensors")
    if image.dim() not in (3, 4) or image.shape[-3] != 3:
        raise ValueError(f"image has shape {tuple(image.shape)}, expected [3,H,W] or [B,3,H,W]")
    if target.requires_grad:
        raise ValueError("the SSIM loss is differentiated with respect to image only: target must not require grad")
    single = image.dim() == 3
    B, H, W = (1 if single else image.shape[0]), int(image.shape[-2]), int(image.shape[-1])
    if target.dim() != image.dim() or target.shape[:-2] != image.shape[:-2] or target.shape[-1] != W:
        raise ValueError(f"target has shape {tuple(target.shape)}, expected {list(image.shape[:-2]) + ['*', W]}")
    if sizes is None:
        sizes = [(H, W)] * B
    else:
        sizes = [(int(h), int(w)) for h, w in (sizes.tolist() if torch.is_tensor(sizes) else sizes)]
        if len(sizes) != B:
            raise ValueError("one (h, w) per sample")
    check_sizes(sizes)
    if any(h > H or w > W for h, w in sizes):
        raise ValueError(f"a sample is larger than the image's {H} x {W} pixels")
    if target.shape[-2] < max(h for h, _ in sizes):
        raise ValueError(f"target has {target.shape[-2]} rows, the tallest sample {max(h for h, _ in sizes)}")
    if not image.is_cuda:
        x, y = (image[None], target[None]) if single else (image, target)
        vals = [ssim_torch(x[b, :, :h, :w], y[b, :, :h, :w].to(x.dtype), loss_weight) for b, (h, w) in enumerate(sizes)]
        stacked = torch.stack(vals)
        total = stacked.sum() / B
        return (total, stacked.detach()) if return_per_sample else total
    target = target.detach().to(device=image.device, dtype=torch.float32).contiguous()
    x = image if image.dtype == torch.float32 else image.float()
    total, per = _SsimLoss.apply(x[None] if single else x, target[None] if single else target, tuple(sizes), float(loss_weight),
                                 image.requires_grad and torch.is_grad_enabled())
    return (total, per) if return_per_sample else total
