"""`split_and_joint_image(tile_batch=k)` on the GPU: groups of tiles rendered as batched canvases, each tile's owned rectangle
assigned to its place in a picture that is allocated once.

The expected picture is built here from `_cabi.batch_forward_u8` / `batch_forward` on the same groups of tiles, pasted in raster
order under `_paste_rule`.  These are renders of another plan of the same Gaussians, and the 12-px LR tiles with one Gaussian
per LR pixel run the two-level search kernel (k_render_fwd2: no tile lists, below the split kernel's density), which appends the
survivors of its first level to a list in LDS with one atomicAdd per wave (fwd_block) -- the order in which a workgroup's waves
arrive decides the order of every pixel's sum, so two runs give sums that differ in their last bits (measured at this shape:
up to a third of the floats, by at most 2.4e-7; no byte).  The comparisons therefore hold what two such orders can differ by:
2e-6 (values of order 1, a few hundred fp32 additions: the bar test_tiled_driver.py already holds between two canvas
compositions at this shape) and one 8-bit level -- an address error on random data is of order 1 / of many levels.  Pixels that
no tile owns are exactly zero."""
import math

import pytest
import torch

import tiled_models
from gsasr_amd.split_and_joint_image import _paste_rule, _tile_groups, split_and_joint_image

pytestmark = pytest.mark.gpu
F32_TOL, U8_TOL = 2e-6, 1


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the MI355X box)"
    return torch.device("cuda:0")


# ---- the driver ----------------------------------------------------------------------------------------------------------------
KW = dict(if_dmax=True, dmax_mode="fix", dmax=0.4)


def drive(lq, scale, overlap=3, crop=2, **kw):
    sm = torch.tensor([scale, scale], device=lq.device)
    return split_and_joint_image(lq, scale, 12, overlap, tiled_models.model_g, tiled_models.model_fea2gs, sm, crop_size=crop, **KW, **kw)


def by_groups(lq, scale, tile_batch, out_uint8, overlap=3, crop=2):
    """the expected picture: the tiles rendered by `_cabi.batch_forward_u8` / `batch_forward` in the driver's groups, pasted in
    raster order under `_paste_rule`"""
    from gsasr_amd import _cabi
    from gsasr_amd.gaussian_splatting import _batch_step_sizes, max_canvas_batch
    import torch.nn.functional as F
    sm = torch.tensor([scale, scale], device=lq.device)
    split, stride = 12, 12 - overlap
    h, w = lq.shape[-2:]
    nh, nw = math.ceil((h - overlap) / stride), math.ceil((w - overlap) / stride)
    pad = F.pad(lq, (0, nw * stride + overlap - w, 0, nh * stride + overlap - h), mode="reflect")
    size = math.ceil(split * scale)
    stride_sr = size - math.ceil(overlap * scale)
    sv = torch.tensor([scale], device=lq.device)
    tiles = []
    for group in _tile_groups(nh * nw, tile_batch, max_canvas_batch(size)):
        gp = torch.stack([tiled_models.model_fea2gs(tiled_models.model_g(pad[:, :, (k // nw) * stride: (k // nw) * stride + split,
                                                                             (k % nw) * stride: (k % nw) * stride + split]), sv)[0]
                          for k in group]).float().contiguous()
        steps = _batch_step_sizes([scale] * len(group), [sm] * len(group), 1.2, "scale_modify", lq.device)      # (the driver's own)
        sizes = [(size, size)] * len(group)
        if out_uint8:
            tiles.extend(_cabi.batch_forward_u8(gp, steps, sizes, 0.4)[0])
        else:
            tiles.extend(_cabi.batch_forward(gp, steps, sizes, 0.4, _cabi.FLAG_FORWARD_ONLY)[0][:, :, :size])
    rows, cols = (nh - 1) * stride_sr + size, (nw - 1) * stride_sr + size
    sr = torch.zeros((rows, cols, 3), dtype=torch.uint8, device=lq.device) if out_uint8 else torch.zeros((3, rows, cols), device=lq.device)
    fractional = scale != int(scale)
    for i in range(nh):
        for j in range(nw):
            top, left = _paste_rule(i, j, nh, nw, crop, fractional)
            y0, x0 = i * stride_sr, j * stride_sr
            if out_uint8:
                sr[y0 + top: y0 + size, x0 + left: x0 + size] = tiles[i * nw + j][top:, left:]
            else:
                sr[:, y0 + top: y0 + size, x0 + left: x0 + size] = tiles[i * nw + j][:, top:, left:]
    return (sr if out_uint8 else sr.unsqueeze(0)), nh * nw


@pytest.fixture(scope="module")
def lq(dev):
    return torch.rand(1, 3, 40, 52, generator=torch.Generator().manual_seed(5)).to(dev)


def close(got, want, what):
    """the driver's bars (module docstring): one 8-bit level, 2e-6"""
    diff = (got.float() - want.float()).abs()
    print(f"{what}: {int((diff > 0).sum())} of {diff.numel()} differ, max {float(diff.max()):.3e}")
    assert got.shape == want.shape and got.dtype == want.dtype, what
    assert float(diff.max()) <= (U8_TOL if got.dtype == torch.uint8 else F32_TOL), what


@pytest.mark.parametrize("tile_batch", [7, 29])
@pytest.mark.parametrize("scale", [2.0, 2.5])
def test_driver_is_the_paste_of_the_same_groups(scale, tile_batch, lq):
    """5 x 6 tiles; 29 forces the regrouping (28 + 2).  uint8 and float"""
    assert [len(g) for g in _tile_groups(30, 29, 64)] == [28, 2]
    for out_uint8 in (True, False):
        want, n = by_groups(lq, scale, tile_batch, out_uint8)
        got = drive(lq, scale, tile_batch=tile_batch, out_uint8=out_uint8)
        assert n == 30
        close(got, want, f"scale {scale} tile_batch {tile_batch} uint8 {out_uint8}")


def test_driver_leaves_unowned_pixels_zero(lq):
    """overlap 1, crop 4 at x2: the SR overlap is 2 pixels, so two rows / columns between neighbouring tiles belong to nobody"""
    for out_uint8 in (True, False):
        want, _ = by_groups(lq, 2.0, 7, out_uint8, overlap=1, crop=4)
        got = drive(lq, 2.0, overlap=1, crop=4, tile_batch=7, out_uint8=out_uint8)
        close(got, want, f"holes uint8 {out_uint8}")
        pic = got if out_uint8 else got[0].permute(1, 2, 0)
        assert not pic[24:26].any() and not pic[:, 24:26].any() and bool(pic[:24, :24].any()) and bool(pic[26:40, 26:40].any())


@pytest.mark.parametrize("scale", [2.0, 2.5])
def test_driver_out_size_is_the_slice(scale, lq):
    for out_uint8 in (True, False):
        full = drive(lq, scale, tile_batch=7, out_uint8=out_uint8)
        got = drive(lq, scale, tile_batch=7, out_uint8=out_uint8, out_size=(70, 90))
        assert tuple(got.shape) == ((70, 90, 3) if out_uint8 else (1, 3, 70, 90))
        close(got, (full[:70, :90] if out_uint8 else full[:, :, :70, :90]).contiguous(), f"out_size scale {scale} uint8 {out_uint8}")


@pytest.mark.parametrize("scale", [2.0, 2.5])
def test_driver_against_the_default_path(scale, lq):
    """`tile_batch=7` against `tile_batch=None` (one canvas of all 30 tiles, pasted): the same sums in canvases composed
    differently -- float within 2e-6, uint8 within one level"""
    a, b = drive(lq, scale, tile_batch=7), drive(lq, scale)
    err = float((a - b).abs().max())
    print(f"scale {scale}: float max|diff| {err:.3e}")
    assert a.shape == b.shape and err <= 2e-6
    a8, b8 = drive(lq, scale, tile_batch=7, out_uint8=True, bgr=True), drive(lq, scale, out_uint8=True, bgr=True)
    lev = int((a8.int() - b8.int()).abs().max())
    print(f"scale {scale}: uint8 max level diff {lev}")
    assert a8.shape == b8.shape and lev <= 1


def test_driver_with_a_single_tile_left_over(dev):
    """3 x 3 tiles at tile_batch=2: four canvases of two and ONE tile, which takes the single-image calls and the same
    assignment of its rectangle -- against the default path, uint8 (b, g, r) and float, with and without out_size"""
    assert [len(g) for g in _tile_groups(9, 2, 64)] == [2, 2, 2, 2, 1]
    small = torch.rand(1, 3, 30, 30, generator=torch.Generator().manual_seed(8)).to(dev)
    for scale in (2.0, 2.5):
        for kw in (dict(), dict(out_uint8=True, bgr=True)):
            want = drive(small, scale, **kw)
            close(drive(small, scale, tile_batch=2, **kw), want, f"left-over tile, scale {scale} {kw}")
            rows, cols = want.shape[0] - 7 if kw else want.shape[2] - 7, 33
            cut = want[:rows, :cols] if kw else want[:, :, :rows, :cols]
            close(drive(small, scale, tile_batch=2, out_size=(rows, cols), **kw), cut.contiguous(), f"left-over tile, out_size, scale {scale} {kw}")
