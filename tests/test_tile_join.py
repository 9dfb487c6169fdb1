"""Tiled inference in bounded memory (`split_and_joint_image(tile_batch=k)`), the parts that need no GPU: the ownership
rectangles of `tile_places` against a painted map, the grouping, the driver's CPU branch against the reference's golden canvases
and the argument rules of the driver."""
import glob
import itertools
import math
import os

import numpy as np
import pytest
import torch

import tiled_models
from gsasr_amd.split_and_joint_image import _paste_rule, _tile_groups, split_and_joint_image, tile_places

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "tiled_*.npz")))


def _painted(nh, nw, size, stride, crop, fractional):
    """the index of the tile that ends up on top of every pixel: tile indices pasted in raster order under `_paste_rule`"""
    m = np.full(((nh - 1) * stride + size, (nw - 1) * stride + size), -1, dtype=np.int32)
    for i in range(nh):
        for j in range(nw):
            top, left = _paste_rule(i, j, nh, nw, crop, fractional)
            m[i * stride + top: i * stride + size, j * stride + left: j * stride + size] = i * nw + j
    return m


def _check_places(m, places):
    """every tile's owned set is its rectangle, the rectangles are disjoint, what is left is the map's -1s"""
    seen = np.zeros(m.shape, dtype=np.int32)
    for k, (y0, x0, y1, x1, dy, dx) in enumerate(places):
        assert 0 <= y0 <= y1 and 0 <= x0 <= x1 and dy >= 0 and dx >= 0
        own = np.zeros(m.shape, dtype=bool)
        if y1 > y0 and x1 > x0:
            assert dy + y1 - y0 <= m.shape[0] and dx + x1 - x0 <= m.shape[1]
            own[dy: dy + y1 - y0, dx: dx + x1 - x0] = True
        assert np.array_equal(own, m == k), k
        seen += own
    assert seen.max(initial=0) <= 1
    assert np.array_equal(seen == 0, m == -1)


def test_tile_places_against_a_painted_map():
    """6 875 combinations; with out_rows / out_cols the same after cropping the map.  Some leave pixels nobody owns."""
    n, holes = 0, 0
    for split, overlap in itertools.product((8, 12, 16), (1, 2, 3, 5)):
        if not overlap < split // 2:
            continue
        for scale, crop in itertools.product((1.3, 2, 2.5, 3, 4), (0, 1, 2, 4, 7)):
            size, fractional = math.ceil(split * scale), scale != int(scale)
            stride = size - math.ceil(overlap * scale)
            for nh, nw in itertools.product(range(1, 6), range(1, 6)):
                m = _painted(nh, nw, size, stride, crop, fractional)
                places = tile_places(nh, nw, size, stride, crop, fractional)
                assert all(p[2] <= size and p[3] <= size for p in places)
                _check_places(m, places)
                n += 1
                holes += bool((m == -1).any())
                if (nh + nw + crop) % 3 == 0:      # a third of them again through a cropped picture
                    rows, cols = max(1, m.shape[0] - stride // 2 - 1), max(1, m.shape[1] * 2 // 3)
                    _check_places(m[:rows, :cols], tile_places(nh, nw, size, stride, crop, fractional, rows, cols))
    assert n == 6875 and holes == 1152


def test_tile_groups():
    assert _tile_groups(30, 7, 64) == [list(range(a, min(a + 7, 30))) for a in range(0, 30, 7)]
    assert [len(g) for g in _tile_groups(30, 29, 64)] == [28, 2]         # never a canvas of one tile
    assert [len(g) for g in _tile_groups(30, 64, 17)] == [17, 13]        # the canvas bounds a group as well
    assert [len(g) for g in _tile_groups(1, 5, 64)] == [1]
    assert [len(g) for g in _tile_groups(9, 2, 64)] == [2, 2, 2, 2, 1]     # groups of two have no tile to spare: a single tile is left
    assert [len(g) for g in _tile_groups(7, 3, 64)] == [3, 2, 2]
    assert sum(_tile_groups(30, 29, 64), []) == list(range(30))


def _run(z, **kw):
    sc = float(z["scale"])
    return split_and_joint_image(torch.from_numpy(z["lq"]), sc, int(z["split_size"]), int(z["overlap_size"]), tiled_models.model_g,
                                 tiled_models.model_fea2gs, torch.tensor([sc, sc]), crop_size=int(z["crop_size"]),
                                 cuda_rendering=False, **kw)


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[6:-4] for p in GOLDEN])
def test_tile_batch_matches_reference_cpu(path):
    """the CPU branch of `tile_batch`: the same grouping, per-tile renders, the owned rectangles assigned -- the reference's
    canvas (test_tiled_driver.py's tolerances), its top-left corner with `out_size`, the default path's bytes with `out_uint8`"""
    z = np.load(path)
    for k in (2, 3, 64):
        out = _run(z, tile_batch=k)
        assert tuple(out.shape) == z["out"].shape
        np.testing.assert_allclose(out.numpy(), z["out"], rtol=1e-5, atol=1e-6)
    H, W = z["out"].shape[-2:]
    rows, cols = H - 3, max(1, W // 2 + 1)
    out = _run(z, tile_batch=3, out_size=(rows, cols))
    assert tuple(out.shape) == (1, 3, rows, cols)
    np.testing.assert_allclose(out.numpy(), z["out"][:, :, :rows, :cols], rtol=1e-5, atol=1e-6)
    assert torch.equal(_run(z, tile_batch=3, out_uint8=True), _run(z, out_uint8=True))
    assert torch.equal(_run(z, tile_batch=2, out_uint8=True, bgr=True, out_size=(rows, cols)), _run(z, out_uint8=True, bgr=True)[:rows, :cols])


def test_tile_batch_argument_checks():
    lq = torch.rand(1, 3, 20, 20)
    args = (2.0, 8, 2, tiled_models.model_g, tiled_models.model_fea2gs, torch.tensor([2.0, 2.0]))
    with pytest.raises(ValueError, match="tile_batch"):
        split_and_joint_image(lq, *args, cuda_rendering=False, tile_batch=1)
    with pytest.raises(ValueError, match="one image"):
        split_and_joint_image(torch.rand(2, 3, 20, 20), *args, cuda_rendering=False, tile_batch=2)
    with pytest.raises(ValueError, match="needs tile_batch"):
        split_and_joint_image(lq, *args, cuda_rendering=False, out_size=(10, 10))
    full = split_and_joint_image(lq, *args, cuda_rendering=False, tile_batch=2)
    H, W = full.shape[-2:]
    for bad in ((H + 1, W), (H, W + 1), (0, W)):
        with pytest.raises(ValueError, match="out_size"):
            split_and_joint_image(lq, *args, cuda_rendering=False, tile_batch=2, out_size=bad)
    assert torch.equal(split_and_joint_image(lq, *args, cuda_rendering=False, tile_batch=2, out_size=(H, W)), full)
    # distribute=True outside a multi-rank job is one rank: allowed
    assert torch.equal(split_and_joint_image(lq, *args, cuda_rendering=False, tile_batch=2, distribute=True), full)
