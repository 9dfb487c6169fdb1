"""The forward kernels' SEARCH at the sizes where its helpers change path (csrc/splat_common.h: seg_table, fwd_candidate /
SegCursor, coarse_pass, fine_test, survivor_walk; csrc/splat_forward.hip: fwd_record, fwd_stage_eval), image against the
float64 oracle at the image bar of tests/test_hip_parity.py (1e-4 absolute on images of O(1) values).  The image is not
bit-reproducible from run to run (the survivors' order is not), so nothing here asserts bit identity.

Geometry is made exact by an explicit cutoff tau = 32: a window's half-extent is min(dmax, 8 sigma) in pixels, cells are
16 x 16 px, a Gaussian with a half-extent above 128 px is in the "large" class.  What each case pins:

  * segments: a tile's table holds one segment per cell row within the class' reach plus one for the large class.  1 cell
    row + empty / non-empty large class (16 x 16 px); 9 .. 17 cell rows down a column of Gaussians that fill a 120-px box, so the
    table crosses 16 -> 17 -> 18 segments: the row-shift scan up to 16, the permute scan above (64 x 272, 64 x 1040 and, for
    the one-wave-per-sub-tile kernel, 1024 x 512).  More than 18 cell rows cannot be planned: the reach of the normal class
    ends at 128 px, so a 16-row tile sees at most (15 + 2 * 128) / 16 + 1 of them -- the permute scan's last step (33+
    segments) is out of reach of any plan, and so is a case for it.
  * chunks: clusters of 1, 63, 64, 65, 4*64, 4*64+1, 8*64, 8*64+1 and 1100 candidates, each alone within reach of its tile,
    and empty tiles between them: the last live coarse slot of a wave and the first dead one, with four waves per tile
    (1024 x 512: 4096 sub-tiles) and with eight (368 x 176); 1100 candidates need a second round.  Dense Gaussians on
    64 x 32 px: > 1024 candidates in every tile.
  * a chunk over three and more segments: ~20 candidates per cell row, 6-7 rows in reach.
  * the dmax box: hits that need the in-kernel test and hits that do not in one chunk, then none, then all.
  * the other kernels that share the helpers: the split kernel (dense 192 x 192), the list kernels (dense 256 x 256; a
    capacity the lists overflow, which falls back to the one-level walk) and the wide kernel.  (The 8 x 8 kernel is a
    development switch read once per process; no test of the suite selects it.)
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

IMG_ATOL = 1e-4     # tests/test_hip_parity.py, IMG_ATOL
TAU = 32.0          # half-extent = 8 sigma


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the MI355X box)"
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def _px(sig_px, cx, cy, h, w, rho=None):
    """kernel-frame parameters of Gaussians given in pixels: sigma (x, y) and centre (x, y) on an h x w grid"""
    hx, hy = 0.5 * (w - 1), 0.5 * (h - 1)
    sig_px = np.asarray(sig_px, np.float64).reshape(-1, 2)
    n = sig_px.shape[0]
    sig = np.zeros((n, 3), np.float32)
    sig[:, 0], sig[:, 1] = sig_px[:, 0] / hx, sig_px[:, 1] / hy
    if rho is not None:
        sig[:, 2] = rho
    xy = np.stack([np.asarray(cx, np.float64) / hx - 1.0, np.asarray(cy, np.float64) / hy - 1.0], 1).astype(np.float32)
    return sig, xy


def _check(sig, xy, col, h, w, dmax, dev, cutoff=TAU, flags=0, list_cap=0, fwd_flags=0):
    from gsasr_amd import _cabi
    from oracle import gs_oracle
    sig, xy, col = (np.ascontiguousarray(a, dtype=np.float32) for a in (sig, xy, col))
    plan = _cabi.plan(_t(sig, dev), _t(xy, dev), _t(col, dev), h, w, dmax, cutoff=cutoff, flags=flags, list_cap=list_cap)
    img = torch.full((h, w, 3), float("nan"), device=dev)
    _cabi.forward(plan, img, overwrite=True, flags=fwd_flags)
    torch.cuda.synchronize()
    img = img.cpu().numpy()
    ref = gs_oracle.forward_f64(sig, xy, col, h, w, dmax)
    assert np.isfinite(img).all()
    assert float(np.abs(ref).max()) <= 4.0, "the 1e-4 absolute bar is stated for images of O(1) values"
    err = np.abs(img - ref)
    at = np.unravel_index(int(err.argmax()), err.shape)
    assert err.max() <= IMG_ATOL, f"image max|err| {err.max():.3e} at (row, col, ch) {at}, tile row {at[0] // 16}"
    return img, ref


def _grid(rng, h, w, x1, step, sigma_px):
    """one small Gaussian per step x step px block of the columns [0, x1), jittered inside it"""
    gx, gy = np.meshgrid(np.arange(0, x1, step), np.arange(0, h, step))
    cx = gx.ravel() + rng.uniform(0.5, step - 0.5, gx.size)
    cy = gy.ravel() + rng.uniform(0.5, step - 0.5, gx.size)
    return np.full((gx.size, 2), sigma_px), cx, np.minimum(cy, h - 1.0)


# ---------------------------------------------------------------------------------------------------
# segments
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("large", [False, True], ids=["large-empty", "one-large"])
def test_one_cell_row(large, dev):
    """16 x 16 px, 3 Gaussians: one cell row, the large class empty; then one of them wide enough for the large class"""
    h = w = 16
    sig, xy = _px([[1.2, 0.9], [0.8, 1.5], [1.0, 1.0]], [3.3, 9.1, 12.6], [4.2, 10.7, 2.4], h, w, rho=[0.3, -0.5, 0.0])
    col = np.array([[0.9, 0.2, 0.4], [0.1, 0.8, 0.5], [0.6, 0.6, 0.1]], np.float32)
    if large:
        sig[1, 0] = 22.0 / (0.5 * (w - 1))       # 8 * 22 px > 128 px
    for dmax in (None, 0.4):
        if large and dmax is not None:
            continue                             # (the box would cut the window back into the normal class)
        _check(sig, xy, col, h, w, dmax, dev)


TALL = [(272, 64, False), (1040, 64, False), (512, 1024, False), (272, 64, True)]


@pytest.mark.parametrize("h,w,wide", TALL, ids=["64x272", "64x1040", "1024x512-four-waves", "64x272-wide"])
def test_cell_rows_across_the_scan_boundary(h, w, wide, dev):
    """The bounded op with a box of 120 px and, in every cell row of the first 64 columns, one Gaussian far taller than the
    box (sigma_y 100 px): its window is the box, 120 px up and down -- the normal class' reach -- and at the box edge it still
    adds half its colour.  Down the column the tables hold 9, 10, .. 17 cell rows (+ the large class' segment: 16, 17, 18
    segments around tile rows 6, 7, 8), and a candidate dropped or taken twice at either end of the table is far above the
    bar (under a cutoff alone the table's end rows would only hold terms of e^-32).  Every tile row is compared."""
    from gsasr_amd import _cabi
    rng = np.random.default_rng(h + w + int(wide))
    s_px, cx, cy = _grid(rng, h, w, 64, 8, 1.0)
    n_small, rows = s_px.shape[0], (h + 15) // 16
    s_px = np.concatenate([s_px, np.stack([rng.uniform(2.0, 3.0, rows), np.full(rows, 100.0)], 1)])
    cx = np.concatenate([cx, rng.uniform(4.0, 60.0, rows)])
    cy = np.concatenate([cy, np.minimum(16.0 * np.arange(rows) + rng.uniform(1.0, 15.0, rows), h - 1.0)])
    sig, xy = _px(s_px, cx, cy, h, w, rho=np.concatenate([rng.uniform(-0.6, 0.6, n_small), np.zeros(rows)]))
    col = np.concatenate([rng.uniform(0.05, 0.4, (n_small, 3)), rng.uniform(0.02, 0.1, (rows, 3))])
    hx, hy = 0.5 * (w - 1), 0.5 * (h - 1)
    dmax = 120.0 / hy
    assert dmax * hy <= 128.0 and dmax * hx >= 7.0, "the box keeps the tall ones in the normal class and leaves the small ones whole in x"
    flags = _cabi.FLAG_FWD_WIDE if wide else 0
    _check(sig, xy, col, h, w, dmax, dev, flags=flags, fwd_flags=flags, list_cap=-1)


# ---------------------------------------------------------------------------------------------------
# chunks
# ---------------------------------------------------------------------------------------------------
COUNTS = [1, 63, 64, 65, 4 * 64, 4 * 64 + 1, 8 * 64, 8 * 64 + 1, 1100]


def _clusters(h, w, seed):
    """cluster k: COUNTS[k] Gaussians of sigma 0.5 px (half-extent 4 px) inside ONE cell, 128 px / 4 cell rows from the next"""
    rng = np.random.default_rng(seed)
    s_px, cx, cy, col = [], [], [], []
    for k, n in enumerate(COUNTS):
        x0, y0 = 40.0 + 128.0 * (k % 3), 24.0 + 64.0 * (k // 3)
        cx.append(x0 + rng.uniform(-6.0, 6.0, n))
        cy.append(y0 + rng.uniform(-6.0, 6.0, n))
        s_px.append(np.full((n, 2), 0.5))
        col.append(rng.uniform(0.2, 1.0, (n, 3)) * min(1.0, 40.0 / n))
    s_px, cx, cy, col = np.concatenate(s_px), np.concatenate(cx), np.concatenate(cy), np.concatenate(col)
    sig, xy = _px(s_px, cx, cy, h, w, rho=rng.uniform(-0.5, 0.5, s_px.shape[0]))
    return sig, xy, col


@pytest.mark.parametrize("h,w", [(176, 368), (512, 1024)], ids=["eight-waves-per-tile", "four-waves-per-tile"])
def test_candidate_totals_per_tile(h, w, dev):
    """tiles with 0, 1, 63, 64, 65, 256, 257, 512, 513 and 1100 candidates (4 and 8 waves x 64: the last live slot and the first
    dead one; 1100: a second round), the rest of the image empty"""
    assert (((w + 7) // 8) * ((h + 15) // 16) >= 4096) == (w == 1024)      # the rule that picks one or two waves per sub-tile
    sig, xy, col = _clusters(h, w, 3)
    for dmax in (0.05, None) if w < 1024 else (0.05,):
        img, ref = _check(sig, xy, col, h, w, dmax, dev, list_cap=-1)
        assert float(np.abs(img[h - 16:, w - 32:]).max()) == 0.0 and float(np.abs(ref[h - 16:, w - 32:]).max()) < 1e-12    # the empty corner
    for k in range(len(COUNTS)):     # every cluster did land on pixels
        y, x = 24 + 64 * (k // 3), 40 + 128 * (k % 3)
        assert float(ref[y - 8:y + 8, x - 8:x + 8].max()) > 0.05


def test_second_round_everywhere(dev):
    """dense Gaussians on 64 x 32 px: every tile has more than 1024 candidates (two and more rounds of the coarse pass)"""
    rng = np.random.default_rng(11)
    h, w, n = 32, 64, 2600
    sig, xy = _px(rng.uniform(0.4, 1.1, (n, 2)), rng.uniform(0, w - 1, n), rng.uniform(0, h - 1, n), h, w, rho=rng.uniform(-0.7, 0.7, n))
    col = rng.uniform(0.0, 0.2, (n, 3))
    for list_cap in (-1, 0):
        _check(sig, xy, col, h, w, 0.5, dev, list_cap=list_cap)


def test_chunk_over_three_segments(dev):
    """sparse cells: ~20 candidates per cell row within reach (64 px wide = 4 cells of ~5), half-extents up to 44 px: a tile's
    table has 6-7 short segments and every chunk of 64 runs over three or four of them"""
    rng = np.random.default_rng(12)
    h, w, n = 160, 64, 200
    s_px = rng.uniform(1.0, 5.5, (n, 2))
    sig, xy = _px(s_px, rng.uniform(0, w - 1, n), rng.uniform(0, h - 1, n), h, w, rho=rng.uniform(-0.6, 0.6, n))
    col = rng.uniform(0.0, 0.5, (n, 3))
    for dmax in (None, 0.9):
        _check(sig, xy, col, h, w, dmax, dev, list_cap=-1)


@pytest.mark.parametrize("box_px", [16.0, 48.0, 4.0], ids=["some-need-the-box", "none", "all"])
def test_box_test_mixed_in_one_chunk(box_px, dev):
    """half-extents of 8 px and 32 px side by side, dmax at 16 px (the wide ones are cut by the box and take the in-kernel
    test, the narrow ones do not), at 48 px (none) and at 4 px (all)"""
    rng = np.random.default_rng(13)
    h = w = 64
    n = 240
    s_px = np.where(rng.random((n, 1)) < 0.5, 1.0, 4.0) * np.ones((1, 2))
    sig, xy = _px(s_px, rng.uniform(0, w - 1, n), rng.uniform(0, h - 1, n), h, w, rho=rng.uniform(-0.6, 0.6, n))
    col = rng.uniform(0.0, 0.3, (n, 3))
    _check(sig, xy, col, h, w, box_px / (0.5 * (w - 1)), dev, list_cap=-1)
    _check(sig, xy, col, h, w, box_px / (0.5 * (w - 1)), dev, cutoff=0.0)


# ---------------------------------------------------------------------------------------------------
# the other kernels on the same helpers
# ---------------------------------------------------------------------------------------------------
def _synth(h_lr, w_lr, scale, seed, gpp=1):
    from gsasr_amd import synthetic
    sig, xy, col, H, W = synthetic.kernel_inputs(h_lr, w_lr, scale, seed=seed, gpp=gpp)
    return sig.numpy(), xy.numpy(), col.numpy(), H, W


def test_two_waves_per_sub_tile_128(dev):
    """128 x 128 px, 1024 Gaussians: the two-level kernel with two waves per sub-tile (fewer than 4096 sub-tiles, not dense)"""
    sig, xy, col, H, W = _synth(32, 32, 4.0, seed=14)
    assert (H, W, sig.shape[0]) == (128, 128, 1024) and 4 * sig.shape[0] < H * W
    for dmax in (0.1, None):
        _check(sig, xy, col, H, W, dmax, dev, cutoff=0.0)
        _check(sig, xy, col, H, W, dmax, dev, cutoff=0.0, list_cap=-1)


def test_dense_crop_split_kernel(dev):
    """a dense 192 x 192 crop, 16 Gaussians per LR pixel: fewer than 4096 sub-tiles on a dense plan (k_render_fwd_split)"""
    sig, xy, col, H, W = _synth(48, 48, 4.0, seed=15, gpp=16)
    assert (H, W) == (192, 192) and 4 * sig.shape[0] >= H * W
    _check(sig, xy, col / 4.0, H, W, 0.5, dev, cutoff=0.0, list_cap=-1)


@pytest.mark.parametrize("list_cap", [0, 24], ids=["lists", "lists-overflow"])
def test_dense_list_plan(list_cap, dev):
    """dense 256 x 256, 16 per LR pixel: the list kernels (record pairs); with 24 entries per tile every list overflows and the
    tile is rendered by the one-level walk over the segment table"""
    sig, xy, col, H, W = _synth(64, 64, 4.0, seed=16, gpp=16)
    assert (H, W) == (256, 256) and 4 * sig.shape[0] >= H * W
    _check(sig, xy, col / 4.0, H, W, 0.1, dev, cutoff=0.0, list_cap=list_cap)
