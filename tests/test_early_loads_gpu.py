"""The first round trips of the render kernels, against the CPU oracle.

Backward (bwd_sweep, gsasr_amd/csrc/splat_bwd_sweep.h): in the plain instantiation the gradient pixels of a wave's first trip
are requested together with the px / py tables, before anything of the tables is known, and the sweep that follows starts from
that set; the unrolled instantiation walks the same blocks without the early set and is held to the same cases.  What can go
wrong is which load a trip consumes: no full trip at all, one, an odd number, a ragged last trip, a second 64-row block, a
second 64-column strip, lanes that fetched but lie outside the dmax box.
Forward (fwd_block, splat_forward.hip): the two-level walk prefetches a survivor's window one chunk of 64 ahead (fetching its
record along with it was measured level and is not in the tree: DESIGN.md 3.2); what can go wrong are the chunk boundaries of
the survivor list and survivors that do not hit the wave's sub-tile.

Hand-placed Gaussians on a 96 x 80 image.  Windows are made exact to the pixel by an explicit cutoff: with tau = 24 a window
reaches k = sqrt(2 tau) (1 + 1e-6) sigmas from the centre (splat_common.h: gaussian_box), and a row band of the plan clips it
in y -- a band has no room for the plan to pad a window's rows to whole trips, so the window's height is the band's.  `_cols`
restates the window rule so that each test can assert that it sweeps the widths it is meant to.

Bars: those of tests/test_hip_parity.py, restated -- image 1e-4 absolute; every gradient tensor within 2e-4 of its max-abs, every
row within (5e-4 + 5e-6 / sqrt(kappa)) of its own max-abs + 1e-5 of the tensor's, and every column and element to
tests/gradbars.py.
"""
import math

import numpy as np
import pytest
import torch

import gradbars

pytestmark = pytest.mark.gpu

W, H = 96, 80
TAU = 24.0
K = math.sqrt(2.0 * TAU) * (1.0 + 1e-6)
EPS = 0.02                     # WINDOW_EPS (px)
IMG_ATOL = 1e-4
GRAD_RTOL = 2e-4
WIDTHS = (9, 16, 17, 21, 22, 32, 33, 64, 70)      # LX = 16 | 16 | 21 | 21 | 32 | 32 | 64 | 64 | 64 + a second strip
BANDS = ((30, 31), (30, 35), (30, 36), (30, 37), (30, 42), (30, 43), (5, 75), (79, 80))    # 1, 5, 6, 7, 12, 13, 70 rows; the last row


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the MI355X box)"
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def _gauss(cx, cy, ex, ey, w=W, h=H):
    """(sx, sy, x, y) of a Gaussian centred on pixel (cx, cy) whose cutoff ellipse reaches ex / ey pixels"""
    hx, hy = 0.5 * (w - 1), 0.5 * (h - 1)
    return ex / (K * hx), ey / (K * hy), cx / hx - 1.0, cy / hy - 1.0


def _cols(sx, x, w=W, dmax=None):
    """first and last column of the window (gaussian_box, restated), from the float32 values the kernels see"""
    hx = 0.5 * (w - 1)
    sx, x = float(np.float32(sx)), float(np.float32(x))
    ext = float(np.float32(K)) * abs(sx)
    if dmax is not None:
        ext = min(ext, float(np.float32(dmax)))
    c = (x + 1.0) * hx
    return max(math.ceil(c - ext * hx - EPS), 0), min(math.floor(c + ext * hx + EPS), w - 1)


def _width_case(wd, cy, ey=40.25):
    """a Gaussian whose window is exactly `wd` columns (centre on a pixel for odd, between two for even widths: a quarter pixel
    of slack on either side, against WINDOW_EPS = 0.02)"""
    cx = 48.0 if wd % 2 else 47.5
    ex = (wd - 1) / 2 + 0.25 if wd % 2 else wd / 2 - 0.25
    return _gauss(cx, cy, ex, ey)


def _scene(rows4, n_total, seed):
    """sigmas, coords, colors of the hand-placed Gaussians `rows4` = [(sx, sy, x, y)], filled up to `n_total` with Gaussians far
    off the image (the plan's dead class: they only set the number the kernel-choice rule reads)"""
    rng = np.random.default_rng(seed)
    n = max(n_total, len(rows4))
    sig = np.zeros((n, 3), np.float32)
    xy = np.full((n, 2), 3.0, np.float32)
    sig[:, 0] = sig[:, 1] = 0.01
    for i, (sx, sy, x, y) in enumerate(rows4):
        sig[i] = (sx, sy, rng.uniform(-0.6, 0.6))
        xy[i] = (x, y)
    col = rng.uniform(0.1, 1.0, (n, 3)).astype(np.float32)
    return sig, xy, col


def _relmax(got, want):
    return float(np.abs(got - want).max() / max(1e-12, np.abs(want).max()))


def _row_tol(want, sig):
    kappa = np.maximum(1.0 - np.asarray(sig)[:, 2].astype(np.float64) ** 2, 1e-12)[:, None]
    return (5e-4 + 5e-6 / np.sqrt(kappa)) * np.abs(want).max(axis=1, keepdims=True) + 1e-5 * np.abs(want).max() + 1e-30


def _check_grads(grads, gref, sig, what):
    for got, want, name in zip(grads, gref, ("sigmas", "coords", "colors")):
        assert np.isfinite(got).all(), (what, name)
        rel = _relmax(got, want)
        assert rel <= GRAD_RTOL, f"{what}: grad {name} rel err {rel:.3e}"
        bad = np.abs(got - want) > _row_tol(want, sig)
        assert not bad.any(), (what, name, int(np.argwhere(bad)[0][0]), float(np.abs(got - want)[bad].max()), float(np.abs(want).max()))
    gradbars.check_kernel(grads, gref, sig, 0.0, what)


def _backward(sig, xy, col, wgt, rows, dmax, dev, mode="overwrite"):
    """the Gaussian-stationary backward (k_render_bwd) of the band `rows` through the C ABI; numpy gradients"""
    from gsasr_amd import _cabi
    a, b, c = _t(sig, dev), _t(xy, dev), _t(col, dev)
    plan = _cabi.plan(a, b, c, H, W, dmax, rows=rows, cutoff=TAU, flags=_cabi.FLAG_BWD_GAUSSIAN)
    g = _t(wgt[rows[0]:rows[1]], dev)
    if mode == "packed":
        out = torch.full((sig.shape[0], 8), float("nan"), device=dev)
        _cabi.backward_to_packed(plan, a, b, c, g, out, overwrite=True)
        o = out.cpu().numpy()
        return o[:, 0:3], o[:, 3:5], o[:, 5:8]
    if mode == "accumulate":       # the reference's contract: the caller zero-fills, the call adds -- twice: 2 x the gradient, exactly
        gs = [torch.zeros_like(t) for t in (a, b, c)]
        _cabi.backward(plan, a, b, c, g, *gs, overwrite=False)
        _cabi.backward(plan, a, b, c, g, *gs, overwrite=False)
        return tuple(0.5 * t.cpu().numpy() for t in gs)
    gs = [torch.full_like(t, float("nan")) for t in (a, b, c)]
    _cabi.backward(plan, a, b, c, g, *gs, overwrite=True)
    return tuple(t.cpu().numpy() for t in gs)


def _oracle_bwd(sig, xy, col, wgt, rows, dmax):
    from oracle import gs_oracle
    return gs_oracle.backward_f64(sig, xy, col, wgt[rows[0]:rows[1]], dmax, h=H, rows=rows)


@pytest.fixture(scope="module")
def wgt():
    return np.random.default_rng(5).uniform(-1.0, 1.0, (H, W, 3)).astype(np.float32)


def _unrolled(n, rows):
    """the host's rule (gsasr_splat_backward): the unrolled sweep from 32 band pixels per Gaussian up"""
    return (rows[1] - rows[0]) * W >= 32.0 * n


@pytest.mark.parametrize("rows", BANDS, ids=[f"rows{a}-{b}" for a, b in BANDS])
@pytest.mark.parametrize("unroll", [False, True], ids=["plain", "unrolled"])
def test_backward_every_width_and_height(unroll, rows, wgt, dev):
    """windows 9 ... 70 columns wide (all four lane layouts, a second strip) on bands of 1, 5, 6, 7, 12, 13 and 70 rows: no full
    trip, ragged trips, one / two / an odd number of full trips, a second 64-row block -- and the band of the LAST image row, where
    the second row of a lane's pair lies past the slab.  Both instantiations: the host picks by Gaussians per band pixel."""
    cy = 0.5 * (rows[0] + rows[1] - 1) + 0.37      # (off the rows' centre: on a one-row band d/d sigma_y would vanish with dy)
    cases = [_width_case(wd, cy) for wd in WIDTHS]
    for (sx, _, x, _), wd in zip(cases, WIDTHS):
        c0, c1 = _cols(sx, x)
        assert c1 - c0 + 1 == wd and 0 < c0 and c1 < W - 1
    h = rows[1] - rows[0]
    # plain: more than band pixels / 32 Gaussians in the call; unrolled: at most that many (a band of one row holds three)
    groups = [cases] if not unroll else [cases[i:i + 3 * h] for i in range(0, len(cases), 3 * h)]
    for k, grp in enumerate(groups):
        sig, xy, col = _scene(grp, 0 if unroll else 300, seed=10 + k)
        assert _unrolled(sig.shape[0], rows) == unroll
        got = _backward(sig, xy, col, wgt, rows, None, dev)
        _check_grads(got, _oracle_bwd(sig, xy, col, wgt, rows, None), sig, f"widths {rows} unroll {unroll} group {k}")


@pytest.mark.parametrize("unroll", [False, True], ids=["plain", "unrolled"])
def test_backward_windows_clipped_at_every_edge(unroll, wgt, dev):
    """windows that the image cuts on the left, right, top, bottom and in the corners, whole image"""
    rows = (0, H)
    cases = []
    for cx, cy in ((2.0, 40.0), (93.5, 40.0), (48.0, 1.0), (47.5, 78.0), (1.5, 2.0), (94.0, 77.5), (0.0, 79.0), (95.0, 0.0)):
        for ex, ey in ((10.25, 6.25), (4.25, 16.25), (16.25, 3.25)):
            cases.append(_gauss(cx, cy, ex, ey))
    clipped = sum(1 for sx, _, x, _ in cases if _cols(sx, x)[0] == 0 or _cols(sx, x)[1] == W - 1)
    assert clipped >= 12
    sig, xy, col = _scene(cases, 0 if unroll else 300, seed=20)
    assert _unrolled(sig.shape[0], rows) == unroll
    got = _backward(sig, xy, col, wgt, rows, None, dev)
    _check_grads(got, _oracle_bwd(sig, xy, col, wgt, rows, None), sig, f"clipped unroll {unroll}")


@pytest.mark.parametrize("rows", [(0, H), (0, 40), (24, 71)], ids=["two-rows-per-chunk", "one-row-per-chunk", "band"])
def test_backward_large_class_row_chunks(rows, wgt, dev):
    """Gaussians wider than the plan's 128-px cap: the large class, whose window is split into 64 row chunks over all waves
    (atomic path).  96 columns = two strips of 64 lanes; on 80 rows a chunk is one full trip of two rows, on 40 rows a single
    row -- no full trip, the early set IS the ragged trip -- and on the 47-row band (row0 = 24) the last chunks are empty."""
    cases = [_gauss(40.0, 0.5 * (rows[0] + rows[1]), 140.0, 60.0), _gauss(70.5, rows[0] + 3.0, 60.0, 135.0),
             _gauss(20.0, rows[1] - 2.0, 150.0, 150.0), _width_case(21, rows[0] + 5.0, ey=6.25)]
    sig, xy, col = _scene(cases, 300, seed=30)
    got = _backward(sig, xy, col, wgt, rows, None, dev)
    _check_grads(got, _oracle_bwd(sig, xy, col, wgt, rows, None), sig, f"large class {rows}")


@pytest.mark.parametrize("unroll", [False, True], ids=["plain", "unrolled"])
def test_backward_dmax_box_cuts_columns_of_the_window(unroll, wgt, dev):
    """bounded op with a box of just under 10 px in x: the windows are the box's, their Gaussians are wider (the plan sets the
    `test` bit), and for a centre on a pixel the box edge falls 0.01 px inside the window's first and last column -- those lanes
    fetch their pixels with the early loads and must contribute nothing.  On a row band (row0 = 17), 12 rows."""
    rows = (17, 29)
    hx = 0.5 * (W - 1)
    dmax = (10.0 - 0.01) / hx
    cases = [_gauss(cx, cy, 30.0, 30.0) for cx, cy in ((30.0, 22.0), (60.0, 20.0), (47.5, 25.0), (12.0, 23.5), (5.0, 18.0), (88.0, 28.0))]
    cases += [_gauss(50.0, 22.0, 5.25, 5.25)]       # (one the box does not bind)
    c0, c1 = _cols(cases[0][0], cases[0][2], dmax=dmax)
    assert (c0, c1) == (20, 40) and abs(float(np.float32(2.0 * 20 / (W - 1) - 1.0)) - float(np.float32(cases[0][2]))) > float(np.float32(dmax))
    sig, xy, col = _scene(cases, 0 if unroll else 300, seed=40)
    assert _unrolled(sig.shape[0], rows) == unroll
    got = _backward(sig, xy, col, wgt, rows, dmax, dev)
    _check_grads(got, _oracle_bwd(sig, xy, col, wgt, rows, dmax), sig, f"dmax box unroll {unroll}")


@pytest.mark.parametrize("mode", ["accumulate", "packed"])
def test_backward_accumulating_and_packed_gradients(mode, wgt, dev):
    """the same sweep behind the two other ways of writing its result: added to the caller's arrays (overwrite=False), and as one
    [N, 8] array {d sx, d sy, d rho, d x, d y, d r, d g, d b}"""
    rows = (8, 21)
    cases = [_width_case(wd, 14.0, ey=9.25) for wd in WIDTHS]
    sig, xy, col = _scene(cases, 300, seed=50)
    got = _backward(sig, xy, col, wgt, rows, None, dev, mode=mode)
    _check_grads(got, _oracle_bwd(sig, xy, col, wgt, rows, None), sig, f"{mode} gradients")


# ---- forward: the survivor list of a 32 x 16 tile ------------------------------------------------------------------------------------
def _tile_gaussians(bx0, by0, n, rng, w, h, one_subtile=False):
    """n small Gaussians whose windows (at most 3.5 px around the centre) lie inside the tile at (bx0, by0) -- with `one_subtile`
    inside its leftmost 8 columns, so that three of the tile's four waves meet survivors and no hit"""
    out = []
    for _ in range(n):
        cx = bx0 + (rng.uniform(3.7, 4.3) if one_subtile else rng.uniform(5.0, 27.0))
        cy = by0 + rng.uniform(5.0, 11.0)
        e = rng.uniform(2.0, 3.45)
        out.append(_gauss(cx, cy, e, e, w, h))
    return out


def _forward_case(w, h, counts, dmax, rows, dev, seed):
    from gsasr_amd import _cabi
    from oracle import gs_oracle
    rng = np.random.default_rng(seed)
    cases = []
    for (tx, ty, one), n in counts.items():
        grp = _tile_gaussians(32 * tx, 16 * ty, n, rng, w, h, one_subtile=one)
        for sx, _, x, _ in grp:      # every window inside its tile (or its first sub-tile)
            c0, c1 = _cols(sx, x, w)
            assert 32 * tx <= c0 and c1 <= 32 * tx + (7 if one else 31)
        cases += grp
    sig, xy, col = _scene(cases, 0, seed)
    col *= 0.2                      # (up to 129 Gaussians on a tile: keep the pixel sums O(1), the bar is absolute)
    a, b, c = _t(sig, dev), _t(xy, dev), _t(col, dev)
    # list_cap = -1: no tile lists, so the two-level walk (k_render_fwd2) renders it
    plan = _cabi.plan(a, b, c, h, w, dmax, cutoff=TAU, flags=_cabi.FLAG_FORWARD_ONLY, list_cap=-1)
    img = torch.full((h, w, 3), float("nan"), device=dev)
    _cabi.forward(plan, img, overwrite=True)
    assert bool(torch.isfinite(img).all())
    ref = gs_oracle.forward_f64(sig, xy, col, h, w, dmax, rows=rows)
    err = float(np.abs(img[rows[0]:rows[1]].cpu().numpy() - ref).max())
    assert float(np.abs(ref).max()) > 0.05
    assert err <= IMG_ATOL, f"image max|err| {err:.3e}"
    # and nothing anywhere else (an empty tile's wave prefetches nothing and stores zeros)
    assert float(img[rows[1]:].abs().max()) == 0.0 if rows[1] < h else True


# survivors per tile (tile column, tile row, all in the first sub-tile): chunk boundaries at 64 and 128; tile (0, 0) stays empty
COUNTS = {(1, 0, False): 1, (2, 0, False): 63, (0, 1, False): 64, (1, 1, False): 65, (2, 1, False): 129, (0, 2, True): 65,
          (1, 3, False): 128, (2, 4, True): 1}


@pytest.mark.parametrize("dmax", [None, 0.5], ids=["unbounded", "dmax0.5"])
def test_forward_survivor_lists_two_waves_per_subtile(dmax, dev):
    """96 x 80: 60 sub-tiles, far below 4096, so two waves share a sub-tile's list (PARTS = 2: chunks alternate between them; with
    65 survivors the second wave's only chunk holds one, with 64 it holds none)"""
    _forward_case(W, H, COUNTS, dmax, (0, H), dev, seed=60)


def test_forward_survivor_lists_one_wave_per_subtile(dev):
    """512 x 1024 = 4096 sub-tiles: one wave per sub-tile walks the whole list (PARTS = 1), the same tiles in the image's top
    rows; the oracle renders those 80 rows"""
    _forward_case(512, 1024, COUNTS, 0.5, (0, 80), dev, seed=61)
