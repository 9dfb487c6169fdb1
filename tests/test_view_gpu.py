"""A rectangular window of the HR grid on the GPU (gsasr_view, the `_view` entry points, generate_2D_gaussian_splatting_view).

Bars, with their sources: image 1e-4 absolute against oracle.gs_oracle.forward_f64 (tests/test_hip_parity.py: IMG_ATOL);
gradients 2e-4 of the tensor's max-abs and per Gaussian `_row_tol` (the same file) against backward_f64; "the same sums in
another order" 2e-5 * max(1, largest value) (tests/test_tune.py).  The oracle renders rows [y0, y0 + h) of the FULL grid and
is cropped; for gradients it gets the window's weights zero-padded to the full width.

The forward is not bit-reproducible in general (the order of a pixel's sum follows wave timing), so the exact tests render
Gaussians whose windows do not overlap: one term per pixel (tests/test_u8_output_gpu.py).  Here the windows are the dmax boxes
of the bounded op (12 px each way, far inside the support under tau = 104): the kernels' own per-pixel box test decides which
pixels get the term, on the same float coordinates whatever sub-tile a pixel falls into -- a window's sub-tiles are aligned to
ITS origin, not the grid's."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import gradbars

pytestmark = pytest.mark.gpu
IMG_ATOL = 1e-4
GRAD_RTOL = 2e-4
ORDER_RTOL = 2e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the MI355X box)"
    return torch.device("cuda:0")


def _row_tol(want, sig):
    kappa = np.maximum(1.0 - np.asarray(sig)[:, 2].astype(np.float64) ** 2, 1e-12)[:, None]
    return (5e-4 + 5e-6 / np.sqrt(kappa)) * np.abs(want).max(axis=1, keepdims=True) + 1e-5 * np.abs(want).max() + 1e-30


def check_grads(got, want, sig, what="", independent=False, min_share=0.0):
    """`independent`: `want` is the float64 truth, not another kernel of this build -- then every column is held to its own bar,
    element by element (tests/gradbars.py), besides the tensor and row bars"""
    for g, w, name in zip(got, want, ("sigmas", "coords", "colors")):
        g, w = np.asarray(g, np.float64), np.asarray(w, np.float64)
        assert np.isfinite(g).all(), name
        rel = float(np.abs(g - w).max() / max(1e-12, np.abs(w).max()))
        print(f"{what} grad {name}: rel err {rel:.3e}")
        assert rel <= GRAD_RTOL, (what, name, rel)
        bad = np.abs(g - w) > _row_tol(w, sig)
        assert not bad.any(), (what, name, int(np.argwhere(bad)[0][0]), float(np.abs(g - w)[bad].max()), float(np.abs(w).max()))
    if independent:
        gradbars.check_kernel(got, want, sig, min_share, what)


PALETTE = [(1.3, -0.4, 0.9), (0.35, 1.0, 2.5), (-1.0, 0.6, 1.1), (5.0, 0.08, 0.999), (0.7, 1.7, -0.2), (1.05, 0.2, 0.5)]
GRID = 512
BOX_PX = 12.0
TAU = 104.0


def separated(H, W, s_total=0, spacing=64, sigma_px=4.0, seed=0):
    """kernel-frame Gaussians on a `spacing`-px lattice (centres at 32 + 64 k, jittered by up to a pixel), std 3.2 .. 4 px,
    |rho| <= 0.4; record 1 is a NaN record and NaN records pad the list to `s_total` (a dense plan is a matter of the COUNT)"""
    rng = np.random.RandomState(seed)
    ny, nx = H // spacing, W // spacing
    gy, gx = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    n = ny * nx
    px = (gx.ravel() + 0.5) * spacing + rng.uniform(-1, 1, n)
    py = (gy.ravel() + 0.5) * spacing + rng.uniform(-1, 1, n)
    sig = np.stack([sigma_px * rng.uniform(0.8, 1.0, n) * 2 / (W - 1), sigma_px * rng.uniform(0.8, 1.0, n) * 2 / (H - 1),
                    rng.uniform(-0.4, 0.4, n)], 1)
    xy = np.stack([px * 2 / (W - 1) - 1, py * 2 / (H - 1) - 1], 1)
    col = np.array([PALETTE[i % len(PALETTE)] for i in range(n)]) * rng.uniform(0.9, 1.0, (n, 1))
    rec = np.concatenate([sig, xy, col], 1).astype(np.float32)
    out = np.full((max(n + 1, s_total), 8), np.nan, np.float32)
    out[0] = rec[0]
    out[2: n + 1] = rec[1:]
    t = torch.from_numpy(out)
    return t[:, 0:3].contiguous(), t[:, 3:5].contiguous(), t[:, 5:8].contiguous()


def box_dmax(n=GRID):
    return 2.0 * BOX_PX / (n - 1)


# forward families: name -> (records, forward flag, list_cap); each selects its kernel on the 512^2 grid AND on its windows
# (the launcher's rules, gsasr_amd/csrc/splat_forward.hip)
FORWARD = {
    "narrow-search": (0, "narrow", -1),         # the two-level walk
    "wide-search": (0, "wide", -1),             # 16 x 16 sub-tiles
    "narrow-lists": (0, "narrow", 256),         # tile lists, 32 x 16-px tiles
    "wide-lists": (0, "wide", 256),             # tile lists, 32 x 32-px tiles
    "split-pairs": (65536, "narrow", -1),       # a dense plan without lists below 4096 sub-tiles: the split kernel, record pairs
}
BACKWARD = ["BWD_GAUSSIAN", "BWD_TILE", "BWD_HOME"]


def fwd_flag(width):
    from gsasr_amd import _cabi
    return _cabi.FLAG_FWD_WIDE if width == "wide" else _cabi.FLAG_FWD_NARROW


def render(plan, flags=0):
    from gsasr_amd import _cabi
    d = plan.dims
    img = torch.full((d.h, d.w, 3), float("nan"), device=plan.device)
    _cabi.forward(plan, img, overwrite=True, flags=flags)
    return img


def gradients(plan, sig, xy, col, wgt):
    from gsasr_amd import _cabi
    out = [torch.full_like(t, float("nan")) for t in (sig, xy, col)]
    _cabi.backward(plan, sig, xy, col, wgt.contiguous(), *out, overwrite=True)
    return [t.cpu().numpy() for t in out]


# ---- (4) identity view ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(FORWARD))
def test_identity_view_forward_is_the_whole_image_call(name, dev):
    from gsasr_amd import _cabi
    s_total, width, cap = FORWARD[name]
    sig, xy, col = (t.to(dev) for t in separated(GRID, GRID, s_total, seed=len(name)))
    flag = fwd_flag(width)
    kw = dict(cutoff=TAU, flags=flag | _cabi.FLAG_FORWARD_ONLY, list_cap=cap)
    plain = _cabi.plan(sig, xy, col, GRID, GRID, box_dmax(), **kw)
    ident = _cabi.plan(sig, xy, col, GRID, GRID, box_dmax(), view=(GRID, GRID, 0, 0), **kw)
    assert ident.view is not None and plain.view is None
    a, b = render(plain, flag), render(ident, flag)
    assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 1.0
    assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())
    assert np.array_equal(_cabi.forward_u8(plain, flags=flag).cpu().numpy(), _cabi.forward_u8(ident, flags=flag).cpu().numpy())
    crop = (GRID - 21, GRID - 37)
    assert np.array_equal(_cabi.forward_u8(plain, crop=crop, bgr=True, flags=flag).cpu().numpy(),
                          _cabi.forward_u8(ident, crop=crop, bgr=True, flags=flag).cpu().numpy())
    # the workspaces are interchangeable: an identity view IS the plain call (same note, same layout)
    L = _cabi.lib()
    img = torch.empty(GRID, GRID, 3, device=dev)
    d = _cabi._dims_with(ident, _cabi.FLAG_OVERWRITE_IMAGE | flag)
    assert L.gsasr_splat_forward(ctypes.byref(d), ident.workspace.data_ptr(), ident.workspace.numel(), img.data_ptr(),
                                 torch.cuda.current_stream(dev).cuda_stream) == 0
    assert np.array_equal(img.cpu().numpy(), a.cpu().numpy())


@pytest.mark.parametrize("kernel", BACKWARD)
@pytest.mark.parametrize("bounded", [True, False], ids=["bounded", "unbounded"])
def test_identity_view_backward_is_the_whole_image_call(kernel, bounded, dev):
    from gsasr_amd import _cabi
    sig, xy, col = (t.to(dev) for t in separated(GRID, GRID, seed=7))
    wgt = torch.rand(GRID, GRID, 3, generator=torch.Generator().manual_seed(2)).to(dev)
    kw = dict(cutoff=0.0 if bounded else 32.0, flags=getattr(_cabi, "FLAG_" + kernel))
    dm = box_dmax() if bounded else None
    plain = _cabi.plan(sig, xy, col, GRID, GRID, dm, **kw)
    ident = _cabi.plan(sig, xy, col, GRID, GRID, dm, view=(GRID, GRID, 0, 0), **kw)
    ga, gb = gradients(plain, sig, xy, col, wgt), gradients(ident, sig, xy, col, wgt)
    for a, b in zip(ga, gb):
        assert np.isfinite(a).all() and np.abs(a).max() > 0
        assert np.array_equal(a, b)


# ---- (5) exact placement -------------------------------------------------------------------------------------------------
# (y0, x0, h, w) on the 512^2 grid, lattice points at 32 + 64 k with boxes of +-12 px:
WINDOWS = {
    # origin and size multiples of nothing; left edge cuts the boxes at x = 96 +- 12 (centres inside), the right edge 230 those
    # at 224 (centres inside); the top edge 100 cuts the boxes at y = 96 (centres OUTSIDE), the bottom edge 215 those at 224
    "straddled-edges": (100, 90, 115, 140),
    "odd-interior": (37, 51, 203, 149),
    "thin": (150, 3, 19, 333),
    "tall": (5, 281, 411, 23),
    "top-left-corner": (0, 0, 131, 77),
    "top-right-corner": (0, 512 - 93, 167, 93),
    "bottom-left-corner": (512 - 75, 0, 75, 201),
    "bottom-right-corner": (512 - 141, 512 - 139, 141, 139),
    "left-and-right-edge": (200, 0, 57, 512),
    "top-and-bottom-edge": (0, 217, 512, 45),
    "between-the-lattice": (110, 110, 36, 36),      # no centre inside: only parts of boxes, or nothing
}


@pytest.mark.parametrize("name", sorted(FORWARD))
@pytest.mark.parametrize("window", sorted(WINDOWS))
def test_view_is_the_slice_of_the_whole_render_exactly(window, name, dev):
    from gsasr_amd import _cabi
    y0, x0, h, w = WINDOWS[window]
    assert any(v % 8 for v in (y0, x0, h, w)) or "corner" in window or "edge" in window
    s_total, width, cap = FORWARD[name]
    sig, xy, col = (t.to(dev) for t in separated(GRID, GRID, s_total, seed=3 + len(name)))
    flag = fwd_flag(width)
    kw = dict(cutoff=TAU, flags=flag | _cabi.FLAG_FORWARD_ONLY, list_cap=cap)
    whole = render(_cabi.plan(sig, xy, col, GRID, GRID, box_dmax(), **kw), flag)
    want = whole[y0:y0 + h, x0:x0 + w].cpu().numpy()
    plan = _cabi.plan(sig, xy, col, h, w, box_dmax(), view=(GRID, GRID, y0, x0), **kw)
    got = render(plan, flag).cpu().numpy()
    assert np.isfinite(got).all()
    assert np.array_equal(got, want), (int((got != want).sum()), float(np.abs(got - want).max()))
    if window == "straddled-edges":
        for edge in (want[0], want[-1], want[:, 0], want[:, -1]):
            assert np.abs(edge).max() > 1e-3        # a Gaussian is cut by each of the four edges
    if window != "between-the-lattice":
        assert np.abs(want).max() > 0.3
    # ... and the 8-bit store of the window: the quantised window, cropped and swapped
    crop = (h - 1, w - 2)
    got8 = _cabi.forward_u8(plan, crop=crop, bgr=True, flags=flag).cpu().numpy()
    want8 = (np.clip(want[: crop[0], : crop[1], ::-1], 0, 1) * np.float32(255.0)).round().astype(np.uint8)
    assert np.array_equal(got8, want8)


@pytest.mark.parametrize("kernel", BACKWARD)
@pytest.mark.parametrize("window", ["straddled-edges", "bottom-right-corner", "between-the-lattice"])
def test_view_gradients_of_separated_gaussians(window, kernel, dev):
    """the same input through the backward kernels: against the whole-image backward fed the zero-padded weights (a Gaussian's
    sum runs over its pixels in an order that follows the window's alignment: the suite's gradient bars, not bits)"""
    from gsasr_amd import _cabi
    y0, x0, h, w = WINDOWS[window]
    sig, xy, col = (t.to(dev) for t in separated(GRID, GRID, seed=11))
    wgt = torch.rand(h, w, 3, generator=torch.Generator().manual_seed(4)).to(dev)
    pad = torch.zeros(GRID, GRID, 3, device=dev)
    pad[y0:y0 + h, x0:x0 + w] = wgt
    kw = dict(cutoff=TAU, flags=getattr(_cabi, "FLAG_" + kernel))
    want = gradients(_cabi.plan(sig, xy, col, GRID, GRID, box_dmax(), **kw), sig, xy, col, pad)
    got = gradients(_cabi.plan(sig, xy, col, h, w, box_dmax(), view=(GRID, GRID, y0, x0), **kw), sig, xy, col, wgt)
    live = ~np.isnan(sig.cpu().numpy()[:, 0])
    check_grads([g[live] for g in got], [g[live] for g in want], sig.cpu().numpy()[live], window)
    assert all(not g[~live].any() for g in got)


# ---- (6) oracle parity, dense ---------------------------------------------------------------------------------------------
DENSE_WINDOW = (37, 51, 100, 90)
OPS = {"bounded": 0.1, "unbounded": None, "bounded-wide-box": 1.5}


@functools.lru_cache(maxsize=None)
def dense_case(gpp, op):
    """GSASR-shaped Gaussians on a 256^2 grid (64^2 LR pixels x4) + one LARGE-class Gaussian (std 40 px: half-extent > 128 px
    under every cutoff where the op's box allows it) centred outside the window; the oracle's window and gradients"""
    from gsasr_amd import synthetic
    from oracle import gs_oracle
    sig, xy, col, H, W = synthetic.kernel_inputs(64, 64, 4.0, seed=17 + gpp, gpp=gpp)
    big = torch.tensor([[40.0 * 2 / (W - 1), 40.0 * 2 / (H - 1), 0.3, 230.0 * 2 / (W - 1) - 1, 20.0 * 2 / (H - 1) - 1, 0.3, 0.2, 0.25]])
    sig, xy, col = torch.cat([sig, big[:, 0:3]]), torch.cat([xy, big[:, 3:5]]), torch.cat([col, big[:, 5:8]])
    y0, x0, h, w = DENSE_WINDOW
    dmax = OPS[op]
    a, b, c = sig.numpy(), xy.numpy(), col.numpy()
    ref = gs_oracle.forward_f64(a, b, c, H, W, dmax, rows=(y0, y0 + h))[:, x0:x0 + w]
    wgt = torch.rand(h, w, 3, generator=torch.Generator().manual_seed(9))
    pad = np.zeros((h, W, 3), np.float32)
    pad[:, x0:x0 + w] = wgt.numpy()
    gref = gs_oracle.backward_f64(a, b, c, pad, dmax, h=H, rows=(y0, y0 + h))
    # Gaussians whose only part inside the window is tail: centred more than 3 std outside it, with a gradient all the same
    cx, cy = (b[:, 0] + 1) * 0.5 * (W - 1), (b[:, 1] + 1) * 0.5 * (H - 1)
    sx, sy = np.abs(a[:, 0]) * 0.5 * (W - 1), np.abs(a[:, 1]) * 0.5 * (H - 1)
    outside = (cx < x0 - 3 * sx) | (cx > x0 + w - 1 + 3 * sx) | (cy < y0 - 3 * sy) | (cy > y0 + h - 1 + 3 * sy)
    assert (outside & (np.abs(gref[2]).max(axis=1) > 0)).sum() > 10
    return sig, xy, col, H, W, ref, wgt, gref


@pytest.mark.parametrize("kernel", BACKWARD)
@pytest.mark.parametrize("cutoff", [0.0, 104.0, -1.0], ids=["adaptive", "tau104", "nocut"])
@pytest.mark.parametrize("gpp,op", [(1, "bounded"), (1, "unbounded"), (1, "bounded-wide-box"), (16, "bounded"), (16, "unbounded")])
def test_dense_window_against_the_oracle(gpp, op, cutoff, kernel, dev):
    from gsasr_amd import _cabi
    sig, xy, col, H, W, ref, wgt, gref = dense_case(gpp, op)
    y0, x0, h, w = DENSE_WINDOW
    a, b, c = sig.to(dev), xy.to(dev), col.to(dev)
    plan = _cabi.plan(a, b, c, h, w, OPS[op], cutoff=cutoff, flags=getattr(_cabi, "FLAG_" + kernel), view=(H, W, y0, x0))
    got = render(plan).cpu().numpy()
    err = float(np.abs(got - ref).max())
    print(f"image max|err| {err:.3e} (largest value {np.abs(ref).max():.3f})")
    assert np.isfinite(got).all() and err <= IMG_ATOL
    check_grads(gradients(plan, a, b, c, wgt.to(dev)), gref, sig.numpy(), f"{gpp}/{op}/{cutoff}/{kernel}", independent=True,
                min_share=gradbars.SYNTHETIC_SHARE)


# ---- (7) fused step ------------------------------------------------------------------------------------------------------
def raw_parameters(H, W, scale, n_total, seed=0):
    """raw decoder-style parameters [n,9] whose activations are Gaussians on a 96-px lattice with a std of <= 3 px and a dmax
    box of 12 px (see the module docstring); padding records have alpha = sigmoid(-200) = 0"""
    rng = np.random.RandomState(seed)
    ny, nx = H // 96, W // 96
    gy, gx = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    n = ny * nx
    logit = lambda p: np.log(p / (1 - p))
    step = 1.2 / scale
    p = np.zeros((n_total, 9), np.float32)
    p[:, 3] = -200.0
    p[:, 7:9] = 0.5
    p[:n, 0] = logit(3.0 * step * rng.uniform(0.8, 1.0, n))
    p[:n, 1] = logit(3.0 * step * rng.uniform(0.8, 1.0, n))
    p[:n, 2] = rng.uniform(-0.4, 0.4, n)
    p[:n, 3] = rng.uniform(2.0, 8.0, n)
    p[:n, 4:7] = rng.uniform(-3.0, 7.0, (n, 3))
    p[:n, 7] = ((gx.ravel() + 0.5) * 96 + rng.uniform(-1, 1, n)) / W
    p[:n, 8] = ((gy.ravel() + 0.5) * 96 + rng.uniform(-1, 1, n)) / H
    return torch.from_numpy(p)


@pytest.mark.parametrize("source", ["step_size", "scale_modify"])
@pytest.mark.parametrize("window", [(50, 130, 171, 149), (0, 0, 288, 384), (288 - 67, 384 - 99, 67, 99)], ids=["interior", "identity", "corner"])
def test_fused_step_view_is_prologue_plan_forward(window, source, dev):
    """gsasr_step_forward_view / _sm_view on raw parameters == gsasr_prologue_forward for the FULL grid + plan_view + forward,
    bit for bit (one term per pixel: no order), and the 8-bit step == the quantised float view of the same plan.  The step entry
    points take the process default of the cutoff: tau = 104 here, so that the window and the whole image (whose data-derived
    cutoffs could differ) skip the same -- no -- pixels of a box"""
    from gsasr_amd import _cabi
    old = _cabi.get_default_cutoff()
    _cabi.set_default_cutoff(TAU)
    try:
        _fused_step_view_case(window, source, dev)
    finally:
        _cabi.set_default_cutoff(old)


def _fused_step_view_case(window, source, dev):
    from gsasr_amd import _cabi
    H, W, scale = 288, 384, 8.0
    y0, x0, h, w = window
    p = raw_parameters(H, W, scale, 64, seed=3).to(dev)
    dm = 2.0 * BOX_PX / (W - 1)
    step = torch.full((1,), 1.2 / scale, device=dev)
    src = dict(step=step) if source == "step_size" else dict(step=None, scale_modify=torch.tensor([scale, scale], device=dev))
    img, plan = _cabi.step_forward(p, src.pop("step"), h, w, dm, view=(H, W, y0, x0), **src)
    assert tuple(img.shape) == (3, h, w)
    sig, xy, col = _cabi.prologue_forward(p, step, H, W)
    flags = _cabi.FLAG_CHW_IMAGE | _cabi.FLAG_OVERWRITE_IMAGE
    ref_plan = _cabi.plan(sig, xy, col, h, w, dm, flags=flags, view=(H, W, y0, x0))
    want = torch.full((3, h, w), float("nan"), device=dev)
    _cabi.forward(ref_plan, want, overwrite=True, chw=True)
    assert float(want.max()) > 0.5
    assert np.array_equal(img.cpu().numpy(), want.cpu().numpy())
    # ... which is the slice of the whole fused step
    whole, _ = _cabi.step_forward(p, step, H, W, dm)
    assert np.array_equal(img.cpu().numpy(), whole[:, y0:y0 + h, x0:x0 + w].cpu().numpy())
    src = dict(step=step) if source == "step_size" else dict(step=None, scale_modify=torch.tensor([scale, scale], device=dev))
    crop = (h - 3, w - 5)
    got8, plan8 = _cabi.step_forward_u8(p, src.pop("step"), h, w, dm, crop=crop, bgr=True, view=(H, W, y0, x0), **src)
    assert plan8.dims.flags & _cabi.FLAG_FORWARD_ONLY
    want8 = (np.clip(img.permute(1, 2, 0).cpu().numpy()[: crop[0], : crop[1], ::-1], 0, 1) * np.float32(255.0)).round().astype(np.uint8)
    assert np.array_equal(got8.cpu().numpy(), want8)


def within_one_level(u8, ref_hwc, halfwidth):
    """no value differs from quantise(ref) by more than 1, and one differs at all only where clamp(ref) * 255 lies within
    `halfwidth` levels of a half-integer"""
    ref = np.asarray(ref_hwc, np.float32)
    t = (np.clip(ref, 0, 1) * np.float32(255.0)).astype(np.float64)
    want = np.clip(ref, 0, 1) * np.float32(255.0)
    want = want.round().astype(np.uint8)
    exempt = np.abs(t - np.floor(t) - 0.5) <= halfwidth
    diff = np.abs(u8.astype(np.int32) - want.astype(np.int32))
    print(f"values {diff.size}, differing {int((diff != 0).sum())}, exempt share {exempt.mean():.4f}, max difference {int(diff.max())}")
    return bool(diff.max() <= 1 and not (diff != 0)[~exempt].any())


@pytest.mark.parametrize("kernel", BACKWARD)
@pytest.mark.parametrize("dmax", [0.1, None], ids=["bounded", "unbounded"])
def test_fused_step_view_backward_against_the_oracle(dmax, kernel, dev):
    """raw parameters -> window -> d/d parameters: gsasr_step_forward_view + gsasr_step_backward_view against
    oracle(host_ref.prologue) and torch's chain rule through host_ref.prologue in double"""
    from gsasr_amd import _cabi, synthetic
    from oracle import gs_oracle, host_ref
    h_lr, w_lr, scale, gpp = 48, 40, 4.0, 4
    H, W = 192, 160
    y0, x0, h, w = 41, 23, 97, 83
    p = synthetic.gs_parameters(h_lr, w_lr, seed=23, gpp=gpp)
    sm = torch.tensor([scale, scale])
    sig, xy, col, _ = host_ref.prologue(p, (H, W), sm)
    ref = gs_oracle.forward_f64(sig.numpy(), xy.numpy(), col.numpy(), H, W, dmax, rows=(y0, y0 + h))[:, x0:x0 + w]
    wgt = torch.rand(h, w, 3, generator=torch.Generator().manual_seed(6))
    pad = np.zeros((h, W, 3), np.float32)
    pad[:, x0:x0 + w] = wgt.numpy()
    g = gs_oracle.backward_f64(sig.numpy(), xy.numpy(), col.numpy(), pad, dmax, h=H, rows=(y0, y0 + h))
    pr = p.clone().double().requires_grad_(True)
    s2, x2, c2, _ = host_ref.prologue(pr, (H, W), sm.double())
    torch.autograd.backward([s2, x2, c2], [torch.from_numpy(a) for a in g])
    want = pr.grad.numpy()
    pg = p.to(dev)
    for chw in (True, False):
        flags = getattr(_cabi, "FLAG_" + kernel) | (_cabi.FLAG_CHW_GRAD if chw else 0)
        img, plan = _cabi.step_forward(pg, None, h, w, dmax, flags, scale_modify=sm.to(dev), view=(H, W, y0, x0))
        err = float(np.abs(img.permute(1, 2, 0).cpu().numpy() - ref).max())
        print(f"image max|err| {err:.3e}")
        assert err <= IMG_ATOL
        grad = wgt.permute(2, 0, 1).contiguous().to(dev) if chw else wgt.to(dev)
        have = _cabi.step_backward(plan, pg, None, grad, chw=chw).cpu().numpy()
        rel = float(np.abs(have - want).max() / np.abs(want).max())
        print(f"d/d parameters rel err {rel:.3e}")
        assert np.isfinite(have).all() and rel <= GRAD_RTOL
        gradbars.check_raw(have, want, p, gradbars.SYNTHETIC_SHARE, f"step view {kernel} dmax {dmax} chw {chw}")
    # the 8-bit step on dense input: at most one level off the quantised float window, only within 1e-4 of a rounding boundary
    got8, _ = _cabi.step_forward_u8(pg, None, h, w, dmax, scale_modify=sm.to(dev), view=(H, W, y0, x0))
    assert within_one_level(got8.cpu().numpy(), img.permute(1, 2, 0).cpu().numpy(), 255 * 1e-4)


# ---- (8) plan safety -----------------------------------------------------------------------------------------------------
def test_a_plan_belongs_to_its_view(dev):
    from gsasr_amd import _cabi
    L = _cabi.lib()
    st = torch.cuda.current_stream(dev).cuda_stream
    sig, xy, col = (t.to(dev) for t in separated(GRID, GRID, seed=5))
    h, w = 150, 170
    view = (GRID, GRID, 40, 60)
    viewed = _cabi.plan(sig, xy, col, h, w, box_dmax(), view=view)
    plain = _cabi.plan(sig, xy, col, h, w, box_dmax())
    img = torch.zeros(h, w, 3, device=dev)
    g = [torch.zeros_like(t) for t in (sig, xy, col)]
    ptrs = [t.data_ptr() for t in (sig, xy, col, img, *g)]

    def fwd(plan, v):
        d, ws = plan.dims, plan.workspace
        if v is None:
            return L.gsasr_splat_forward(ctypes.byref(d), ws.data_ptr(), ws.numel(), img.data_ptr(), st)
        return L.gsasr_splat_forward_view(ctypes.byref(d), ctypes.byref(_cabi.View(*v)), ws.data_ptr(), ws.numel(), img.data_ptr(), st)

    def bwd(plan, v):
        d, ws = plan.dims, plan.workspace
        if v is None:
            return L.gsasr_splat_backward(*ptrs, ctypes.byref(d), ws.data_ptr(), ws.numel(), st)
        return L.gsasr_splat_backward_view(*ptrs, ctypes.byref(d), ctypes.byref(_cabi.View(*v)), ws.data_ptr(), ws.numel(), st)

    others = [(GRID, GRID, 41, 60), (GRID, GRID, 40, 61), (GRID + 1, GRID, 40, 60), (GRID, GRID + 64, 40, 60), (GRID, GRID, 60, 40),
              (h, w, 0, 0)]
    for call in (fwd, bwd):
        assert call(viewed, view) == 0 and call(plain, None) == 0
        assert call(viewed, None) == -3, L.gsasr_last_error()       # GSASR_ERR_PLAN: the plain entry point on a view's plan
        assert call(plain, view) == -3
        for other in others:
            assert call(viewed, other) == -3, other                 # (the last one is the identity view: the plain call)
        assert call(plain, (h, w, 0, 0)) == 0
    # the 8-bit forward and the step backward check the same note
    out = torch.zeros(h, w, 3, dtype=torch.uint8, device=dev)
    assert L.gsasr_splat_forward_u8(ctypes.byref(viewed.dims), viewed.workspace.data_ptr(), viewed.workspace.numel(), out.data_ptr(), h, w,
                                    3 * w, 0, st) == -3
    p = raw_parameters(288, 384, 8.0, 64).to(dev)
    _, sp = _cabi.step_forward(p, torch.full((1,), 0.15, device=dev), 100, 120, 0.1, view=(288, 384, 10, 20))
    gp = torch.empty_like(p)
    args = (p.data_ptr(), None, torch.zeros(100, 120, 3, device=dev).data_ptr(), gp.data_ptr(), ctypes.byref(sp.dims))
    tail = (sp.workspace.data_ptr(), sp.workspace.numel(), st)
    assert L.gsasr_step_backward_view(*args, ctypes.byref(_cabi.View(288, 384, 10, 20)), *tail) == 0
    assert L.gsasr_step_backward_view(*args, ctypes.byref(_cabi.View(288, 384, 11, 20)), *tail) == -3
    assert L.gsasr_step_backward(*args, *tail) == -3
    torch.cuda.synchronize()


# ---- (9) at size ---------------------------------------------------------------------------------------------------------
def order_check(got, want, what):
    bar = ORDER_RTOL * max(1.0, float(np.abs(want).max()))
    err = float(np.abs(got - want).max())
    print(f"{what}: max|view - slice| {err:.3e}, bar {bar:.3e} (largest value {np.abs(want).max():.3f})")
    assert np.isfinite(got).all() and err <= bar, (what, err, bar)


@pytest.mark.parametrize("corner", [False, True], ids=["interior", "corner"])
def test_config3_shaped_window_against_the_own_whole_render(corner, dev):
    """a 1024^2 window of a 6144^2 grid (512^2 LR pixels x12, one Gaussian per LR pixel: 262 144): the slice of this library's
    own whole render, at the bar for the same sums in another order"""
    from gsasr_amd import _cabi, synthetic
    sig, xy, col, H, W = synthetic.kernel_inputs(512, 512, 12.0, seed=41)
    a, b, c = sig.to(dev), xy.to(dev), col.to(dev)
    y0, x0 = (H - 1024, W - 1024) if corner else (2549, 2603)
    whole = render(_cabi.plan(a, b, c, H, W, 0.1, flags=_cabi.FLAG_FORWARD_ONLY))
    want = whole[y0:y0 + 1024, x0:x0 + 1024].cpu().numpy()
    del whole
    got = render(_cabi.plan(a, b, c, 1024, 1024, 0.1, flags=_cabi.FLAG_FORWARD_ONLY, view=(H, W, y0, x0))).cpu().numpy()
    order_check(got, want, "config 3, 1024^2 window")


@pytest.mark.parametrize("corner", [False, True], ids=["interior", "corner"])
def test_c2x16_shaped_window_against_the_own_whole_render(corner, dev):
    """a 512^2 window of a 1024^2 grid at sixteen Gaussians per LR pixel (1 M): image as above; gradients against the
    whole-image backward fed the zero-padded weights, at the suite's gradient bars"""
    from gsasr_amd import _cabi, synthetic
    sig, xy, col, H, W = synthetic.kernel_inputs(256, 256, 4.0, seed=43, gpp=16)
    a, b, c = sig.to(dev), xy.to(dev), col.to(dev)
    y0, x0 = (512, 512) if corner else (237, 251)
    plan_w = _cabi.plan(a, b, c, H, W, 0.1)
    want = render(plan_w)[y0:y0 + 512, x0:x0 + 512].cpu().numpy()
    plan_v = _cabi.plan(a, b, c, 512, 512, 0.1, view=(H, W, y0, x0))
    order_check(render(plan_v).cpu().numpy(), want, "c2x16, 512^2 window")
    wgt = torch.rand(512, 512, 3, generator=torch.Generator().manual_seed(8)).to(dev)
    pad = torch.zeros(H, W, 3, device=dev)
    pad[y0:y0 + 512, x0:x0 + 512] = wgt
    check_grads(gradients(plan_v, a, b, c, wgt), gradients(plan_w, a, b, c, pad), sig.numpy(), "c2x16")


# ---- (10) host function --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(if_dmax=True, dmax_mode="fix", dmax=0.3), dict(if_dmax=True, dmax_mode="dynamic", dmax=25),
                                dict(if_dmax=False)], ids=["fix0.3", "dynamic25", "unbounded"])
def test_host_function_on_the_gpu(kw, dev):
    from gsasr_amd import gaussian_splatting as gsp, synthetic
    H, W, scale = 96, 80, 4.0
    window = (13, 9, 61, 47)
    y0, x0, h, w = window
    p = synthetic.gs_parameters(24, 20, seed=29, gpp=2)
    sm = torch.tensor([scale, scale])
    wgt = torch.rand(3, h, w, generator=torch.Generator().manual_seed(3)).to(dev)
    for sm_dev in (sm.to(dev), (scale, scale)):
        pv = p.to(dev).requires_grad_(True)
        got = gsp.generate_2D_gaussian_splatting_view((H, W), pv, scale, sm_dev, window, **kw)
        assert tuple(got.shape) == (3, h, w) and got.is_cuda and got.requires_grad
        (got * wgt).sum().backward()
        pw = p.to(dev).requires_grad_(True)
        full = gsp.generate_2D_gaussian_splatting_step((H, W), pw, scale, sm_dev, **kw)
        err = float((got.detach() - full.detach()[:, y0:y0 + h, x0:x0 + w]).abs().max())
        assert err <= ORDER_RTOL * max(1.0, float(full.abs().max())), err
        (full[:, y0:y0 + h, x0:x0 + w] * wgt).sum().backward()
        a, b = pv.grad.cpu().numpy(), pw.grad.cpu().numpy()
        rel = float(np.abs(a - b).max() / np.abs(b).max())
        print(f"d/d parameters, view against the whole-image function: rel {rel:.3e}")
        assert np.isfinite(a).all() and rel <= GRAD_RTOL
    # 8-bit, window: within a level of the quantised float window (exactly so away from the rounding boundaries)
    got8 = gsp.generate_2D_gaussian_splatting_step_uint8((H, W), p.to(dev), scale, sm.to(dev), window=window, crop=(h - 2, w - 1),
                                                         bgr=True, **kw)
    assert got8.dtype == torch.uint8 and tuple(got8.shape) == (h - 2, w - 1, 3)
    ref = got.detach().permute(1, 2, 0)[: h - 2, : w - 1].flip(-1).cpu().numpy()
    assert within_one_level(got8.cpu().numpy(), ref, 255 * 1e-4)
    gsp.deferred_asserts.flush()
    with pytest.raises(RuntimeError, match="no fallback"):
        gsp.generate_2D_gaussian_splatting_view((H, W), p.to(dev).reshape(2, -1, 9), scale, sm, window)


def pixel_centred_parameters(H, W, n, seed):
    """raw parameters whose Gaussians sit on pixel centres of the H x W grid (H, W powers of two: the means are exact floats),
    with activated sigmas in [0.08, 0.15]"""
    rng = np.random.RandomState(seed)
    logit = lambda v: np.log(v / (1 - v))
    p = np.zeros((n, 9), np.float32)
    p[:, 0] = logit(rng.uniform(0.08, 0.15, n))
    p[:, 1] = logit(rng.uniform(0.08, 0.15, n))
    p[:, 2] = rng.uniform(-0.6, 0.6, n)
    p[:, 3] = rng.uniform(0.0, 3.0, n)
    p[:, 4:7] = rng.uniform(-2.0, 2.0, (n, 3))
    cells = rng.choice(H * W, n, replace=False)
    p[:, 7] = ((cells % W) + 0.5) / W
    p[:, 8] = ((cells // W) + 0.5) / H
    return torch.from_numpy(p)


@pytest.mark.parametrize("scale", [8.5, 2.0], ids=["x8.5-141steps", "x2-33steps"])
def test_host_function_on_the_gpu_against_its_cpu_result(scale, dev):
    """The window on CUDA tensors against the same call on CPU tensors, at the image bar of 1e-4.

    The CPU result is `rendering_python`, the reference's `cuda_rendering=False` path -- "an approximation of the kernels": every
    Gaussian is sampled on num_step = int(20 / step) points per axis, `step` apart in sigma units (one sample per HR pixel),
    divided by its largest SAMPLE + 1e-4 and resampled bilinearly at kernel index  i + num_step / 2 - W q  for pixel i and mean
    q.  It is the splat itself -- to the error worked out here -- exactly where that approximation is exact, and the cases are
    those inputs (on arbitrary ones it is off by 0.1 and more, for the whole-image function just the same):
      * the index is an integer (no interpolation) and a sample sits on the peak iff num_step is odd and W q is a half-integer:
        means on pixel centres, and scales with an odd step count -- x8.5: int(141.67) = 141, x2: int(33.33) = 33, both far
        from the next integer (x4 gives 66: measured 0.93 off);
      * the normalisation leaves a relative amplitude error of 1e-4 * 2 pi sx sy sqrt(1 - rho^2) <= 1.4e-5 for sigmas <= 0.15,
        times the sum of the colours on a pixel (<= 2 here): <= 3e-5;
      * fp32 grid coordinates put the index off an integer by <= 1e-5 samples: <= 1e-5 of a neighbour's value.
    In all < 5e-5 against the bar's 1e-4; on CPU tensors alone the python rendering of these inputs is 2.1e-5 (x8.5) and 1.2e-5
    (x2) from the oracle, and the kernels are held to the oracle at 1e-4 by the tests above."""
    from gsasr_amd import gaussian_splatting as gsp
    H, W = 128, 64
    window = (29, 7, 71, 45)
    y0, x0, h, w = window
    p = pixel_centred_parameters(H, W, 700, seed=3)
    sm = torch.tensor([scale, scale])
    assert int(10 * 2 / (1.2 / sm[0])) % 2 == 1
    cpu = gsp.generate_2D_gaussian_splatting_view((H, W), p, scale, sm, window, if_dmax=False)
    assert float(cpu.max()) > 0.5
    for sm_dev in (sm.to(dev), (scale, scale)):
        got = gsp.generate_2D_gaussian_splatting_view((H, W), p.to(dev), scale, sm_dev, window, if_dmax=False)
        err = float((got.cpu() - cpu).abs().max())
        print(f"window: max|gpu - cpu| {err:.3e} (largest value {float(cpu.max()):.3f})")
        assert got.is_cuda and tuple(got.shape) == (3, h, w) and err <= IMG_ATOL
    # the bounded op with a box no Gaussian's support reaches (dmax 0.5 = 15 px and more each way; supports end below 7 px) is the same image
    got = gsp.generate_2D_gaussian_splatting_view((H, W), p.to(dev), scale, sm.to(dev), window, if_dmax=True, dmax_mode="fix", dmax=0.5)
    err = float((got.cpu() - cpu).abs().max())
    print(f"window, bounded op: max|gpu - cpu| {err:.3e}")
    assert err <= IMG_ATOL
    gsp.deferred_asserts.flush()
