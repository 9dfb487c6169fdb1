"""One window of the HR grid per sample of a batched canvas, on the GPU (gsasr_view with dims.batch = B > 1;
generate_2D_gaussian_splatting_batch(windows=...)).

Bars, by name from tests/test_view_gpu.py: IMG_ATOL = 1e-4 against oracle.gs_oracle.forward_f64; gradients GRAD_RTOL = 2e-4 of
the tensor's max-abs and `_row_tol` per Gaussian against backward_f64; ORDER_RTOL = 2e-5 * max(1, largest value) for "the same
sums in another order".  The oracle renders each sample's rows [y0, y0 + h) of its FULL grid and is cropped; for gradients it
gets the window's weights zero-padded to the full width, as the view test does.

Exact tests render separated Gaussians (`separated()` of the view test: one term per pixel under tau = 104, the dmax boxes
decide which pixels get it).  One dmax serves a whole call and is in normalised units, so the boxes are 12 px on the widest
grid and smaller on the others -- never overlapping on the 64-px lattice."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_view_gpu import (BOX_PX, GRAD_RTOL, IMG_ATOL, ORDER_RTOL, TAU, _row_tol, check_grads, order_check, raw_parameters, separated,
                           within_one_level)

pytestmark = pytest.mark.gpu
BACKWARD = ["BWD_GAUSSIAN", "BWD_TILE", "BWD_HOME"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the MI355X box)"
    return torch.device("cuda:0")


# ---- dense input: four samples, each on its own grid at its own scale ------------------------------------------------------
# (h_lr, w_lr, scale): 576 LR pixels each, so that every sample has the same number of Gaussians; grids 48 x 48 (x2), 72 x 128
# (x4), 256 x 144 (x8), 288 x 288 (x12)
SAMPLES = [(24, 24, 2.0), (18, 32, 4.0), (32, 18, 8.0), (24, 24, 12.0)]
GPP = 2
# (y0, x0, h, w): the first touches the far corner of its grid; the last lies right of every centre of its sample (whose
# Gaussians are squeezed into columns < 130 of 288, std ~5 px): nothing but tails
LAYOUTS = {
    "mixed": [(18, 8, 30, 40), (10, 37, 50, 61), (100, 20, 64, 57), (40, 136, 72, 48)],
    "uniform": [(16, 8, 32, 40), (10, 37, 32, 40), (100, 20, 32, 40), (40, 136, 32, 40)],      # the geo_h path
}
OPS = {"bounded": 0.1, "unbounded": None}


@functools.lru_cache(maxsize=None)
def dense_inputs():
    from gsasr_amd import synthetic
    out = []
    for b, (hl, wl, scale) in enumerate(SAMPLES):
        sig, xy, col, H, W = synthetic.kernel_inputs(hl, wl, scale, seed=31 + b, gpp=GPP)
        if b == 3:
            xy = xy.clone()
            xy[:, 0] = (xy[:, 0] + 1.0) * 0.45 - 1.0
        out.append((sig, xy, col, H, W))
    return out


@functools.lru_cache(maxsize=None)
def dense_case(layout, op):
    """inputs, windows and the oracle's windows / gradients per sample"""
    from oracle import gs_oracle
    dmax = OPS[op]
    refs, wgts, grefs = [], [], []
    for b, ((sig, xy, col, H, W), (y0, x0, h, w)) in enumerate(zip(dense_inputs(), LAYOUTS[layout])):
        a, c, k = sig.numpy(), xy.numpy(), col.numpy()
        refs.append(gs_oracle.forward_f64(a, c, k, H, W, dmax, rows=(y0, y0 + h))[:, x0:x0 + w])
        wgt = torch.rand(h, w, 3, generator=torch.Generator().manual_seed(9 + b))
        pad = np.zeros((h, W, 3), np.float32)
        pad[:, x0:x0 + w] = wgt.numpy()
        grefs.append(gs_oracle.backward_f64(a, c, k, pad, dmax, h=H, rows=(y0, y0 + h)))
        wgts.append(wgt)
    # the tails-only sample: no centre inside its window or within two pixels of it, and a gradient all the same
    sig, xy, col, H, W = dense_inputs()[3]
    assert float(((xy[:, 0] + 1) * 0.5 * (W - 1)).max()) < LAYOUTS[layout][3][1] - 2
    assert np.abs(refs[3]).max() > 1e-4 and np.abs(grefs[3][2]).max() > 0
    return refs, wgts, grefs


def canvas_inputs(dev, pad_to=0):
    """the four samples as one sample-major list, each padded with NaN records (dead to every plan) to `pad_to` Gaussians"""
    parts = []
    for sig, xy, col, _, _ in dense_inputs():
        n = sig.shape[0]
        fill = max(0, pad_to - n)
        parts.append([torch.cat([t, torch.full((fill, t.shape[1]), float("nan"))]) for t in (sig, xy, col)])
    return [torch.cat([p[k] for p in parts]).contiguous().to(dev) for k in range(3)], max(pad_to, dense_inputs()[0][0].shape[0])


def sizes_views(layout):
    wins = LAYOUTS[layout]
    return [(h, w) for _, _, h, w in wins], [(H, W, y0, x0) for (_, _, _, H, W), (y0, x0, _, _) in zip(dense_inputs(), wins)]


def slot_of(plan):
    return plan.dims.slot


def render(plan, fill=float("nan")):
    from gsasr_amd import _cabi
    d = plan.dims
    img = torch.full((d.h, d.w, 3), fill, device=plan.device)
    _cabi.forward(plan, img, overwrite=True)
    return img


def canvas_weights(plan, wgts, dev, junk=True):
    """the samples' weights in their slots; the padding holds junk the backward must not read"""
    d = plan.dims
    g = torch.full((d.h, d.w, 3), 7.0 if junk else 0.0, device=dev)
    for b, wgt in enumerate(wgts):
        g[b * d.slot: b * d.slot + wgt.shape[0], : wgt.shape[1]] = wgt.to(dev)
    return g


def gradients(plan, sig, xy, col, grad):
    from gsasr_amd import _cabi
    out = [torch.full_like(t, float("nan")) for t in (sig, xy, col)]
    _cabi.backward(plan, sig, xy, col, grad.contiguous(), *out, overwrite=True)
    return [t.cpu().numpy() for t in out]


def check_canvas(plan, layout, op, sig, xy, col, n_per, dev, what):
    refs, wgts, grefs = dense_case(layout, op)
    img = render(plan).cpu().numpy()
    slot = slot_of(plan)
    for b, ref in enumerate(refs):
        h, w = ref.shape[:2]
        got = img[b * slot: b * slot + h, :w]
        err = float(np.abs(got - ref).max())
        print(f"{what} sample {b}: image max|err| {err:.3e} (largest value {np.abs(ref).max():.3f})")
        assert np.isfinite(got).all() and err <= IMG_ATOL, (what, b, err)
        # padding of the slot: exactly zero under GSASR_FLAG_OVERWRITE_IMAGE
        assert not img[b * slot + h: (b + 1) * slot].any() and not img[b * slot: (b + 1) * slot, w:].any()
    got = gradients(plan, sig, xy, col, canvas_weights(plan, wgts, dev))
    n = dense_inputs()[0][0].shape[0]
    for b, gref in enumerate(grefs):
        live = slice(b * n_per, b * n_per + n)
        check_grads([g[live] for g in got], gref, dense_inputs()[b][0].numpy(), f"{what} sample {b}", independent=True)
        assert all(not g[b * n_per + n: (b + 1) * n_per].any() for g in got)       # NaN records: exactly zero


# ---- (1) oracle parity ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cutoff", [0.0, 104.0], ids=["adaptive", "tau104"])
@pytest.mark.parametrize("op", sorted(OPS))
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_canvas_of_windows_against_the_oracle(layout, op, cutoff, dev):
    from gsasr_amd import _cabi
    (sig, xy, col), n_per = canvas_inputs(dev)
    sizes, views = sizes_views(layout)
    plan = _cabi.plan(sig, xy, col, 0, 0, OPS[op], cutoff=cutoff, sizes=sizes, views=views)
    assert plan.view is not None and plan.dims.batch == 4
    check_canvas(plan, layout, op, sig, xy, col, n_per, dev, f"{layout}/{op}/{cutoff}")


# ---- (2) every kernel ----------------------------------------------------------------------------------------------------
# forward families of a canvas (the launcher's rules, gsasr_amd/csrc/splat_forward.hip; the wide forward renders single images
# only): name -> (Gaussians per sample after NaN padding, list_cap).  The rules read the Gaussians the windows can expect
# (policy_dims): 1 143 for the 1 152 real ones per sample, 8 128 when padded to 8 192 -- more than a quarter of the canvas'
# 19 520 pixels, a dense plan, which without lists on fewer than 4 096 sub-tiles is the split kernel with record pairs.
FORWARD = {"search": (0, -1), "lists": (0, 256), "split-pairs": (8192, -1), "lists-pairs": (8192, 256)}
# ... and the home-tile backward picks its tile shape by expected Gaussians per cell (80 cells): 14 -> 64 x 32 px, four waves;
# 37 -> 32 x 32, four waves; 101 -> 32 x 16, eight waves (splat_backward.hip)
HOME_PADS = {"64x32": 0, "32x32": 3000, "32x16": 8192}


@pytest.mark.parametrize("kernel", BACKWARD)
@pytest.mark.parametrize("family", sorted(FORWARD))
def test_every_forward_family_and_backward_kernel(family, kernel, dev):
    from gsasr_amd import _cabi
    pad_to, cap = FORWARD[family]
    (sig, xy, col), n_per = canvas_inputs(dev, pad_to)
    sizes, views = sizes_views("mixed")
    plan = _cabi.plan(sig, xy, col, 0, 0, OPS["bounded"], flags=getattr(_cabi, "FLAG_" + kernel), list_cap=cap, sizes=sizes, views=views)
    check_canvas(plan, "mixed", "bounded", sig, xy, col, n_per, dev, f"{family}/{kernel}")


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("tiles", sorted(HOME_PADS))
def test_home_tile_backward_in_every_tile_shape(tiles, layout, dev):
    from gsasr_amd import _cabi
    (sig, xy, col), n_per = canvas_inputs(dev, HOME_PADS[tiles])
    sizes, views = sizes_views(layout)
    plan = _cabi.plan(sig, xy, col, 0, 0, OPS["unbounded"], flags=_cabi.FLAG_BWD_HOME, sizes=sizes, views=views)
    check_canvas(plan, layout, "unbounded", sig, xy, col, n_per, dev, f"home {tiles}/{layout}")


# ---- (3) the same result as the per-sample `_view` plans -------------------------------------------------------------------
GRIDS = [(512, 512), (384, 448), (256, 320), (448, 256)]
SEP_WINDOWS = [(100, 90, 115, 140), (384 - 141, 448 - 139, 141, 139), (37, 51, 160, 149), (110, 110, 36, 36)]      # straddled edges, a corner,
#                                                                                                   an interior, between the lattice
SEP_N = 72          # records per sample: the 8 x 8 lattice of the largest grid + the NaN record, padded


def sep_dmax():
    return 2.0 * BOX_PX / (512 - 1)


def separated_canvas(dev, s_total=SEP_N):
    per = [separated(H, W, s_total, seed=3 + b) for b, (H, W) in enumerate(GRIDS)]
    assert all(p[0].shape[0] == s_total for p in per)
    return per, [torch.cat([p[k] for p in per]).contiguous().to(dev) for k in range(3)]


@pytest.mark.parametrize("family", ["search", "lists", "split-pairs"])
def test_separated_canvas_is_the_per_sample_views_exactly(family, dev):
    from gsasr_amd import _cabi
    s_total = 65536 if family == "split-pairs" else SEP_N          # (a dense plan is a matter of the COUNT)
    cap = FORWARD[family][1]
    per, (sig, xy, col) = separated_canvas(dev, s_total)
    sizes = [(h, w) for _, _, h, w in SEP_WINDOWS]
    views = [(H, W, y0, x0) for (H, W), (y0, x0, _, _) in zip(GRIDS, SEP_WINDOWS)]
    kw = dict(cutoff=TAU, flags=_cabi.FLAG_FORWARD_ONLY, list_cap=cap)
    plan = _cabi.plan(sig, xy, col, 0, 0, sep_dmax(), sizes=sizes, views=views, **kw)
    img = render(plan).cpu().numpy()
    u8 = _cabi.forward_u8(plan).cpu().numpy()
    assert u8.shape == (4, max(h for h, _ in sizes), max(w for _, w in sizes), 3)
    slot = slot_of(plan)
    for b, ((s1, x1, c1), (h, w), view) in enumerate(zip(per, sizes, views)):
        one = _cabi.plan(s1.to(dev), x1.to(dev), c1.to(dev), h, w, sep_dmax(), view=view, **kw)
        want = render(one).cpu().numpy()
        got = img[b * slot: b * slot + h, :w]
        assert np.isfinite(got).all() and np.array_equal(got, want), (b, int((got != want).sum()))
        if b != 3:
            assert np.abs(want).max() > 0.3
        assert not img[b * slot + h: (b + 1) * slot].any() and not img[b * slot: (b + 1) * slot, w:].any()
        # (7) the 8-bit store of the same plan: the quantised float canvas, exactly; zero outside the window
        want8 = (np.clip(want, 0, 1) * np.float32(255.0)).round().astype(np.uint8)
        assert np.array_equal(u8[b, :h, :w], want8)
        assert not u8[b, h:].any() and not u8[b, :, w:].any()
    for edge in (img[0, :140], img[114, :140], img[:115, 0], img[:115, 139]):
        assert np.abs(edge).max() > 1e-3            # sample 0: a Gaussian is cut by each of the four edges


@pytest.mark.parametrize("kernel", BACKWARD)
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_dense_canvas_is_the_per_sample_views_in_another_order(layout, kernel, dev):
    from gsasr_amd import _cabi
    (sig, xy, col), n_per = canvas_inputs(dev)
    sizes, views = sizes_views(layout)
    _, wgts, _ = dense_case(layout, "bounded")
    flags = getattr(_cabi, "FLAG_" + kernel)
    plan = _cabi.plan(sig, xy, col, 0, 0, 0.1, flags=flags, sizes=sizes, views=views)
    img = render(plan).cpu().numpy()
    got = gradients(plan, sig, xy, col, canvas_weights(plan, wgts, dev))
    slot = slot_of(plan)
    for b, ((s1, x1, c1, _, _), (h, w), view) in enumerate(zip(dense_inputs(), sizes, views)):
        a, c, k = s1.to(dev), x1.to(dev), c1.to(dev)
        one = _cabi.plan(a, c, k, h, w, 0.1, flags=flags, view=view)
        order_check(img[b * slot: b * slot + h, :w], render(one).cpu().numpy(), f"{layout}/{kernel} sample {b}")
        want = gradients(one, a, c, k, wgts[b].to(dev))
        check_grads([g[b * n_per: (b + 1) * n_per] for g in got], want, s1.numpy(), f"{layout}/{kernel} sample {b}")


# ---- (4) identity views --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", BACKWARD)
def test_identity_views_are_the_plain_canvas_bit_for_bit(kernel, dev):
    """(separated Gaussians: the forward's sums have one term; the backward kernels are deterministic per plan on them)"""
    from gsasr_amd import _cabi
    per, (sig, xy, col) = separated_canvas(dev)
    sizes = list(GRIDS)
    ident = [(H, W, 0, 0) for H, W in GRIDS]
    kw = dict(cutoff=TAU, flags=getattr(_cabi, "FLAG_" + kernel))
    plain = _cabi.plan(sig, xy, col, 0, 0, sep_dmax(), sizes=sizes, **kw)
    viewed = _cabi.plan(sig, xy, col, 0, 0, sep_dmax(), sizes=sizes, views=ident, **kw)
    assert plain.view is None and viewed.view is not None
    a, b = render(plain).cpu().numpy(), render(viewed).cpu().numpy()
    assert np.isfinite(a).all() and np.abs(a).max() > 1.0 and np.array_equal(a, b)
    wgt = torch.rand(plain.dims.h, plain.dims.w, 3, generator=torch.Generator().manual_seed(2)).to(dev)
    for ga, gb in zip(gradients(plain, sig, xy, col, wgt), gradients(viewed, sig, xy, col, wgt)):
        assert np.isfinite(ga).all() and np.abs(ga).max() > 0 and np.array_equal(ga, gb)
    # the workspaces are interchangeable: identity views ARE the plain call (same note, same layout)
    L = _cabi.lib()
    img = torch.empty(plain.dims.h, plain.dims.w, 3, device=dev)
    d = _cabi._dims_with(viewed, _cabi.FLAG_OVERWRITE_IMAGE)
    assert viewed.workspace.numel() == plain.workspace.numel()
    assert L.gsasr_splat_forward(ctypes.byref(d), viewed.workspace.data_ptr(), viewed.workspace.numel(), img.data_ptr(),
                                 torch.cuda.current_stream(dev).cuda_stream) == 0
    assert np.array_equal(img.cpu().numpy(), a)


def test_identity_windows_of_the_host_function_are_the_plain_batch(dev):
    from gsasr_amd import gaussian_splatting as gsp
    p, sr, scales = host_inputs(dev)
    sms = torch.tensor([[s, s] for s in scales], device=dev)
    # (the same library call -- whole-grid views are normalised away -- on a dense input: the order of a pixel's sum is all
    # that may differ between two runs)
    plain = gsp.generate_2D_gaussian_splatting_batch(sr, p, scales, sms, dmax_mode="fix", dmax=0.1)
    whole = gsp.generate_2D_gaussian_splatting_batch(sr, p, scales, sms, dmax_mode="fix", dmax=0.1, windows=[(0, 0, h, w) for h, w in sr])
    assert plain.shape == whole.shape and float(plain.max()) > 0.5
    order_check(whole.cpu().numpy(), plain.cpu().numpy(), "whole-grid windows against the plain batch")
    gsp.deferred_asserts.flush()


# ---- (5) plan errors -----------------------------------------------------------------------------------------------------
def test_a_plan_belongs_to_its_views(dev):
    from gsasr_amd import _cabi
    L = _cabi.lib()
    st = torch.cuda.current_stream(dev).cuda_stream
    per, (sig, xy, col) = separated_canvas(dev)
    sizes = [(h, w) for _, _, h, w in SEP_WINDOWS]
    views = [(H, W, y0, x0) for (H, W), (y0, x0, _, _) in zip(GRIDS, SEP_WINDOWS)]
    viewed = _cabi.plan(sig, xy, col, 0, 0, sep_dmax(), sizes=sizes, views=views)
    plain = _cabi.plan(sig, xy, col, 0, 0, sep_dmax(), sizes=sizes)
    d = viewed.dims
    img = torch.zeros(d.h, d.w, 3, device=dev)
    g = [torch.zeros_like(t) for t in (sig, xy, col)]
    ptrs = [t.data_ptr() for t in (sig, xy, col, img, *g)]

    def arr(vs):
        return (_cabi.View * len(vs))(*[_cabi.View(*v) for v in vs])

    def fwd(plan, vs):
        ws = plan.workspace
        if vs is None:
            return L.gsasr_splat_forward(ctypes.byref(plan.dims), ws.data_ptr(), ws.numel(), img.data_ptr(), st)
        return L.gsasr_splat_forward_view(ctypes.byref(plan.dims), arr(vs), ws.data_ptr(), ws.numel(), img.data_ptr(), st)

    def bwd(plan, vs):
        ws = plan.workspace
        if vs is None:
            return L.gsasr_splat_backward(*ptrs, ctypes.byref(plan.dims), ws.data_ptr(), ws.numel(), st)
        return L.gsasr_splat_backward_view(*ptrs, ctypes.byref(plan.dims), arr(vs), ws.data_ptr(), ws.numel(), st)

    moved = [list(views) for _ in range(3)]
    moved[0][3] = (448, 256, 110, 111)                 # the last sample's origin
    moved[1][0] = (513, 512, 100, 90)                  # the first sample's grid
    moved[2][1] = (384, 448, 243, 308)                 # a sample in the middle
    ident = [(h, w, 0, 0) for h, w in sizes]
    for call in (fwd, bwd):
        assert call(viewed, views) == 0 and call(plain, None) == 0
        assert call(viewed, None) == -3, L.gsasr_last_error()       # GSASR_ERR_PLAN: the plain entry point on the views' plan
        assert call(plain, views) == -3
        for other in moved:
            assert call(viewed, other) == -3, other
        assert call(viewed, ident) == -3                            # (identity views: the plain call)
        assert call(plain, ident) == 0
    out = torch.zeros(4, 8, 8, 3, dtype=torch.uint8, device=dev)
    assert L.gsasr_splat_forward_u8(ctypes.byref(d), viewed.workspace.data_ptr(), viewed.workspace.numel(), out.data_ptr(), 8, 8, 24, 0, st) == -3
    # views with a band: GSASR_ERR_ARG, whatever the workspace holds
    band = _cabi.Dims.from_buffer_copy(d)
    band.row1 = d.h - 16
    assert L.gsasr_splat_forward_view(ctypes.byref(band), arr(views), viewed.workspace.data_ptr(), viewed.workspace.numel(), img.data_ptr(), st) == -1
    assert L.gsasr_splat_backward_view(*ptrs, ctypes.byref(band), arr(views), viewed.workspace.data_ptr(), viewed.workspace.numel(), st) == -1
    # the step forms check the same note
    p, sr, scales = host_inputs(dev)
    steps = torch.tensor([1.2 / s for s in scales], device=dev)
    hsizes = [(h, w) for _, _, h, w in HOST_WINDOWS]
    hviews = [(H, W, y0, x0) for (H, W), (y0, x0, _, _) in zip(sr, HOST_WINDOWS)]
    _, sp = _cabi.batch_forward(p, steps, hsizes, 0.1, views=hviews)
    gp = torch.empty_like(p)
    grad = torch.zeros(sp.dims.batch, sp.dims.slot, sp.dims.w, 3, device=dev)
    args = (p.data_ptr(), None, grad.data_ptr(), gp.data_ptr(), ctypes.byref(sp.dims))
    tail = (sp.workspace.data_ptr(), sp.workspace.numel(), st)
    assert L.gsasr_step_backward_view(*args, arr(hviews), *tail) == 0
    other = list(hviews)
    other[2] = (other[2][0], other[2][1], other[2][2] + 1, other[2][3])
    assert L.gsasr_step_backward_view(*args, arr(other), *tail) == -3
    assert L.gsasr_step_backward(*args, *tail) == -3
    torch.cuda.synchronize()


# ---- (6) adversarial cutoff ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stacked", [1.0, 0.5])
def test_adversarial_stack_inside_one_window_keeps_the_error_bound(stacked, dev):
    """tests/test_adaptive_cutoff.py's construction (N Gaussians of colour 1 and ~2 px std on ONE spot), inside the window of one
    sample of a canvas whose other samples are GSASR-shaped: the default render stays within eps * max|colour| of the
    never-skip render (cutoff < 0) of the same call -- plus, as there, the fp32 noise of summing up to N terms in another
    grouping, 5e-6 of the value"""
    from gsasr_amd import _cabi, synthetic
    EPS = 1e-5
    n = 8192
    g = np.random.default_rng(5)
    parts = []
    for b, scale in enumerate((4.0, 8.0, 2.0)):
        sig, xy, col, H, W = synthetic.kernel_inputs(48, 48, scale, seed=11 + b, gpp=4)
        parts.append([t[:n].numpy().copy() for t in (sig, xy, col)] + [H, W])
    sig, xy, col, H, W = parts[1]          # the x8 sample (384^2) takes the stack
    m = int(n * stacked)
    xy[:m] = np.array([0.113, -0.207], np.float32)        # pixel (152, 213) of 384^2
    sig[:m, 0] = 0.01 + 0.001 * g.random(m)               # ~2 px
    sig[:m, 1] = 0.01 + 0.001 * g.random(m)
    sig[:m, 2] = 0.0
    col[:m] = 1.0
    views = [(192, 192, 40, 50), (384, 384, 100, 160), (96, 96, 0, 0)]
    sizes = [(120, 100), (110, 128), (96, 64)]
    assert 100 < 152 < 210 and 160 < 213 < 288
    ts = [torch.from_numpy(np.concatenate([p[k] for p in parts])).to(dev) for k in range(3)]
    dmax = 0.25
    img = render(_cabi.plan(*ts, 0, 0, dmax, sizes=sizes, views=views)).cpu().numpy()
    ref = render(_cabi.plan(*ts, 0, 0, dmax, cutoff=-1.0, sizes=sizes, views=views)).cpu().numpy()
    assert ref.max() > 0.5 * m
    err = np.abs(img - ref)
    print(f"stacked {m}: max err {err.max():.3e}, largest value {ref.max():.1f}")
    assert (err <= EPS * 1.002 + 5e-6 * np.abs(ref)).all(), float((err - 5e-6 * np.abs(ref)).max())
    # ... and on GSASR-shaped input, where the windows' cutoff is the data's and terms ARE skipped (the bound is not vacuous)
    sig2, xy2, col2, _, _ = synthetic.kernel_inputs(48, 48, 8.0, seed=12, gpp=4)
    ts2 = [torch.cat([torch.from_numpy(parts[0][k]), (sig2, xy2, col2)[k][:n], torch.from_numpy(parts[2][k])]).to(dev) for k in range(3)]
    ref2 = render(_cabi.plan(*ts2, 0, 0, dmax, cutoff=-1.0, sizes=sizes, views=views)).cpu().numpy()
    err2 = np.abs(render(_cabi.plan(*ts2, 0, 0, dmax, sizes=sizes, views=views)).cpu().numpy() - ref2)
    print(f"GSASR-shaped: max err {err2.max():.3e} (largest value {ref2.max():.3f})")
    assert err2.max() > 0.0
    assert (err2 <= EPS * float(np.abs(ts2[2].cpu().numpy()).max()) * 1.002 + 5e-6 * np.abs(ref2)).all()


# ---- (7) 8-bit output, (8) the host function -------------------------------------------------------------------------------
HOST_SAMPLES = [(24, 20, 4.0), (20, 24, 2.0), (16, 30, 8.0), (30, 16, 12.0)]          # 480 LR pixels each
HOST_WINDOWS = [(13, 9, 61, 47), (40 - 22, 48 - 31, 22, 31), (50, 100, 64, 96), (200, 60, 40, 96)]


def host_inputs(dev, gpp=2):
    from gsasr_amd import synthetic
    p = torch.stack([synthetic.gs_parameters(hl, wl, seed=29 + b, gpp=gpp) for b, (hl, wl, _) in enumerate(HOST_SAMPLES)]).to(dev)
    sr = [(int(hl * s), int(wl * s)) for hl, wl, s in HOST_SAMPLES]
    return p, sr, [s for _, _, s in HOST_SAMPLES]


def test_batch_forward_u8_with_views(dev):
    from gsasr_amd import _cabi
    # dense input: within a level of the quantised float canvas of the same call, only at rounding boundaries
    p, sr, scales = host_inputs(dev)
    steps = torch.tensor([1.2 / s for s in scales], device=dev)
    sizes = [(h, w) for _, _, h, w in HOST_WINDOWS]
    views = [(H, W, y0, x0) for (H, W), (y0, x0, _, _) in zip(sr, HOST_WINDOWS)]
    img, _ = _cabi.batch_forward(p, steps, sizes, 0.1, views=views)
    got8, plan8 = _cabi.batch_forward_u8(p, steps, sizes, 0.1, views=views)
    hmax, wmax = max(h for h, _ in sizes), max(w for _, w in sizes)
    assert tuple(got8.shape) == (4, hmax, wmax, 3) and plan8.dims.flags & _cabi.FLAG_FORWARD_ONLY
    assert float(img.max()) > 0.5
    assert within_one_level(got8.cpu().numpy(), img[:, :, :hmax].permute(0, 2, 3, 1).cpu().numpy(), 255 * 1e-4)
    # separated input (tau = 104 as the process default: the step entry points take it): exactly, with crop and byte order
    old = _cabi.get_default_cutoff()
    _cabi.set_default_cutoff(TAU)
    try:
        grids = [(288, 384, 8.0), (192, 288, 4.0), (384, 192, 12.0)]
        wins = [(50, 130, 171, 149), (192 - 67, 288 - 99, 67, 99), (100, 20, 150, 160)]
        ps = torch.stack([raw_parameters(H, W, s, 64, seed=3 + b) for b, (H, W, s) in enumerate(grids)]).to(dev)
        steps = torch.tensor([1.2 / s for _, _, s in grids], device=dev)
        sizes = [(h, w) for _, _, h, w in wins]
        views = [(H, W, y0, x0) for (H, W, _), (y0, x0, _, _) in zip(grids, wins)]
        dm = 2.0 * BOX_PX / (384 - 1)
        img, _ = _cabi.batch_forward(ps, steps, sizes, dm, views=views)
        crop = (160, 150)
        got8, _ = _cabi.batch_forward_u8(ps, steps, sizes, dm, crop=crop, bgr=True, views=views)
        want8 = (np.clip(img.permute(0, 2, 3, 1).cpu().numpy()[:, : crop[0], : crop[1], ::-1], 0, 1) * np.float32(255.0)).round().astype(np.uint8)
        assert float(img.max()) > 0.5 and np.array_equal(got8.cpu().numpy(), want8)
        # ... and each slot is the single-view step of its sample, bit for bit
        for b, ((H, W, s), (y0, x0, h, w)) in enumerate(zip(grids, wins)):
            one, _ = _cabi.step_forward(ps[b].contiguous(), steps[b: b + 1], h, w, dm, view=(H, W, y0, x0))
            assert np.array_equal(img[b, :, :h, :w].cpu().numpy(), one.cpu().numpy())
    finally:
        _cabi.set_default_cutoff(old)


@pytest.mark.parametrize("kw", [dict(if_dmax=True, dmax_mode="fix", dmax=0.3), dict(if_dmax=False)], ids=["fix0.3", "unbounded"])
@pytest.mark.parametrize("source", ["device-pairs", "python-numbers"])
def test_host_function_under_autograd(source, kw, dev):
    from gsasr_amd import gaussian_splatting as gsp
    p, sr, scales = host_inputs(dev)
    sms = torch.tensor([[s, s] for s in scales], device=dev) if source == "device-pairs" else [(s, s) for s in scales]
    hmax, wmax = max(w[2] for w in HOST_WINDOWS), max(w[3] for w in HOST_WINDOWS)
    wgt = torch.rand(4, 3, hmax, wmax, generator=torch.Generator().manual_seed(3)).to(dev)
    pb = p.clone().requires_grad_(True)
    got = gsp.generate_2D_gaussian_splatting_batch(sr, pb, scales, sms, windows=HOST_WINDOWS, **kw)
    assert tuple(got.shape) == (4, 3, hmax, wmax) and got.is_cuda and got.requires_grad
    (got * wgt).sum().backward()
    pl = p.clone().requires_grad_(True)
    outs = [gsp.generate_2D_gaussian_splatting_view(sr[b], pl[b], scales[b], sms[b], HOST_WINDOWS[b], **kw) for b in range(4)]
    want = torch.stack([F.pad(o, (0, wmax - o.shape[2], 0, hmax - o.shape[1])) for o in outs])
    order_check(got.detach().cpu().numpy(), want.detach().cpu().numpy(), f"{source}: batch against the stack of views")
    for b, (_, _, h, w) in enumerate(HOST_WINDOWS):      # the padding is exactly zero
        assert not got[b, :, h:].any() and not got[b, :, :, w:].any()
    (want * wgt).sum().backward()
    a, b_ = pb.grad.cpu().numpy(), pl.grad.cpu().numpy()
    rel = float(np.abs(a - b_).max() / np.abs(b_).max())
    print(f"{source}: d/d parameters, one batched call against the per-sample views: rel {rel:.3e}")
    assert np.isfinite(a).all() and np.abs(b_).max() > 0 and rel <= GRAD_RTOL
    # per Gaussian (row): the raw parameter rho sits in column 2; tanh keeps |rho| < 1, the row bar reads it as the view test does
    rows_a, rows_b = a.reshape(-1, 9), b_.reshape(-1, 9)
    rho = np.tanh(p.cpu().numpy().reshape(-1, 9)[:, 2:3]) * 0.999999
    bad = np.abs(rows_a - rows_b) > _row_tol(rows_b, np.concatenate([rho, rho, rho], 1))
    assert not bad.any(), (int(np.argwhere(bad)[0][0]), float(np.abs(rows_a - rows_b)[bad].max()))
    gsp.deferred_asserts.flush()


def test_host_function_fallbacks_have_the_same_shape_and_values(dev):
    """a per-sample dmax (dmax_mode='dynamic' on differing sr_sizes) takes the loop over the view function: same shape, and the
    values of the per-sample calls themselves"""
    from gsasr_amd import gaussian_splatting as gsp
    p, sr, scales = host_inputs(dev)
    sms = [torch.tensor([s, s], device=dev) for s in scales]
    got = gsp.generate_2D_gaussian_splatting_batch(sr, p, scales, sms, windows=HOST_WINDOWS, dmax_mode="dynamic", dmax=25)
    hmax, wmax = max(w[2] for w in HOST_WINDOWS), max(w[3] for w in HOST_WINDOWS)
    assert tuple(got.shape) == (4, 3, hmax, wmax)
    for b, (y0, x0, h, w) in enumerate(HOST_WINDOWS):
        one = gsp.generate_2D_gaussian_splatting_view(sr[b], p[b], scales[b], sms[b], HOST_WINDOWS[b], dmax_mode="dynamic", dmax=25)
        order_check(got[b, :, :h, :w].cpu().numpy(), one.cpu().numpy(), f"dynamic dmax, sample {b}")
    # one size for all: the canvas again, dmax resolved against sr_sizes (not the windows)
    sr1, wins1 = [sr[0]] * 4, [HOST_WINDOWS[0], (0, 0, 30, 40), (96 - 20, 80 - 10, 20, 10), (5, 5, 61, 47)]
    got = gsp.generate_2D_gaussian_splatting_batch(sr1, p, [4.0] * 4, [sms[0]] * 4, windows=wins1, dmax_mode="dynamic", dmax=25)
    for b, (y0, x0, h, w) in enumerate(wins1):
        full = gsp.generate_2D_gaussian_splatting_step(sr1[b], p[b], 4.0, sms[0], dmax_mode="dynamic", dmax=25)
        order_check(got[b, :, :h, :w].cpu().numpy(), full[:, y0:y0 + h, x0:x0 + w].cpu().numpy(), f"dynamic dmax on one size, sample {b}")
    gsp.deferred_asserts.flush()
