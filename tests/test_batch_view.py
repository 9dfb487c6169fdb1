"""One window of the HR grid per sample of a batched canvas (gsasr_view with dims.batch = B > 1; the `windows` keyword of
generate_2D_gaussian_splatting_batch): what can be checked without a GPU -- the argument checks of the header, workspace
sizing, the bindings' shape cache and pool key, and the host function on CPU tensors.  tests/test_batch_view_gpu.py has the
rendering."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from gsasr_amd import _cabi

SIZES = [(40, 52), (33, 20), (16, 16)]                                   # the windows
VIEWS = [(300, 400, 17, 29), (100, 90, 67, 70), (64, 64, 0, 0)]          # full_h, full_w, y0, x0: one touches its grid's corner


def canvas(sizes=SIZES, **kw):
    return _cabi.make_batch_dims(32, sizes, max(w for _, w in sizes), max(h for h, _ in sizes), kw.pop("dmax", 0.1), **kw)


def views(vs):
    return (_cabi.View * len(vs))(*[_cabi.View(*v) for v in vs])


def both_sizes(d, v):
    L = _cabi.lib()
    return L.gsasr_splat_workspace_bytes_view(ctypes.byref(d), v), L.gsasr_step_workspace_bytes_view(ctypes.byref(d), v)


def test_a_canvas_of_windows_has_a_workspace():
    """(the parent answers 0: a view went with one whole image only)"""
    d = canvas()
    a, b = both_sizes(d, views(VIEWS))
    assert a > 0 and b > a
    L = _cabi.lib()
    # the table of views is all a canvas of windows adds to the plain canvas of the same slots
    assert a == L.gsasr_splat_workspace_bytes(ctypes.byref(d)) + 16 * _cabi.MAX_BATCH
    # uniform windows (the training case) likewise
    du = canvas([(32, 48)] * 3)
    assert both_sizes(du, views([(256, 384, 5, 7), (128, 192, 96, 144), (64, 96, 0, 0)]))[0] > 0


BAD = {
    "a window leaves its grid below": (canvas, [VIEWS[0], (100, 90, 68, 70), VIEWS[2]]),
    "a window leaves its grid on the right": (canvas, [VIEWS[0], VIEWS[1], (64, 31, 0, 16)]),
    "negative origin": (canvas, [(300, 400, -1, 29), VIEWS[1], VIEWS[2]]),
    "grid above the limit": (canvas, [(32768, 400, 17, 29), VIEWS[1], VIEWS[2]]),
    "grid smaller than the window": (canvas, [VIEWS[0], VIEWS[1], (15, 64, 0, 0)]),
    "continuous plan": (lambda: canvas(flags=_cabi.FLAG_CONTINUOUS), VIEWS),
}


@pytest.mark.parametrize("case", sorted(BAD), ids=lambda c: c.replace(" ", "_"))
def test_illegal_canvases_of_windows_are_refused(case):
    make, vs = BAD[case]
    d, v = make(), views(vs)
    assert both_sizes(d, v) == (0, 0)
    L = _cabi.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    # (the argument checks come before anything reads the null workspace)
    assert L.gsasr_splat_plan_view(p, p, p, ctypes.byref(d), v, None, 0, None) == -1
    assert L.gsasr_step_forward_view(p, p, ctypes.byref(d), v, None, 0, p, None) == -1
    assert L.gsasr_step_backward_view(p, p, p, p, ctypes.byref(d), v, None, 0, None) == -1
    assert L.gsasr_last_error()


def test_windows_that_do_not_fit_their_slot_are_refused():
    v = views(VIEWS)
    # a window taller than the slot / wider than the canvas, a 1-pixel window: the dims' own checks, per sample
    d = canvas()
    d.sample_hw[2] = d.slot + 1
    assert both_sizes(d, v) == (0, 0)
    d = canvas()
    d.sample_hw[3] = d.w + 1
    assert both_sizes(d, v) == (0, 0)
    d = canvas()
    d.sample_hw[4] = 1
    assert both_sizes(d, v) == (0, 0)
    # a row band of the canvas
    d = canvas()
    d.row1 = d.h - 16
    assert both_sizes(d, v) == (0, 0)
    d = canvas()
    d.row0 = 16
    assert both_sizes(d, v) == (0, 0)
    # a legal call gets past the argument checks: GSASR_ERR_WORKSPACE for the null workspace
    d = canvas()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    assert _cabi.lib().gsasr_splat_plan_view(p, p, p, ctypes.byref(d), v, None, 0, None) == -2


def test_identity_views_are_the_plain_canvas():
    L = _cabi.lib()
    d = canvas()
    plain = L.gsasr_splat_workspace_bytes(ctypes.byref(d)), L.gsasr_step_workspace_bytes(ctypes.byref(d))
    ident = views([(h, w, 0, 0) for h, w in SIZES])
    assert both_sizes(d, ident) == plain
    assert both_sizes(d, None) == plain
    # one sample off its origin and the table is there
    assert both_sizes(d, views([(40, 52, 0, 0), (33, 20, 0, 0), (17, 16, 1, 0)]))[0] == plain[0] + 16 * _cabi.MAX_BATCH
    # a plain canvas and a single window are sized as before this change (the bytes its parent answered for these shapes)
    assert plain == (36352, 43264)
    one, v = _cabi.make_dims(64, 40, 52, 0.1), _cabi.View(300, 400, 17, 29)
    assert both_sizes(one, ctypes.byref(v)) == (30208, 34560)


def test_kernel_choice_rules_see_the_windows_expected_gaussians():
    """the canvas is judged with sum_b nper * h_b w_b / (full_h_b full_w_b): 16 x 192^2 windows of 768^2 grids whose samples hold
    one Gaussian per pixel of the WINDOW would be a dense plan by its own s -- and carry tile lists -- where the windows can
    expect a sixteenth of them"""
    L = _cabi.lib()
    B, n = 16, 192 * 192
    d = _cabi.make_batch_dims(n, [(192, 192)] * B, 192, 192, 0.1, flags=_cabi.FLAG_FORWARD_ONLY)
    v = views([(768, 768, 13 * b, 7 * b) for b in range(B)])
    no_lists = _cabi.make_batch_dims(n, [(192, 192)] * B, 192, 192, 0.1, flags=_cabi.FLAG_FORWARD_ONLY)
    no_lists.list_cap = -1
    n_view = L.gsasr_splat_workspace_bytes_view(ctypes.byref(d), v)
    assert n_view == L.gsasr_splat_workspace_bytes(ctypes.byref(no_lists)) + 16 * _cabi.MAX_BATCH < L.gsasr_splat_workspace_bytes(ctypes.byref(d))


def test_python_shape_cache_and_pool_key_tell_the_views_apart():
    a = _cabi._canvas_shape(32, SIZES, 0.1, 0)
    b = _cabi._canvas_shape(32, SIZES, 0.1, 0, views=VIEWS)
    c = _cabi._canvas_shape(32, SIZES, 0.1, 0, views=[VIEWS[0], VIEWS[1], (64, 64, 1, 0)])
    assert a is not b and b is not c and b is _cabi._canvas_shape(32, SIZES, 0.1, 0, views=VIEWS)
    assert _cabi._view_of(a[0][0]) is None
    for variant in b[0]:
        v = _cabi._view_of(variant)
        assert [(x.full_h, x.full_w, x.y0, x.x0) for x in v] == VIEWS
    dev = torch.device("cpu")
    assert len({_cabi._pool_key(x[0][0], x[1], dev, 0) for x in (a, b, c)}) == 3
    p = _cabi.Plan(b[0][0], torch.empty(0), dev)
    assert p.view is _cabi._view_of(b[0][0])
    with pytest.raises(RuntimeError):
        _cabi._canvas_shape(32, SIZES, 0.1, 0, views=VIEWS[:2])
    with pytest.raises(RuntimeError):
        _cabi._canvas_shape(32, SIZES, 0.1, 0, views=[VIEWS[0], (100, 90, 68, 70), VIEWS[2]])


def parameters(b, n=96, seed=5):
    g = torch.Generator().manual_seed(seed)
    p = 0.5 * torch.randn(b, n, 9, generator=g)
    p[:, :, 7:9] = torch.rand(b, n, 2, generator=g)
    return p


SR = [(40, 36), (24, 60), (33, 33)]
SCALES = [4.0, 2.0, 3.0]
WINDOWS = [(3, 5, 17, 11), (0, 0, 2, 36), (16, 20, 17, 13)]      # the last one touches its grid's far corner


def test_host_function_on_cpu_tensors_is_the_padded_stack_of_slices():
    """(the parent has no such keyword)"""
    from gsasr_amd import gaussian_splatting as gsp
    p = parameters(3).requires_grad_(True)
    sms = [torch.tensor([s, s]) for s in SCALES]
    got = gsp.generate_2D_gaussian_splatting_batch(SR, p, SCALES, sms, windows=WINDOWS)
    hmax, wmax = max(w[2] for w in WINDOWS), max(w[3] for w in WINDOWS)
    assert tuple(got.shape) == (3, 3, hmax, wmax)
    want = []
    for b, (y0, x0, h, w) in enumerate(WINDOWS):
        sx, sy, rho, xy, col = gsp._activate(p[b])
        full = gsp.rendering_python(sx, sy, rho, xy, col, SR[b], gsp._step_size(SCALES[b], sms[b], 1.2, 'scale_modify'), device=p.device)
        want.append(F.pad(full[:, y0:y0 + h, x0:x0 + w], (0, wmax - w, 0, hmax - h)))
    want = torch.stack(want)
    assert torch.equal(got, want) and float(got.detach().abs().max()) > 0
    # ... and the stack the docstring writes out
    stack = torch.stack([F.pad(gsp.generate_2D_gaussian_splatting_view(SR[b], p[b], SCALES[b], sms[b], WINDOWS[b]),
                               (0, wmax - WINDOWS[b][3], 0, hmax - WINDOWS[b][2])) for b in range(3)])
    assert torch.equal(got, stack)
    wgt = torch.rand(got.shape, generator=torch.Generator().manual_seed(1))
    g_got, = torch.autograd.grad((got * wgt).sum(), p)
    g_want, = torch.autograd.grad((want * wgt).sum(), p)
    assert torch.equal(g_got, g_want) and float(g_got.abs().max()) > 0
    # a [B,2] tensor of sizes and a single sample take the same path
    got_t = gsp.generate_2D_gaussian_splatting_batch(torch.tensor(SR), p, SCALES, sms, windows=WINDOWS)
    assert torch.equal(got_t, got)
    one = gsp.generate_2D_gaussian_splatting_batch(SR[:1], p[:1], SCALES[:1], sms[:1], windows=WINDOWS[:1])
    assert torch.equal(one[0], got[0, :, :17, :11])


def test_host_function_checks_its_windows():
    from gsasr_amd import gaussian_splatting as gsp
    p = parameters(3)
    sms = [torch.tensor([s, s]) for s in SCALES]
    pts = torch.zeros(3, 4, 2, dtype=torch.long)
    with pytest.raises(ValueError):
        gsp.generate_2D_gaussian_splatting_batch(SR, p, SCALES, sms, windows=WINDOWS, sample_coords=pts)
    with pytest.raises(ValueError):
        gsp.generate_2D_gaussian_splatting_batch(SR, p, SCALES, sms, windows=WINDOWS, query_coords=pts.float())
    with pytest.raises(ValueError):
        gsp.generate_2D_gaussian_splatting_batch(SR, p, SCALES, sms, windows=WINDOWS[:2])
    for bad in ((0, 0, 1, 8), (30, 0, 11, 8), (0, 30, 8, 7), (-1, 0, 8, 8), (0, 0, 8), None):
        with pytest.raises(ValueError):
            gsp.generate_2D_gaussian_splatting_batch(SR, p, SCALES, sms, windows=[bad, WINDOWS[1], WINDOWS[2]])


def test_without_the_keyword_nothing_changes():
    import inspect
    from gsasr_amd import gaussian_splatting as gsp
    params = list(inspect.signature(gsp.generate_2D_gaussian_splatting_batch).parameters.values())
    assert params[-1].name == "windows" and params[-1].default is None      # behind every existing parameter
    assert [q.name for q in params[:4]] == ["sr_sizes", "gs_parameters", "scales", "scale_modifies"]
    p = parameters(3)
    sms = [torch.tensor([s, s]) for s in SCALES]
    want = torch.stack([F.pad(gsp.generate_2D_gaussian_splatting_step(SR[b], p[b], SCALES[b], sms[b], cuda_rendering=False),
                              (0, 60 - SR[b][1], 0, 40 - SR[b][0])) for b in range(3)])
    # whole-grid windows are the images of the per-sample loop
    whole = gsp.generate_2D_gaussian_splatting_batch(SR, p, SCALES, sms, windows=[(0, 0, h, w) for h, w in SR])
    assert tuple(whole.shape) == (3, 3, 40, 60) and torch.equal(whole, want)
    # the plain call on CPU tensors goes to the rasterizer's argument check, as it did (tests/test_batch_view_gpu.py compares
    # the plain call on the GPU with whole-grid windows, bit for bit)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        gsp.generate_2D_gaussian_splatting_batch(SR, p, SCALES, sms)
