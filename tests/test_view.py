"""A rectangular window of the HR grid (gsasr_view, the `_view` entry points; generate_2D_gaussian_splatting_view): what can be
checked without a GPU -- the ABI surface, every argument check of the header (they come before anything touches the workspace
or the device), workspace sizing, and the host function on CPU tensors.  tests/test_view_gpu.py has the rendering."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from gsasr_amd import _cabi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VIEW_SYMBOLS = ("gsasr_splat_workspace_bytes_view", "gsasr_step_workspace_bytes_view", "gsasr_splat_plan_view",
                "gsasr_splat_forward_view", "gsasr_splat_forward_u8_view", "gsasr_splat_backward_view", "gsasr_step_forward_view",
                "gsasr_step_forward_u8_view", "gsasr_step_backward_view")


def test_header_bindings_and_library_agree_on_the_view_entry_points():
    hdr = open(os.path.join(ROOT, "include", "gsasr_splat.h")).read()
    assert re.search(r"typedef struct gsasr_view \{\s*int full_h, full_w;[^}]*int y0, x0;[^}]*\} gsasr_view;", hdr)
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(gsasr_[a-z_0-9]+)\s*\(", hdr))
    L = ctypes.CDLL(_cabi.LIB_PATH)
    for name in VIEW_SYMBOLS:
        assert name in declared and name in _cabi.EXPORTS and hasattr(L, name), name
        assert re.search(name + r"\([^;]*const gsasr_view \*", hdr), name      # each takes the view next to the dims
    assert declared == set(_cabi.EXPORTS), declared ^ set(_cabi.EXPORTS)
    # new entry points only: version and struct stay
    assert _cabi.lib().gsasr_abi_version() == 7 and "#define GSASR_SPLAT_ABI_VERSION 7" in hdr
    assert ctypes.sizeof(_cabi.Dims) == 64 and ctypes.sizeof(_cabi.View) == 16


def window_dims(**kw):
    """a legal window: 40 x 52 pixels"""
    return _cabi.make_dims(64, 40, 52, kw.pop("dmax", 0.1), **kw)


def batched_dims():
    d = _cabi.make_batch_dims(32, [(40, 52), (33, 20)], 52, 40, 0.1)
    return d


GOOD_VIEW = (300, 400, 17, 29)
# name -> (dims, view): everything the header calls GSASR_ERR_ARG
BAD = {
    "row band": (lambda: window_dims(rows=(0, 24)), GOOD_VIEW),
    "row band from row 8": (lambda: window_dims(rows=(8, 40)), GOOD_VIEW),
    "batched canvas": (batched_dims, GOOD_VIEW),
    "leaves the grid below": (window_dims, (300, 400, 261, 29)),
    "leaves the grid on the right": (window_dims, (300, 400, 17, 349)),
    "negative y0": (window_dims, (300, 400, -1, 29)),
    "negative x0": (window_dims, (300, 400, 17, -5)),
    "window larger than the grid": (window_dims, (39, 400, 0, 0)),
    "full_h < 2": (window_dims, (1, 400, 0, 0)),
    "full_w above the limit": (window_dims, (300, 32768, 0, 0)),
    "full_h above the limit": (window_dims, (40000, 400, 17, 29)),
    "bad dims": (lambda: _cabi.make_dims(64, 1, 52, 0.1), GOOD_VIEW),
}


def call_entry(name, d, v):
    """the entry point `name` with dims / view and host stand-ins for every pointer (never dereferenced: the argument checks
    come first); a legal call then fails on the workspace, GSASR_ERR_WORKSPACE"""
    L = _cabi.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    dp, vp = ctypes.byref(d), ctypes.byref(v)
    if name == "gsasr_splat_plan_view":
        return L.gsasr_splat_plan_view(p, p, p, dp, vp, None, 0, None)
    if name == "gsasr_splat_forward_view":
        return L.gsasr_splat_forward_view(dp, vp, None, 0, p, None)
    if name == "gsasr_splat_forward_u8_view":
        return L.gsasr_splat_forward_u8_view(dp, vp, None, 0, p, 8, 8, 24, 0, None)
    if name == "gsasr_splat_backward_view":
        return L.gsasr_splat_backward_view(p, p, p, p, p, p, p, dp, vp, None, 0, None)
    if name == "gsasr_step_forward_view":
        return L.gsasr_step_forward_view(p, p, dp, vp, None, 0, p, None)
    if name == "gsasr_step_forward_sm_view":
        return L.gsasr_step_forward_sm_view(p, p, 2, 1.2, None, dp, vp, None, 0, p, None)
    if name == "gsasr_step_forward_u8_view":
        return L.gsasr_step_forward_u8_view(p, p, dp, vp, None, 0, p, 8, 8, 24, 0, None)
    if name == "gsasr_step_forward_sm_u8_view":
        return L.gsasr_step_forward_sm_u8_view(p, p, 2, 1.2, None, dp, vp, None, 0, p, 8, 8, 24, 0, None)
    assert name == "gsasr_step_backward_view"
    return L.gsasr_step_backward_view(p, p, p, p, dp, vp, None, 0, None)


ENTRIES = [n for n in _cabi.EXPORTS if n.endswith("_view") and "workspace_bytes" not in n]


@pytest.mark.parametrize("case", sorted(BAD), ids=lambda c: c.replace(" ", "_"))
def test_illegal_views_are_refused_before_anything_is_enqueued(case):
    make, view = BAD[case]
    d, v = make(), _cabi.View(*view)
    L = _cabi.lib()
    assert L.gsasr_splat_workspace_bytes_view(ctypes.byref(d), ctypes.byref(v)) == 0
    assert L.gsasr_step_workspace_bytes_view(ctypes.byref(d), ctypes.byref(v)) == 0
    assert set(ENTRIES) >= set(VIEW_SYMBOLS[2:])
    for name in ENTRIES:
        assert call_entry(name, d, v) == -1, (name, L.gsasr_last_error())      # GSASR_ERR_ARG
        assert L.gsasr_last_error()


def test_a_legal_view_is_sized_by_the_window():
    L = _cabi.lib()
    d, v = window_dims(), _cabi.View(*GOOD_VIEW)
    for name in ENTRIES:
        assert call_entry(name, d, v) == -2, name       # past the argument checks: GSASR_ERR_WORKSPACE (null workspace)
    for fn, fn_view in ((L.gsasr_splat_workspace_bytes, L.gsasr_splat_workspace_bytes_view),
                        (L.gsasr_step_workspace_bytes, L.gsasr_step_workspace_bytes_view)):
        n = fn_view(ctypes.byref(d), ctypes.byref(v))
        full = fn(ctypes.byref(_cabi.make_dims(64, 300, 400, 0.1)))
        assert 0 < n < full                             # the cell tables and px / py follow the window, not the grid
        assert n == fn(ctypes.byref(d))                 # ... at this density the same layout as a 40 x 52 image
    # windows touching the grid's far corner, and the whole grid as a view of itself, are legal
    assert L.gsasr_splat_workspace_bytes_view(ctypes.byref(d), ctypes.byref(_cabi.View(300, 400, 260, 348))) > 0
    whole = _cabi.make_dims(64, 300, 400, 0.1)
    assert L.gsasr_splat_workspace_bytes_view(ctypes.byref(whole), ctypes.byref(_cabi.View(300, 400, 0, 0))) == \
        L.gsasr_splat_workspace_bytes(ctypes.byref(whole))
    # a null view is the plain entry point
    assert L.gsasr_splat_workspace_bytes_view(ctypes.byref(whole), None) == L.gsasr_splat_workspace_bytes(ctypes.byref(whole))


def test_kernel_choice_rules_see_the_windows_expected_gaussians():
    """density is read as h * w / s: with the s of the whole grid a 1024^2 window of a 6144^2 grid at one Gaussian per 16
    pixels (config 3's shape) would count as a dense plan -- one Gaussian per 4 pixels and more -- and carry tile lists.  The
    rules are evaluated with s * (h * w) / (full_h * full_w); the workspace size shows it."""
    L = _cabi.lib()
    s = 1536 * 1536
    win, v = _cabi.make_dims(s, 1024, 1024, 0.1, flags=_cabi.FLAG_FORWARD_ONLY), _cabi.View(6144, 6144, 2560, 2560)
    n_view = L.gsasr_splat_workspace_bytes_view(ctypes.byref(win), ctypes.byref(v))
    n_plain = L.gsasr_splat_workspace_bytes(ctypes.byref(win))
    no_lists = _cabi.make_dims(s, 1024, 1024, 0.1, flags=_cabi.FLAG_FORWARD_ONLY, list_cap=-1)
    assert n_view == L.gsasr_splat_workspace_bytes(ctypes.byref(no_lists)) < n_plain
    # a registered choice is keyed on whole-image shapes: not looked up for a view of the same dims
    try:
        _cabi.set_kernel_choice(win, 0, 512)
        assert L.gsasr_splat_workspace_bytes(ctypes.byref(win)) != n_plain
        assert L.gsasr_splat_workspace_bytes_view(ctypes.byref(win), ctypes.byref(v)) == n_view
        # ... nor under the dims the rules are evaluated with
        live = _cabi.make_dims(s * 1024 * 1024 // (6144 * 6144), 1024, 1024, 0.1, flags=_cabi.FLAG_FORWARD_ONLY)
        _cabi.set_kernel_choice(live, 0, 512)
        assert L.gsasr_splat_workspace_bytes_view(ctypes.byref(win), ctypes.byref(v)) == n_view
    finally:
        _cabi.clear_kernel_choices()


def test_python_shape_cache_and_pool_key_tell_a_view_from_an_image():
    a = _cabi._image_shape(_cabi._SPLAT_BYTES, 64, 40, 52, 0.1, 0)
    b = _cabi._image_shape(_cabi._SPLAT_BYTES, 64, 40, 52, 0.1, 0, view=GOOD_VIEW)
    c = _cabi._image_shape(_cabi._SPLAT_BYTES, 64, 40, 52, 0.1, 0, view=(300, 400, 18, 29))
    assert a is not b and b is not c
    assert _cabi._view_of(a[0][0]) is None
    for variant in b[0]:
        v = _cabi._view_of(variant)
        assert (v.full_h, v.full_w, v.y0, v.x0) == GOOD_VIEW
    dev = torch.device("cpu")
    keys = {_cabi._pool_key(x[0][0], x[1], dev, 0) for x in (a, b, c)}
    assert len(keys) == 3
    p = _cabi.Plan(b[0][0], torch.empty(0), dev)
    assert p.view is _cabi._view_of(b[0][0])
    assert _cabi._view_of(_cabi._dims_with(p, _cabi.FLAG_OVERWRITE_IMAGE)) is p.view       # flag copies keep the view
    with pytest.raises(RuntimeError):
        _cabi._image_shape(_cabi._SPLAT_BYTES, 64, 40, 52, 0.1, 0, view=(300, 400, 280, 29))


def parameters(n=96, seed=5):
    g = torch.Generator().manual_seed(seed)
    p = 0.5 * torch.randn(n, 9, generator=g)
    p[:, 7:9] = torch.rand(n, 2, generator=g)
    return p


@pytest.mark.parametrize("window", [(3, 5, 17, 11), (0, 0, 2, 36), (23, 25, 17, 11), (0, 0, 40, 36)])
def test_host_function_on_cpu_tensors_is_the_slice(window):
    from gsasr_amd import gaussian_splatting as gsp
    H, W = 40, 36
    y0, x0, h, w = window
    sm = torch.tensor([4.0, 4.0])
    p = parameters().requires_grad_(True)
    full = gsp.generate_2D_gaussian_splatting_step((H, W), p, 4.0, sm, cuda_rendering=False)
    for kw in (dict(cuda_rendering=False), dict()):       # CPU tensors take the python rendering either way
        got = gsp.generate_2D_gaussian_splatting_view((H, W), p, 4.0, sm, window, **kw)
        assert tuple(got.shape) == (3, h, w) and torch.equal(got, full[:, y0:y0 + h, x0:x0 + w])
    wgt = torch.rand(3, h, w, generator=torch.Generator().manual_seed(1))
    g_view, = torch.autograd.grad((got * wgt).sum(), p)
    g_full, = torch.autograd.grad((full[:, y0:y0 + h, x0:x0 + w] * wgt).sum(), p)
    assert torch.equal(g_view, g_full) and float(g_view.abs().max()) > 0
    # 8-bit: crop and channel order apply to the window
    whole = gsp.generate_2D_gaussian_splatting_step_uint8((H, W), p, 4.0, sm)
    got8 = gsp.generate_2D_gaussian_splatting_step_uint8((H, W), p, 4.0, sm, window=window)
    assert got8.dtype == torch.uint8 and torch.equal(got8, whole[y0:y0 + h, x0:x0 + w])
    crop = (max(1, h - 3), max(1, w - 4))
    got8 = gsp.generate_2D_gaussian_splatting_step_uint8((H, W), p, 4.0, sm, window=window, crop=crop, bgr=True)
    assert torch.equal(got8, whole[y0:y0 + crop[0], x0:x0 + crop[1]].flip(-1))
    assert np.unique(whole.numpy()).size > 20


def test_host_function_checks_its_window():
    from gsasr_amd import gaussian_splatting as gsp
    p, sm = parameters(), torch.tensor([4.0, 4.0])
    for bad in ((0, 0, 1, 8), (30, 0, 11, 8), (0, 30, 8, 7), (-1, 0, 8, 8), (0, 0, 8), None):
        with pytest.raises(ValueError):
            gsp.generate_2D_gaussian_splatting_view((40, 36), p, 4.0, sm, bad, cuda_rendering=False)
    with pytest.raises(ValueError):
        gsp.generate_2D_gaussian_splatting_step_uint8((40, 36), p, 4.0, sm, window=(0, 0, 41, 8))
    with pytest.raises(ValueError):
        gsp.generate_2D_gaussian_splatting_step_uint8((40, 36), p, 4.0, sm, window=(0, 0, 8, 8), crop=(9, 8))
    # dmax_mode resolves against sr_size, not the window (CPU rendering ignores dmax; the resolver is shared)
    assert gsp._resolve_dmax(25, "dynamic", (40, 36)) == 27 / 36
