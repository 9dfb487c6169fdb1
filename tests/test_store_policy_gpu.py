"""The output stores of the step's kernels (the image, the gradients, the plan arrays), against the CPU oracle.

The stores go through one helper that names their cache policy (store_out, gsasr_amd/csrc/splat_common.h: the interleaved image
is stored write-through, the rest plain).  A policy may not change a value, an address or which bytes are written.
What can go wrong in a store path shows at the smallest shapes: exactly one 32 x 16 tile, images ragged in both directions, a row
band, the accumulate form (load + add + store) on memory that is not zero, the planar and 8-bit forms, a canvas with padding --
and in what lies next to the output: every output is allocated inside a larger NaN-filled buffer whose other bytes must not change.

Bars: those of tests/test_hip_parity.py, restated -- image 1e-4 absolute; every gradient tensor within 2e-4 of its max-abs, every
row within (5e-4 + 5e-6 / sqrt(kappa)) of its own max-abs + 1e-5 of the tensor's, every column and element to tests/gradbars.py.
8-bit pixels: the oracle's rint(clamp(v, 0, 1) * 255), exactly where v * 255 is further than 0.05 from a rounding boundary (the
image bar is 1e-4 * 255 = 0.0255 levels), within one level elsewhere.
"""
import functools
import math

import numpy as np
import pytest
import torch

import gradbars

pytestmark = pytest.mark.gpu

IMG_ATOL = 1e-4
GRAD_RTOL = 2e-4
GUARD = 1024                     # elements in front of and behind every output
SHAPES = {"one-tile-16x32": (16, 32, None), "ragged-24x40": (24, 40, None), "ragged-17x33": (17, 33, None),
          "band-8-24-of-40x40": (40, 40, (8, 24))}
DMAX = {"dmax0.1": 0.1, "unbounded": None}
IMG0 = 0.25                      # what the image holds before an accumulating forward
GRAD0 = 2.0 ** -10               # ... and the gradient arrays before an accumulating backward


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the MI355X box)"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _scene(h, w, seed=0):
    """60 - 100 Gaussians on the x4 LR grid of an h x w image (jittered raster order, LR-pixel sized), and an image gradient"""
    rng = np.random.default_rng(seed + 1000 * h + w)
    lh, lw = math.ceil(h / 4), math.ceil(w / 4)
    gpp = 2 if lh * lw < 60 else 1
    n = lh * lw * gpp
    assert 60 <= n <= 100
    jj, ii = np.meshgrid(np.arange(lw), np.arange(lh), indexing="xy")
    cx = np.repeat((jj.ravel() + 0.5) / lw, gpp) + rng.uniform(-0.5, 0.5, n) / lw
    cy = np.repeat((ii.ravel() + 0.5) / lh, gpp) + rng.uniform(-0.5, 0.5, n) / lh
    xy = np.stack([cx, cy], 1) * 2.0 - 1.0
    s = rng.uniform(0.2, 1.0, (n, 2)) * 4.0 / 1.2 * 2.0 / np.array([w - 1, h - 1])
    sig = np.concatenate([s, rng.uniform(-0.8, 0.8, (n, 1))], 1)
    col = rng.uniform(0.05, 0.6, (n, 3))
    wgt = rng.uniform(-1.0, 1.0, (h, w, 3))
    return tuple(np.ascontiguousarray(a, dtype=np.float32) for a in (sig, xy, col, wgt))


@functools.lru_cache(maxsize=None)
def _oracle(h, w, rows, dmax):
    """(image, gradients) of the band `rows` in float64: computed once per case, shared by every test that needs it"""
    from oracle import gs_oracle
    sig, xy, col, wgt = _scene(h, w)
    r = rows or (0, h)
    img = gs_oracle.forward_f64(sig, xy, col, h, w, dmax, rows=r)
    grads = gs_oracle.backward_f64(sig, xy, col, wgt[r[0]:r[1]], dmax, h=h, rows=r)
    assert float(np.abs(img).max()) > 0.05 and all(float(np.abs(g).max()) > 0.0 for g in grads)
    return img, grads


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


class Guarded:
    """a contiguous tensor of `shape` inside a larger buffer filled with NaN (dtype uint8: with 0xA5)"""

    def __init__(self, shape, dev, fill, dtype=torch.float32):
        n = int(np.prod(shape))
        poison = float("nan") if dtype.is_floating_point else 0xA5
        self.buf = torch.full((GUARD + n + GUARD,), poison, dtype=dtype, device=dev)
        self.t = self.buf[GUARD:GUARD + n].view(*shape)
        self.t.fill_(fill)
        self.before = self._bits().clone()

    def _bits(self):
        b = self.buf.view(torch.int32) if self.buf.dtype == torch.float32 else self.buf
        return torch.cat([b[:GUARD], b[-GUARD:]])

    def check(self, what):
        assert bool((self._bits() == self.before).all()), f"{what}: bytes next to the output changed"


def _relmax(got, want):
    return float(np.abs(got - want).max() / max(1e-12, np.abs(want).max()))


def _row_tol(want, sig):
    kappa = np.maximum(1.0 - np.asarray(sig)[:, 2].astype(np.float64) ** 2, 1e-12)[:, None]
    return (5e-4 + 5e-6 / np.sqrt(kappa)) * np.abs(want).max(axis=1, keepdims=True) + 1e-5 * np.abs(want).max() + 1e-30


def _check_grads(grads, gref, sig, what, columns=True):
    for got, want, name in zip(grads, gref, ("sigmas", "coords", "colors")):
        assert np.isfinite(got).all(), (what, name)
        rel = _relmax(got, want)
        print(f"{what}: grad {name} rel err {rel:.3e}")
        assert rel <= GRAD_RTOL, f"{what}: grad {name} rel err {rel:.3e}"
        bad = np.abs(got - want) > _row_tol(want, sig)
        assert not bad.any(), (what, name, int(np.argwhere(bad)[0][0]), float(np.abs(got - want)[bad].max()), float(np.abs(want).max()))
    if columns:
        gradbars.check_kernel(tuple(np.asarray(g, dtype=np.float32) for g in grads), gref, sig, 0.0, what)


def _check_image(got, ref, what):
    assert np.isfinite(got).all(), what
    err = float(np.abs(got - ref).max())
    print(f"{what}: image max|err| {err:.3e}")
    assert err <= IMG_ATOL, f"{what}: image max|err| {err:.3e}"


def _run(h, w, rows, dmax, dev, overwrite, plan_flags=0, fwd_flags=0, list_cap=0, chw=False, backward=True):
    """plan, forward and backward of one case through the C ABI with every output in a guarded buffer; returns the numpy image
    [rows, w, 3] and gradients with what the outputs held before taken off again (float64)"""
    from gsasr_amd import _cabi
    sig, xy, col, wgt = _scene(h, w)
    r = rows or (0, h)
    a, b, c = _t(sig, dev), _t(xy, dev), _t(col, dev)
    plan = _cabi.plan(a, b, c, h, w, dmax, rows=rows, flags=plan_flags | (0 if backward else _cabi.FLAG_FORWARD_ONLY), list_cap=list_cap)
    nr = r[1] - r[0]
    img = Guarded((3, nr, w) if chw else (nr, w, 3), dev, float("nan") if overwrite else IMG0)
    _cabi.forward(plan, img.t, overwrite=overwrite, chw=chw, flags=fwd_flags)
    img.check("image")
    out = img.t.double().cpu().numpy() - (0.0 if overwrite else IMG0)
    if chw:
        out = out.transpose(1, 2, 0)
    grads = None
    if backward:
        gs = [Guarded(t.shape, dev, float("nan") if overwrite else GRAD0) for t in (a, b, c)]
        _cabi.backward(plan, a, b, c, _t(wgt[r[0]:r[1]], dev), *[g.t for g in gs], overwrite=overwrite)
        for g, name in zip(gs, ("grad sigmas", "grad coords", "grad colors")):
            g.check(name)
        grads = tuple(g.t.double().cpu().numpy() - (0.0 if overwrite else GRAD0) for g in gs)
    return out, grads


@pytest.mark.parametrize("overwrite", [True, False], ids=["overwrite", "accumulate"])
@pytest.mark.parametrize("dmax", list(DMAX), ids=list(DMAX))
@pytest.mark.parametrize("shape", list(SHAPES), ids=list(SHAPES))
def test_image_and_gradients_with_guards(shape, dmax, overwrite, dev):
    """image and gradients of the Gaussian-stationary backward (whose wave writes its gradient itself: bwd_write) against the
    oracle, stored over NaN or added to a non-zero image / non-zero gradients; nothing outside the outputs changes"""
    from gsasr_amd import _cabi
    h, w, rows = SHAPES[shape]
    ref, gref = _oracle(h, w, rows, DMAX[dmax])
    img, grads = _run(h, w, rows, DMAX[dmax], dev, overwrite, plan_flags=_cabi.FLAG_BWD_GAUSSIAN)
    what = f"{shape} {dmax} {'overwrite' if overwrite else 'accumulate'}"
    _check_image(img, ref, what)
    # (accumulate: GRAD0 + g is rounded to an ulp of the sum, so elements far below GRAD0 are not held to their own bar)
    _check_grads(grads, gref, _scene(h, w)[0], what, columns=overwrite)


@pytest.mark.parametrize("family", ["search", "list", "wide"])
@pytest.mark.parametrize("overwrite", [True, False], ids=["overwrite", "accumulate"])
def test_forward_kernel_families_share_the_store(family, overwrite, dev):
    """the 8 x 16 kernels from the search and from the plan's tile lists (fwd_store), and the wide kernel (fwd_store_px), on the
    24 x 40 image"""
    from gsasr_amd import _cabi
    h, w, rows = SHAPES["ragged-24x40"]
    flags = _cabi.FLAG_FWD_WIDE if family == "wide" else _cabi.FLAG_FWD_NARROW
    cap = {"search": -1, "list": 512, "wide": -1}[family]
    ref, _ = _oracle(h, w, rows, 0.1)
    img, _ = _run(h, w, rows, 0.1, dev, overwrite, plan_flags=flags, fwd_flags=flags, list_cap=cap, backward=False)
    _check_image(img, ref, f"forward {family}")


@pytest.mark.parametrize("overwrite", [True, False], ids=["overwrite", "accumulate"])
@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
def test_planar_image_store(wide, overwrite, dev):
    """FLAG_CHW_IMAGE: three planes [3, rows, w], through both store functions"""
    from gsasr_amd import _cabi
    h, w, rows = SHAPES["ragged-24x40"]
    flags = _cabi.FLAG_FWD_WIDE if wide else _cabi.FLAG_FWD_NARROW
    ref, _ = _oracle(h, w, rows, None)
    img, _ = _run(h, w, rows, None, dev, overwrite, plan_flags=flags, fwd_flags=flags, chw=True, backward=False)
    _check_image(img, ref, f"planar wide={wide}")


@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
def test_u8_image_store_with_pitch_and_guards(wide, dev):
    """forward_u8 into the interior of a larger byte buffer whose rows are 8 bytes longer than the pixels: the bytes are the
    oracle's quantised pixels, and the row padding and the rows around stay what they were"""
    from gsasr_amd import _cabi
    h, w, rows = SHAPES["ragged-24x40"]
    sig, xy, col, _ = _scene(h, w)
    flags = _cabi.FLAG_FWD_WIDE if wide else _cabi.FLAG_FWD_NARROW
    plan = _cabi.plan(_t(sig, dev), _t(xy, dev), _t(col, dev), h, w, 0.1, flags=_cabi.FLAG_FORWARD_ONLY | flags)
    pitch = 3 * w + 8
    big = torch.full((h + 2, pitch), 0xA5, dtype=torch.uint8, device=dev)
    out = big[1:-1, 4:4 + 3 * w].unflatten(1, (w, 3))
    _cabi.forward_u8(plan, out=out, flags=flags)
    got = big.cpu().numpy()
    px = got[1:-1, 4:4 + 3 * w].reshape(h, w, 3).astype(np.int64)
    got[1:-1, 4:4 + 3 * w] = 0xA5
    assert (got == 0xA5).all(), "bytes next to the 8-bit pixels changed"
    ref, _ = _oracle(h, w, rows, 0.1)
    v = np.clip(ref, 0.0, 1.0) * 255.0
    want = np.rint(v).astype(np.int64)
    assert int(np.abs(px - want).max()) <= 1
    safe = np.abs(v - np.floor(v) - 0.5) > 0.05
    assert safe.mean() > 0.8 and (px[safe] == want[safe]).all()
    assert int(px.max()) > 30


@pytest.mark.parametrize("kernel", ["GAUSSIAN", "TILE", "HOME"])
@pytest.mark.parametrize("overwrite", [True, False], ids=["overwrite", "accumulate"])
def test_backward_kernels_the_abi_can_force(kernel, overwrite, dev):
    """the Gaussian-stationary kernel (bwd_write), the tile-stationary one (gather) and the home-tile one on the 24 x 40 image,
    bounded op, guarded gradient arrays"""
    from gsasr_amd import _cabi
    h, w, rows = SHAPES["ragged-24x40"]
    ref, gref = _oracle(h, w, rows, 0.1)
    img, grads = _run(h, w, rows, 0.1, dev, overwrite, plan_flags=getattr(_cabi, "FLAG_BWD_" + kernel))
    _check_image(img, ref, f"backward {kernel}: image")
    _check_grads(grads, gref, _scene(h, w)[0], f"backward {kernel}", columns=overwrite)


def test_batched_canvas_padding(dev):
    """two samples of different heights: through batch_forward (a fresh planar canvas: each sample equals its own call, the
    padding is exactly zero) and through the plan API accumulating into a canvas that holds 0.25 (the padding is never touched)"""
    import ctypes
    from gsasr_amd import _cabi, synthetic
    sizes = [(24, 40), (17, 33)]
    B, hm, wm = 2, 24, 40
    p = torch.stack([synthetic.gs_parameters(6, 10, seed=70 + b) for b in range(B)]).to(dev)
    steps = torch.tensor([1.2 / 4.0, 1.2 / 4.0], device=dev)
    out, _ = _cabi.batch_forward(p, steps, sizes, 0.1, _cabi.FLAG_FORWARD_ONLY)
    slot = out.shape[2]
    assert tuple(out.shape) == (B, 3, slot, wm) and slot >= hm
    for b, (h, w) in enumerate(sizes):
        one, _ = _cabi.step_forward(p[b], steps[b:b + 1], h, w, 0.1, _cabi.FLAG_FORWARD_ONLY)
        assert float(one.abs().max()) > 0.05
        assert float((out[b, :, :h, :w] - one).abs().max()) <= 2e-6
        pad = out[b].clone()
        pad[:, :h, :w] = 0
        assert float(pad.abs().max()) == 0.0
    # kernel-frame inputs through gsasr_splat_plan / forward: HWC canvas, accumulate, inside a guarded buffer
    per = [_scene(h, w)[:3] for h, w in sizes]
    n = min(a[0].shape[0] for a in per)
    sig, xy, col = (_t(np.concatenate([a[k][:n] for a in per]), dev) for k in range(3))
    d = _cabi.make_batch_dims(n, sizes, wm, hm, 0.1)
    L = _cabi.lib()
    ws = torch.empty(L.gsasr_splat_workspace_bytes(ctypes.byref(d)), dtype=torch.uint8, device=dev)
    st = _cabi._stream(dev)
    _cabi.check(L.gsasr_splat_plan(sig.data_ptr(), xy.data_ptr(), col.data_ptr(), ctypes.byref(d), ws.data_ptr(), ws.numel(), st), "plan")
    img = Guarded((B, d.slot, wm, 3), dev, IMG0)
    _cabi.check(L.gsasr_splat_forward(ctypes.byref(d), ws.data_ptr(), ws.numel(), img.t.data_ptr(), st), "fwd")
    img.check("canvas")
    from oracle import gs_oracle
    for b, (h, w) in enumerate(sizes):
        ref = gs_oracle.forward_f64(per[b][0][:n], per[b][1][:n], per[b][2][:n], h, w, 0.1)
        _check_image(img.t[b, :h, :w].double().cpu().numpy() - IMG0, ref, f"canvas sample {b}")
        rest = img.t[b].clone()
        rest[:h, :w] = IMG0
        assert float((rest - IMG0).abs().max()) == 0.0


def test_cached_plan_outputs_are_read_on_the_stream(dev):
    """plan, forward and backward twice on one workspace (the plans alternate its parity), then a reduction of the image and of
    a gradient array enqueued behind them on the same stream: it must see what a reduction after a synchronise sees (a store
    that left the cache by another road than the reader's load would show here as stale lines)"""
    from gsasr_amd import _cabi
    h, w, rows = SHAPES["band-8-24-of-40x40"]
    sig, xy, col, wgt = _scene(h, w)
    a, b, c = _t(sig, dev), _t(xy, dev), _t(col, dev)
    g = _t(wgt[rows[0]:rows[1]], dev)
    img = torch.full((rows[1] - rows[0], w, 3), float("nan"), device=dev)
    gs = [torch.full_like(t, float("nan")) for t in (a, b, c)]
    for k in range(2):
        plan = _cabi.plan(a, b, c, h, w, 0.1, rows=rows, flags=_cabi.FLAG_BWD_GAUSSIAN)
        img.fill_(float(k))                 # (lines of the image in the reader's cache before the kernels store them)
        _ = img.sum().item()
        _cabi.forward(plan, img, overwrite=True)
        _cabi.backward(plan, a, b, c, g, *gs, overwrite=True)
        first = [img.double().sum(), gs[0].double().sum(), gs[2].double().abs().sum()]
        torch.cuda.synchronize()
        again = [img.double().sum(), gs[0].double().sum(), gs[2].double().abs().sum()]
        for x, y in zip(first, again):
            assert x.item() == y.item(), k
        ref, gref = _oracle(h, w, rows, 0.1)
        assert abs(first[0].item() - ref.sum()) <= IMG_ATOL * ref.size
        _check_image(img.double().cpu().numpy(), ref, f"cached plan {k}")
        _check_grads(tuple(t.double().cpu().numpy() for t in gs), gref, sig, f"cached plan {k}")
