"""Bicubic imresize on the GPU where tests/test_imresize_gpu.py does not reach (csrc/splat_resize.hip): taps staged in several
chunks of 256, every W-pass tile width with a ragged last tile, more than 256 taps per output, windows wider than the image,
lengths 1..8, a mixed batch that changes one sample's tile width and table pitch, and a caller's scratch between NaN guards.
The axis cases and the proof that they reach these paths are in tests/test_imresize_wide.py.

Bars (none comes from what the kernels give).
  a. The matrix, entry by entry: `entry_bar` of tests/test_imresize_wide.py, 4 * 2^-24 * S_ij + 1e-12 with S_ij the absolute sum
     of the float64 weights folding onto (i, j); exactly 0 where none folds.
  b. Random images: per element gamma * (|A_h| |x| |A_w|^T) forward and gamma * (|A_h|^T |g| |A_w|) for the adjoint, with
     gamma = (p_h + p_w + 4) * 2^-24: a running-error bound, one rounding per weight, one per fma, one store per pass, on the
     element's own scale (at 1/64 about 3e-5 of values of 3e-4; ADJ_BAR of tests/test_imresize_gpu.py is 1e-5 absolute there).
     <A x, y> = <x, A^T y> to gamma relative to sum |A x| |y|.
  c. Bits: every output accumulates its taps in ascending order whatever the tiling, so a sample alone and the same sample in
     a batch that forces another tile width and table pitch on it (100 x 80 -> 10 x 10: tile 24 and pitch 42 alone, tile 8 and
     pitch 258 behind a 640-pixel sample at 1/64) give equal bits, forward and backward.
Every case prints what it measured."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from test_imresize import adjoint_f64, resize_f64      # noqa: E402
import wsguard      # noqa: E402
from test_imresize_gpu import padded_batch      # noqa: E402
from test_imresize_wide import (ALL_OK, AXIS_CASES, SMALL_BAD, case_id, check_entries, matrices,      # noqa: E402
                                taps_per_output)

from gsasr_amd import _cabi      # noqa: E402
from gsasr_amd import resize as R      # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
BY_LENGTH = {c[0]: c for c in AXIS_CASES}
BY_LENGTH.update({5: (5, 12, 2.5, True), 7: (7, 2, 1 / 3, True)})
# (H case, W case) by input length
PAIRS = [(640, 640), (1100, 129), (128, 288), (225, 200), (31, 244), (5, 7)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the MI355X box)"
    return torch.device("cuda:0")


# ---- a. the matrix through each kernel ----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ALL_OK, ids=case_id)
def test_matrix_entry_by_entry_through_each_kernel(dev, case):
    n, m, s, aa = case
    eye_n, eye_m = torch.eye(n, device=dev)[None, None], torch.eye(m, device=dev)[None, None]
    # W pass: [n,n] -> [n,m] = A^T;  H pass: [n,n] -> [m,n] = A
    fw = _cabi.imresize(eye_n, torch.full((1, 1, n, m), float("nan"), device=dev), (1.0, s), antialiasing=aa)
    fh = _cabi.imresize(eye_n, torch.full((1, 1, m, n), float("nan"), device=dev), (s, 1.0), antialiasing=aa)
    # W adjoint: grad_in [m,n] = I A;  H adjoint: grad_in [n,m] = A^T I
    bw = _cabi.imresize(torch.full((1, 1, m, n), float("nan"), device=dev), eye_m, (1.0, s), antialiasing=aa, backward=True)
    bh = _cabi.imresize(torch.full((1, 1, n, m), float("nan"), device=dev), eye_m, (s, 1.0), antialiasing=aa, backward=True)
    got = {"W pass": (fw, True), "H pass": (fh, False), "W adjoint": (bw, False), "H adjoint": (bh, True)}
    ratios = {k: check_entries(t[0, 0].cpu().numpy(), case, transposed=tr) for k, (t, tr) in got.items()}
    print(f"imresize matrix {case_id(case)} (p = {taps_per_output(s, aa)}): worst entry / bar " +
          ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))


# ---- b. random images against float64, each element to its own running-error bound ---------------------------------------
def bounds(x, g, hcase, wcase):
    """(forward bound [..., mh, mw], adjoint bound [..., h, w], gamma) for input x and grad_out g (float64 arrays)"""
    Sh, Sw = matrices(hcase)[1], matrices(wcase)[1]
    gamma = (taps_per_output(*hcase[2:]) + taps_per_output(*wcase[2:]) + 4) * U
    return gamma * (Sh @ np.abs(x) @ Sw.T), gamma * (Sh.T @ np.abs(g) @ Sw), gamma


def check_image(y, gx, x, g, hcase, wcase, what):
    """y, gx: float32 results on the sample's own pixels; x, g: the float32 inputs.  All NumPy `[C, ., .]`."""
    assert hcase[3] and wcase[3]
    scales, out_hw = (hcase[2], wcase[2]), (hcase[1], wcase[1])
    x64, g64 = x.astype(np.float64), g.astype(np.float64)
    fb, ab, gamma = bounds(x64, g64, hcase, wcase)
    want_y, want_gx = resize_f64(x64, out_hw, scales), adjoint_f64(g64, x.shape[-2:], scales)
    ef, ea = np.abs(y - want_y), np.abs(gx - want_gx)
    lhs, rhs = float((y.astype(np.float64) * g64).sum()), float((x64 * gx.astype(np.float64)).sum())
    dot = float((np.abs(y.astype(np.float64)) * np.abs(g64)).sum())
    print(f"imresize {what} {x.shape[-2]}x{x.shape[-1]} -> {out_hw[0]}x{out_hw[1]} (p = {taps_per_output(*hcase[2:])}, "
          f"{taps_per_output(*wcase[2:])}; gamma {gamma:.2e}): forward max err {ef.max():.3e} on max|y| {np.abs(want_y).max():.3e}, "
          f"worst err / bound {(ef / np.maximum(fb, 1e-300)).max():.3f}; adjoint max err {ea.max():.3e} on max|A^T g| "
          f"{np.abs(want_gx).max():.3e}, worst err / bound {(ea / np.maximum(ab, 1e-300)).max():.3f}; "
          f"|<Ax,y> - <x,A^T y>| / sum|Ax||y| {abs(lhs - rhs) / dot:.3e}")
    assert y.dtype == np.float32 and gx.dtype == np.float32 and y.shape == want_y.shape and gx.shape == want_gx.shape
    assert (ef <= fb).all(), what
    assert (ea <= ab).all(), what
    assert abs(lhs - rhs) <= gamma * dot, what


@pytest.mark.parametrize("nh,nw", PAIRS, ids=[f"{a}x{b}" for a, b in PAIRS])
def test_random_images_against_f64(dev, nh, nw):
    hcase, wcase = BY_LENGTH[nh], BY_LENGTH[nw]
    rng = np.random.default_rng(1000 + nh + 7 * nw)
    x = rng.random((1, 2, nh, nw), dtype=np.float32)
    g = rng.random((1, 2, hcase[1], wcase[1]), dtype=np.float32) * 2 - 1
    xd = torch.from_numpy(x).to(dev).requires_grad_(True)
    y = R.imresize_batch(xd, scales=[(hcase[2], wcase[2])], out_size=(hcase[1], wcase[1]))
    gx, = torch.autograd.grad(y, xd, torch.from_numpy(g).to(dev))
    check_image(y.detach().cpu().numpy()[0], gx.cpu().numpy()[0], x[0], g[0], hcase, wcase, "random image")


# ---- c. bits do not depend on the tile width or the table pitch ------------------------------------------------------------
def axis_case(n, m):
    return (n, m, m / n, True)


BATCHES = {
    # 640 at 1/64 forces p = 258 and tile width 8 on everybody; alone, 100 x 80 runs one chunk per (wider) tile
    "10x10": ([(640, 640), (100, 80), (10, 10), (25, 40), (4, 5)], (10, 10)),
    "37x45": ([(640, 640), (222, 225), (4, 5)], (37, 45)),
    # every sample full size at one scale: the shared-scale route, no per-sample sizes
    "37x45_shared": ([(222, 225), (222, 225)], (37, 45)),
}


@pytest.mark.parametrize("name", list(BATCHES))
def test_batch_bits_equal_each_sample_alone(dev, name):
    sizes, out = BATCHES[name]
    C = 2
    x = padded_batch(sizes, C, dev, 41).requires_grad_(True)
    go = (torch.rand(len(sizes), C, *out, generator=torch.Generator().manual_seed(42)) * 2 - 1).to(dev)
    y = R.imresize_batch(x, sizes, out_size=out)
    gx, = torch.autograd.grad(y, x, go)
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(gx).all())
    for b, (h, w) in enumerate(sizes):
        one = x.detach()[b:b + 1, :, :h, :w].contiguous().requires_grad_(True)
        y1 = R.imresize_batch(one, out_size=out)
        g1, = torch.autograd.grad(y1, one, go[b:b + 1])
        assert torch.equal(y[b], y1[0]), (name, b, "forward")
        assert torch.equal(gx[b, :, :h, :w], g1[0]), (name, b, "backward")
        assert float(gx[b, :, h:, :].abs().sum()) == 0.0 and float(gx[b, :, :, w:].abs().sum()) == 0.0
        check_image(y[b].detach().cpu().numpy(), g1[0].cpu().numpy(), one.detach()[0].cpu().numpy(), go[b].cpu().numpy(),
                    axis_case(h, out[0]), axis_case(w, out[1]), f"batch {name} sample {b}")


# ---- d. a caller's scratch: every word read was written by the same call, nothing outside it is touched ------------------
GUARD = 256
SCRATCH_SHAPES = {
    "1100x129": ([(1100, 129)], (11, 3), [(1 / 100, 1 / 43)]),
    "mixed_batch": (BATCHES["10x10"][0], (10, 10), None),
    "288x288": ([(288, 288)], (9, 9), [(1 / 32, 1 / 32)]),
}


@pytest.mark.parametrize("name", list(SCRATCH_SHAPES))
def test_scratch_between_nan_guards(dev, name):
    sizes, out, scales = SCRATCH_SHAPES[name]
    scales = [(out[0] / h, out[1] / w) for h, w in sizes] if scales is None else scales
    B, C = len(sizes), 2
    x = padded_batch(sizes, C, dev, 43, fill=0.0)
    H, W = x.shape[2:]
    go = (torch.rand(B, C, *out, generator=torch.Generator().manual_seed(44)) * 2 - 1).to(dev)
    d = _cabi.make_resize(B, C, H, W, out[0], out[1], scales, sizes)
    words = int(_cabi.lib().gsasr_resize_scratch_bytes(ctypes.byref(d))) // 4
    assert words > 0
    for backward in (False, True):
        def run(scratch=None):
            if backward:
                return _cabi.imresize(torch.full((B, C, H, W), 3.0, device=dev), go, scales, sizes, backward=True, scratch=scratch)
            return _cabi.imresize(x, torch.full((B, C, *out), 3.0, device=dev), scales, sizes, scratch=scratch)

        want = run()
        buf = torch.full((words + 2 * GUARD,), float("nan"), device=dev)
        before = buf.view(torch.int32).clone()
        mid = buf[GUARD:GUARD + words]
        assert mid.is_contiguous() and mid.data_ptr() % 16 == 0
        got = run(mid)
        torch.cuda.synchronize()
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (name, backward)
        after = buf.view(torch.int32)
        assert torch.equal(after[:GUARD], before[:GUARD]) and torch.equal(after[GUARD + words:], before[GUARD + words:]), (name, backward)
        assert bool((before == before[0]).all()) and bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + words:]).all())
        for fill in ("zero", "seeded"):         # the scratch from the other kinds of garbage (tests/wsguard.py), the guards as they are
            mid.copy_(torch.from_numpy(wsguard.fill_bytes(fill, 4 * words, seed=7)).view(torch.float32))
            assert torch.equal(run(mid).view(torch.int32), want.view(torch.int32)), (name, backward, fill)
            assert torch.equal(after[:GUARD], before[:GUARD]) and torch.equal(after[GUARD + words:], before[GUARD + words:]), (name, backward, fill)
        with pytest.raises(RuntimeError, match="smaller than gsasr_resize_scratch_bytes"):
            run(buf[GUARD:GUARD + words - 1])


# ---- e. rejected lengths ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SMALL_BAD, ids=case_id)
def test_rejected_small_lengths(dev, case):
    n, m, s, _ = case
    with pytest.raises(ValueError):
        R.imresize_new(torch.rand(1, n, n, device=dev), s, s)
    x, out = torch.rand(1, 1, n, n, device=dev), torch.empty(1, 1, m, m, device=dev)
    with pytest.raises(RuntimeError, match="beyond one reflection"):
        _cabi.imresize(x, out, (s, s))
