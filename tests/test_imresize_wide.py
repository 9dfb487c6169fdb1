"""The axis cases of tests/test_imresize_wide_gpu.py, and proof on the CPU that they reach what they claim: windows staged in
more than one chunk of RZ_SPAN taps, every W-pass tile width 8..64 with a ragged last tile, more than 256 taps, windows wider
than the image (p > n, both reflections inside one window) and the lengths 1..8.

Each case is one axis, (n inputs, m outputs, scale, antialias).  The library exposes no choice of tile width or chunking, so this
file restates the rule of csrc/splat_resize.hip (`resize_geometry_check`, `k_resize_cols`) from the constants it reads out of
that file with a regular expression -- a changed constant fails `test_the_list_reaches_its_paths`, it does not silently empty it
-- and pins what the rule gives on every case in EXPECT.  Only outputs are compared with the library: where 1/s is odd,
u - kw/2 is an integer, a fused multiply-add may put the device's `floor` one lower, and p = ceil(kw) + 2 exists so that this
changes nothing.

The entry bar (`entry_bar`).  A resize at scale exactly 1 is exact (weights 0 and 1), so resizing the identity matrix along one
axis writes out that axis' matrix.  Entry (i, j) is the sum of the at most three float32-rounded weights whose taps fold onto
input j (directly, reflected at the near end, reflected at the far end), added by fma: one rounding per weight and at most two
for the additions, 3 * 2^-24 * S_ij with S_ij the sum of the |weights| folding there.  One more for a double rounding where the
float64 weight of another implementation of the same formula differs in its last bits from NumPy's: 4 * 2^-24 * S_ij + 1e-12
(the additive term: the cubic's cancellation next to its zeros, a few 1e-16 absolute in float64).  Where no tap folds onto
(i, j), S_ij = 0 and the entry must be exactly 0.  `test_cpu_path_meets_the_entry_bar` shows the bar is reachable: the
package's float32 torch path meets it on every case."""
import functools
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
from test_imresize import dense_f64, taps_f64      # noqa: E402

from gsasr_amd import resize as R      # noqa: E402

# (n inputs, m outputs, scale, antialias)
AXIS_CASES = [
    (128, 2, 1 / 64, True),         # p = 258 > n: both reflections in one window, p >= 256
    (640, 10, 1 / 64, True),        # p = 258, two tiles (8 + 2), three and two chunks
    (1100, 11, 1 / 100, True),      # p = 402, five chunks; 1100 rows = 34 * 32 + 12
    (288, 9, 1 / 32, True),         # two chunks with p < 256; a last tile of one column
    (129, 3, 1 / 43, True),         # span 260: a second chunk of 4 taps
    (200, 20, 1 / 10, True),        # tile width 16
    (232, 29, 1 / 8, True),         # 24
    (222, 37, 1 / 6, True),         # 32
    (225, 45, 1 / 5, True),         # 40; u - kw/2 is an exact integer (odd 1/s)
    (252, 56, 1 / 4.5, True),       # 48
    (244, 61, 1 / 4, True),         # 56
    (97, 14, 1 / 7, True),          # odd 1/s again
    (31, 78, 2.5, True),            # upscale, tile width 64 (64 + 14)
    (97, 24, 1 / 4, False),         # `shrink` false at s < 1
]
SMALL_SCALES = (1.0, 2.5, 4.0, 0.5, 1 / 3, 0.75)
SMALL_PAIRS = [(n, max(1, round(n * s)), s, True) for n in range(1, 9) for s in SMALL_SCALES]


def _accepted(case):
    try:
        dense_f64(*case)
        return True
    except ValueError:
        return False


SMALL_OK = [c for c in SMALL_PAIRS if _accepted(c)]
SMALL_BAD = [c for c in SMALL_PAIRS if not _accepted(c)]
ALL_OK = AXIS_CASES + SMALL_OK


def case_id(case):
    n, m, s, aa = case
    return f"{n}to{m}_s{s:.4g}" + ("" if aa else "_noaa")


# what the kernel's rule gives when the case is the W axis and the H axis runs at scale 1 (p = 6):
# (p, tile width, columns of each tile, chunks of each tile)
EXPECT = {
    (128, 2): (258, 8, [2], [2]),
    (640, 10): (258, 8, [8, 2], [3, 2]),
    (1100, 11): (402, 8, [8, 3], [5, 3]),
    (288, 9): (130, 8, [8, 1], [2, 1]),
    (129, 3): (174, 8, [3], [2]),
    (200, 20): (42, 16, [16, 4], [1, 1]),
    (232, 29): (34, 24, [24, 5], [1, 1]),
    (222, 37): (26, 32, [32, 5], [1, 1]),
    (225, 45): (22, 40, [40, 5], [1, 1]),
    (252, 56): (20, 48, [48, 8], [1, 1]),
    (244, 61): (18, 56, [56, 5], [1, 1]),
    (97, 14): (30, 32, [14], [1]),            # floor(226 / 7) + 1 = 33 -> 32
    (31, 78): (6, 64, [64, 14], [1, 1]),
    (97, 24): (6, 56, [24], [1]),             # no antialiasing: p = 6, floor(250 / 4) + 1 = 63 -> 56
}


# ---- the rule of csrc/splat_resize.hip, restated ---------------------------------------------------------------------------
def kernel_constants():
    src = open(os.path.join(ROOT, "gsasr_amd", "csrc", "splat_resize.hip")).read()
    got = {}
    for name in ("RZ_SPAN", "RZ_TOX_MAX", "RZ_ROWS"):
        m = re.findall(rf"constexpr\s+int\s+{name}\s*=\s*(\d+)\s*;", src)
        assert len(m) == 1, f"{name} is not defined exactly once as an integer literal in splat_resize.hip"
        got[name] = int(m[0])
    return got


def taps_per_output(s, aa):
    return math.ceil(4 / s if (s < 1 and aa) else 4.0) + 2


def tile_width(pw, smin, K):
    """`resize_geometry_check`: the widest tile whose taps fit one staged chunk, a multiple of 8 in 8 .. RZ_TOX_MAX"""
    fit = math.floor((K["RZ_SPAN"] - pw) * smin) + 1.0 if pw < K["RZ_SPAN"] else 8.0
    return K["RZ_TOX_MAX"] if fit >= K["RZ_TOX_MAX"] else 8 if fit < 8.0 else int(fit) // 8 * 8


def tiling(case, K, pw=None, smin=None):
    """(tile width, [columns per tile], [chunks per tile], [staged span per tile]) of the case as the W axis of `k_resize_cols`"""
    n, m, s, aa = case
    p = taps_per_output(s, aa)
    tox = tile_width(max(p, 6) if pw is None else pw, s if smin is None else smin, K)
    left = taps_f64(n, m, s, aa)[0][:, 0]
    cols, chunks, spans = [], [], []
    for ox0 in range(0, m, tox):
        nx = min(tox, m - ox0)
        span = int(left[ox0 + nx - 1] + p - left[ox0])
        cols.append(nx)
        spans.append(span)
        chunks.append(-(-span // K["RZ_SPAN"]))
    return tox, cols, chunks, spans


# ---- float64 matrices, computed once and shared (read-only) -------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def matrices(case):
    """(A, S): the axis' dense [m,n] float64 matrix (`dense_f64`) and the same built from |w|, the absolute sum of the taps that
    fold onto (i, j)"""
    n, m, s, aa = case
    A = dense_f64(n, m, s, aa)
    k, w = taps_f64(n, m, s, aa)
    r = np.where(k < 0, -1 - k, np.where(k >= n, 2 * n - 1 - k, k))
    inside = (r >= 0) & (r < n)
    S = np.zeros((m, n))
    np.add.at(S, (np.repeat(np.arange(m), k.shape[1]), np.clip(r, 0, n - 1).ravel()), np.where(inside, np.abs(w), 0.0).ravel())
    A.setflags(write=False)
    S.setflags(write=False)
    return A, S


def entry_bar(S):
    return 4 * 2.0 ** -24 * S + 1e-12


def check_entries(got, case, transposed=False):
    """`got`: float32 [m,n] (or [n,m] when `transposed`) against the case's matrix, entry by entry.  Returns the worst ratio of
    an error to its bar; asserts the bar and exact zeros where no tap folds."""
    A, S = matrices(case)
    got = np.asarray(got, dtype=np.float64)
    got = got.T if transposed else got
    assert got.shape == A.shape, (got.shape, A.shape)
    ratio = float((np.abs(got - A) / entry_bar(S)).max())
    stray = int(np.count_nonzero(got[S == 0]))
    assert stray == 0, f"{case_id(case)}: {stray} entries onto which no tap folds are not exactly 0"
    assert ratio <= 1.0, f"{case_id(case)}: worst entry at {ratio:.3f} of its bar"
    return ratio


# ---- the tests -------------------------------------------------------------------------------------------------------------
def test_the_list_reaches_its_paths():
    K = kernel_constants()
    assert K == {"RZ_SPAN": 256, "RZ_TOX_MAX": 64, "RZ_ROWS": 32}, K
    assert len({c[:2] for c in AXIS_CASES}) == len(AXIS_CASES) == len(EXPECT)
    widths, chunk_counts, all_spans, ragged = set(), set(), [], set()
    for case in AXIS_CASES:
        n, m, s, aa = case
        p = taps_per_output(s, aa)
        tox, cols, chunks, spans = tiling(case, K)
        assert (p, tox, cols, chunks) == EXPECT[(n, m)], (case_id(case), p, tox, cols, chunks)
        widths.add(tox)
        chunk_counts.update(chunks)
        all_spans += spans
        ragged.add(cols[-1])
    assert widths == {8, 16, 24, 32, 40, 48, 56, 64}, widths
    assert {1, 2, 3, 5} <= chunk_counts, chunk_counts
    assert any(K["RZ_SPAN"] < sp <= K["RZ_SPAN"] + 8 for sp in all_spans), all_spans          # a second chunk of a few taps
    assert any(taps_per_output(s, aa) > n for n, _, s, aa in AXIS_CASES)                      # both reflections in one window
    assert any(taps_per_output(s, aa) >= K["RZ_SPAN"] for _, _, s, aa in AXIS_CASES)
    assert 1 in ragged and any(c % 8 for c in ragged)
    assert any(_window_starts_on_an_integer(c) for c in AXIS_CASES)
    # the W-pass test feeds an n x n identity: n rows through tiles of RZ_ROWS
    assert any(n % K["RZ_ROWS"] for n, _, _, _ in AXIS_CASES) and any(n > K["RZ_ROWS"] and n % K["RZ_ROWS"] for n, _, _, _ in AXIS_CASES)
    assert (1100 % K["RZ_ROWS"], 1100 // K["RZ_ROWS"]) == (12, 34)
    # the mixed batch of the GPU file: alone, 100 x 80 -> 10 x 10 takes a wider tile and one chunk; behind a 640-pixel sample
    # at 1/64 the table pitch is 258, the tile 8
    alone = tiling((80, 10, 10 / 80, True), K, pw=max(taps_per_output(0.1, True), taps_per_output(0.125, True)), smin=0.125)
    mixed = tiling((80, 10, 10 / 80, True), K, pw=258, smin=1 / 64)
    assert alone[0] > 8 and alone[2] == [1] and mixed[0] == 8 and mixed[1] == [8, 2]


def _window_starts_on_an_integer(case):
    n, m, s, aa = case
    kw = 4 / s if (s < 1 and aa) else 4.0
    u = np.arange(1, m + 1, dtype=np.float64) / s + 0.5 * (1 - 1 / s)
    return bool((u - kw / 2 == np.floor(u - kw / 2)).all())


def test_small_lengths_split_as_counted():
    assert len(SMALL_PAIRS) == 48 and len(SMALL_OK) == 38 and len(SMALL_BAD) == 10
    assert any(taps_per_output(s, aa) > n for n, _, s, aa in SMALL_OK)
    for case in SMALL_BAD:
        with pytest.raises(ValueError):
            R.axis_taps(*case)


def test_the_library_draws_the_line_at_the_same_pairs():
    """the host check of gsasr_resize_scratch_bytes (no device needed): 0 and "beyond one reflection" on the rejected pairs, a
    size on every accepted case"""
    import ctypes

    from gsasr_amd import _cabi
    L = _cabi.lib()
    for n, m, s, aa in SMALL_BAD:
        assert L.gsasr_resize_scratch_bytes(ctypes.byref(_cabi.make_resize(1, 1, n, n, m, m, (s, s)))) == 0, (n, m, s)
        assert b"beyond one reflection" in L.gsasr_last_error()
    for n, m, s, aa in ALL_OK:
        flags = 0 if aa else _cabi.RESIZE_NO_ANTIALIAS
        assert L.gsasr_resize_scratch_bytes(ctypes.byref(_cabi.make_resize(1, 1, n, n, m, m, (s, s), None, flags))) > 0, (n, m, s)


@pytest.mark.parametrize("case", ALL_OK, ids=case_id)
def test_axis_taps_agree_with_the_dense_matrix(case):
    n, m, s, aa = case
    idx, w = R.axis_taps(n, m, s, aa)
    A = np.zeros((m, n))
    np.add.at(A, (np.repeat(np.arange(m), idx.shape[1]), idx.numpy().ravel()), w.numpy().ravel())
    D, S = matrices(case)
    assert np.abs(A - D).max() <= 1e-15
    # |A| <= S entry by entry, with equality where nothing cancels; every row of A sums to 1
    assert (np.abs(D) <= S + 1e-18).all() and np.abs(D.sum(1) - 1).max() <= 1e-14


@pytest.mark.parametrize("case", ALL_OK, ids=case_id)
def test_cpu_path_meets_the_entry_bar(case):
    """`R.resize_torch` in float32 on the identity: along W it writes A^T, along H it writes A"""
    n, m, s, aa = case
    eye = torch.eye(n, dtype=torch.float32)
    along_w = R.resize_torch(eye, (n, m), (1.0, s), aa).numpy()        # [n, m] = A^T
    along_h = R.resize_torch(eye, (m, n), (s, 1.0), aa).numpy()        # [m, n] = A
    assert along_w.dtype == np.float32 and along_h.dtype == np.float32
    rw = check_entries(along_w, case, transposed=True)
    rh = check_entries(along_h, case)
    print(f"{case_id(case)}: cpu float32 worst entry / bar: W pass {rw:.3f}, H pass {rh:.3f}")
