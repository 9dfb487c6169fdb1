"""MATLAB-compatible bicubic imresize (gsasr_amd/resize.py; include/gsasr_splat.h: gsasr_resize) on the CPU: the package's torch
restatement against the reference's recorded outputs (tests/golden/imresize_*.npz, written by tests/golden/make_golden_imresize.py)
and against this file's own float64 restatement in NumPy (`taps_f64`, `dense_f64`, `resize_f64`: dense matrices, no code shared
with the package), the accepted input kinds, both size rules, every ValueError, and every GSASR_ERR_ARG of the C entry points.

Bars.  Each fixture records d_ref = max |reference - resize_f64| on its case: the reference's own float32 error.  A float32
subject is held to max(1e-6, 4 * d_ref) against resize_f64 (the factor covers another summation order of the taps: 7 to 66 on
the first nine cases, 130 to 402 on the three that stage more than one chunk, whose reference sums as many) and to that plus
d_ref against the fixture; a float64 subject to 1e-12 against resize_f64 (402 taps * 2 passes * 2^-53 * sum|w| 1.25 = 1.1e-13)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from gsasr_amd import _cabi
from gsasr_amd import resize as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")

# name -> the call: fn(img, *scales, antialiasing) on an input regenerated from `seed`; `kind`: "chw" torch tensor (c,h,w),
# "hw" NumPy array (h,w)
CASES = {
    "identity_48": dict(h=48, w=48, c=3, fn="imresize_new", scales=(1.0, 1.0), aa=True, kind="chw", out=(48, 48), seed=11),
    "53_to_48": dict(h=53, w=53, c=3, fn="imresize_new", scales=(48 / 53, 48 / 53), aa=True, kind="chw", out=(48, 48), seed=12),
    "97_to_48": dict(h=97, w=97, c=3, fn="imresize_new", scales=(48 / 97, 48 / 97), aa=True, kind="chw", out=(48, 48), seed=13),
    "131x67_by_2p7": dict(h=131, w=67, c=3, fn="imresize_new", scales=(1 / 2.7, 1 / 2.7), aa=True, kind="chw", out=(49, 25), seed=14),
    "416_to_26": dict(h=416, w=416, c=1, fn="imresize", scales=(1 / 16,), aa=True, kind="chw", out=(26, 26), seed=15),
    "20x31_up_ceil": dict(h=20, w=31, c=3, fn="imresize", scales=(2.5,), aa=True, kind="chw", out=(50, 78), seed=16),
    "20x31_up_round": dict(h=20, w=31, c=3, fn="imresize_new", scales=(2.5, 2.5), aa=True, kind="chw", out=(50, 78), seed=16),
    "97_to_48_no_aa": dict(h=97, w=97, c=3, fn="imresize_new", scales=(48 / 97, 48 / 97), aa=False, kind="chw", out=(48, 48), seed=13),
    "53_to_48_2d": dict(h=53, w=53, c=1, fn="imresize_new", scales=(48 / 53, 48 / 53), aa=True, kind="hw", out=(48, 48), seed=17),
    # more than one staged chunk of 256 taps per W-pass tile: p = 258, 130, (402, 174)
    "640_to_10": dict(h=640, w=640, c=1, fn="imresize", scales=(1 / 64,), aa=True, kind="chw", out=(10, 10), seed=18),
    "288_to_9": dict(h=288, w=288, c=1, fn="imresize_new", scales=(1 / 32, 1 / 32), aa=True, kind="chw", out=(9, 9), seed=19),
    "1100x129_by_100_43": dict(h=1100, w=129, c=1, fn="imresize_new", scales=(1 / 100, 1 / 43), aa=True, kind="chw", out=(11, 3), seed=20),
}


def case_input(case) -> np.ndarray:
    """the case's input as float32 NumPy: (c,h,w), or (h,w) for a 2-D case"""
    shape = (case["h"], case["w"]) if case["kind"] == "hw" else (case["c"], case["h"], case["w"])
    return np.random.default_rng(case["seed"]).random(shape, dtype=np.float32)


def case_scales(case):
    s = case["scales"]
    return (s[0], s[0]) if len(s) == 1 else s


# ---- this file's float64 restatement of the formulas (the issue's / the header's), in NumPy -----------------------------
def cubic_f64(x):
    a = np.abs(x)
    return np.where(a <= 1, 1.5 * a ** 3 - 2.5 * a ** 2 + 1, np.where(a <= 2, -0.5 * a ** 3 + 2.5 * a ** 2 - 4 * a + 2, 0.0))


def taps_f64(n, m, s, aa=True):
    """(0-based tap positions before reflection [m,p], normalised weights [m,p])"""
    shrink = s < 1 and aa
    kw = 4 / s if shrink else 4.0
    p = math.ceil(kw) + 2
    u = np.arange(1, m + 1, dtype=np.float64) / s + 0.5 * (1 - 1 / s)
    k = np.floor(u - kw / 2)[:, None] + np.arange(p)[None, :]
    w = s * cubic_f64((u[:, None] - k) * s) if shrink else cubic_f64(u[:, None] - k)
    return k.astype(np.int64) - 1, w / w.sum(1, keepdims=True)


def dense_f64(n, m, s, aa=True):
    """the axis' linear map as a dense [m,n] float64 matrix; ValueError where a non-zero tap lies beyond one reflection"""
    k, w = taps_f64(n, m, s, aa)
    r = np.where(k < 0, -1 - k, np.where(k >= n, 2 * n - 1 - k, k))
    bad = (r < 0) | (r >= n)
    if (bad & (w != 0)).any():
        raise ValueError("a tap with non-zero weight lies beyond one reflection")
    A = np.zeros((m, n))
    np.add.at(A, (np.repeat(np.arange(m), k.shape[1]), np.clip(r, 0, n - 1).ravel()), np.where(bad, 0.0, w).ravel())
    return A


def resize_f64(x, out_hw, scales, aa=True):
    """x `[..., h, w]` -> float64 `[..., out_h, out_w]`"""
    x = np.asarray(x, dtype=np.float64)
    Ah, Aw = dense_f64(x.shape[-2], out_hw[0], scales[0], aa), dense_f64(x.shape[-1], out_hw[1], scales[1], aa)
    return Ah @ x @ Aw.T


def adjoint_f64(g, in_hw, scales, aa=True):
    """g `[..., out_h, out_w]` -> A^T g, float64 `[..., h, w]`"""
    g = np.asarray(g, dtype=np.float64)
    Ah, Aw = dense_f64(in_hw[0], g.shape[-2], scales[0], aa), dense_f64(in_hw[1], g.shape[-1], scales[1], aa)
    return Ah.T @ g @ Aw


_FIX = {}


def fixture(name):
    """(reference output float32, d_ref) of a case; the recorded parameters are checked against CASES"""
    if name not in _FIX:
        z = np.load(os.path.join(GOLDEN, f"imresize_{name}.npz"))
        c = CASES[name]
        assert int(z["seed"]) == c["seed"] and tuple(z["in_hw"]) == (c["h"], c["w"]) and bool(z["antialiasing"]) == c["aa"]
        assert np.allclose(z["scales"], case_scales(c), rtol=0, atol=0) and str(z["fn"]) == c["fn"]
        _FIX[name] = (z["out"], float(z["ref_dist"]))
    return _FIX[name]


def bar_f64(d_ref):
    return max(1e-6, 4 * d_ref)


def run_case(case, x):
    fn = getattr(R, case["fn"])
    return fn(x, *case["scales"], antialiasing=case["aa"])


# ---- the fixtures and the restatements ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_cpu_path_against_fixture_and_f64(name):
    case = CASES[name]
    ref, d_ref = fixture(name)
    x = case_input(case)
    want = resize_f64(x, case["out"], case_scales(case), case["aa"])
    # what the generator recorded is what this file computes now
    assert abs(np.abs(ref - want).max() - d_ref) <= 1e-12 and d_ref <= 2e-5
    got = run_case(case, x if case["kind"] == "hw" else torch.from_numpy(x))
    got = got if case["kind"] == "hw" else got.numpy()
    assert got.dtype == np.float32 and got.shape == ref.shape == want.shape
    e64, eref = np.abs(got - want).max(), np.abs(got - ref).max()
    print(f"{name}: |cpu - f64| {e64:.3e} (bar {bar_f64(d_ref):.3e}), |cpu - reference| {eref:.3e}, reference's own {d_ref:.3e}")
    assert e64 <= bar_f64(d_ref) and eref <= bar_f64(d_ref) + d_ref
    got64 = run_case(case, torch.from_numpy(x.astype(np.float64) if case["kind"] == "chw" else x.astype(np.float64)[None]))
    assert got64.dtype == torch.float64 and np.abs(got64.numpy().reshape(want.shape) - want).max() <= 1e-12


def test_identity_is_exact():
    x = case_input(CASES["identity_48"])
    assert np.array_equal(R.imresize_new(torch.from_numpy(x), 1.0, 1.0).numpy(), x)
    assert np.array_equal(fixture("identity_48")[0], x)


def test_fixtures_are_small_and_hold_numbers_only():
    for name in CASES:
        path = os.path.join(GOLDEN, f"imresize_{name}.npz")
        assert os.path.getsize(path) < 256 * 1024
        z = np.load(path, allow_pickle=False)
        assert set(z.files) == {"fn", "seed", "in_hw", "channels", "scales", "antialiasing", "out", "ref_dist"}


def test_length_26_at_one_sixteenth_raises_as_the_reference_does():
    with pytest.raises(ValueError, match="beyond one reflection"):
        R.imresize(torch.rand(1, 26, 26), 1 / 16)
    with pytest.raises(ValueError, match="beyond one reflection"):
        R.imresize(np.random.rand(416, 26).astype(np.float32), 1 / 16)
    with pytest.raises(ValueError):
        dense_f64(26, 2, 1 / 16)
    dense_f64(416, 26, 1 / 16)        # 25 deep, inside one reflection
    # package and restatement draw the line at the same lengths, and both outcomes occur
    seen = set()
    for n in range(20, 72):
        seen.add(_ok(n))
        if _ok(n):
            R.axis_taps(n, math.ceil(n / 16), 1 / 16)
        else:
            with pytest.raises(ValueError):
                R.axis_taps(n, math.ceil(n / 16), 1 / 16)
    assert seen == {True, False}


def _ok(n):
    try:
        dense_f64(n, math.ceil(n / 16), 1 / 16)
        return True
    except ValueError:
        return False


def test_nonzero_taps_lie_inside_the_window():
    """non-zero taps are in [left + 1, left + p - 2]: a floor that is off by one changes nothing"""
    for n, m, s, aa in ((53, 48, 48 / 53, True), (416, 26, 1 / 16, True), (20, 50, 2.5, True), (97, 48, 48 / 97, False), (131, 49, 1 / 2.7, True)):
        _, w = taps_f64(n, m, s, aa)
        assert (w[:, 0] == 0).all() and (w[:, -1] == 0).all() and np.abs(w.sum(1) - 1).max() < 1e-15
        assert np.abs(w).sum(1).max() <= 1.27        # (1.267 without antialiasing at 48 / 97; 1.25 is the antialiased kernel's)


def test_axis_taps_agree_with_the_dense_matrix():
    for n, m, s, aa in ((53, 48, 48 / 53, True), (416, 26, 1 / 16, True), (31, 78, 2.5, True), (97, 48, 48 / 97, False)):
        idx, w = R.axis_taps(n, m, s, aa)
        A = np.zeros((m, n))
        np.add.at(A, (np.repeat(np.arange(m), idx.shape[1]), idx.numpy().ravel()), w.numpy().ravel())
        assert np.abs(A - dense_f64(n, m, s, aa)).max() <= 1e-15


# ---- input kinds and size rules ----------------------------------------------------------------------------------------
def test_numpy_and_tensor_kinds():
    rng = np.random.default_rng(3)
    hwc = rng.random((21, 30, 3), dtype=np.float32)
    chw = torch.from_numpy(np.ascontiguousarray(hwc.transpose(2, 0, 1)))
    a = R.imresize(hwc, 0.5)
    b = R.imresize(chw, 0.5)
    assert isinstance(a, np.ndarray) and a.shape == (11, 15, 3) and a.dtype == np.float32
    assert torch.is_tensor(b) and tuple(b.shape) == (3, 11, 15) and np.array_equal(a.transpose(2, 0, 1), b.numpy())
    g = R.imresize(hwc[:, :, 1], 0.5)
    t = R.imresize(chw[1], 0.5)
    assert isinstance(g, np.ndarray) and g.shape == (11, 15) and np.array_equal(g, a[:, :, 1])
    assert torch.is_tensor(t) and tuple(t.shape) == (11, 15) and np.array_equal(t.numpy(), g)
    assert R.imresize(hwc.astype(np.float64), 0.5).dtype == np.float32       # (the reference's `.float()`)
    assert R.imresize(torch.from_numpy(hwc[:, :, 0]).to(torch.uint8), 0.5).dtype == torch.float32


def test_size_rules():
    x = torch.rand(1, 20, 31)
    assert tuple(R.imresize(x, 2.5).shape) == (1, 50, 78) and tuple(R.imresize_new(x, 2.5, 2.5).shape) == (1, 50, 78)
    y = torch.rand(1, 21, 31)       # 52.5 and 77.5: ceil -> 53, 78; Python's round -> 52 (to even), 78
    assert tuple(R.imresize(y, 2.5).shape) == (1, 53, 78) and tuple(R.imresize_new(y, 2.5, 2.5).shape) == (1, 52, 78)
    z = torch.rand(1, 10, 10)       # 3.3: ceil -> 4, round -> 3
    assert tuple(R.imresize(z, 0.33).shape) == (1, 4, 4) and tuple(R.imresize_new(z, 0.33, 0.33).shape) == (1, 3, 3)
    assert tuple(R.imresize_new(z, 0.5, 2.0).shape) == (1, 5, 20)


def test_batch_on_the_cpu_equals_the_single_calls_and_differentiates():
    g = torch.Generator().manual_seed(2)
    sizes = [(24, 24), (27, 26), (31, 31)]
    x = torch.full((3, 2, 31, 31), float("nan"), dtype=torch.float64)
    for b, (h, w) in enumerate(sizes):
        x[b, :, :h, :w] = torch.rand(2, h, w, generator=g, dtype=torch.float64)
    x.requires_grad_(True)
    y = R.imresize_batch(x, sizes, out_size=(12, 12))
    assert tuple(y.shape) == (3, 2, 12, 12) and bool(torch.isfinite(y).all())
    for b, (h, w) in enumerate(sizes):
        assert torch.equal(y[b].detach(), R.imresize_new(x[b, :, :h, :w].detach(), 12 / h, 12 / w))
    go = torch.rand(3, 2, 12, 12, generator=g, dtype=torch.float64)
    gx, = torch.autograd.grad(y, x, go)
    for b, (h, w) in enumerate(sizes):
        want = adjoint_f64(go[b].numpy(), (h, w), (12 / h, 12 / w))
        assert np.abs(gx[b, :, :h, :w].numpy() - want).max() <= 1e-12
        assert float(gx[b, :, h:, :].abs().sum()) == 0 and float(gx[b, :, :, w:].abs().sum()) == 0
    # scales instead of out_size, one number for all
    assert torch.equal(R.imresize_batch(x.detach()[:1, :, :24, :24], scales=0.5), y[:1].detach())


def test_value_errors():
    x = torch.rand(2, 3, 24, 24)
    bad = [
        lambda: R.imresize([[1.0]], 0.5),
        lambda: R.imresize(torch.rand(2, 3, 8, 8), 0.5),
        lambda: R.imresize(np.zeros((2, 3, 8, 8), np.float32), 0.5),
        lambda: R.imresize(torch.rand(3, 8, 8), 0.0),
        lambda: R.imresize(torch.rand(3, 8, 8), -1.0),
        lambda: R.imresize(torch.rand(3, 8, 8), float("nan")),
        lambda: R.imresize_new(torch.rand(3, 8, 8), 0.01, 0.01),          # round(0.08) = 0: no pixel
        lambda: R.imresize(torch.rand(3, 0, 8), 0.5),
        lambda: R.imresize_batch(x),                                      # neither scales nor out_size
        lambda: R.imresize_batch(x[0], out_size=(12, 12)),
        lambda: R.imresize_batch(x.long(), out_size=(12, 12)),
        lambda: R.imresize_batch(x, [(24, 24)], out_size=(12, 12)),       # one size for two samples
        lambda: R.imresize_batch(x, [(24, 24), (25, 24)], out_size=(12, 12)),
        lambda: R.imresize_batch(x, [(24, 24), (0, 24)], out_size=(12, 12)),
        lambda: R.imresize_batch(x, out_size=(0, 12)),
        lambda: R.imresize_batch(x, [(24, 24), (20, 24)], scales=0.5),    # 12 and 10 rows
        lambda: R.imresize_batch(x, scales=[0.5, 0.5, 0.5]),
        lambda: R.imresize_batch(x, scales=0.5, out_size=(13, 12)),
        lambda: R.imresize_batch(x, scales=0.001),
        lambda: R.imresize_batch(torch.rand(1, 1, 26, 26), out_size=(2, 2), scales=1 / 16),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"call {i} raised nothing")


def test_package_exports():
    import gsasr_amd
    assert gsasr_amd.imresize is R.imresize and gsasr_amd.imresize_new is R.imresize_new and gsasr_amd.imresize_batch is R.imresize_batch


# ---- the C ABI ------------------------------------------------------------------------------------------------------------
RESIZE_SYMBOLS = ("gsasr_resize_scratch_bytes", "gsasr_imresize", "gsasr_imresize_backward")
HOST = (ctypes.c_double * 64)()
PTR = ctypes.cast(HOST, ctypes.c_void_p).value      # a host stand-in for every device pointer: never dereferenced


def test_header_bindings_and_library_agree_on_the_resize_entry_points():
    hdr = open(os.path.join(ROOT, "include", "gsasr_splat.h")).read()
    assert re.search(r"typedef struct gsasr_resize \{[^}]*int batch, channels;[^}]*int in_h, in_w;[^}]*const int \*sample_hw;[^}]*"
                     r"const double \*scales;[^}]*int out_h, out_w;[^}]*const float \*in;[^}]*size_t in_pitch, in_plane, in_stride;[^}]*"
                     r"float \*out;[^}]*size_t out_pitch, out_plane, out_stride;[^}]*unsigned flags;[^}]*void \*scratch;[^}]*\} gsasr_resize;", hdr)
    for name, value in (("NO_ANTIALIAS", 1), ("ACCUMULATE", 2), ("SHARED_SCALE", 4)):
        assert re.search(rf"#define GSASR_RESIZE_{name} {value}u\b", hdr) and getattr(_cabi, "RESIZE_" + name) == value
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(gsasr_[a-z_0-9]+)\s*\(", code))
    L = ctypes.CDLL(_cabi.LIB_PATH)
    for name in RESIZE_SYMBOLS:
        assert name in declared and name in _cabi.EXPORTS and hasattr(L, name), name
    assert declared == set(_cabi.EXPORTS), declared ^ set(_cabi.EXPORTS)
    # additive: the version and every existing struct stay
    assert _cabi.lib().gsasr_abi_version() == 7 and "#define GSASR_SPLAT_ABI_VERSION 7" in hdr
    assert ctypes.sizeof(_cabi.Dims) == 64 and ctypes.sizeof(_cabi.Ssim) == 80 and ctypes.sizeof(_cabi.Metrics) == 96
    assert ctypes.sizeof(_cabi.Resize) == 120
    for words in ("mirrored once", "left untouched", "ceil(kw) + 2", "HOST array", "GSASR_RESIZE_SHARED_SCALE [2]", "rows (H) first"):
        assert words in hdr, words
    from gsasr_amd import build
    assert "splat_resize" in build.PARTS
    assert '#include "splat_resize.hip"' in open(os.path.join(ROOT, "gsasr_amd", "csrc", "gsasr_splat.hip")).read()


def descriptor(batch=1, channels=3, in_h=53, in_w=53, out_h=48, out_w=48, scales=(48 / 53, 48 / 53), sizes=None, flags=0, **kw):
    d = _cabi.make_resize(batch, channels, in_h, in_w, out_h, out_w, scales, sizes, flags)
    f = dict(inp=PTR, out=PTR, scratch=PTR)
    f.update(kw)
    for k, v in f.items():
        setattr(d, k, v)
    return d


def _null_scales():
    d = descriptor()
    d.scales = None
    return d


BAD = {
    "null in": lambda: descriptor(inp=None),
    "null out": lambda: descriptor(out=None),
    "null scratch": lambda: descriptor(scratch=None),
    "null scales": _null_scales,
    "batch 0": lambda: descriptor(batch=0),
    "batch 65": lambda: descriptor(batch=65),
    "channels 0": lambda: descriptor(channels=0),
    "in_h 0": lambda: descriptor(in_h=0),
    "in_w 32768": lambda: descriptor(in_w=32768, scales=(48 / 53, 48 / 32768)),
    "out_h 0": lambda: descriptor(out_h=0),
    "out_w 32768": lambda: descriptor(out_w=32768, scales=(48 / 53, 32768 / 53)),
    "sample taller than its slot": lambda: descriptor(sizes=[(54, 53)]),
    "sample wider than its slot": lambda: descriptor(sizes=[(53, 54)]),
    "sample without a pixel": lambda: descriptor(sizes=[(0, 53)]),
    "in pitch below the row": lambda: descriptor(in_pitch=4 * 53 - 4),
    "out pitch below the row": lambda: descriptor(out_pitch=4 * 48 - 4),
    "pitch no multiple of 4": lambda: descriptor(in_pitch=4 * 53 + 2),
    "misaligned scratch": lambda: descriptor(scratch=PTR + 4),
    "misaligned in": lambda: descriptor(inp=PTR + 2),
    "scale 0": lambda: descriptor(scales=(0.0, 48 / 53)),
    "negative scale": lambda: descriptor(scales=(48 / 53, -1.0)),
    "nan scale": lambda: descriptor(scales=(float("nan"), 48 / 53)),
    "infinite scale": lambda: descriptor(scales=(float("inf"), 48 / 53)),
    "unknown flag": lambda: descriptor(flags=8),
    "26 pixels at 1/16 (rows)": lambda: descriptor(in_h=26, in_w=416, out_h=2, out_w=26, scales=(1 / 16, 1 / 16)),
    "26 pixels at 1/16 (columns of one sample)": lambda: descriptor(batch=2, in_h=416, in_w=416, out_h=26, out_w=26, scales=(1 / 16, 1 / 16),
                                                                  sizes=[(416, 416), (416, 26)]),
    "scale 1e-9": lambda: descriptor(scales=(1e-9, 48 / 53)),
}


@pytest.mark.parametrize("what", list(BAD))
def test_argument_errors_before_anything_is_enqueued(what):
    L = _cabi.lib()
    d = BAD[what]()
    for fn in (L.gsasr_imresize, L.gsasr_imresize_backward):
        assert fn(ctypes.byref(d), None) == -1, what
        assert len(L.gsasr_last_error()) > 0
    if what not in ("null in", "null out", "null scratch", "misaligned scratch", "misaligned in"):      # (not looked at by the size query)
        assert L.gsasr_resize_scratch_bytes(ctypes.byref(d)) == 0, what


def test_null_descriptor_and_accumulate_in_the_forward():
    L = _cabi.lib()
    assert L.gsasr_imresize(None, None) == -1 and L.gsasr_imresize_backward(None, None) == -1 and L.gsasr_resize_scratch_bytes(None) == 0
    assert L.gsasr_imresize(ctypes.byref(descriptor(flags=_cabi.RESIZE_ACCUMULATE)), None) == -1
    assert b"ACCUMULATE" in L.gsasr_last_error()


def test_scratch_bytes_of_good_descriptors():
    L = _cabi.lib()
    n = L.gsasr_resize_scratch_bytes(ctypes.byref(descriptor()))
    # at least the intermediate [3, 48, 53] and the two weight tables of 48 outputs * 7 taps
    assert n >= 4 * (3 * 48 * 53 + 2 * 48 * 7) and n % 16 == 0
    big = L.gsasr_resize_scratch_bytes(ctypes.byref(descriptor(batch=2, in_h=416, in_w=416, out_h=26, out_w=26, scales=(1 / 16, 1 / 16))))
    assert big >= 4 * (2 * 3 * 26 * 416 + 2 * 2 * 26 * 66)
    per = L.gsasr_resize_scratch_bytes(ctypes.byref(descriptor(batch=2, scales=[(48 / 53, 48 / 53), (1.0, 1.0)], sizes=[(53, 53), (48, 48)])))
    assert per > 0
    # the pointers are not looked at
    assert L.gsasr_resize_scratch_bytes(ctypes.byref(descriptor(inp=None, out=None, scratch=None))) == n
