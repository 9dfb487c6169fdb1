"""Training batches from decoded images (gsasr_amd/data.py; include/gsasr_splat.h: gsasr_batch) on the CPU: the package's torch
path against the reference's recorded batches (tests/golden/batch_*.npz, written by tests/golden/make_golden_batch.py from the
reference's dataset code: float crop, imresize_new, augment, img2tensor, F.pad), `draw_batch` against a restatement of the
dataset's draws on the same `random.Random`, every ValueError, and the header.

Bars.  `gt` is data movement and one correctly rounded division: exactly equal.  `lq` within 1e-6 absolute of the reference's,
the bar tests/test_imresize.py holds `resize_torch` to on its small cases (these have at most 22 taps a pass)."""
import ctypes
import math
import os
import random
import re

import numpy as np
import pytest
import torch

from gsasr_amd import _cabi
from gsasr_amd import data as D
from gsasr_amd.resize import axis_taps

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")

ALL8 = [(h, v, r) for r in (0, 1) for v in (0, 1) for h in (0, 1)]       # (hflip, vflip, rot90)
# name -> one source image regenerated from `seed` (uint8 [h,w,3], BGR), the samples cut from it, lr_size and gt_pad
CASES = {
    "d4_29": dict(hw=(37, 41), seed=21, crops=[(5, 7, 29, 29)] * 8, flags=ALL8, lr=(6, 6), pad=None),
    "last_row_col": dict(hw=(37, 41), seed=22, crops=[(8, 12, 29, 29)], flags=[(1, 0, 1)], lr=(6, 6), pad=None),
    "13": dict(hw=(20, 23), seed=23, crops=[(3, 4, 13, 13)], flags=[(0, 1, 0)], lr=(6, 6), pad=None),
    "rect_12x20": dict(hw=(30, 33), seed=24, crops=[(2, 5, 12, 20)] * 4, flags=[(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0)], lr=(3, 5), pad=None),
    "pad_31": dict(hw=(37, 41), seed=25, crops=[(0, 0, 13, 13), (4, 9, 21, 21), (8, 12, 29, 29)], flags=[(0, 0, 0), (1, 1, 1), (0, 1, 1)],
                   lr=(6, 6), pad=(31, 31)),
}


def case_source(case) -> np.ndarray:
    return np.random.default_rng(case["seed"]).integers(0, 256, case["hw"] + (3,), dtype=np.uint8)


def case_pad(case):
    return case["pad"] or (max(c[2] for c in case["crops"]), max(c[3] for c in case["crops"]))


def run_case(case, src: torch.Tensor, **kw):
    """make_batch on a case, `src` on either device"""
    f = case["flags"]
    return D.make_batch([src] * len(f), case["crops"], case["lr"], [a[0] for a in f], [a[1] for a in f], [a[2] for a in f],
                        gt_pad=case["pad"], **kw)


_FIX = {}


def fixture(name):
    """(source uint8, reference gt, reference lq) of a case; the recorded parameters are checked against CASES"""
    if name not in _FIX:
        z = np.load(os.path.join(GOLDEN, f"batch_{name}.npz"), allow_pickle=False)
        c = CASES[name]
        assert set(z.files) == {"src", "crops", "flags", "lr", "gt_pad", "gt", "lq"}
        assert np.array_equal(z["src"], case_source(c)) and z["crops"].tolist() == [list(v) for v in c["crops"]]
        assert z["flags"].tolist() == [list(v) for v in c["flags"]] and tuple(z["lr"]) == c["lr"] and tuple(z["gt_pad"]) == case_pad(c)
        _FIX[name] = (z["src"], z["gt"], z["lq"])
    return _FIX[name]


# ---- the fixtures ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_cpu_path_against_the_reference(name):
    case = CASES[name]
    src, gt, lq = fixture(name)
    B = len(case["crops"])
    Gh, Gw = case_pad(case)
    out = run_case(case, torch.from_numpy(src))
    assert set(out) == {"gt", "lq", "gt_size", "scale_modify", "pad_h", "pad_w"}
    assert out["gt"].dtype == torch.float32 and tuple(out["gt"].shape) == (B, 3, Gh, Gw) == gt.shape
    assert out["lq"].dtype == torch.float32 and tuple(out["lq"].shape) == (B, 3) + case["lr"] == lq.shape
    assert np.array_equal(out["gt"].numpy(), gt)
    e = np.abs(out["lq"].numpy() - lq).max()
    print(f"{name}: gt equal, |lq - reference| {e:.3e} (bar 1e-6)")
    assert e <= 1e-6
    assert out["gt_size"].dtype == torch.int64 and out["gt_size"].tolist() == [[c[2], c[3]] for c in case["crops"]]
    assert out["scale_modify"].dtype == torch.float32
    assert torch.equal(out["scale_modify"], torch.tensor([[c[2] / case["lr"][0], c[3] / case["lr"][1]] for c in case["crops"]]))
    assert out["pad_h"].tolist() == [Gh - c[2] for c in case["crops"]] and out["pad_w"].tolist() == [Gw - c[3] for c in case["crops"]]
    for b, c in enumerate(case["crops"]):       # (square where transposed: the extent is the crop's)
        assert not out["gt"][b, :, c[2]:].any() and not out["gt"][b, :, :, c[3]:].any()


def test_the_fixtures_cover_the_cases_of_the_issue():
    assert sorted(CASES["d4_29"]["flags"]) == sorted({(h, v, r) for h in (0, 1) for v in (0, 1) for r in (0, 1)}) and len(ALL8) == 8
    c = CASES["last_row_col"]
    assert c["crops"][0][0] + c["crops"][0][2] == c["hw"][0] and c["crops"][0][1] + c["crops"][0][3] == c["hw"][1]
    assert CASES["13"]["crops"][0][2:] == (13, 13) and CASES["rect_12x20"]["lr"] == (3, 5)
    assert all(f[2] == 0 for f in CASES["rect_12x20"]["flags"])
    assert [c[2] for c in CASES["pad_31"]["crops"]] == [13, 21, 29] and CASES["pad_31"]["pad"] == (31, 31)
    for name, case in CASES.items():
        assert os.path.getsize(os.path.join(GOLDEN, f"batch_{name}.npz")) < 64 * 1024
        for _, _, gh, gw in case["crops"]:      # the reflection condition holds on every case
            axis_taps(gh, case["lr"][0], case["lr"][0] / gh)
            axis_taps(gw, case["lr"][1], case["lr"][1] / gw)


def test_pad_pixels_are_exactly_zero_and_the_samples_are_the_crops():
    case = CASES["pad_31"]
    src = torch.from_numpy(fixture("pad_31")[0])
    out = run_case(case, src)
    for b, ((y0, x0, gh, gw), (h, v, r)) in enumerate(zip(case["crops"], case["flags"])):
        crop = (src[y0:y0 + gh, x0:x0 + gw].float() / 255).permute(2, 0, 1).flip(0)
        want = crop.flip(-1) if h else crop
        want = want.flip(-2) if v else want
        want = want.transpose(1, 2) if r else want
        assert torch.equal(out["gt"][b, :, :gh, :gw], want)
        assert float(out["gt"][b, :, gh:].abs().sum()) == 0 and float(out["gt"][b, :, :, gw:].abs().sum()) == 0
    rgb = run_case(case, src, bgr=False)
    assert torch.equal(rgb["gt"], out["gt"].flip(1)) and torch.equal(rgb["lq"], out["lq"].flip(1))


def test_sample_coords_on_the_cpu():
    case = CASES["d4_29"]
    src = torch.from_numpy(fixture("d4_29")[0])
    full = run_case(case, src)
    pts = torch.tensor([[0, 0], [28, 28], [-1, -29], [3, 17], [3, 17], [29, 0], [0, -30]]).repeat(8, 1, 1)
    out = run_case(case, src, sample_coords=pts)
    assert set(out) == {"gt", "lq", "gt_size", "scale_modify", "sample_coords"} and out["sample_coords"] is pts
    assert tuple(out["gt"].shape) == (8, 3, 7) and torch.equal(out["lq"], full["lq"])
    for b in range(8):
        g = full["gt"][b]
        want = torch.stack([g[:, 0, 0], g[:, 28, 28], g[:, 28, 0], g[:, 3, 17], g[:, 3, 17], torch.zeros(3), torch.zeros(3)], 1)
        assert torch.equal(out["gt"][b], want)


# ---- draw_batch -------------------------------------------------------------------------------------------------------------
def dataset_draws(rng, sizes, lr, scale_list, round_mode, use_hflip, use_rot, cap):
    """continuous_bicubic_downsample_dataset.py:53-66 (`cap`: the _sa1b variant's :53-56) and transforms.py:119-121, restated"""
    out = []
    for h, w in sizes:
        if len(scale_list) == 2:
            top = min(min(h / lr, w / lr), scale_list[1]) if cap else scale_list[1]
            scale = float(rng.uniform(scale_list[0], top))
        else:
            scale = rng.choice(scale_list)
        lr_size = torch.tensor([lr, lr])
        if round_mode == "ceil":
            gt = [math.ceil(scale * lr_size[0]), math.ceil(scale * lr_size[1])]
        else:
            gt = [round(scale * lr_size[0].item()), round(scale * lr_size[1].item())]
        y0 = rng.randint(0, h - gt[0])
        x0 = rng.randint(0, w - gt[1])
        hflip = use_hflip and rng.random() < 0.5
        vflip = use_rot and rng.random() < 0.5
        rot90 = use_rot and rng.random() < 0.5
        out.append(((y0, x0, gt[0], gt[1]), scale, bool(hflip), bool(vflip), bool(rot90)))
    return out


DRAWS = {
    "ceil": dict(scale_list=[1, 4], round_mode="ceil"),
    "round": dict(scale_list=[1, 4], round_mode="round"),
    "choice of three": dict(scale_list=[2, 3, 4]),
    "no hflip": dict(scale_list=[1, 4], use_hflip=False),
    "no rot": dict(scale_list=[1, 4], use_rot=False),
    "neither": dict(scale_list=[1.5, 2, 3.25], use_hflip=False, use_rot=False),
    "capped": dict(scale_list=[1, 8], cap_scale_to_image=True),
}


@pytest.mark.parametrize("what", list(DRAWS))
def test_draw_batch_makes_the_datasets_draws(what):
    kw = dict(round_mode="ceil", use_hflip=True, use_rot=True, cap_scale_to_image=False)
    kw.update(DRAWS[what])
    sizes = [(200 + 7 * i, 260 - 2 * i) for i in range(25)]
    for seed in range(8):
        mine, theirs = random.Random(seed), random.Random(seed)
        args, scales = D.draw_batch(sizes, 48, kw["scale_list"], mine, kw["round_mode"], kw["use_hflip"], kw["use_rot"], kw["cap_scale_to_image"])
        want = dataset_draws(theirs, sizes, 48, kw["scale_list"], kw["round_mode"], kw["use_hflip"], kw["use_rot"], kw["cap_scale_to_image"])
        assert set(args) == {"crops", "hflip", "vflip", "rot90"}
        assert args["crops"] == [w[0] for w in want] and scales == [w[1] for w in want]
        assert args["hflip"] == [w[2] for w in want] and args["vflip"] == [w[3] for w in want] and args["rot90"] == [w[4] for w in want]
        assert mine.getstate() == theirs.getstate()       # as many draws, no more
        if not kw["use_hflip"]:
            assert not any(args["hflip"])
        if not kw["use_rot"]:
            assert not any(args["vflip"]) and not any(args["rot90"])
        for (y0, x0, gh, gw), (h, w), s in zip(args["crops"], sizes, scales):      # 8 * 25 = 200 draws
            assert 0 <= y0 and y0 + gh <= h and 0 <= x0 and x0 + gw <= w and gh == gw
            if what == "capped":
                assert s <= min(h, w) / 48
    # fewer draws without the flips: 3 per sample instead of 6
    a, b = random.Random(5), random.Random(5)
    D.draw_batch(sizes[:1], 48, [1, 4], a, use_hflip=False, use_rot=False)
    g = math.ceil(float(b.uniform(1, 4)) * torch.tensor(48))
    b.randint(0, sizes[0][0] - g), b.randint(0, sizes[0][1] - g)
    assert a.random() == b.random()


def test_draw_batch_feeds_make_batch_and_refuses_small_images():
    rng = random.Random(3)
    imgs = [torch.randint(0, 256, (60 + i, 70, 3), dtype=torch.uint8) for i in range(3)]
    args, scales = D.draw_batch([t.shape[:2] for t in imgs], 12, [1, 4], rng)
    out = D.make_batch(imgs, lr_size=12, **args)
    assert tuple(out["lq"].shape) == (3, 3, 12, 12) and out["gt_size"].tolist() == [[c[2], c[3]] for c in args["crops"]]
    with pytest.raises(ValueError):
        D.draw_batch([(40, 200)], 12, [3.5, 4], random.Random(0))         # 42 rows at the least
    with pytest.raises(ValueError):
        D.draw_batch([(64, 64)], (12, 16), [1, 2], random.Random(0))      # transpositions of a rectangular LR
    with pytest.raises(ValueError):
        D.draw_batch([(64, 64)], 12, [1, 2], random.Random(0), round_mode="floor")
    args, _ = D.draw_batch([(64, 64)], (12, 16), [1, 2], random.Random(0), use_rot=False)
    assert args["crops"][0][2] != args["crops"][0][3] and args["rot90"] == [False]


# ---- ValueErrors ------------------------------------------------------------------------------------------------------------
def test_value_errors():
    img = torch.randint(0, 256, (40, 50, 3), dtype=torch.uint8)
    ok = (3, 4, 24, 24)
    bad = {
        "float image": lambda: D.make_batch([img.float()], [ok], 6),
        "non-contiguous image": lambda: D.make_batch([img.transpose(0, 1)], [ok], 6),
        "strided image": lambda: D.make_batch([img[:, ::2]], [ok], 6),
        "four channels": lambda: D.make_batch([torch.zeros(40, 50, 4, dtype=torch.uint8)], [ok], 6),
        "a tensor, not a sequence": lambda: D.make_batch(img, [ok], 6),
        "window below the image": lambda: D.make_batch([img], [(17, 4, 24, 24)], 6),
        "window right of the image": lambda: D.make_batch([img], [(3, 27, 24, 24)], 6),
        "negative offset": lambda: D.make_batch([img], [(-1, 4, 24, 24)], 6),
        "empty window": lambda: D.make_batch([img], [(3, 4, 0, 24)], 6),
        "rot90 with a rectangular lr_size": lambda: D.make_batch([img], [ok], (6, 8), rot90=[True]),
        "rot90 of a rectangular crop": lambda: D.make_batch([img], [(3, 4, 24, 30)], 6, rot90=[True]),
        "B = 0": lambda: D.make_batch([], [], 6),
        "B = 65": lambda: D.make_batch([img] * 65, [ok] * 65, 6),
        "mixed devices": lambda: D.make_batch([img, img.to("meta")], [ok, ok], 6),
        "gt_pad below a sample": lambda: D.make_batch([img], [ok], 6, gt_pad=(24, 23)),
        "one crop for two images": lambda: D.make_batch([img, img], [ok], 6),
        "two flags for one image": lambda: D.make_batch([img], [ok], 6, hflip=[True, False]),
        "lr_size 0": lambda: D.make_batch([img], [ok], 0),
        "reflection condition": lambda: D.make_batch([img], [ok], 1),       # 24 pixels to 1: taps beyond one reflection
        "float sample_coords": lambda: D.make_batch([img], [ok], 6, sample_coords=torch.zeros(1, 5, 2)),
        "sample_coords of another batch": lambda: D.make_batch([img], [ok], 6, sample_coords=torch.zeros(2, 5, 2, dtype=torch.long)),
    }
    for what, call in bad.items():
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"{what}: raised nothing")
    assert tuple(D.make_batch([img], [ok], (6, 8))["lq"].shape) == (1, 3, 6, 8)
    assert tuple(D.make_batch([img] * 64, [ok] * 64, 6)["gt"].shape) == (64, 3, 24, 24)


def test_package_exports():
    import gsasr_amd
    assert gsasr_amd.make_batch is D.make_batch and gsasr_amd.draw_batch is D.draw_batch


# ---- the C ABI --------------------------------------------------------------------------------------------------------------
BATCH_SYMBOLS = ("gsasr_batch_scratch_bytes", "gsasr_batch_make", "gsasr_batch_pick")
HOST = (ctypes.c_double * 512)()
PTR = (ctypes.cast(HOST, ctypes.c_void_p).value + 255) & ~255      # a host stand-in for every device pointer: never dereferenced


def test_header_bindings_and_library_agree_on_the_batch_entry_points():
    hdr = open(os.path.join(ROOT, "include", "gsasr_splat.h")).read()
    assert re.search(r"typedef struct gsasr_batch \{[^}]*int batch;[^}]*const unsigned char \*const \*src;[^}]*const int \*src_hw;[^}]*"
                     r"const int \*window;[^}]*const unsigned char \*aug;[^}]*int gt_h, gt_w;[^}]*float \*gt;[^}]*int lr_h, lr_w;[^}]*"
                     r"float \*lq;[^}]*unsigned flags;[^}]*void \*scratch;[^}]*\} gsasr_batch;", hdr)
    for name, value in (("HFLIP", 1), ("VFLIP", 2), ("TRANSPOSE", 4), ("BGR", 1), ("NO_ANTIALIAS", 2)):
        assert re.search(rf"#define GSASR_BATCH_{name} {value}u\b", hdr) and getattr(_cabi, "BATCH_" + name) == value
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(gsasr_[a-z_0-9]+)\s*\(", code))
    L = ctypes.CDLL(_cabi.LIB_PATH)
    for name in BATCH_SYMBOLS:
        assert name in declared and name in _cabi.EXPORTS and hasattr(L, name), name
    assert declared == set(_cabi.EXPORTS), declared ^ set(_cabi.EXPORTS)
    # additive: the version and every existing struct stay
    assert _cabi.lib().gsasr_abi_version() == 7 and "#define GSASR_SPLAT_ABI_VERSION 7" in hdr
    assert ctypes.sizeof(_cabi.Dims) == 64 and ctypes.sizeof(_cabi.Resize) == 120 and ctypes.sizeof(_cabi.Batch) == 88
    for words in ("not meant to be captured", "horizontal flip, vertical flip, transposition", "wraps once", "HOST array [4 * batch]",
                  "one correctly rounded division", "no memset is launched"):
        assert words in hdr, words
    from gsasr_amd import build
    assert "splat_data" in build.PARTS
    assert '#include "splat_data.hip"' in open(os.path.join(ROOT, "gsasr_amd", "csrc", "gsasr_splat.hip")).read()


def descriptor(n=1, src=None, hw=(40, 50), window=(3, 4, 24, 24), aug=0, gt_hw=(24, 24), lr_hw=(6, 6), flags=1, **kw):
    d = _cabi.make_batch_desc([PTR if src is None else src] * n, [hw] * n, [window] * n, None if aug is None else [aug] * n, gt_hw, lr_hw, flags)
    f = dict(gt=PTR, lq=PTR, scratch=PTR)
    f.update(kw)
    for k, v in f.items():
        setattr(d, k, v)
    return d


def _null(field):
    def make():
        d = descriptor()
        setattr(d, field, None)
        return d
    return make


def _null_image():
    d = descriptor(n=2)
    d._src[1] = 0
    return d


BAD = {     # name -> (descriptor, refused by: m = make, p = pick, s = the size query)
    "batch 0": (lambda: descriptor(n=0), "mps"),
    "batch 65": (lambda: descriptor(n=65), "mps"),
    "null src array": (_null("src"), "mps"),
    "null src_hw": (_null("src_hw"), "mps"),
    "null window": (_null("window"), "mps"),
    "null source image": (_null_image, "mps"),
    "null lq": (lambda: descriptor(lq=None), "m"),
    "null scratch": (lambda: descriptor(scratch=None), "m"),
    "misaligned gt": (lambda: descriptor(gt=PTR + 2), "m"),
    "misaligned lq": (lambda: descriptor(lq=PTR + 1), "m"),
    "misaligned scratch": (lambda: descriptor(scratch=PTR + 16), "m"),
    "source of 0 rows": (lambda: descriptor(hw=(0, 50)), "mps"),
    "source of 32768 columns": (lambda: descriptor(hw=(40, 32768)), "mps"),
    "window below its source": (lambda: descriptor(window=(17, 4, 24, 24)), "mps"),
    "window right of its source": (lambda: descriptor(window=(3, 27, 24, 24)), "mps"),
    "negative offset": (lambda: descriptor(window=(3, -1, 24, 24)), "mps"),
    "window with no pixel": (lambda: descriptor(window=(3, 4, 24, 0)), "mps"),
    "gt_h 0": (lambda: descriptor(gt_hw=(0, 24)), "ms"),
    "gt_w 32768": (lambda: descriptor(gt_hw=(24, 32768)), "ms"),
    "lr_h 0": (lambda: descriptor(lr_hw=(0, 6)), "ms"),
    "lr_w 32768": (lambda: descriptor(lr_hw=(6, 32768)), "ms"),
    "GT slot narrower than the sample": (lambda: descriptor(gt_hw=(24, 23)), "ms"),
    "GT slot lower than the transposed sample": (lambda: descriptor(window=(3, 4, 20, 24), gt_hw=(20, 24), aug=4), "ms"),
    "transposed with a rectangular LR": (lambda: descriptor(aug=4, lr_hw=(6, 8)), "ms"),
    "unknown flag": (lambda: descriptor(flags=4), "mps"),
    "unknown augmentation bit": (lambda: descriptor(aug=8), "mps"),
    "reflection condition (24 pixels to 1)": (lambda: descriptor(lr_hw=(1, 6)), "ms"),
}


@pytest.mark.parametrize("what", list(BAD))
def test_argument_errors_before_anything_is_enqueued(what):
    L = _cabi.lib()
    make, who = BAD[what]
    d = make()
    assert L.gsasr_batch_make(ctypes.byref(d), None) == -1, what
    assert len(L.gsasr_last_error()) > 0
    if "p" in who:
        assert L.gsasr_batch_pick(ctypes.byref(d), PTR, 5, PTR, None) == -1, what
    if "s" in who:
        assert L.gsasr_batch_scratch_bytes(ctypes.byref(d)) == 0, what
    else:
        assert L.gsasr_batch_scratch_bytes(ctypes.byref(d)) > 0, what


def test_null_descriptor_pick_arguments_and_scratch_bytes():
    L = _cabi.lib()
    assert L.gsasr_batch_make(None, None) == -1 and L.gsasr_batch_pick(None, PTR, 5, PTR, None) == -1 and L.gsasr_batch_scratch_bytes(None) == 0
    d = descriptor()
    for args in ((None, 5, PTR), (PTR, 5, None), (PTR, 0, PTR), (PTR, (1 << 24) + 1, PTR), (PTR + 2, 5, PTR), (PTR, 5, PTR + 1)):
        assert L.gsasr_batch_pick(ctypes.byref(d), args[0], args[1], args[2], None) == -1, args
    assert b"reflection" in (L.gsasr_batch_scratch_bytes(ctypes.byref(descriptor(lr_hw=(1, 6)))), L.gsasr_last_error())[1]
    n = L.gsasr_batch_scratch_bytes(ctypes.byref(descriptor()))
    # at least the float crop [3, 24, 24] and the resize's intermediate [3, 6, 24]; with an augmented sample the LR [3, 6, 6] besides
    assert n >= 4 * (3 * 24 * 24 + 3 * 6 * 24) and n % 256 == 0
    assert L.gsasr_batch_scratch_bytes(ctypes.byref(descriptor(aug=1))) >= n + 4 * 3 * 6 * 6
    assert L.gsasr_batch_scratch_bytes(ctypes.byref(descriptor(aug=None))) == n
    assert L.gsasr_batch_scratch_bytes(ctypes.byref(descriptor(gt=None, lq=None, scratch=None))) == n      # the pointers are not looked at
