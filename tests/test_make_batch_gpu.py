"""Training batches from decoded images on the GPU (gsasr_batch_make / gsasr_batch_pick: csrc/splat_data.hip) against the package's
CPU path (gsasr_amd/data.py, held to the reference's recorded batches by tests/test_make_batch.py).

Bars.  `gt` is data movement and one correctly rounded division: the GPU's bits are the CPU path's.  `lq` is the library's own
resize of the un-augmented crops followed by the flips: the GPU's bits are those of `imresize_batch` + `torch.flip` /
`transpose` on the device; against the reference's recorded `lq`, and against the CPU path where a test says so, 1e-6 absolute
(the bar tests/test_imresize.py holds the small cases to: at most 22 taps a pass here)."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import wsguard      # noqa: E402
from test_make_batch import ALL8, CASES, fixture, run_case      # noqa: E402

from gsasr_amd import _cabi      # noqa: E402
from gsasr_amd import data as D      # noqa: E402
from gsasr_amd import resize as R      # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the MI355X box)"
    return torch.device("cuda:0")


def source(h, w, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8))


def augment(t, flags):
    h, v, r = flags
    t = t.flip(-1) if h else t
    t = t.flip(-2) if v else t
    return t.transpose(-1, -2) if r else t


def lq_composition(images, crops, lr, flags, bgr=True):
    """the library's own resize of the un-augmented float crops, then torch's flips, on the images' device.  (The crops are
    divided on the CPU: torch's GPU division by a Python scalar multiplies by the reciprocal, which is not the reference's
    correctly rounded `astype(float32) / 255.`)"""
    B = len(images)
    hm, wm = max(c[2] for c in crops), max(c[3] for c in crops)
    x = torch.zeros(B, 3, hm, wm, device=images[0].device)
    for b, (t, (y0, x0, gh, gw)) in enumerate(zip(images, crops)):
        chw = (t[y0:y0 + gh, x0:x0 + gw].cpu().float() / 255).permute(2, 0, 1).to(t.device)
        x[b, :, :gh, :gw] = chw.flip(0) if bgr else chw
    y = R.imresize_batch(x, [(c[2], c[3]) for c in crops], out_size=lr)
    return torch.stack([augment(y[b], flags[b]) for b in range(B)])


def both(dev, images, crops, lr, flags, **kw):
    """make_batch on the GPU, checked: gt against the CPU path's bits, lq against the composition's.  Returns (gpu, cpu)."""
    lr = (lr, lr) if isinstance(lr, int) else lr
    f = [[a[i] for a in flags] for i in range(3)]
    cpu = D.make_batch(images, crops, lr, *f, **kw)
    on = [t.to(dev) for t in images]
    gpu = D.make_batch(on, crops, lr, *f, **kw)
    assert gpu["gt"].device.type == "cuda" and gpu["gt"].dtype == torch.float32 and gpu["gt"].shape == cpu["gt"].shape
    assert torch.equal(gpu["gt"].cpu(), cpu["gt"]), "gt differs from the CPU path"
    assert gpu["lq"].shape == cpu["lq"].shape
    assert torch.equal(gpu["lq"], lq_composition(on, crops, lr, flags, kw.get("bgr", True))), "lq differs from imresize_batch + flips"
    for k in ("gt_size", "scale_modify", "pad_h", "pad_w"):
        assert (k in gpu) == (k in cpu) and (k not in gpu or (gpu[k].device.type == "cpu" and torch.equal(gpu[k], cpu[k])))
    return gpu, cpu


@pytest.mark.parametrize("name", list(CASES))
def test_fixture_cases(name, dev):
    case = CASES[name]
    src, gt, lq = fixture(name)
    gpu, _ = both(dev, [torch.from_numpy(src)] * len(case["crops"]), case["crops"], case["lr"], case["flags"], gt_pad=case["pad"])
    assert np.array_equal(gpu["gt"].cpu().numpy(), gt)
    e = np.abs(gpu["lq"].cpu().numpy() - lq).max()
    print(f"{name}: gt equal, |lq - reference| {e:.3e} (bar 1e-6)")
    assert e <= 1e-6
    rgb = run_case(case, torch.from_numpy(src).to(dev), bgr=False)
    assert torch.equal(rgb["gt"], gpu["gt"].flip(1)) and torch.equal(rgb["lq"], gpu["lq"].flip(1))


@pytest.mark.parametrize("width", [1, 63, 64, 65, 129])
def test_row_segments_on_every_byte_phase(width, dev):
    """crop widths around the 32-pixel tile and the 64-lane wave, at x0 = 1, 2, 3 of a source whose rows are 3 * 137 bytes apart: a
    row's first byte falls on every phase of a dword, and the phase changes from row to row"""
    src = source(11, 137, 30 + width)
    crops, flags = [], []
    for x0 in (1, 2, 3, 137 - width):
        for h in (0, 1):
            crops.append((x0 % 3, x0, 9, width))
            flags.append((h, x0 & 1, 0))
    both(dev, [src] * len(crops), crops, (3, max(1, width // 4)), flags)


@pytest.mark.parametrize("n", [33, 65])
def test_transposed_samples_across_tiles(n, dev):
    """one and two tiles of 32 pixels and one pixel more, each way, every transposed combination next to its untransposed one"""
    srcs = [source(n + 6, n + 9, 40 + n + b) for b in range(8)]
    crops = [(b % 5, 8 - b, n, n) for b in range(8)]
    both(dev, srcs, crops, 16, ALL8)
    both(dev, srcs, crops, 16, ALL8, gt_pad=(n + 31, n + 2))


def test_window_at_the_last_offset_of_an_image_on_an_odd_address(dev):
    """the window ends with the image's last byte; the image starts one, two and three bytes into its allocation, and with three
    ends where the allocation ends: nothing outside the image is needed"""
    h, w = 19, 21
    flat = torch.from_numpy(np.random.default_rng(7).integers(0, 256, 3 + h * w * 3, dtype=np.uint8))
    crops = [(0, 0, 13, 13), (h - 13, w - 13, 13, 13), (0, 0, h, w), (h - 13, w - 13, 13, 13)]
    flags = [(0, 0, 0), (0, 0, 0), (1, 1, 0), (1, 0, 1)]
    f = [[a[i] for a in flags] for i in range(3)]
    for lead in (1, 2, 3):      # (3: the image ends with its allocation)
        cpu_img = flat[lead:lead + h * w * 3].view(h, w, 3)
        on = flat.to(dev)[lead:lead + h * w * 3].view(h, w, 3)
        assert on.data_ptr() % 4 == lead and on.is_contiguous()
        cpu = D.make_batch([cpu_img] * 4, crops, 6, *f)
        gpu = D.make_batch([on] * 4, crops, 6, *f)
        assert torch.equal(gpu["gt"].cpu(), cpu["gt"])
        assert torch.equal(gpu["lq"], lq_composition([on] * 4, crops, (6, 6), flags))


def test_a_sample_alone_and_inside_a_batch(dev):
    sizes = [40, 35, 21, 33, 37]
    srcs = [source(50 + b, 61 - b, 60 + b) for b in range(5)]
    crops = [(3 + b, 5 - b, s, s) for b, s in enumerate(sizes)]
    flags = [(1, 0, 1), (0, 1, 0), (1, 1, 1), (0, 0, 1), (1, 0, 0)]
    gpu, _ = both(dev, srcs, crops, 8, flags)
    alone, _ = both(dev, srcs[2:3], crops[2:3], 8, flags[2:3])
    assert torch.equal(alone["gt"][0], gpu["gt"][2, :, :21, :21]) and torch.equal(alone["lq"][0], gpu["lq"][2])
    assert not gpu["gt"][2, :, 21:].any() and not gpu["gt"][2, :, :, 21:].any()
    # the same source tensor twice, with different windows and flags
    twice, _ = both(dev, [srcs[0], srcs[1], srcs[0]], [crops[0], crops[1], (0, 1, 40, 40)], 8, flags[:3])
    assert torch.equal(twice["gt"][0], gpu["gt"][0]) and torch.equal(twice["lq"][0], gpu["lq"][0])


def test_batch_of_64(dev):
    srcs = [source(12 + b % 5, 14 + b % 7, 100 + b) for b in range(64)]
    crops = [(b % 4, b % 6, 9, 9) for b in range(64)]
    gpu, cpu = both(dev, srcs, crops, 4, [ALL8[b % 8] for b in range(64)])
    e = float((gpu["lq"].cpu() - cpu["lq"]).abs().max())
    print(f"64 samples of 9 x 9 to 4 x 4: |lq - CPU path| {e:.3e} (bar 1e-6)")
    assert e <= 1e-6


def test_sample_coords(dev):
    n = 29
    srcs = [source(n + 4, n + 7, 200 + b) for b in range(8)]
    crops = [(b % 4, b % 7, n, n) for b in range(8)]
    g = torch.Generator().manual_seed(5)
    pts = torch.randint(-n, n, (8, 100, 2), generator=g)
    pts[:, 10] = pts[:, 11]                                     # a repeat
    pts[:, 20] = torch.tensor([-1, -n])                         # the last row, the first column
    pts[:, 30] = torch.tensor([n, 0])                           # out of range
    pts[:, 31] = torch.tensor([3, -n - 1])                      # out of range after one wrap
    f = [[a[i] for a in ALL8] for i in range(3)]
    full = D.make_batch(srcs, crops, 6, *f)
    cpu = D.make_batch(srcs, crops, 6, *f, sample_coords=pts)
    on = [t.to(dev) for t in srcs]
    for coords in (pts.to(dev), pts.to(dev).to(torch.int32)):
        gpu = D.make_batch(on, crops, 6, *f, sample_coords=coords)
        assert set(gpu) == {"gt", "lq", "gt_size", "scale_modify", "sample_coords"} and gpu["sample_coords"] is coords
        assert tuple(gpu["gt"].shape) == (8, 3, 100) and torch.equal(gpu["gt"].cpu(), cpu["gt"])
        assert torch.equal(gpu["lq"], lq_composition(on, crops, (6, 6), ALL8))
    r, c = pts[..., 0] % n, pts[..., 1] % n                     # (Python's wrap of the in-range points)
    want = torch.stack([full["gt"][b][:, r[b], c[b]] for b in range(8)])
    want[:, :, 30] = 0
    want[:, :, 31] = 0
    assert torch.equal(gpu["gt"].cpu(), want) and bool(want[:, :, 20].any())


def test_guards_and_repeatability(dev):
    srcs = [source(40, 45, 300 + b).to(dev) for b in range(3)]
    crops = [(1, 2, 33, 33), (0, 0, 21, 40), (5, 3, 35, 17)]
    aug = [_cabi.BATCH_HFLIP | _cabi.BATCH_TRANSPOSE, _cabi.BATCH_VFLIP, 0]
    Gh, Gw, lr, G = 37, 41, 8, 64
    n_gt, n_lq = 3 * 3 * Gh * Gw, 3 * 3 * lr * lr
    d = _cabi.make_batch_desc([t.data_ptr() for t in srcs], [(40, 45)] * 3, crops, aug, (Gh, Gw), (lr, lr), _cabi.BATCH_BGR)
    n_scratch = int(_cabi.lib().gsasr_batch_scratch_bytes(ctypes.byref(d)))
    assert n_scratch > 0 and n_scratch % 256 == 0
    outs = []
    for fill in (None, None, "zero", "seeded"):      # the scratch as allocated (0xA5), twice, then from the fills of tests/wsguard.py
        fl = torch.full((G + n_gt + G + n_lq + G,), float("nan"), device=dev)
        by = torch.full((256 + n_scratch + 256,), 0xA5, dtype=torch.uint8, device=dev)
        gt = fl[G:G + n_gt].view(3, 3, Gh, Gw)
        lq = fl[G + n_gt + G:G + n_gt + G + n_lq].view(3, 3, lr, lr)
        scratch = by[256:256 + n_scratch]
        assert scratch.data_ptr() % 256 == 0
        if fill:
            scratch.copy_(torch.from_numpy(wsguard.fill_bytes(fill, n_scratch, seed=7)))
        _cabi.batch_make(srcs, crops, aug, gt, lq, scratch=scratch)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(gt).all()) and bool(torch.isfinite(lq).all())
        assert bool(torch.isnan(fl[:G]).all()) and bool(torch.isnan(fl[G + n_gt:G + n_gt + G]).all()) and bool(torch.isnan(fl[-G:]).all())
        assert bool((by[:256] == 0xA5).all()) and bool((by[-256:] == 0xA5).all())
        outs.append((gt.clone(), lq.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert all(torch.equal(o[0], outs[0][0]) and torch.equal(o[1], outs[0][1]) for o in outs[2:])
    f = [[bool(a & m) for a in aug] for m in (1, 2, 4)]
    cpu = D.make_batch([t.cpu() for t in srcs], crops, lr, *f, gt_pad=(Gh, Gw))
    assert torch.equal(outs[0][0].cpu(), cpu["gt"])


def test_the_batch_feeds_the_fused_loss(dev):
    """draw -> make_batch -> generate_2D_gaussian_splatting_batch_loss: the loss and its gradient have the bits they have with the
    CPU-made batch copied to the device"""
    from gsasr_amd import gaussian_splatting as gsp, synthetic
    srcs = [source(40, 44, 400 + b) for b in range(3)]
    crops, flags = [(2, 3, 24, 24), (0, 1, 20, 20), (9, 11, 18, 18)], [(1, 0, 0), (0, 1, 1), (1, 1, 1)]
    f = [[a[i] for a in flags] for i in range(3)]
    cpu = D.make_batch(srcs, crops, 6, *f)
    gpu = D.make_batch([t.to(dev) for t in srcs], crops, 6, *f)
    p = torch.stack([synthetic.gs_parameters(6, 8, seed=9 + b) for b in range(3)]).to(dev)
    assert p.shape[1] == 48
    got = []
    for batch in (gpu, cpu):
        q = p.clone().requires_grad_(True)
        loss = gsp.generate_2D_gaussian_splatting_batch_loss(batch["gt_size"], q, [4.0] * 3, batch["scale_modify"], batch["gt"].to(dev), loss="l1", dmax=0.3)
        g, = torch.autograd.grad(loss, q)
        got.append((loss.detach(), g))
    assert bool(torch.isfinite(got[0][0])) and float(got[0][0]) > 0
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])


def test_c_program_batch(tmp_path):
    """the batch from plain C (tests/c_abi/c_abi_batch_check.c): built with gcc against libgsasr_splat.so, run on the GPU"""
    lib = _cabi.LIB_PATH
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc and os.path.exists(lib)
    exe = str(tmp_path / "c_abi_batch_check")
    subprocess.check_call([cc, "-O1", "-std=c11", "-D__HIP_PLATFORM_AMD__", f"-I{rocm}/include", f"-I{ROOT}/include",
                           os.path.join(HERE, "c_abi", "c_abi_batch_check.c"), lib, f"-L{rocm}/lib", "-lamdhip64", "-lm",
                           f"-Wl,-rpath,{os.path.dirname(lib)}", f"-Wl,-rpath,{rocm}/lib", "-o", exe])
    out = subprocess.run(["timeout", "-k", "10", "120", exe], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "C-ABI BATCH CHECK OK" in out.stdout, out.stdout + out.stderr
