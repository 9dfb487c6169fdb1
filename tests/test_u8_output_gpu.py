"""8-bit image output on the GPU (gsasr_splat_forward_u8 and the step / batch forms): the store itself, exactly, through every
forward kernel; dense input against the library's own float image; and against the oracle.

`quantise` is the reference's epilogue written out (inference_paper.py:134-140, basicsr/utils/img_util.py:73-96):
clamp_(0, 1) -> HWC -> (x * 255.0).round().astype(uint8); the crop and the channel swap are applied by the callers here.

The forward is not bit-reproducible from run to run in general (its tile walk fills an LDS candidate list through atomicAdd on a
shared counter, so the order of a pixel's sum follows wave timing).  The exact tests therefore render Gaussians that are so far
apart that no pixel is reached by the windows of two of them (`separated`): one term per pixel, no order."""
import ctypes
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")
RASTER = sorted(glob.glob(os.path.join(GOLDEN, "raster_*.npz")))
TAU = 6.0       # explicit support cutoff of the exact cases: windows of sigma * sqrt(12) = 3.47 sigma


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the MI355X box)"
    return torch.device("cuda:0")


def quantise(hwc: torch.Tensor) -> np.ndarray:
    return (hwc.detach().cpu().clone().clamp_(0, 1).numpy() * 255.0).round().astype(np.uint8)


# colours (r, g, b) cycled over the Gaussians: above 1 (upper clamp), negative (lower clamp), small (the low levels)
PALETTE = [(1.3, -0.4, 0.9), (0.35, 1.0, 2.5), (-1.0, 0.6, 1.1), (5.0, 0.08, 0.999), (0.7, 1.7, -0.2), (1.05, 0.2, 0.5)]


def separated(H, W, s_total=None, spacing=64, sigma_px=4.0, seed=0):
    """kernel-frame Gaussians on a `spacing`-px lattice (centres jittered by up to a pixel), std <= sigma_px pixels, |rho| <= 0.4.
    With TAU a window is at most 3.47 * 4 + 1 = 15 px wide each way; a wave renders whole sub-tiles (up to 16 px), so a Gaussian
    is evaluated at most 15 + 1 + 15 = 31 px from its lattice point: less than half the spacing.  Record 1 is a NaN record (a
    dead Gaussian) and NaN records pad the list to `s_total` (a dense plan is a matter of the COUNT of records)."""
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
    total = max(n + 1, s_total or 0)
    out = np.full((total, 8), np.nan, np.float32)
    out[0] = rec[0]
    out[2: n + 1] = rec[1:]
    t = torch.from_numpy(out)
    return t[:, 0:3].contiguous(), t[:, 3:5].contiguous(), t[:, 5:8].contiguous()


def box_dmax(H, W):
    """a dmax box of at most 20 px each way: the bounded op's own in-kernel test then zeroes anything farther, exactly"""
    return 40.0 / (max(H, W) - 1)


def canary_target(nrows, cols, pad, dev, batch=0):
    """a uint8 buffer filled with a pattern, three rows longer than the image, and the strided view of it that the forward
    writes: rows of 3 * cols + pad bytes"""
    pitch = 3 * cols + pad
    n = max(batch, 1) * nrows
    buf = (torch.arange((n + 3) * pitch, device=dev) % 251).to(torch.uint8)
    before = buf.clone()
    shape, strides = ((batch, nrows, cols, 3), (nrows * pitch, pitch, 3, 1)) if batch else ((nrows, cols, 3), (pitch, 3, 1))
    return buf, before, buf.as_strided(shape, strides)


def canary_intact(buf, before, nrows, cols, pad, batch=0):
    pitch = 3 * cols + pad
    n = max(batch, 1) * nrows
    a, b = buf.cpu().numpy(), before.cpu().numpy()
    tail_ok = np.array_equal(a[n * pitch:], b[n * pitch:])
    a, b = a[: n * pitch].reshape(n, pitch), b[: n * pitch].reshape(n, pitch)
    return tail_ok and np.array_equal(a[:, 3 * cols:], b[:, 3 * cols:])


VARIANTS = [dict(crop=False, pad=0, bgr=False), dict(crop=True, pad=0, bgr=False), dict(crop=True, pad=13, bgr=False),
            dict(crop=False, pad=0, bgr=True), dict(crop=True, pad=5, bgr=True)]


def check_plan_exact(plan, dev, fwd_flags=0, levels=True):
    """forward_u8 of `plan` == quantise(crop(float image of forward on the same plan and kernel flags)), for every variant: no
    crop; a crop that is a multiple of neither 8 nor 16 either way; row padding and rows behind the image that must survive;
    swapped channels.  One image or a row band of one."""
    from gsasr_amd import _cabi
    d = plan.dims
    r0, r1, H, W = d.row0, d.row1, d.h, d.w
    img = torch.full((r1 - r0, W, 3), float("nan"), device=dev)
    _cabi.forward(plan, img, overwrite=True, flags=fwd_flags)
    assert bool(torch.isfinite(img).all())
    if levels:
        assert float(img.min()) < 0.0 and float(img.max()) > 1.0        # both clamps fire
    for v in VARIANTS:
        crop = (H - 21, W - 37) if v["crop"] else (H, W)
        assert not v["crop"] or all(c % 8 and c % 16 for c in crop)
        nrows = min(r1, crop[0]) - r0
        want = quantise(img[:nrows, : crop[1]])
        if v["bgr"]:
            want = want[:, :, ::-1]
        if v["pad"]:
            buf, before, out = canary_target(nrows, crop[1], v["pad"], dev)
            got = _cabi.forward_u8(plan, crop=crop, bgr=v["bgr"], out=out, flags=fwd_flags)
            assert got.data_ptr() == buf.data_ptr()
            assert canary_intact(buf, before, nrows, crop[1], v["pad"]), v
        else:
            got = _cabi.forward_u8(plan, crop=crop if v["crop"] else None, bgr=v["bgr"], flags=fwd_flags)
        assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape
        assert np.array_equal(got.cpu().numpy(), want), (v, int((got.cpu().numpy() != want).sum()))
        if levels and not v["crop"] and r1 - r0 == H:
            # the ramps sweep every level.  A level near the top is hit by 2 pi sigma^2 / 255 = 0.3 px per Gaussian and channel
            # brighter than 1: 20 and more pixels per level from 64 Gaussians, ~5 from the 16 of a 256^2 image (the one shape
            # that selects PER_SUB), where a few levels may stay empty
            assert len(np.unique(want)) >= (256 if H * W >= 512 * 512 else 240), len(np.unique(want))


# name -> (H, W, records, plan flag, list_cap): the shape that selects each forward kernel (the launcher's rules
# in gsasr_amd/csrc/splat_forward.hip: sub-tiles of 8 x 16 px, workgroup tiles of 32 x 16 px)
KERNELS = {
    # sparse, no lists, 2048 sub-tiles < 4096: the two-level walk with two waves per sub-tile
    "fwd2-parts2": (512, 512, 0, "narrow", -1),
    # 64 x 64 = 4096 sub-tiles: one wave per sub-tile
    "fwd2-parts1": (1024, 512, 0, "narrow", -1),
    # ... and its record-pair form: a dense plan without lists, too many sub-tiles for the split kernel
    "fwd2-parts1-pairs": (1024, 512, 131072, "narrow", -1),
    # explicit lists on 128 tiles: half-list waves even out the load -> one workgroup per sub-tile (PER_SUB)
    "list-persub": (256, 256, 0, "narrow", 256),
    # 256 tiles: the tile form, 1024 sub-tiles < 6144 -> two waves per sub-tile
    "list-parts2": (512, 256, 0, "narrow", 256),
    # 1536 tiles, 6144 sub-tiles: the tile form, one wave per sub-tile
    "list-parts1": (768, 1024, 0, "narrow", 256),
    # a dense plan (one record per four pixels) evaluates record PAIRS; without lists and below 4096 sub-tiles: the split kernel
    "split-pairs": (512, 512, 65536, "narrow", -1),
    # dense with the library's own choice (list_cap 0): lists from 2048 sub-tiles, 512 tiles -> the tile form, two waves, pairs
    "dense-default": (512, 512, 65536, "narrow", 0),
    "list-persub-pairs": (256, 256, 16384, "narrow", 256),
    # the wide forward (16 x 16 sub-tiles), search and 32 x 32-px tile lists
    "fwd16": (512, 512, 0, "wide", -1),
    "fwd16-ragged": (250, 300, 0, "wide", -1),
    "fwd16-list": (512, 512, 0, "wide", 256),
}


def kernel_case(name, dmax_on, dev, forward_only=True, rows=None):
    from gsasr_amd import _cabi
    H, W, s_total, width, cap = KERNELS[name]
    flag = _cabi.FLAG_FWD_WIDE if width == "wide" else _cabi.FLAG_FWD_NARROW
    sig, xy, col = separated(H, W, s_total, seed=len(name))
    plan = _cabi.plan(sig.to(dev), xy.to(dev), col.to(dev), H, W, box_dmax(H, W) if dmax_on else None, rows=rows, cutoff=TAU,
                      flags=flag | (_cabi.FLAG_FORWARD_ONLY if forward_only else 0), list_cap=cap)
    assert _cabi.forward_subtile_width(plan, flag) == (16 if width == "wide" else 8)
    return plan, flag


@pytest.mark.parametrize("dmax_on", [True, False], ids=["bounded", "unbounded"])
@pytest.mark.parametrize("name", sorted(KERNELS))
def test_store_is_exact_through_every_forward_kernel(name, dmax_on, dev):
    plan, flag = kernel_case(name, dmax_on, dev, forward_only=(len(name) % 2 == 0))
    check_plan_exact(plan, dev, flag)


def test_store_is_exact_through_the_fine_forward():
    """k_render_fwd8 sits behind a development switch that is read once per process: a child process with the switch set runs
    the sparse case of this file"""
    env = dict(os.environ, GSASR_SPLAT_DEV="1", GSASR_SPLAT_FWD8="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert r.returncode == 0 and "fwd8 exact" in r.stdout, (r.stdout[-1500:], r.stderr[-1500:])


@pytest.mark.parametrize("name", ["fwd2-parts2", "list-persub", "fwd16", "fwd16-list", "split-pairs"])
@pytest.mark.parametrize("rows", [(37, 203), (16, None)], ids=["rows37-203", "rows16-end"])
def test_store_is_exact_on_a_row_band(name, rows, dev):
    """a band that does not start at row 0: `out` is the band's first row, the crop counts in rows of the whole grid (the
    first band ends above the crop's last row, the second below it)"""
    plan, flag = kernel_case(name, True, dev, rows=(rows[0], rows[1] or KERNELS[name][0]))
    check_plan_exact(plan, dev, flag)


@pytest.mark.parametrize("dmax_on", [True, False], ids=["bounded", "unbounded"])
@pytest.mark.parametrize("cap", [-1, 256], ids=["search", "lists"])
def test_store_is_exact_on_a_batched_canvas_with_ragged_samples(dmax_on, cap, dev):
    """samples of different sizes in one canvas: every sample's rectangle [crop_rows, crop_cols] holds its own pixels and 0
    beyond its own h_b x w_b, like the float canvas' padding"""
    from gsasr_amd import _cabi
    sizes = [(200, 256), (131, 190), (192, 77), (256, 250)]
    B, n_per = len(sizes), 24
    parts = [separated(h, w, n_per, seed=50 + b) for b, (h, w) in enumerate(sizes)]
    assert all(p[0].shape[0] == n_per for p in parts)
    sig, xy, col = (torch.cat([p[k] for p in parts]).to(dev) for k in range(3))
    d = _cabi.make_batch_dims(n_per, sizes, 256, 256, 40.0 / 255 if dmax_on else None, cutoff=TAU, flags=_cabi.FLAG_FORWARD_ONLY)
    d.list_cap = cap
    L = _cabi.lib()
    nbytes = L.gsasr_splat_workspace_bytes(ctypes.byref(d))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _cabi.check(L.gsasr_splat_plan(sig.data_ptr(), xy.data_ptr(), col.data_ptr(), ctypes.byref(d), ws.data_ptr(), nbytes,
                                   torch.cuda.current_stream(dev).cuda_stream), "gsasr_splat_plan")
    plan = _cabi.Plan(d, ws, dev)
    img = torch.full((B * d.slot, d.w, 3), float("nan"), device=dev)
    _cabi.forward(plan, img, overwrite=True)
    img = img.reshape(B, d.slot, d.w, 3)
    assert bool(torch.isfinite(img).all()) and float(img.min()) < 0.0 and float(img.max()) > 1.0
    for v in VARIANTS:
        crop = (256 - 21, 256 - 37) if v["crop"] else (256, 256)
        want = quantise(img[:, : crop[0], : crop[1]])
        if v["bgr"]:
            want = want[..., ::-1]
        if v["pad"]:
            buf, before, out = canary_target(crop[0], crop[1], v["pad"], dev, batch=B)
            got = _cabi.forward_u8(plan, crop=crop, bgr=v["bgr"], out=out)
            assert canary_intact(buf, before, crop[0], crop[1], v["pad"], batch=B), v
        else:
            got = _cabi.forward_u8(plan, crop=crop if v["crop"] else None, bgr=v["bgr"])
        assert tuple(got.shape) == want.shape and np.array_equal(got.cpu().numpy(), want), v
        for b, (h, w) in enumerate(sizes):      # beyond the sample's own grid: zeros
            g = got[b].cpu().numpy()
            assert not g[h:].any() and not g[:, w:].any()
            assert g[:h, :w].any()


def raw_parameters(H, W, scale, n_total, seed=0):
    """raw decoder-style parameters [n,9] whose activations (oracle/host_ref.py; utils/gaussian_splatting.py:174-180) are
    Gaussians on a 96-px lattice with a std of <= 3 px: under the adaptive cutoff (tau <= 18.5 here: windows of <= 6.1 sigma
    = 18.3 px) a Gaussian is evaluated at most 18.3 + 1 + 1 + 15 < 48 px from its lattice point.  Colours sigmoid * alpha < 1."""
    rng = np.random.RandomState(seed)
    ny, nx = H // 96, W // 96
    gy, gx = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    n = ny * nx
    logit = lambda p: np.log(p / (1 - p))
    step = 1.2 / scale
    p = np.zeros((n_total, 9), np.float32)
    p[:, 3] = -200.0                                  # alpha = sigmoid(-200) = 0 in fp32 for the padding records: colour 0
    p[:, 7:9] = 0.5
    p[:n, 0] = logit(3.0 * step * rng.uniform(0.8, 1.0, n))       # sigma_px = sigma / step
    p[:n, 1] = logit(3.0 * step * rng.uniform(0.8, 1.0, n))
    p[:n, 2] = rng.uniform(-0.4, 0.4, n)
    p[:n, 3] = rng.uniform(2.0, 8.0, n)
    p[:n, 4:7] = rng.uniform(-3.0, 7.0, (n, 3))
    p[:n, 7] = ((gx.ravel() + 0.5) * 96 + rng.uniform(-1, 1, n)) / W
    p[:n, 8] = ((gy.ravel() + 0.5) * 96 + rng.uniform(-1, 1, n)) / H
    return torch.from_numpy(p)


@pytest.mark.parametrize("source", ["step_size", "scale_modify"])
@pytest.mark.parametrize("dmax_on", [True, False], ids=["bounded", "unbounded"])
def test_fused_step_u8_is_exact(source, dmax_on, dev):
    """gsasr_step_forward_u8 / gsasr_step_forward_sm_u8: prologue + plan + 8-bit forward; the float forward on the plan the
    call left behind gives the image to quantise"""
    from gsasr_amd import _cabi
    H, W, scale = 288, 384, 8.0
    p = raw_parameters(H, W, scale, 64, seed=3).to(dev)
    dm = 40.0 / (W - 1) if dmax_on else None
    for v in VARIANTS:
        crop = (H - 21, W - 37) if v["crop"] else (H, W)
        buf = before = None
        out = None
        if v["pad"]:
            buf, before, out = canary_target(crop[0], crop[1], v["pad"], dev)
        kw = dict(crop=crop if v["crop"] else None, bgr=v["bgr"], out=out)
        if source == "step_size":
            got, plan = _cabi.step_forward_u8(p, torch.full((1,), 1.2 / scale, device=dev), H, W, dm, **kw)
        else:
            got, plan = _cabi.step_forward_u8(p, None, H, W, dm, scale_modify=torch.tensor([scale, scale], device=dev), **kw)
        assert plan.dims.flags & _cabi.FLAG_FORWARD_ONLY
        img = torch.full((H, W, 3), float("nan"), device=dev)
        _cabi.forward(plan, img, overwrite=True)
        want = quantise(img[: crop[0], : crop[1]])
        if v["bgr"]:
            want = want[:, :, ::-1]
        assert want.max() > 200 and len(np.unique(want)) > 200
        assert tuple(got.shape) == want.shape and np.array_equal(got.cpu().numpy(), want), v
        if v["pad"]:
            assert canary_intact(buf, before, crop[0], crop[1], v["pad"]), v


def test_host_api_uint8_on_the_gpu(dev):
    """generate_2D_gaussian_splatting_step_uint8 on CUDA tensors: the fused 8-bit step, equal to the quantised float image of
    the same call's plan (through the python-number and the device `scale_modify`), no graph, and no silent fallback"""
    from gsasr_amd import _cabi, gaussian_splatting as gsp
    H, W, scale = 288, 384, 8.0
    p = raw_parameters(H, W, scale, 64, seed=4).to(dev).requires_grad_(True)
    _, plan = _cabi.step_forward_u8(p.detach(), torch.full((1,), 1.2 / scale, device=dev), H, W, 0.1)
    img = torch.empty(H, W, 3, device=dev)
    _cabi.forward(plan, img, overwrite=True)
    for sm in ((scale, scale), torch.tensor([scale, scale], device=dev)):
        for crop, bgr in ((None, False), ((267, 347), True)):
            got = gsp.generate_2D_gaussian_splatting_step_uint8((H, W), p, scale, sm, dmax=0.1, crop=crop, bgr=bgr)
            want = quantise(img if crop is None else img[: crop[0], : crop[1]])
            assert got.dtype == torch.uint8 and not got.requires_grad and got.is_cuda
            assert np.array_equal(got.cpu().numpy(), want[:, :, ::-1] if bgr else want)
    with pytest.raises(RuntimeError, match="no fallback"):
        gsp.generate_2D_gaussian_splatting_step_uint8((H, W), p.detach().reshape(2, -1, 9), scale, (scale, scale))
    gsp.deferred_asserts.flush()


def test_u8_forward_in_a_hipgraph(dev):
    """enqueue only, no host synchronisation: plan + 8-bit forward capture into one graph; a replay on new Gaussians gives
    the eager result"""
    from gsasr_amd import _cabi
    H, W = 256, 256
    inputs = [tuple(t.to(dev) for t in separated(H, W, seed=s)) for s in (11, 12)]
    static = [t.clone() for t in inputs[0]]
    out = torch.zeros(H - 21, W - 37, 3, dtype=torch.uint8, device=dev)

    def step():
        plan = _cabi.plan(*static, H, W, box_dmax(H, W), cutoff=TAU, flags=_cabi.FLAG_FORWARD_ONLY)
        _cabi.forward_u8(plan, crop=(H - 21, W - 37), bgr=True, out=out)
        return plan

    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        keep = step()
    for a, b in zip(static, inputs[1]):
        a.copy_(b)
    graph.replay()
    torch.cuda.synchronize()
    plan = _cabi.plan(*inputs[1], H, W, box_dmax(H, W), cutoff=TAU, flags=_cabi.FLAG_FORWARD_ONLY)
    img = torch.empty(H, W, 3, device=dev)
    _cabi.forward(plan, img, overwrite=True)
    want = quantise(img[: H - 21, : W - 37])[:, :, ::-1]
    assert np.array_equal(out.cpu().numpy(), want)
    del keep


def test_python_target_checks(dev):
    from gsasr_amd import _cabi
    plan, flag = kernel_case("fwd2-parts2", True, dev)
    H, W = plan.dims.h, plan.dims.w
    for bad in (torch.zeros(H, W, 3, device=dev), torch.zeros(H, W - 1, 3, dtype=torch.uint8, device=dev),
                torch.zeros(H, W, 4, dtype=torch.uint8, device=dev)[:, :, :3], torch.zeros(H, W, 3, dtype=torch.uint8)):
        with pytest.raises(RuntimeError):
            _cabi.forward_u8(plan, out=bad)
    for crop in ((0, 5), (H + 1, W), (H, W + 44)):
        with pytest.raises(RuntimeError):
            _cabi.forward_u8(plan, crop=crop)


def test_c_program_u8(tmp_path):
    """the 8-bit forward from plain C (tests/c_abi/c_abi_u8_check.c): built with gcc against libgsasr_splat.so, run on the GPU"""
    import shutil
    from gsasr_amd import _cabi
    lib = _cabi.LIB_PATH
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc and os.path.exists(lib)
    exe = str(tmp_path / "c_abi_u8_check")
    subprocess.check_call([cc, "-O1", "-std=c11", "-D__HIP_PLATFORM_AMD__", f"-I{rocm}/include", f"-I{ROOT}/include",
                           os.path.join(HERE, "c_abi", "c_abi_u8_check.c"), lib, f"-L{rocm}/lib", "-lamdhip64", "-lm",
                           f"-Wl,-rpath,{os.path.dirname(lib)}", f"-Wl,-rpath,{rocm}/lib", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "C-ABI U8 CHECK OK" in out.stdout, out.stdout + out.stderr


def tiled_models_on(dev):
    sys.path.insert(0, HERE)
    import tiled_models
    return tiled_models


@pytest.mark.parametrize("name", ["tiled_int_s4_12x40_onerow.npz", "tiled_frac_s2p5_18x22.npz", "tiled_int_s2_20x26.npz"])
def test_tiled_driver_uint8_on_the_gpu(name, dev):
    """tiles through the batched 8-bit canvas (dense, overlapping Gaussians: sums in any order), pasted as uint8: within one
    level of the quantised float canvas of the same driver, and equal where the float value is not next to a rounding boundary"""
    from gsasr_amd.split_and_joint_image import split_and_joint_image
    tm = tiled_models_on(dev)
    z = np.load(os.path.join(GOLDEN, name))
    sc = float(z["scale"])
    args = (torch.from_numpy(z["lq"]).to(dev), sc, int(z["split_size"]), int(z["overlap_size"]), tm.model_g, tm.model_fea2gs,
            torch.tensor([sc, sc], device=dev))
    ref = split_and_joint_image(*args, crop_size=int(z["crop_size"]))
    got = split_and_joint_image(*args, crop_size=int(z["crop_size"]), out_uint8=True)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (ref.shape[2], ref.shape[3], 3)
    ok, share = within_one_level(got.cpu().numpy(), ref[0].permute(1, 2, 0), 255 * 2e-5)
    assert ok
    bgr = split_and_joint_image(*args, crop_size=int(z["crop_size"]), out_uint8=True, bgr=True)
    assert within_one_level(bgr.cpu().numpy()[:, :, ::-1], ref[0].permute(1, 2, 0), 255 * 2e-5)[0]


def within_one_level(u8, ref_hwc, halfwidth):
    """the comparison rule of the two inexact checks: no value differs from quantise(ref) by more than 1, and one differs at all
    only where clamp(ref) * 255 lies within `halfwidth` (scaled by max(1, max|ref|)) of a half-integer.  Returns (ok, the share
    of values so exempt -- computed from `ref` alone)."""
    ref = ref_hwc.detach().cpu().float() if torch.is_tensor(ref_hwc) else torch.from_numpy(np.asarray(ref_hwc, np.float32))
    want = quantise(ref)
    t = (ref.clamp(0, 1).numpy() * np.float32(255.0)).astype(np.float64)
    exempt = np.abs(t - np.floor(t) - 0.5) <= halfwidth * max(1.0, float(ref.abs().max()))
    diff = np.abs(u8.astype(np.int32) - want.astype(np.int32))
    n_diff = int((diff != 0).sum())
    print(f"values {diff.size}, differing {n_diff}, exempt share {exempt.mean():.4f}, max difference {int(diff.max())}")
    return bool(diff.max() <= 1 and not (diff != 0)[~exempt].any()), float(exempt.mean())


@pytest.mark.parametrize("case", [(256, 256, 4.0, 1), (64, 64, 4.0, 16)], ids=["config2", "16-per-LR-px"])
@pytest.mark.parametrize("dmax", [0.1, None], ids=["bounded", "unbounded"])
def test_dense_input_against_the_own_float_image(case, dmax, dev):
    """overlapping Gaussians, sums in whatever order the waves ran: u8 vs quantise(own float image, same plan).  The bar is
    "the same sums in another order", 2e-5 of the largest value (tests/test_tune.py): at most one level, and any difference
    only within 255 * 2e-5 * max(1, max|v|) of a rounding boundary; at most 3 % of the values may be that close (expected
    2 * 0.0051 * max|v|: 1-2 %)."""
    from gsasr_amd import _cabi, synthetic
    h_lr, w_lr, scale, gpp = case
    sig, xy, col, H, W = synthetic.kernel_inputs(h_lr, w_lr, scale, seed=61, gpp=gpp)
    a, b, c = sig.to(dev), xy.to(dev), col.to(dev)
    img = torch.empty(H, W, 3, device=dev)
    _cabi.forward(_cabi.plan(a, b, c, H, W, dmax, flags=_cabi.FLAG_FORWARD_ONLY), img, overwrite=True)
    c = c * (1.9 / float(img.max()))          # the float image's maximum: just below 2
    plan = _cabi.plan(a, b, c, H, W, dmax, flags=_cabi.FLAG_FORWARD_ONLY)
    _cabi.forward(plan, img, overwrite=True)
    assert 1.0 < float(img.max()) <= 2.0
    got = _cabi.forward_u8(plan)
    ok, share = within_one_level(got.cpu().numpy(), img, 255 * 2e-5)
    assert ok
    assert share <= 0.03, share


def oracle_shares(ref):
    t = np.clip(ref, 0, 1).astype(np.float32) * np.float32(255.0)
    exempt = np.abs(t - np.floor(t) - 0.5) <= 0.0255 + 1e-3
    return float(exempt.mean()), float(((ref > 0.02) & (ref < 0.98)).mean())


def against_oracle(u8, ref):
    """the project's pixel bar is 1e-4 absolute = 0.0255 of an 8-bit step: at most one level anywhere, a difference at all only
    where the oracle's clamp(v) * 255 is within 0.0255 + 1e-3 of a half-integer"""
    want = (np.clip(ref, 0, 1) * np.float32(255.0)).round().astype(np.uint8)
    t = np.clip(ref, 0, 1).astype(np.float32) * np.float32(255.0)
    exempt = np.abs(t - np.floor(t) - 0.5) <= 0.0255 + 1e-3
    diff = np.abs(u8.astype(np.int32) - want.astype(np.int32))
    print(f"values {diff.size}, differing {int((diff != 0).sum())}, of them exempt {int((diff != 0)[exempt].sum())}, "
          f"max difference {int(diff.max())}")
    assert diff.max() <= 1
    assert not (diff != 0)[~exempt].any()


def test_config2_shaped_input_against_the_oracle(dev):
    """256 x 256 LR x4, one Gaussian per LR pixel (config 2), dmax 0.1: a band of 256 rows of the 8-bit image against
    quantise(fp32 oracle).  Seed and colour scale were chosen on the CPU with the oracle alone: 5.3 % of its values are exempt
    (a smooth distribution gives 2 * 0.0265) and 99 % lie strictly inside (0.02, 0.98)."""
    from gsasr_amd import _cabi, synthetic
    from oracle import gs_oracle
    sig, xy, col, H, W = synthetic.kernel_inputs(256, 256, 4.0, seed=31)
    rows = (384, 640)
    ref = gs_oracle.forward_f32(sig.numpy(), xy.numpy(), col.numpy(), H, W, 0.1, rows=rows)
    exempt, inside = oracle_shares(ref)
    print(f"oracle: exempt share {exempt:.4f}, inside (0.02, 0.98) {inside:.4f}")
    assert exempt <= 0.08 and inside >= 0.50
    plan = _cabi.plan(sig.to(dev), xy.to(dev), col.to(dev), H, W, 0.1, flags=_cabi.FLAG_FORWARD_ONLY)
    got = _cabi.forward_u8(plan).cpu().numpy()
    against_oracle(got[rows[0]: rows[1]], ref)
    band = _cabi.plan(sig.to(dev), xy.to(dev), col.to(dev), H, W, 0.1, rows=rows, flags=_cabi.FLAG_FORWARD_ONLY)
    against_oracle(_cabi.forward_u8(band).cpu().numpy(), ref)


@pytest.mark.parametrize("path", RASTER, ids=[os.path.basename(p)[7:-4] for p in RASTER])
def test_golden_vectors_against_the_oracle(path, dev):
    """the reference-captured raster fixtures, narrow and wide kernels.  They are small and mostly background (1-80 % of their
    values inside (0.02, 0.98), colours up to 7.5), so the 50 % condition is asserted on the synthetic input above; the cap on
    the exempt share holds for each of them"""
    from gsasr_amd import _cabi
    from oracle import gs_oracle
    z = np.load(path)
    dmax = None if float(z["dmax"]) < 0 else float(z["dmax"])
    H, W = int(z["h"]), int(z["w"])
    ref = gs_oracle.forward_f32(z["sigmas"], z["coords"], z["colors"], H, W, dmax)
    exempt, inside = oracle_shares(ref)
    print(f"oracle: exempt share {exempt:.4f}, inside (0.02, 0.98) {inside:.4f}")
    assert exempt <= 0.08
    a, b, c = (torch.from_numpy(z[k]).float().contiguous().to(dev) for k in ("sigmas", "coords", "colors"))
    plan = _cabi.plan(a, b, c, H, W, dmax, flags=_cabi.FLAG_FORWARD_ONLY)
    for flag in (_cabi.FLAG_FWD_NARROW, _cabi.FLAG_FWD_WIDE):
        against_oracle(_cabi.forward_u8(plan, flags=flag).cpu().numpy(), ref)


if __name__ == "__main__":      # (test_store_is_exact_through_the_fine_forward: GSASR_SPLAT_DEV=1 GSASR_SPLAT_FWD8=1)
    sys.path.insert(0, ROOT)
    device = torch.device("cuda:0")
    for bounded in (True, False):
        fine_plan, fine_flag = kernel_case("fwd2-parts2", bounded, device)
        check_plan_exact(fine_plan, device, fine_flag)
    print("fwd8 exact")
