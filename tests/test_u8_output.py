"""8-bit image output, the part that runs without a GPU: the host API on CPU tensors, the tiled driver with `out_uint8`, the
new C entry points' declarations and their argument checks (the library loads and validates without a device).

`quantise` is the reference's own epilogue written out (inference_paper.py:134-140, basicsr/utils/img_util.py:73-96):
x[:, :, :gt_h, :gt_w] -> .cpu().clamp_(0, 1) -> [[2, 1, 0]] + transpose to HWC -> (x * 255.0).round().astype(uint8)."""
import ctypes
import os
import re
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from gsasr_amd import _cabi, gaussian_splatting as gsp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def quantise(x, crop=None, bgr=False):
    """planar float [3,H,W] (or [1,3,H,W]) torch tensor -> uint8 [h, w, 3] numpy, as the reference's inference scripts do"""
    x = x.detach().reshape(3, x.shape[-2], x.shape[-1])
    if crop is not None:
        x = x[:, :crop[0], :crop[1]]
    a = x.cpu().clone().clamp_(0, 1).numpy()
    if bgr:
        a = a[[2, 1, 0]]
    a = a.transpose(1, 2, 0)
    return (a * 255.0).round().astype(np.uint8)


@pytest.mark.parametrize("crop", [None, (33, 45), (1, 1)], ids=["full", "crop33x45", "crop1x1"])
@pytest.mark.parametrize("bgr", [False, True], ids=["rgb", "bgr"])
def test_step_uint8_on_cpu_equals_the_quantised_step(crop, bgr):
    """a golden prologue case on CPU tensors: the uint8 entry point == quantise(the float entry point)"""
    z = np.load(os.path.join(GOLDEN, "prologue_s4_40x52_fix.npz"))
    sc, size = float(z["scale"]), z["sr_size"].tolist()
    p = torch.from_numpy(z["gs_parameters"])
    # brighter colours, so that the upper clamp fires (sums above 1) next to black pixels (the host API's colours are >= 0:
    # the lower clamp never does here)
    p = p.clone()
    p[:, 3:7] += 3.0
    sm = torch.tensor([sc, sc])
    ref = gsp.generate_2D_gaussian_splatting_step(size, p, sc, sm, cuda_rendering=False)
    assert float(ref.max()) > 1.0 and float(ref.min()) < 0.5 / 255
    got = gsp.generate_2D_gaussian_splatting_step_uint8(size, p, sc, sm, crop=crop, bgr=bgr)
    want = quantise(ref, crop, bgr)
    assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape and not got.requires_grad
    assert np.array_equal(got.numpy(), want)
    assert len(np.unique(want)) > 1 or crop == (1, 1)


def test_step_uint8_keeps_the_step_entry_points_checks():
    p = torch.zeros(4, 9)
    with pytest.raises(AssertionError):
        gsp.generate_2D_gaussian_splatting_step_uint8((8, 8), p, 4.0, torch.tensor([4.0, 3.0]))
    with pytest.raises(UnboundLocalError):
        gsp.generate_2D_gaussian_splatting_step_uint8((8, 8), p, 4.0, torch.tensor([4.0, 4.0]), mode="bogus")
    with pytest.raises(ValueError):
        gsp.generate_2D_gaussian_splatting_step_uint8((8, 8), p, 4.0, torch.tensor([4.0, 4.0]), crop=(9, 8))


def test_quantise_uint8_rounds_half_to_even_and_maps_nan_to_zero():
    v = torch.tensor([0.5 / 255, 1.5 / 255, 2.5 / 255, -1.0, 2.0, float("nan"), 1.0, 0.0]).double()
    img = v.float().reshape(1, 1, -1).expand(3, 1, -1)
    got = gsp.quantise_uint8(img)[0, :, 0].tolist()
    want = (np.clip(np.nan_to_num(img[0, 0].numpy()), 0, 1) * np.float32(255.0)).round().astype(np.uint8).tolist()
    assert got == want and got[3:] == [0, 255, 0, 255, 0]


def _tiled(path, **kw):
    import tiled_models
    from gsasr_amd.split_and_joint_image import split_and_joint_image
    z = np.load(path)
    sc = float(z["scale"])
    return split_and_joint_image(torch.from_numpy(z["lq"]), sc, int(z["split_size"]), int(z["overlap_size"]),
                                 tiled_models.model_g, tiled_models.model_fea2gs, torch.tensor([sc, sc]),
                                 crop_size=int(z["crop_size"]), cuda_rendering=False, **kw)


@pytest.mark.parametrize("name", ["tiled_int_s2_20x26.npz", "tiled_frac_s2p5_18x22.npz"])
@pytest.mark.parametrize("bgr", [False, True], ids=["rgb", "bgr"])
def test_tiled_driver_uint8_equals_its_quantised_float_result(name, bgr):
    """an integer and a fractional scale (the paste rule's irregular case): pasting quantised tiles == quantising the canvas"""
    path = os.path.join(GOLDEN, name)
    ref = _tiled(path)
    got = _tiled(path, out_uint8=True, bgr=bgr)
    want = quantise(ref, None, bgr)
    assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape
    assert np.array_equal(got.numpy(), want)
    assert want.max() > 0


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _tiled_worker(rank, world, port, path, out):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        out[rank] = _tiled(path, distribute=True, out_uint8=True).numpy()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("name", ["tiled_int_s2_20x26.npz", "tiled_frac_s2p5_18x22.npz"])
def test_tiled_driver_uint8_over_two_ranks(name):
    """gloo, world 2: the all_gather moves uint8 stacks and every rank ends with quantise(its own float result)"""
    path = os.path.join(GOLDEN, name)
    want = quantise(_tiled(path))
    out = mp.Manager().dict()
    mp.spawn(_tiled_worker, args=(2, _free_port(), path, out), nprocs=2, join=True)
    for r in range(2):
        assert out[r].dtype == np.uint8 and np.array_equal(out[r], want)


U8_SYMBOLS = ("gsasr_splat_forward_u8", "gsasr_step_forward_u8", "gsasr_step_forward_sm_u8")


def test_header_and_exports_agree_with_the_u8_symbols():
    hdr = open(os.path.join(ROOT, "include", "gsasr_splat.h")).read()
    assert re.search(r"#define\s+GSASR_U8_SWAP_RB\s+1u", hdr) and _cabi.U8_SWAP_RB == 1
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(gsasr_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(_cabi.EXPORTS), declared ^ set(_cabi.EXPORTS)
    L = ctypes.CDLL(_cabi.LIB_PATH)
    for name in U8_SYMBOLS:
        assert name in declared and hasattr(L, name), name
    assert _cabi.lib().gsasr_abi_version() == 7        # new entry points only: struct and version stay
    assert ctypes.sizeof(_cabi.Dims) == 64


BAD_U8 = {
    "crop_rows < 1": dict(rows=0),
    "crop_cols < 1": dict(cols=-3),
    "crop taller than the grid": dict(rows=41),
    "crop wider than the grid": dict(cols=53),
    "pitch < 3 * crop_cols": dict(pitch=3 * 52 - 1),
    "null out": dict(out=None),
    "unknown u8_flags": dict(flags=2),
}


@pytest.mark.parametrize("case", sorted(BAD_U8), ids=lambda c: c.replace(" ", "_"))
@pytest.mark.parametrize("entry", U8_SYMBOLS)
def test_u8_argument_errors_without_a_gpu(entry, case):
    """every GSASR_ERR_ARG case of the header, through all three entry points; the checks come before anything touches the
    workspace or the device, so a host buffer stands in for the pointers (it is never dereferenced)"""
    L = _cabi.lib()
    d = _cabi.make_dims(64, 40, 52, 0.1, flags=_cabi.FLAG_FORWARD_ONLY)
    buf = ctypes.create_string_buffer(4096 + 256)
    ws = (ctypes.addressof(buf) + 255) & ~255
    a = dict(rows=40, cols=52, pitch=3 * 52, out=ws, flags=0)
    a.update(BAD_U8[case])
    tail = (ctypes.byref(d), ws, 4096, a["out"], a["rows"], a["cols"], a["pitch"], a["flags"], None)
    if entry == "gsasr_splat_forward_u8":
        rc = L.gsasr_splat_forward_u8(*tail)
    elif entry == "gsasr_step_forward_u8":
        rc = L.gsasr_step_forward_u8(ws, ws, *tail)
    else:
        rc = L.gsasr_step_forward_sm_u8(ws, ws, 2, 1.2, None, *tail)
    assert rc == -1, (rc, L.gsasr_last_error())                 # GSASR_ERR_ARG
    assert L.gsasr_last_error()


def test_u8_good_arguments_get_past_the_argument_check_without_a_gpu():
    """the same call with valid u8 arguments is refused for its workspace instead (never planned / too small), not its arguments"""
    L = _cabi.lib()
    d = _cabi.make_dims(64, 40, 52, 0.1, flags=_cabi.FLAG_FORWARD_ONLY)
    buf = ctypes.create_string_buffer(4096 + 256)
    ws = (ctypes.addressof(buf) + 255) & ~255
    tail = (ctypes.byref(d), ws, 4096, ws, 33, 45, 3 * 45 + 7, _cabi.U8_SWAP_RB, None)
    assert L.gsasr_splat_forward_u8(*tail) == -3                 # GSASR_ERR_PLAN
    assert L.gsasr_step_forward_u8(ws, ws, *tail) == -2          # GSASR_ERR_WORKSPACE
    bad = _cabi.make_dims(64, 1, 52, 0.1)
    assert L.gsasr_splat_forward_u8(ctypes.byref(bad), *tail[1:]) == -1

