"""Bicubic imresize on the GPU (gsasr_imresize / gsasr_imresize_backward: csrc/splat_resize.hip) against the float64 restatement
and the reference's fixtures of tests/test_imresize.py.

Bars.  Forward, inputs in [0,1]: max(1e-6, 4 * d_ref) absolute against the float64 restatement, d_ref being the reference's own
recorded distance from it on the case (the reference is the yardstick; 4 covers another summation order of the taps: up to 66
on the first nine cases, 130, 258 and 402 on the three that stage more than one chunk), and that plus d_ref against the
reference's fixture.  Adjoint (ADJOINT_CASES, at most 66 taps): 1e-5 * max|grad_out| against the float64 dense A^T -- each pass
is a dot product of at most 66 fp32 terms with sum|w| <= 1.27, 66 * 6e-8 * 1.27 = 5e-6 per pass, two passes; there is no
reference backward (the reference function is no_grad).  <A x, y> = <x, A^T y> to 1e-5 relative.  Every case prints what it
measured.  Shapes are the fixtures' (the smallest that reach each path: p = 7, 13, 66, an upscale, no antialiasing, 2-D, and
p = 130, 258, 402 / 174) plus a padded batch of three sizes, a batch of 17 (past 16), and windows of larger tensors.  Wider
windows, every tile width and bars on each element's own scale: tests/test_imresize_wide_gpu.py."""
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
from test_imresize import CASES, adjoint_f64, bar_f64, case_input, case_scales, fixture, resize_f64, run_case      # noqa: E402

from gsasr_amd import _cabi      # noqa: E402
from gsasr_amd import gaussian_splatting as gsp      # noqa: E402
from gsasr_amd import resize as R      # noqa: E402

pytestmark = pytest.mark.gpu

ADJ_BAR = 1e-5
ADJOINT_CASES = ["53_to_48", "131x67_by_2p7", "416_to_26", "20x31_up_ceil"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the MI355X box)"
    return torch.device("cuda:0")


def to_dev(case, x, dev):
    """the case's input on the device in the kind the call takes: tensors only on the GPU, so a 2-D array goes as a 2-D tensor"""
    return torch.from_numpy(x).to(dev)


# ---- forward ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_forward_against_f64_and_reference(dev, name):
    case = CASES[name]
    ref, d_ref = fixture(name)
    x = case_input(case)
    want = resize_f64(x, case["out"], case_scales(case), case["aa"])
    got = run_case(case, to_dev(case, x, dev))
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == want.shape
    got = got.cpu().numpy()
    e64, eref = np.abs(got - want).max(), np.abs(got - ref).max()
    print(f"imresize {name}: |gpu - f64| {e64:.3e} (bar {bar_f64(d_ref):.3e}), |gpu - reference| {eref:.3e} "
          f"(bar {bar_f64(d_ref) + d_ref:.3e}), reference's own {d_ref:.3e}")
    assert e64 <= bar_f64(d_ref), name
    assert eref <= bar_f64(d_ref) + d_ref, name
    if name == "identity_48":
        assert np.array_equal(got, x)


def test_length_26_at_one_sixteenth_raises(dev):
    with pytest.raises(ValueError, match="beyond one reflection"):
        R.imresize(torch.rand(1, 26, 26, device=dev), 1 / 16)
    # ... and straight through the binding, the library's own check
    x, out = torch.rand(1, 1, 26, 26, device=dev), torch.empty(1, 1, 2, 2, device=dev)
    with pytest.raises(RuntimeError, match="beyond one reflection"):
        _cabi.imresize(x, out, (1 / 16, 1 / 16))


# ---- batch ------------------------------------------------------------------------------------------------------------
def padded_batch(sizes, C, dev, seed, fill=float("nan")):
    g = torch.Generator().manual_seed(seed)
    H, W = max(h for h, _ in sizes), max(w for _, w in sizes)
    x = torch.full((len(sizes), C, H, W), fill)
    for b, (h, w) in enumerate(sizes):
        x[b, :, :h, :w] = torch.rand(C, h, w, generator=g)
    return x.to(dev)


def test_padded_batch_equals_single_calls_and_never_reads_the_padding(dev):
    sizes = [(48, 48), (53, 53), (97, 97)]
    x = padded_batch(sizes, 3, dev, 21)
    y = R.imresize_batch(x, sizes, out_size=(48, 48))
    assert tuple(y.shape) == (3, 3, 48, 48) and bool(torch.isfinite(y).all())
    for b, (h, w) in enumerate(sizes):
        one = R.imresize_new(x[b, :, :h, :w], 48 / h, 48 / w)
        assert torch.equal(y[b], one), b
        want = resize_f64(x[b, :, :h, :w].cpu().numpy(), (48, 48), (48 / h, 48 / w))
        assert np.abs(y[b].cpu().numpy() - want).max() <= bar_f64(fixture(("identity_48", "53_to_48", "97_to_48")[b])[1])


def test_batch_of_17(dev):
    sizes = [(8 + b, 8 + b) for b in range(17)]
    x = padded_batch(sizes, 2, dev, 22)
    y = R.imresize_batch(x, sizes, out_size=(6, 7))
    assert bool(torch.isfinite(y).all())
    worst = 0.0
    for b, (h, w) in enumerate(sizes):
        want = resize_f64(x[b, :, :h, :w].cpu().numpy(), (6, 7), (6 / h, 7 / w))
        worst = max(worst, np.abs(y[b].cpu().numpy() - want).max())
        assert torch.equal(y[b], R.imresize_batch(x[b:b + 1, :, :h, :w].contiguous(), out_size=(6, 7))[0]), b
    print(f"batch of 17, 8x8 .. 24x24 -> 6x7: worst |gpu - f64| {worst:.3e}")
    # at most p = ceil(4 * 24 / 6) + 2 = 18 taps: two passes * (18 products + the weight's and the store's rounding) * 2^-24 * sum|w| 1.27
    assert worst <= 2 * 20 * 2.0 ** -24 * 1.27


def test_pitched_input_and_output(dev):
    """windows of larger tensors, read and written in place; what lies outside the output window stays"""
    g = torch.Generator().manual_seed(23)
    big = torch.rand(2, 3, 70, 90, generator=g).to(dev)
    x = big[:, :, 5:58, 7:60]                               # 53 x 53 at an odd offset
    canvas = torch.full((2, 3, 60, 64), -7.0, device=dev)
    out = canvas[:, :, 3:51, 9:57]
    _cabi.imresize(x, out, (48 / 53, 48 / 53))
    dense = R.imresize_batch(x.contiguous(), out_size=(48, 48))
    assert torch.equal(out, dense)
    mask = torch.ones_like(canvas, dtype=torch.bool)
    mask[:, :, 3:51, 9:57] = False
    assert bool((canvas[mask] == -7.0).all())
    want = resize_f64(x.cpu().numpy(), (48, 48), (48 / 53, 48 / 53))
    assert np.abs(dense.cpu().numpy() - want).max() <= bar_f64(fixture("53_to_48")[1])
    # the public call on a window (strides kept), and the backward into a window
    assert torch.equal(R.imresize_batch(x, out_size=(48, 48)), dense)
    go = torch.rand(2, 3, 60, 64, generator=g).to(dev)[:, :, 3:51, 9:57]
    gcanvas = torch.full((2, 3, 70, 90), 5.0, device=dev)
    gx = gcanvas[:, :, 5:58, 7:60]
    _cabi.imresize(gx, go, (48 / 53, 48 / 53), backward=True)
    want = adjoint_f64(go.cpu().numpy(), (53, 53), (48 / 53, 48 / 53))
    assert np.abs(gx.cpu().numpy() - want).max() <= ADJ_BAR * float(go.max())
    gmask = torch.ones_like(gcanvas, dtype=torch.bool)
    gmask[:, :, 5:58, 7:60] = False
    assert bool((gcanvas[gmask] == 5.0).all())


# ---- adjoint ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ADJOINT_CASES)
def test_adjoint_against_dense_transpose(dev, name):
    case = CASES[name]
    x = torch.from_numpy(case_input(case)).to(dev).requires_grad_(True)
    y = run_case(case, x)
    go = torch.from_numpy(np.random.default_rng(case["seed"] + 100).random(tuple(y.shape), dtype=np.float32) * 2 - 1).to(dev)
    gx, = torch.autograd.grad(y, x, go)
    want = adjoint_f64(go.cpu().numpy(), (case["h"], case["w"]), case_scales(case), case["aa"])
    err, top = np.abs(gx.cpu().numpy() - want).max(), float(go.abs().max())
    lhs = float((y.detach().double() * go.double()).sum())
    rhs = float((x.detach().double() * gx.double()).sum())
    scale = float((y.detach().double().abs() * go.double().abs()).sum())
    print(f"adjoint {name}: |grad_in - A^T g| {err:.3e} (bar {ADJ_BAR * top:.3e}), <Ax,y> {lhs:.9e} <x,A^T y> {rhs:.9e} "
          f"(relative to sum|Ax||y| {abs(lhs - rhs) / scale:.3e})")
    assert err <= ADJ_BAR * top, name
    assert abs(lhs - rhs) <= ADJ_BAR * scale, name


def test_accumulate_adds(dev):
    g = torch.Generator().manual_seed(24)
    go = torch.rand(1, 3, 48, 48, generator=g).to(dev)
    base = torch.rand(1, 3, 53, 53, generator=g).to(dev)
    stored = torch.empty(1, 3, 53, 53, device=dev)
    _cabi.imresize(stored, go, (48 / 53, 48 / 53), backward=True)
    acc = base.clone()
    _cabi.imresize(acc, go, (48 / 53, 48 / 53), backward=True, accumulate=True)
    assert torch.equal(acc, base + stored)


def test_batch_backward_leaves_the_padding_untouched_and_autograd_zeroes_it(dev):
    sizes = [(48, 48), (53, 53), (97, 97)]
    scales = [(48 / h, 48 / w) for h, w in sizes]
    go = torch.rand(3, 3, 48, 48, generator=torch.Generator().manual_seed(25)).to(dev)
    # the C call: only the samples' own pixels are written
    gx = torch.full((3, 3, 97, 97), 9.0, device=dev)
    _cabi.imresize(gx, go, scales, sizes, backward=True)
    for b, (h, w) in enumerate(sizes):
        assert bool((gx[b, :, h:, :] == 9.0).all()) and bool((gx[b, :, :, w:] == 9.0).all())
        want = adjoint_f64(go[b].cpu().numpy(), (h, w), scales[b])
        assert np.abs(gx[b, :, :h, :w].cpu().numpy() - want).max() <= ADJ_BAR * float(go.max())
    # autograd: zeros there, the same numbers on the samples (NaN padding in the input does not leak)
    x = padded_batch(sizes, 3, dev, 26).requires_grad_(True)
    ga, = torch.autograd.grad(R.imresize_batch(x, sizes, out_size=(48, 48)), x, go)
    for b, (h, w) in enumerate(sizes):
        assert torch.equal(ga[b, :, :h, :w], gx[b, :, :h, :w])
        assert float(ga[b, :, h:, :].abs().sum()) == 0.0 and float(ga[b, :, :, w:].abs().sum()) == 0.0


def test_loss_through_resize_and_splat_reaches_the_gaussians(dev):
    """LR consistency: splat 48 x 48 from N = 16 * 12^2 Gaussians, downsample to 12 x 12, compare with an LR target"""
    g = torch.Generator().manual_seed(27)
    n = 16 * 12 * 12
    p = 0.5 * torch.randn(n, 9, generator=g)
    p[..., 7:9] = torch.rand(n, 2, generator=g)
    p = p.to(dev).requires_grad_(True)
    lr = torch.rand(1, 3, 12, 12, generator=g).to(dev)
    hr = gsp.generate_2D_gaussian_splatting_step((48, 48), p, 4.0, [4.0, 4.0])
    assert tuple(hr.shape) == (3, 48, 48)
    down = R.imresize_batch(hr[None], out_size=(12, 12))
    loss = (down - lr).abs().mean()
    loss.backward()
    assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().sum()) > 0
    # the chain rule through the resize is the adjoint of the loss' gradient
    gd = (torch.sign(down.detach() - lr) / down.numel())
    want = adjoint_f64(gd[0].cpu().numpy(), (48, 48), (0.25, 0.25))
    hr2 = hr.detach().clone().requires_grad_(True)
    (R.imresize_batch(hr2[None], out_size=(12, 12)) - lr).abs().mean().backward()
    assert np.abs(hr2.grad.cpu().numpy() - want).max() <= ADJ_BAR * float(gd.abs().max())


# ---- determinism, capture, plain C ---------------------------------------------------------------------------------------
def test_two_calls_give_identical_bits(dev):
    sizes = [(48, 48), (53, 53), (97, 97)]
    x = padded_batch(sizes, 3, dev, 28, fill=0.0).requires_grad_(True)
    go = torch.rand(3, 3, 48, 48, generator=torch.Generator().manual_seed(29)).to(dev)
    runs = []
    for _ in range(2):
        y = R.imresize_batch(x, sizes, out_size=(48, 48))
        gx, = torch.autograd.grad(y, x, go)
        runs.append((y.detach().clone(), gx.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_captured_call_equals_eager(dev):
    g = torch.Generator().manual_seed(30)
    static_x = torch.rand(2, 3, 53, 53, generator=g).to(dev).requires_grad_(True)
    static_go = torch.rand(2, 3, 48, 48, generator=g).to(dev)
    new_x, new_go = torch.rand(2, 3, 53, 53, generator=g).to(dev), torch.rand(2, 3, 48, 48, generator=g).to(dev)

    def step():
        y = R.imresize_batch(static_x, out_size=(48, 48))
        gx, = torch.autograd.grad(y, static_x, static_go)
        return y, gx

    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y_g, gx_g = step()
    with torch.no_grad():
        static_x.copy_(new_x)
        static_go.copy_(new_go)
    graph.replay()
    torch.cuda.synchronize()
    y_e, gx_e = step()
    assert torch.equal(y_g, y_e) and torch.equal(gx_g, gx_e)
    want = resize_f64(new_x.cpu().numpy(), (48, 48), (48 / 53, 48 / 53))
    assert np.abs(y_g.detach().cpu().numpy() - want).max() <= bar_f64(fixture("53_to_48")[1])


def test_autocast_boundary(dev):
    x = torch.rand(1, 3, 53, 53, generator=torch.Generator().manual_seed(31)).to(dev)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = R.imresize_batch(x.bfloat16(), out_size=(48, 48))
    assert y.dtype == torch.float32
    assert torch.equal(y, R.imresize_batch(x.bfloat16().float(), out_size=(48, 48)))


def test_c_program_resize(tmp_path):
    """the resize from plain C (tests/c_abi/c_abi_resize_check.c): built with gcc against libgsasr_splat.so, run on the GPU"""
    lib = _cabi.LIB_PATH
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc and os.path.exists(lib)
    exe = str(tmp_path / "c_abi_resize_check")
    subprocess.check_call([cc, "-O1", "-std=c11", "-D__HIP_PLATFORM_AMD__", f"-I{rocm}/include", f"-I{ROOT}/include",
                           os.path.join(HERE, "c_abi", "c_abi_resize_check.c"), lib, f"-L{rocm}/lib", "-lamdhip64", "-lm",
                           f"-Wl,-rpath,{os.path.dirname(lib)}", f"-Wl,-rpath,{rocm}/lib", "-o", exe])
    out = subprocess.run(["timeout", "-k", "10", "120", exe], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "C-ABI RESIZE CHECK OK" in out.stdout, out.stdout + out.stderr
