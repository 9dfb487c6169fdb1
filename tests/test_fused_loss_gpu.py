"""The pixel loss fused into the forward's store, on the GPU (gsasr_splat_forward_loss, gsasr_step_forward_loss,
generate_2D_gaussian_splatting_loss / _batch_loss).

The formulas are basicsr/losses/basic_loss.py:14-25 (|d|, d^2, sqrt(d^2 + eps); reduction='mean' times loss_weight), the batch
form the loop of basicsr/models/gsasr_model.py:213-235; `tests/test_fused_loss.py::loss_f64` restates them in float64.

Bars, with their sources:
  store      grad_img against c_b * phi'(v - t) formed in torch from the float image OF THE SAME CALL (the finished pixels the kernel
             held in registers): 1e-6 of the tensor's max-abs for MSE and Charbonnier (both sides are at most four fp32 roundings
             of the same operands, ~2.4e-7), exactly +-c_b / 0 for L1; the image `array_equal` to the plain forward's where the
             forward is reproducible (`separated` Gaussians: one term per pixel)
  loss       1e-5 relative against the float64 sum over that image (non-negative terms: a per-lane sum of <= 12 terms, a 6-level
             wave tree and a double reduce are bounded near 2e-6); two calls on one plan return the same bits
  gradients  the project's own (tests/test_hip_parity.py): 2e-4 of the tensor's max-abs AND per Gaussian 5e-4 + 5e-6 / sqrt(1 -
             rho^2) of its row
Sign conditioning: L1 and Charbonnier with eps = 1e-12 have a gradient that is a sign; their targets are t = v_ref + s * u with
s = +-1 and u uniform in [1e-2, 0.5], so every |d| is 100 x the 1e-4 image bar and no pixel is excluded from any comparison."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):      # (also run as a script: test_store_is_exact_through_the_fine_forward)
    if _p not in sys.path:
        sys.path.insert(0, _p)
import gradbars  # noqa: E402
from test_fused_loss import loss_f64  # noqa: E402
from test_u8_output_gpu import KERNELS, TAU, box_dmax, kernel_case, raw_parameters, separated  # noqa: E402

pytestmark = pytest.mark.gpu
KINDS = ("l1", "mse", "charbonnier")
GRAD_RTOL = 2e-4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the MI355X box)"
    return torch.device("cuda:0")


def coef(weight, h, w, batch=1, reduction="mean"):
    """c_b as the header defines it: one fp32 division of the weight by the integer product"""
    return np.float32(weight) if reduction == "sum" else np.float32(weight) / np.float32(3 * h * w * batch)


def torch_grad(v, t, kind, c, eps):
    """c * phi'(v - t) in fp32 torch, the expression of the header"""
    d = v - t
    c = torch.tensor(float(c), dtype=torch.float32, device=v.device)
    if kind == "l1":
        return torch.where(d > 0, c, torch.where(d < 0, -c, torch.zeros_like(c))).expand_as(d)
    if kind == "mse":
        return c * (2.0 * d)
    return c * (d / torch.sqrt(d * d + eps))


def torch_loss(image, target, kind, weight, eps, reduction):
    """basic_loss.py:14-25 as differentiable torch ops: the loss of the unfused reference paths"""
    d = image - target
    phi = d.abs() if kind == "l1" else d * d if kind == "mse" else torch.sqrt(d * d + eps)
    return weight * (phi.mean() if reduction == "mean" else phi.sum())


def conditioned_target(v, seed, zeros=False):
    """t = v + s * u, s = +-1, u uniform in [1e-2, 0.5]: no |v - t| below 1e-2 (with `zeros`, every 11th value is v itself: d = 0)"""
    g = torch.Generator().manual_seed(seed)
    u = (torch.rand(v.shape, generator=g) * 0.49 + 0.01).to(v.device)
    s = (torch.randint(0, 2, v.shape, generator=g) * 2 - 1).to(v.device)
    t = v + s * u
    if zeros:
        flat = t.reshape(-1)
        flat[::11] = v.reshape(-1)[::11]
    return t.contiguous()


def check_store(plan, flag, dev, name=""):
    """test 1 on one plan: every kind, both normalisations, both target and gradient layouts"""
    from gsasr_amd import _cabi
    d = plan.dims
    H, W = d.h, d.w
    img = torch.full((H, W, 3), float("nan"), device=dev)
    _cabi.forward(plan, img, overwrite=True, flags=flag)
    assert bool(torch.isfinite(img).all()) and float(img.abs().max()) > 1.0
    natural = torch.rand(H, W, 3, generator=torch.Generator().manual_seed(H + W)).to(dev)
    worst = {"grad": 0.0, "loss": 0.0}
    for n, kind in enumerate(KINDS):
        for reduction in ("mean", "sum"):
            chw = bool((n + (reduction == "sum")) & 1)       # planar / interleaved target and image
            grad_chw = not chw if kind != "mse" else chw     # ... and the gradient's layout, independently
            weight, eps = 0.75, 1e-6
            t_hwc = conditioned_target(img, 3 * n + 1, zeros=True) if kind == "l1" else natural
            t = t_hwc.permute(2, 0, 1).contiguous() if chw else t_hwc
            args = (_cabi.LOSS_KINDS[kind], _cabi.LOSS_NORMS[reduction], weight, eps)
            loss, grad, stored = _cabi.forward_loss(plan, t, *args, chw=chw, grad_chw=grad_chw, want_image=True, flags=flag)
            again, _, none = _cabi.forward_loss(plan, t, *args, chw=chw, want_grad=False, flags=flag)
            assert none is None
            stored_hwc = stored.permute(1, 2, 0) if chw else stored
            assert np.array_equal(stored_hwc.cpu().numpy(), img.cpu().numpy()), (name, kind, reduction)
            assert np.array_equal(loss.cpu().numpy(), again.cpu().numpy()), (name, kind, reduction)     # the same bits
            assert float(loss[0]) == float(loss[1])
            c = coef(weight, H, W, 1, reduction)
            want = torch_grad(img, t_hwc, kind, c, eps)
            got = grad.permute(1, 2, 0) if grad_chw else grad
            if kind == "l1":
                assert np.array_equal(got.cpu().numpy(), want.cpu().numpy()), (name, reduction)
                vals = set(np.unique(got.cpu().numpy()).tolist())
                assert vals == {float(c), -float(c), 0.0}, vals
            else:
                err = float((got - want).abs().max()) / float(want.abs().max())
                worst["grad"] = max(worst["grad"], err)
                assert err <= 1e-6, (name, kind, reduction, err)
            ref, _ = loss_f64(img.cpu().numpy(), t_hwc.cpu().numpy(), kind, weight, eps, reduction)
            rel = abs(float(loss[0]) - ref) / ref
            worst["loss"] = max(worst["loss"], rel)
            assert rel <= 1e-5, (name, kind, reduction, rel, float(loss[0]), ref)
    print(f"{name}: grad max err {worst['grad']:.3e} of max-abs, loss max rel err {worst['loss']:.3e}")
    return worst


@pytest.mark.parametrize("dmax_on", [True, False], ids=["bounded", "unbounded"])
@pytest.mark.parametrize("name", sorted(KERNELS))
def test_store_is_exact_through_every_forward_kernel(name, dmax_on, dev):
    """Measured on an MI355X over all twelve kernel cases, the fine forward and both ops: MSE / Charbonnier gradient at most
    1.8e-7 of the tensor's max-abs (bar 1e-6), L1 exact, loss at most 5.7e-8 relative to the float64 sum (bar 1e-5), images and
    repeated losses bit-equal."""
    plan, flag = kernel_case(name, dmax_on, dev, forward_only=(len(name) % 2 == 0))
    check_store(plan, flag, dev, name)


def test_store_is_exact_through_the_fine_forward():
    """k_render_fwd8 sits behind a development switch that is read once per process: a child process with the switch set runs
    the sparse case of this file"""
    env = dict(os.environ, GSASR_SPLAT_DEV="1", GSASR_SPLAT_FWD8="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    print(r.stdout[-1500:])
    assert r.returncode == 0 and "fwd8 loss exact" in r.stdout and r.stdout.count("fwd8 partials 4096") == 2, (r.stdout[-1500:], r.stderr[-1500:])


# ---- (2) sign conditioning on overlapping Gaussians --------------------------------------------------------------------
@pytest.mark.parametrize("case", [(64, 64, 4.0, 1), (32, 32, 4.0, 16)], ids=["config2-shaped", "16-per-LR-px"])
@pytest.mark.parametrize("dmax", [0.1, None], ids=["bounded", "unbounded"])
def test_dense_input_signs_and_natural_targets(case, dmax, dev):
    """overlapping Gaussians (sums in whatever order the waves ran): the gradient and the loss against the image the same call
    stored.  L1 and Charbonnier (eps = 1e-12) on sign-conditioned targets around the library's own float image of ANOTHER call --
    every pixel's sign is decided, none is excluded --, MSE and Charbonnier (eps = 1e-6) on natural targets in [0, 1]."""
    from gsasr_amd import _cabi, synthetic
    h_lr, w_lr, scale, gpp = case
    sig, xy, col, H, W = synthetic.kernel_inputs(h_lr, w_lr, scale, seed=61, gpp=gpp)
    plan = _cabi.plan(sig.to(dev), xy.to(dev), col.to(dev), H, W, dmax)
    v_ref = torch.empty(H, W, 3, device=dev)
    _cabi.forward(plan, v_ref, overwrite=True)
    natural = torch.rand(H, W, 3, generator=torch.Generator().manual_seed(5)).to(dev)
    for kind, eps, t in (("l1", 1e-12, conditioned_target(v_ref, 1)), ("charbonnier", 1e-12, conditioned_target(v_ref, 2)),
                         ("mse", 1e-12, natural), ("charbonnier", 1e-6, natural)):
        loss, grad, img = _cabi.forward_loss(plan, t, _cabi.LOSS_KINDS[kind], 0, 1.0, eps, want_image=True)
        assert float((img - v_ref).abs().max()) <= 2e-5 * max(1.0, float(v_ref.abs().max()))      # the same sums in another order
        c = coef(1.0, H, W)
        want = torch_grad(img, t, kind, c, eps)
        if kind == "l1":
            assert np.array_equal(grad.cpu().numpy(), want.cpu().numpy())
            assert np.array_equal(grad.cpu().numpy(), torch_grad(v_ref, t, kind, c, eps).cpu().numpy())       # ... of either image
            assert not (grad == 0).any()
        else:
            err = float((grad - want).abs().max()) / float(want.abs().max())
            print(f"{kind} eps={eps}: grad max err {err:.3e} of max-abs")
            assert err <= 1e-6, (kind, eps, err)
        ref, _ = loss_f64(img.cpu().numpy(), t.cpu().numpy(), kind, 1.0, eps)
        assert abs(float(loss[0]) - ref) <= 1e-5 * ref, (kind, float(loss[0]), ref)


# ---- (3) ragged batch ----------------------------------------------------------------------------------------------------
SIZES = [(200, 256), (131, 190), (192, 77), (256, 250), (97, 101)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cap", [-1, 256], ids=["search", "lists"])
def test_ragged_batch_against_the_reference_loop(cap, kind, dev):
    """five samples of different sizes, none a multiple of 8 or 16 in both directions: L, L_b and grad_img against the loop of
    gsasr_model.py:213-235 on the library's own batched float image; the target is read in place from [B,3,Hmax+3,Wmax]; the
    gradient buffer is untouched outside each sample's rectangle"""
    from gsasr_amd import _cabi
    B, n_per = len(SIZES), 24
    parts = [separated(h, w, n_per, seed=70 + b) for b, (h, w) in enumerate(SIZES)]
    sig, xy, col = (torch.cat([p[k] for p in parts]).to(dev) for k in range(3))
    plan = _cabi.plan(sig, xy, col, 0, 0, 40.0 / 255, cutoff=TAU, list_cap=cap, sizes=SIZES)
    d = plan.dims
    assert d.batch == B and d.slot == 256 and d.w == 256
    target = torch.rand(B, 3, 256 + 3, 256, generator=torch.Generator().manual_seed(3)).to(dev)
    weight, eps = 1.3, 1e-6
    for reduction in ("mean", "sum"):
        for grad_chw in (True, False):
            canary = torch.full((B, 3, d.slot, d.w) if grad_chw else (B * d.slot, d.w, 3), -77.0, device=dev)
            loss, grad, img = _cabi.forward_loss(plan, target, _cabi.LOSS_KINDS[kind], _cabi.LOSS_NORMS[reduction], weight, eps, chw=True,
                                                 grad_chw=grad_chw, want_image=True, grad=canary)
            assert grad.data_ptr() == canary.data_ptr()
            plain = torch.full((B * d.slot, d.w, 3), float("nan"), device=dev)
            _cabi.forward(plan, plain, overwrite=True)
            assert np.array_equal(img.cpu().numpy(), plain.view(B, d.slot, d.w, 3).permute(0, 3, 1, 2).cpu().numpy())
            g = grad if grad_chw else grad.view(B, d.slot, d.w, 3).permute(0, 3, 1, 2)
            total, outside = 0.0, torch.ones_like(g, dtype=torch.bool)
            for b, (h, w) in enumerate(SIZES):
                out, gt = img[b, :, :h, :w], target[b, :, :h, :w]                   # gsasr_model.py:216-231
                ref_b, _ = loss_f64(out.cpu().numpy(), gt.cpu().numpy(), kind, weight, eps, reduction)
                total += ref_b
                assert abs(float(loss[1 + b]) - ref_b) <= 1e-5 * ref_b, (b, float(loss[1 + b]), ref_b)
                want = torch_grad(out, gt, kind, coef(weight, h, w, B, reduction), eps)
                if kind == "l1":
                    assert np.array_equal(g[b, :, :h, :w].cpu().numpy(), want.cpu().numpy()), b
                else:
                    assert float((g[b, :, :h, :w] - want).abs().max()) <= 1e-6 * float(want.abs().max()), b
                outside[b, :, :h, :w] = False
            total = total / B if reduction == "mean" else total
            assert abs(float(loss[0]) - total) <= 1e-5 * total
            assert bool((g[outside] == -77.0).all())                              # canaries around the valid rectangles


# ---- (4) parameter gradients ----------------------------------------------------------------------------------------------
def rho_of(p):
    return 0.999999 * np.tanh(p.detach().cpu().numpy().reshape(-1, 9)[:, 2].astype(np.float64))


def check_param_grads(got, want, p, what="", independent=False, min_share=0.0):
    """the project's bars on d/d gs_parameters [.., 9]; `independent`: `want` is the float64 truth, not the unfused path of this
    build -- then every column is held to its own bar as well, element by element (tests/gradbars.py)"""
    g, w = got.detach().cpu().numpy().reshape(-1, 9).astype(np.float64), want.detach().cpu().numpy().reshape(-1, 9).astype(np.float64)
    assert np.isfinite(g).all(), what
    rel = float(np.abs(g - w).max() / max(1e-30, np.abs(w).max()))
    kappa = np.maximum(1.0 - rho_of(p) ** 2, 1e-12)[:, None]
    tol = (5e-4 + 5e-6 / np.sqrt(kappa)) * np.abs(w).max(axis=1, keepdims=True) + 1e-5 * np.abs(w).max() + 1e-30
    bad = np.abs(g - w) > tol
    print(f"{what}: rel err {rel:.3e} of max-abs {np.abs(w).max():.3e}, rows over their bar {int(bad.any(axis=1).sum())}")
    assert rel <= GRAD_RTOL, (what, rel)
    assert not bad.any(), (what, int(np.argwhere(bad)[0][0]))
    if independent:
        gradbars.check(g, w, rho_of(p), gradbars.RAW_GROUPS, min_share, what, list(gradbars.RAW_NAMES))


class forced_backward:
    def __init__(self, kernel):
        self.kernel = kernel

    def __enter__(self):
        from gsasr_amd import gaussian_splatting as gsp
        self.old, gsp.BACKWARD_KERNEL = gsp.BACKWARD_KERNEL, self.kernel

    def __exit__(self, *a):
        from gsasr_amd import gaussian_splatting as gsp
        gsp.BACKWARD_KERNEL = self.old


def unfused_single(p, H, W, scale, sm, t, kind, weight, eps, reduction, window, dmax_kw):
    from gsasr_amd import gaussian_splatting as gsp
    q = p.detach().clone().requires_grad_(True)
    if window is None:
        img = gsp.generate_2D_gaussian_splatting_step((H, W), q, scale, sm, **dmax_kw)
    else:
        img = gsp.generate_2D_gaussian_splatting_view((H, W), q, scale, sm, window, **dmax_kw)
    value = torch_loss(img, t, kind, weight, eps, reduction)
    value.backward()
    return value.detach(), q.grad, img.detach()


@pytest.mark.parametrize("kernel", ["gaussian", "tile", "home"])
@pytest.mark.parametrize("source", ["step_size", "scale_modify"])
@pytest.mark.parametrize("bounded", [True, False], ids=["bounded", "unbounded"])
def test_parameter_gradients_single_image_and_window(kernel, source, bounded, dev):
    """fused vs unfused of the same build (plain step / view + the torch loss + autograd), every backward kernel, both step-size
    conventions, both ops; a whole image and a window; sign-conditioned targets for L1 and Charbonnier (eps = 1e-12)"""
    from gsasr_amd import gaussian_splatting as gsp, synthetic
    H, W, scale = 128, 96, 4.0
    p = synthetic.gs_parameters(32, 24, seed=11).to(dev).requires_grad_(True)
    sm = torch.tensor([scale, scale], device=dev) if source == "scale_modify" else (scale, scale)
    dmax_kw = dict(dmax=0.15) if bounded else dict(if_dmax=False)
    with forced_backward(kernel):
        for window in (None, (19, 7, 70, 61)):
            _, _, v_ref = unfused_single(p, H, W, scale, sm, torch.zeros(3, *(window[2:] if window else (H, W)), device=dev), "mse",
                                         1.0, 0.0, "mean", window, dmax_kw)
            for kind, eps, reduction in (("l1", 1e-12, "mean"), ("charbonnier", 1e-12, "sum"), ("mse", 1e-12, "mean")):
                t = conditioned_target(v_ref, 7) if kind != "mse" else torch.rand_like(v_ref)
                want_v, want_g, _ = unfused_single(p, H, W, scale, sm, t, kind, 0.6, eps, reduction, window, dmax_kw)
                p.grad = None
                value = gsp.generate_2D_gaussian_splatting_loss((H, W), p, scale, sm, t, loss=kind, loss_weight=0.6, eps=eps,
                                                                reduction=reduction, window=window, **dmax_kw)
                assert value.dim() == 0 and value.requires_grad
                value.backward()
                assert abs(float(value.detach()) - float(want_v)) <= 2e-5 * abs(float(want_v))
                check_param_grads(p.grad, want_g, p, f"{kernel} {source} {kind} window={window}")
    gsp.deferred_asserts.flush()


def batch_case(dev, seed=0, n_lr=(20, 24), gpp=1):
    from gsasr_amd import synthetic
    sizes = [(96, 80), (61, 77), (80, 45), (53, 96)]
    B = len(sizes)
    p = torch.stack([synthetic.gs_parameters(*n_lr, seed=seed + b, gpp=gpp) for b in range(B)]).to(dev)
    return sizes, p, [4.0] * B


def unfused_batch(p, sizes, scales, sms, targets, kind, weight, eps, reduction, windows, dmax_kw):
    """gsasr_model.py:213-235 on the plain batched render"""
    from gsasr_amd import gaussian_splatting as gsp
    q = p.detach().clone().requires_grad_(True)
    out = gsp.generate_2D_gaussian_splatting_batch(sizes, q, scales, sms, windows=windows, **dmax_kw)
    hw = sizes if windows is None else [(w[2], w[3]) for w in windows]
    vals = [torch_loss(out[b, :, :h, :w], targets[b, :, :h, :w], kind, weight, eps, reduction) for b, (h, w) in enumerate(hw)]
    total = sum(vals) / len(vals) if reduction == "mean" else sum(vals)
    total.backward()
    return total.detach(), torch.stack([v.detach() for v in vals]), q.grad, out.detach()


@pytest.mark.parametrize("kernel", ["gaussian", "tile", "home"])
@pytest.mark.parametrize("source", ["step_size", "scale_modify"])
@pytest.mark.parametrize("bounded", [True, False], ids=["bounded", "unbounded"])
def test_parameter_gradients_batch_and_batched_windows(kernel, source, bounded, dev):
    from gsasr_amd import gaussian_splatting as gsp
    sizes, p, scales = batch_case(dev, seed=20)
    B = len(sizes)
    p.requires_grad_(True)
    sms = torch.tensor([[4.0, 4.0]] * B, device=dev) if source == "scale_modify" else [(4.0, 4.0)] * B
    dmax_kw = dict(dmax=0.15) if bounded else dict(if_dmax=False)
    wins = [(5, 3, 60, 71), (0, 0, 61, 77), (17, 9, 33, 30), (2, 40, 50, 56)]
    with forced_backward(kernel):
        for windows in (None, wins):
            hmax, wmax = (96, 96) if windows is None else (61, 77)
            _, _, _, v_ref = unfused_batch(p, sizes, scales, sms, torch.zeros(B, 3, hmax, wmax, device=dev), "mse", 1.0, 0.0, "mean",
                                           windows, dmax_kw)
            for kind, eps, reduction in (("l1", 1e-12, "mean"), ("charbonnier", 1e-12, "mean"), ("mse", 1e-12, "sum")):
                t = conditioned_target(v_ref, 9) if kind != "mse" else torch.rand_like(v_ref)
                want_v, want_b, want_g, _ = unfused_batch(p, sizes, scales, sms, t, kind, 0.6, eps, reduction, windows, dmax_kw)
                p.grad = None
                value, per = gsp.generate_2D_gaussian_splatting_batch_loss(sizes, p, scales, sms, t, loss=kind, loss_weight=0.6, eps=eps,
                                                                           reduction=reduction, windows=windows, return_per_sample=True,
                                                                           **dmax_kw)
                assert value.dim() == 0 and value.requires_grad and not per.requires_grad and tuple(per.shape) == (B,)
                value.backward()
                assert abs(float(value.detach()) - float(want_v)) <= 2e-5 * abs(float(want_v))
                assert float((per - want_b).abs().max()) <= 2e-5 * float(want_b.abs().max())
                check_param_grads(p.grad, want_g, p, f"{kernel} {source} {kind} windows={windows is not None}")
    gsp.deferred_asserts.flush()


def test_stale_memory_below_a_short_sample_does_not_reach_the_gradient(dev):
    """The fused forward writes a sample's own pixels of the gradient buffer only, and the Gaussian-stationary backward loads up
    to seven rows below a window's last row to multiply them by 0 (bwd_block's last trip).  Below a sample shorter than its slot
    those rows are padding: whatever the memory held before.  The caching allocator is primed with NaN blocks of the buffer's
    size, as a test that fills its gradient buffers with NaN leaves it; the host path must hand the kernels a buffer whose
    padding is finite.  (Shapes of tests/test_ssim_loss_gpu.py::test_fused_batch_and_batched_windows, where it showed.)"""
    from gsasr_amd import gaussian_splatting as gsp, synthetic
    sizes = [(11, 16), (24, 40), (17, 11)]
    B, slot, w = len(sizes), 32, 40
    p = torch.stack([synthetic.gs_parameters(12, 20, seed=40 + b) for b in range(B)]).to(dev)
    scales, sms = [2.0] * B, [(2.0, 2.0)] * B
    t = torch.rand(B, 3, 24, w, generator=torch.Generator().manual_seed(1)).to(dev)

    def run(poison):
        q = p.clone().requires_grad_(True)
        if poison:
            junk = [torch.full((B * slot * w * 3,), float("nan"), device=dev) for _ in range(16)]
            del junk
        gsp.generate_2D_gaussian_splatting_batch_loss(sizes, q, scales, sms, t, loss="l1", dmax=0.3).backward()
        return q.grad

    for kernel in ("gaussian", "tile", "home"):
        with forced_backward(kernel):
            dirty, clean = run(True), run(False)
        assert bool(torch.isfinite(dirty).all()), kernel
        assert float((dirty - clean).abs().max()) <= 1e-5 * float(clean.abs().max()), kernel      # (the same sums, atomics in another order)


@pytest.mark.parametrize("shape", ["dense-16-per-LR-px", "config2"])
def test_parameter_gradients_dense_and_config2(shape, dev):
    """one dense shape (16 Gaussians per LR pixel, a 48^2 LR crop at x4) and config 2 at full size (256^2 LR x4: 1024^2,
    65 536 Gaussians), the library's own kernel choices"""
    from gsasr_amd import gaussian_splatting as gsp, synthetic
    lr, gpp = (48, 16) if shape.startswith("dense") else (256, 1)
    H = W = lr * 4
    p = synthetic.gs_parameters(lr, lr, seed=31, gpp=gpp).to(dev).requires_grad_(True)
    sm = torch.tensor([4.0, 4.0], device=dev)
    _, _, v_ref = unfused_single(p, H, W, 4.0, sm, torch.zeros(3, H, W, device=dev), "mse", 1.0, 0.0, "mean", None, dict(dmax=0.1))
    for kind, eps in (("l1", 1e-12), ("charbonnier", 1e-6)):
        t = conditioned_target(v_ref, 13) if kind == "l1" else torch.rand_like(v_ref)
        want_v, want_g, _ = unfused_single(p, H, W, 4.0, sm, t, kind, 1.0, eps, "mean", None, dict(dmax=0.1))
        p.grad = None
        value = gsp.generate_2D_gaussian_splatting_loss((H, W), p, 4.0, sm, t, loss=kind, eps=eps, dmax=0.1)
        value.backward()
        assert abs(float(value.detach()) - float(want_v)) <= 2e-5 * abs(float(want_v))
        check_param_grads(p.grad, want_g, p, f"{shape} {kind}")
    gsp.deferred_asserts.flush()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("bounded", [True, False], ids=["bounded", "unbounded"])
def test_against_the_oracle_end_to_end(kind, bounded, dev):
    """oracle image (float64) -> float64 loss -> oracle backward -> the chain rule of oracle/host_ref.py, against the fused
    step; targets conditioned around the ORACLE's image for L1 and Charbonnier (eps = 1e-12), natural for MSE"""
    from gsasr_amd import gaussian_splatting as gsp, synthetic
    from oracle import gs_oracle, host_ref
    H, W, scale = 64, 48, 4.0
    p = synthetic.gs_parameters(16, 12, seed=41)
    dmax = 0.3 if bounded else None
    q = p.clone().double().requires_grad_(True)
    sig, xy, col, _ = host_ref.prologue(q, (H, W), (scale, scale))
    f32 = [t.detach().float().numpy() for t in (sig, xy, col)]
    ref_img = gs_oracle.forward_f64(*f32, H, W, dmax)                                  # [H,W,3]
    v_ref = torch.from_numpy(ref_img).float().permute(2, 0, 1).contiguous()
    eps = 1e-12
    t = conditioned_target(v_ref, 17) if kind != "mse" else torch.rand(3, H, W, generator=torch.Generator().manual_seed(17))
    want_v, dimg = loss_f64(ref_img, t.permute(1, 2, 0).numpy(), kind, 0.9, eps)
    gs, gc, gk = gs_oracle.backward_f64(*f32, dimg.astype(np.float32), dmax)
    (sig * torch.from_numpy(gs)).sum().add((xy * torch.from_numpy(gc)).sum()).add((col * torch.from_numpy(gk)).sum()).backward()
    pg = p.to(dev).requires_grad_(True)
    kw = dict(dmax=dmax) if bounded else dict(if_dmax=False)
    value, image = gsp.generate_2D_gaussian_splatting_loss((H, W), pg, scale, (scale, scale), t.to(dev), loss=kind, loss_weight=0.9,
                                                           eps=eps, return_image=True, **kw)
    value.backward()
    assert float((image.cpu() - v_ref).abs().max()) <= 1e-4                            # the image bar of tests/test_hip_parity.py
    assert abs(float(value.detach()) - want_v) <= 1e-4 * 0.9 + 1e-5 * want_v           # every |d phi| <= |d v| <= 1e-4
    check_param_grads(pg.grad, q.grad.float(), p, f"oracle {kind}", independent=True, min_share=1.0)


# ---- (5) upstream scalar ------------------------------------------------------------------------------------------------
def test_upstream_scalar(dev):
    from gsasr_amd import gaussian_splatting as gsp, synthetic
    H, W = 96, 80
    p = synthetic.gs_parameters(24, 20, seed=2).to(dev).requires_grad_(True)
    t = torch.rand(3, H, W, device=dev)
    call = lambda: gsp.generate_2D_gaussian_splatting_loss((H, W), p, 4.0, (4.0, 4.0), t, loss="charbonnier", eps=1e-6, dmax=0.3)
    call().backward()
    base = p.grad.clone()
    p.grad = None
    (2.5 * call()).backward()
    check_param_grads(p.grad, 2.5 * base, p, "2.5 * loss")
    p.grad = None
    other = (p[:, 3:7] ** 2).sum()
    (call() + other).backward()
    check_param_grads(p.grad, base + torch.autograd.grad((p[:, 3:7] ** 2).sum(), p)[0], p, "loss + other term")


# Graph captures below follow tests/test_host_path.py: the leaf is NEW and takes part in autograd first on the side stream of the
# warm-up.  That is a precondition of capturing any backward, not of this feature: autograd binds a leaf's gradient accumulator to
# the stream the leaf is first used on, and keeps it while any graph still refers to it.  A leaf that was used on the default
# stream before (and is still referenced by a live graph -- `other` in test_upstream_scalar) makes the engine synchronise the
# capture stream with the default stream inside the capture, which the runtime cannot capture: the process dies in capture_end.
def test_device_scalar_upstream_in_a_graph(dev):
    """the upstream d/d loss as a 0-dim DEVICE tensor, forward + backward inside a graph capture: a host read of it would
    fail the capture; the replay with another value in it scales the gradient"""
    from gsasr_amd import gaussian_splatting as gsp, synthetic
    H, W = 96, 80
    p = synthetic.gs_parameters(24, 20, seed=2).to(dev).requires_grad_(True)
    t = torch.rand(3, H, W, device=dev)
    k = torch.full((), 0.5, device=dev)
    call = lambda: gsp.generate_2D_gaussian_splatting_loss((H, W), p, 4.0, (4.0, 4.0), t, loss="charbonnier", eps=1e-6, dmax=0.3)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for _ in range(2):
            torch.autograd.grad(call(), p, k)
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g, = torch.autograd.grad(call(), p, k)
    k.fill_(-3.0)
    graph.replay()
    torch.cuda.synchronize()
    base, = torch.autograd.grad(call(), p)
    check_param_grads(g, -3.0 * base, p, "device scalar in a graph")


# ---- (6) validation form ------------------------------------------------------------------------------------------------
def test_validation_loss_under_no_grad(dev):
    from gsasr_amd import _cabi, gaussian_splatting as gsp, synthetic
    H, W = 96, 80
    p = synthetic.gs_parameters(24, 20, seed=5).to(dev).requires_grad_(True)
    t = torch.rand(3, H, W, device=dev)
    seen = []
    real = _cabi._step_loss

    def spy(*a, **k):
        out = real(*a, **k)
        seen.append(out)
        return out
    _cabi._step_loss = spy
    try:
        with torch.no_grad():
            value, image = gsp.generate_2D_gaussian_splatting_loss((H, W), p, 4.0, (4.0, 4.0), t, loss="mse", dmax=0.3, return_image=True)
    finally:
        _cabi._step_loss = real
    loss, grad, img, plan = seen[0]
    assert plan.dims.flags & _cabi.FLAG_FORWARD_ONLY and grad is None and not value.requires_grad
    ref, _ = loss_f64(image.cpu().numpy(), t.cpu().numpy(), "mse")
    assert abs(float(value) - ref) <= 1e-5 * ref
    sizes, pb, scales = batch_case(dev, seed=3)
    tb = torch.rand(len(sizes), 3, 96, 96, device=dev)
    with torch.no_grad():
        total, per, images = gsp.generate_2D_gaussian_splatting_batch_loss(sizes, pb, scales, [(4.0, 4.0)] * len(sizes), tb, loss="l1",
                                                                           dmax=0.3, return_per_sample=True, return_images=True)
    refs = [loss_f64(images[b, :, :h, :w].cpu().numpy(), tb[b, :, :h, :w].cpu().numpy(), "l1")[0] for b, (h, w) in enumerate(sizes)]
    assert np.allclose(per.cpu().numpy(), refs, rtol=1e-5, atol=0) and abs(float(total) - np.mean(refs)) <= 1e-5 * np.mean(refs)
    for b, (h, w) in enumerate(sizes):
        assert not images[b, :, h:].any() and not images[b, :, :, w:].any()


# ---- (7) forward + backward in a hipGraph -------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["single", "batch"])
def test_forward_backward_in_a_graph(form, dev):
    """forward + backward captured and replayed on new parameters: the replayed loss within 1e-5, the gradients within the
    project's bars of the eager ones"""
    from gsasr_amd import gaussian_splatting as gsp, synthetic
    if form == "single":
        H, W = 96, 80
        static_p = synthetic.gs_parameters(24, 20, seed=2).to(dev).requires_grad_(True)
        new = synthetic.gs_parameters(24, 20, seed=7).to(dev)
        t = torch.rand(3, H, W, device=dev)
        run = lambda q: gsp.generate_2D_gaussian_splatting_loss((H, W), q, 4.0, (4.0, 4.0), t, loss="charbonnier", eps=1e-6, dmax=0.3)
    else:
        sizes, static_p, scales = batch_case(dev, seed=50)
        static_p.requires_grad_(True)
        new = batch_case(dev, seed=60)[1]
        t = torch.rand(len(sizes), 3, 96, 96, device=dev)
        sms = torch.tensor([[4.0, 4.0]] * len(sizes), device=dev)      # (read by the plan's first kernel: no copy inside the capture)
        run = lambda q: gsp.generate_2D_gaussian_splatting_batch_loss(sizes, q, scales, sms, t, loss="mse", dmax=0.3)

    def step():
        value = run(static_p)
        g, = torch.autograd.grad(value, static_p)
        return value, g

    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        value_g, grad_g = step()
    with torch.no_grad():
        static_p.copy_(new)
    graph.replay()
    torch.cuda.synchronize()
    ref_p = new.clone().requires_grad_(True)
    ref = run(ref_p)
    ref.backward()
    assert abs(float(value_g.detach()) - float(ref.detach())) <= 1e-5 * float(ref.detach())
    check_param_grads(grad_g, ref_p.grad, ref_p, f"graph replay ({form})")


# ---- (8) plain C ---------------------------------------------------------------------------------------------------------
def test_c_program_loss(tmp_path):
    """plan -> gsasr_splat_forward_loss -> gsasr_splat_backward from plain C against a host loop (tests/c_abi/c_abi_loss_check.c)"""
    import shutil
    from gsasr_amd import _cabi
    lib = _cabi.LIB_PATH
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc and os.path.exists(lib)
    exe = str(tmp_path / "c_abi_loss_check")
    subprocess.check_call([cc, "-O1", "-std=c11", "-D__HIP_PLATFORM_AMD__", f"-I{rocm}/include", f"-I{ROOT}/include",
                           os.path.join(HERE, "c_abi", "c_abi_loss_check.c"), lib, f"-L{rocm}/lib", "-lamdhip64", "-lm",
                           f"-Wl,-rpath,{os.path.dirname(lib)}", f"-Wl,-rpath,{rocm}/lib", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "C-ABI LOSS CHECK OK" in out.stdout, out.stdout + out.stderr


def test_half_targets_under_autocast(dev):
    """a bf16 target under autocast is cast once at the fp32 boundary: the value is that of its fp32 copy"""
    from gsasr_amd import gaussian_splatting as gsp, synthetic
    H, W = 64, 48
    p = synthetic.gs_parameters(16, 12, seed=6).to(dev).requires_grad_(True)
    t = torch.rand(3, H, W, device=dev).bfloat16()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        a = gsp.generate_2D_gaussian_splatting_loss((H, W), p, 4.0, (4.0, 4.0), t, loss="l1", dmax=0.3)
    b = gsp.generate_2D_gaussian_splatting_loss((H, W), p, 4.0, (4.0, 4.0), t.float(), loss="l1", dmax=0.3)
    assert a.dtype == torch.float32 and abs(float(a.detach()) - float(b.detach())) <= 1e-5 * float(b.detach())
    a.backward()
    assert bool(torch.isfinite(p.grad).all())


if __name__ == "__main__":      # (test_store_is_exact_through_the_fine_forward: GSASR_SPLAT_DEV=1 GSASR_SPLAT_FWD8=1)
    device = torch.device("cuda:0")
    for bounded in (True, False):
        fine_plan, fine_flag = kernel_case("fwd2-parts2", bounded, device)
        check_store(fine_plan, fine_flag, device, "fwd8")
        # the kernel that ran, by what it leaves in the scratch: k_render_fwd8 stores one partial per 8 x 8-px sub-tile, every
        # other forward one per 8 x 16 or 16 x 16
        from gsasr_amd import _cabi
        dd = fine_plan.dims
        scratch = torch.full((_cabi.lib().gsasr_loss_scratch_bytes(ctypes.byref(dd)) // 4,), float("nan"), device=device)
        _cabi.forward_loss(fine_plan, torch.rand(dd.h, dd.w, 3, device=device), 0, flags=fine_flag, scratch=scratch)
        written = int(torch.isfinite(scratch).sum())
        assert written == ((dd.w + 7) // 8) * ((dd.h + 7) // 8), written
        print(f"fwd8 partials {written}")
    print("fwd8 loss exact")
