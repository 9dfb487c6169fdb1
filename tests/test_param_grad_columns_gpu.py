"""d / d raw decoder parameters [n, 9], column by column, through every route of the step backward.

The prologue's chain rule (0.99999 s(1 - s), 0.999999 (1 - tanh^2), alpha (1 - alpha), 2 / (H - 1) / step and the per-sample
H, W, step) lives in the seven small columns of that gradient; the two mean columns are 30-100 times larger and set the tensor-
level bar.  The chain rule runs in five places (k_prologue_bwd, k_prologue_bwd_gather behind the tile and atomic backward,
prologue_backward_batched with the geometry table and with the view table, the full_h / full_w substitutions of a window), and the
tests of those paths elsewhere compare fused against unfused of the same build.  Here every route is held to the per-column,
per-element bars of tests/gradbars.py against ONE independent truth:

    float64 autograd through oracle.host_ref.prologue around oracle.gs_oracle.backward_f64,

computed once per case (functools.lru_cache), shared, never written.  A window's truth is the oracle on the full grid with the
window's weights zero-padded (tests/test_view_gpu.py).  Shapes: LR grids 12x10 .. 32x24, HR <= 128x128, <= 768 Gaussians a sample,
and LR 12x12 at 16 Gaussians per LR pixel.  Every case has all its rows in the scope of the element bar (min_share 1.0).

The last test takes the chain rule alone (gsasr_prologue_backward) with each activated column swept over -12 .. 12; its yardstick
is torch's fp32 CPU autograd of the same expression against float64, never the kernel's own output.
"""
import functools

import numpy as np
import pytest
import torch

import gradbars
from test_fused_loss_gpu import forced_backward
from test_query_points_gpu import _domain_points, _eval64

pytestmark = pytest.mark.gpu
KERNELS = ["gaussian", "tile", "atomic", "home"]
HOST_KERNELS = ["gaussian", "tile", "home"]        # what gaussian_splatting.BACKWARD_KERNEL can force
OPS = {"bounded": 0.2, "unbounded": None}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the MI355X box)"
    return torch.device("cuda:0")


def kernel_flag(kernel):
    from gsasr_amd import _cabi
    return getattr(_cabi, "FLAG_BWD_" + kernel.upper()) | _cabi.FLAG_CHW_GRAD


# ---- the truth ------------------------------------------------------------------------------------------------------------
def chain_rule_f64(p, hw, sm, g):
    """float64 autograd of host_ref.prologue at raw parameters `p` [n, 9], fed the kernel-frame gradients `g` -> [n, 9]"""
    from oracle import host_ref
    pr = p.clone().double().requires_grad_(True)
    s2, x2, c2, _ = host_ref.prologue(pr, hw, sm.double())
    torch.autograd.backward([s2, x2, c2], [torch.from_numpy(np.asarray(a, np.float64)) for a in g])
    return pr.grad.numpy()


def kernel_frame(p, hw, sm):
    from oracle import host_ref
    sig, xy, col, _ = host_ref.prologue(p, hw, sm)
    return sig.numpy(), xy.numpy(), col.numpy()


def truth(p, hw, sm, wgt, dmax, window=None):
    """d sum(wgt * image) / d p; `wgt` [h, w, 3] numpy, of the window (y0, x0, h, w) if one is given"""
    from oracle import gs_oracle
    H, W = hw
    a, b, c = kernel_frame(p, hw, sm)
    if window is None:
        g = gs_oracle.backward_f64(a, b, c, wgt, dmax)
    else:
        y0, x0, h, w = window
        pad = np.zeros((h, W, 3), np.float32)
        pad[:, x0:x0 + w] = wgt
        g = gs_oracle.backward_f64(a, b, c, pad, dmax, h=H, rows=(y0, y0 + h))
    return chain_rule_f64(p, hw, sm, g)


def parameters(lr, seed, gpp=1):
    from gsasr_amd import synthetic
    p = synthetic.gs_parameters(lr[0], lr[1], seed=seed, gpp=gpp)
    assert float(gradbars.kappa_of(gradbars.raw_rho(p)).min()) >= gradbars.KAPPA_MIN, (lr, seed, gpp)      # min_share 1.0 below
    return p


def weights(h, w, seed):
    from gsasr_amd import synthetic
    return synthetic.grad_image(h, w, seed).numpy()


def scale_pair(s):
    return torch.tensor([s, s], dtype=torch.float32)


def step_source(source, sm, dev):
    """(step, scale_modify) as the step entry points take them: a device step size, or the device scale_modify pair(s) the first
    kernel turns into one -- the backward then runs with step_size = NULL"""
    sm = sm.to(dev)
    if source == "scale_modify":
        return None, sm.contiguous()
    first = sm[..., 0]
    return (1.2 / first).reshape(-1).contiguous(), None


# ---- one image and a window -----------------------------------------------------------------------------------------------
ONE = dict(lr=(24, 32), seed=60, scale=4.0, hw=(96, 128))
WIN = dict(lr=(32, 24), seed=11, scale=4.0, hw=(128, 96), window=(19, 7, 70, 61))      # not the grid, not tile-aligned


@functools.lru_cache(maxsize=None)
def one_image_case(which, op):
    c = ONE if which == "one" else WIN
    p, sm, window = parameters(c["lr"], c["seed"]), scale_pair(c["scale"]), c.get("window")
    h, w = c["hw"] if window is None else window[2:]
    wgt = weights(h, w, c["seed"] + 1)
    return p, c["hw"], sm, wgt, window, truth(p, c["hw"], sm, wgt, OPS[op], window)


def run_step(p, hw, sm, wgt, dmax, window, kernel, source, dev):
    """gsasr_step_forward[_sm][_view] + gsasr_step_backward[_view] with the planar upstream gradient the host API hands over"""
    from gsasr_amd import _cabi
    pg = p.to(dev)
    step, sm_dev = step_source(source, sm, dev)
    h, w = hw if window is None else window[2:]
    view = None if window is None else (hw[0], hw[1], window[0], window[1])
    _, plan = _cabi.step_forward(pg, step, h, w, dmax, kernel_flag(kernel), scale_modify=sm_dev, view=view)
    grad = torch.from_numpy(wgt).permute(2, 0, 1).contiguous().to(dev)
    got = _cabi.step_backward(plan, pg, step, grad, chw=True)
    torch.cuda.synchronize()
    return got.cpu().numpy()


@pytest.mark.parametrize("op", sorted(OPS))
@pytest.mark.parametrize("source", ["step_size", "scale_modify"])
@pytest.mark.parametrize("kernel", KERNELS)
def test_one_image(kernel, source, op, dev):
    p, hw, sm, wgt, _, want = one_image_case("one", op)
    got = run_step(p, hw, sm, wgt, OPS[op], None, kernel, source, dev)
    gradbars.check_raw(got, want, p, 1.0, f"one image/{kernel}/{source}/{op}")


@pytest.mark.parametrize("op", sorted(OPS))
@pytest.mark.parametrize("source", ["step_size", "scale_modify"])
@pytest.mark.parametrize("kernel", KERNELS)
def test_window(kernel, source, op, dev):
    """full_h / full_w stand in for the window's size in both chain-rule kernels"""
    p, hw, sm, wgt, window, want = one_image_case("window", op)
    got = run_step(p, hw, sm, wgt, OPS[op], window, kernel, source, dev)
    gradbars.check_raw(got, want, p, 1.0, f"window/{kernel}/{source}/{op}")


@pytest.mark.parametrize("op", sorted(OPS))
@pytest.mark.parametrize("kernel", HOST_KERNELS)
def test_host_api_image_and_window(kernel, op, dev):
    """the same two cases through generate_2D_gaussian_splatting_step / _view and autograd"""
    from gsasr_amd import gaussian_splatting as gsp
    kw = dict(if_dmax=True, dmax_mode="fix", dmax=OPS[op]) if OPS[op] is not None else dict(if_dmax=False)
    with forced_backward(kernel):
        for which in ("one", "window"):
            p, hw, sm, wgt, window, want = one_image_case(which, op)
            pg = p.to(dev).requires_grad_(True)
            if window is None:
                out = gsp.generate_2D_gaussian_splatting_step(hw, pg, float(sm[0]), sm.to(dev), **kw)
            else:
                out = gsp.generate_2D_gaussian_splatting_view(hw, pg, float(sm[0]), sm.to(dev), window, **kw)
            (out * torch.from_numpy(wgt).permute(2, 0, 1).to(dev)).sum().backward()
            gradbars.check_raw(pg.grad, want, p, 1.0, f"host api {which}/{kernel}/{op}")
    gsp.deferred_asserts.flush()


# ---- a ragged batch of three, another scale per sample ----------------------------------------------------------------------
BATCH_LR, BATCH_SEED = (12, 10), 130
BATCH_SIZES = [(40, 56), (64, 64), (33, 47)]
BATCH_SCALES = {"heights": [h / BATCH_LR[0] for h, _ in BATCH_SIZES],          # 3.33 / 5.33 / 2.75
                "widths": [w / BATCH_LR[1] for _, w in BATCH_SIZES]}           # 5.6 / 6.4 / 4.7
BATCH_WINDOWS = [(5, 3, 30, 41), (11, 9, 40, 50), (0, 2, 33, 40)]             # (y0, x0, h, w), one per sample
BATCH_DMAX = {"heights": 0.25, "widths": None}


@functools.lru_cache(maxsize=None)
def batch_case(scales_by, windows):
    ps = [parameters(BATCH_LR, BATCH_SEED + b) for b in range(len(BATCH_SIZES))]
    sms = [scale_pair(s) for s in BATCH_SCALES[scales_by]]
    wins = BATCH_WINDOWS if windows else [None] * len(ps)
    own = [hw if wn is None else wn[2:] for hw, wn in zip(BATCH_SIZES, wins)]
    wgts = [weights(h, w, 140 + b) for b, (h, w) in enumerate(own)]
    wants = [truth(ps[b], BATCH_SIZES[b], sms[b], wgts[b], BATCH_DMAX[scales_by], wins[b]) for b in range(len(ps))]
    return torch.stack(ps), torch.stack(sms), own, wgts, wins, wants


def run_batch(scales_by, windows, kernel, source, dev):
    from gsasr_amd import _cabi
    p, sms, own, wgts, wins, wants = batch_case(scales_by, windows)
    pg = p.to(dev)
    steps, sm_dev = step_source(source, sms, dev)
    views = [(hw[0], hw[1], wn[0], wn[1]) for hw, wn in zip(BATCH_SIZES, wins)] if windows else None
    _, plan = _cabi.batch_forward(pg, steps, own, BATCH_DMAX[scales_by], kernel_flag(kernel), scale_modify=sm_dev, views=views)
    hm, wm = max(h for h, _ in own), max(w for _, w in own)
    grad = torch.full((len(own), 3, hm + 3, wm), 7.0)          # (whatever lies outside a sample's own pixels is never read)
    for b, (h, w) in enumerate(own):
        grad[b, :, :h, :w] = torch.from_numpy(wgts[b]).permute(2, 0, 1)
    got = _cabi.batch_backward(plan, pg, steps, grad.to(dev), chw=True)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    for b in range(len(own)):
        gradbars.check_raw(got[b], wants[b], p[b], 1.0, f"batch scales by {scales_by} windows={windows}/{kernel}/{source}/sample {b}")


@pytest.mark.parametrize("scales_by", sorted(BATCH_SCALES))
@pytest.mark.parametrize("source", ["step_size", "scale_modify"])
@pytest.mark.parametrize("kernel", KERNELS)
def test_ragged_batch(kernel, source, scales_by, dev):
    """prologue_backward_batched with the geometry table: per-sample H, W and step down the rows"""
    run_batch(scales_by, False, kernel, source, dev)


@pytest.mark.parametrize("scales_by", sorted(BATCH_SCALES))
@pytest.mark.parametrize("kernel", KERNELS)
def test_batched_windows(kernel, scales_by, dev):
    """one window per sample: the view table replaces the geometry table"""
    run_batch(scales_by, True, kernel, "scale_modify" if scales_by == "heights" else "step_size", dev)


@pytest.mark.parametrize("kernel", HOST_KERNELS)
def test_host_api_batch_and_batched_windows(kernel, dev):
    from gsasr_amd import gaussian_splatting as gsp
    with forced_backward(kernel):
        for windows in (False, True):
            p, sms, own, wgts, wins, wants = batch_case("heights", windows)
            pg = p.to(dev).requires_grad_(True)
            out = gsp.generate_2D_gaussian_splatting_batch(BATCH_SIZES, pg, BATCH_SCALES["heights"], [s.to(dev) for s in sms],
                                                           windows=BATCH_WINDOWS if windows else None, dmax=BATCH_DMAX["heights"])
            loss = sum((out[b, :, :h, :w] * torch.from_numpy(wgts[b]).permute(2, 0, 1).to(dev)).sum() for b, (h, w) in enumerate(own))
            loss.backward()
            for b in range(len(own)):
                gradbars.check_raw(pg.grad[b], wants[b], p[b], 1.0, f"host api batch windows={windows}/{kernel}/sample {b}")
    gsp.deferred_asserts.flush()


# ---- sampled pixels and queries ----------------------------------------------------------------------------------------------
POINTS = 300
PT_ONE = dict(lr=(12, 12), seed=170, gpp=4, scale=4.0, hw=(48, 48))
PT_SIZES = [(48, 48), (40, 48), (48, 36), (33, 47)]
PT_SCALES = [4.0, 4.0, 3.0, 2.75]
PT_DMAX = 0.5


def point_truth(p, hw, sm, kind, seed):
    """(points, grad_out [3, S], d sum(grad_out * values) / d p) for integer (`sampled`) or fractional (`query`) positions"""
    from oracle import gs_oracle
    H, W = hw
    g = torch.Generator().manual_seed(seed)
    gout = torch.rand(3, POINTS, generator=g)
    a, b, c = kernel_frame(p, hw, sm)
    if kind == "sampled":
        pts = torch.stack([torch.randint(0, H, (POINTS,), generator=g), torch.randint(0, W, (POINTS,), generator=g)], dim=1)
        pts[5] = pts[7] = pts[3]          # repeated points are independent outputs whose gradients add
        wgt = torch.zeros(H, W, 3)
        wgt.index_put_((pts[:, 0], pts[:, 1]), gout.t().contiguous(), accumulate=True)
        grads = gs_oracle.backward_f64(a, b, c, wgt.numpy(), PT_DMAX)
    else:
        pts = _domain_points(H, W, POINTS, seed=seed)
        _, grads = _eval64(*(torch.from_numpy(t) for t in (a, b, c)), H, W, PT_DMAX, pts, gout)
    return pts, gout, chain_rule_f64(p, hw, sm, grads)


@functools.lru_cache(maxsize=None)
def point_case(kind, batched):
    if not batched:
        p, sm = parameters(PT_ONE["lr"], PT_ONE["seed"], PT_ONE["gpp"]), scale_pair(PT_ONE["scale"])
        return (p, sm) + point_truth(p, PT_ONE["hw"], sm, kind, 31)
    ps = [parameters((12, 12), 180 + b, 4) for b in range(len(PT_SIZES))]
    sms = [scale_pair(s) for s in PT_SCALES]
    per = [point_truth(ps[b], PT_SIZES[b], sms[b], kind, 40 + b) for b in range(len(ps))]
    return torch.stack(ps), torch.stack(sms), torch.stack([t[0] for t in per]), torch.stack([t[1] for t in per]), [t[2] for t in per]


@pytest.mark.parametrize("source", ["step_size", "scale_modify"])
@pytest.mark.parametrize("kind", ["sampled", "query"])
def test_points_of_one_image(kind, source, dev):
    """gsasr_step_sample_backward / gsasr_step_query_backward"""
    from gsasr_amd import _cabi
    p, sm, pts, gout, want = point_case(kind, False)
    pg = p.to(dev)
    step, sm_dev = step_source(source, sm, dev)
    fwd = _cabi.step_sample_forward if kind == "sampled" else _cabi.step_query_forward
    bwd = _cabi.step_sample_backward if kind == "sampled" else _cabi.step_query_backward
    _, plan, state = fwd(pg, step, *PT_ONE["hw"], PT_DMAX, pts.to(dev), scale_modify=sm_dev)
    got = bwd(plan, state, pg, step, gout.to(dev))
    torch.cuda.synchronize()
    gradbars.check_raw(got, want, p, 1.0, f"{kind} points, one image/{source}")


@pytest.mark.parametrize("kind", ["sampled", "query"])
def test_points_of_a_batch(kind, dev):
    """the batch with scales 4 / 4 / 3 / 2.75: the sampled chain rule with the geometry table"""
    from gsasr_amd import _cabi
    p, sms, pts, gout, wants = point_case(kind, True)
    pg = p.to(dev)
    steps, _ = step_source("step_size", sms, dev)
    fwd = _cabi.batch_sample_forward if kind == "sampled" else _cabi.batch_query_forward
    bwd = _cabi.step_sample_backward if kind == "sampled" else _cabi.step_query_backward
    _, plan, state = fwd(pg, steps, PT_SIZES, PT_DMAX, pts.to(dev))
    got = bwd(plan, state, pg, steps, gout.to(dev).contiguous())
    torch.cuda.synchronize()
    for b in range(len(PT_SIZES)):
        gradbars.check_raw(got[b], wants[b], p[b], 1.0, f"{kind} points, batch/sample {b}")


@pytest.mark.parametrize("kind", ["sampled", "query"])
def test_host_api_points(kind, dev):
    """sample_coords / query_coords of generate_2D_gaussian_splatting_step, _query and _batch"""
    from gsasr_amd import gaussian_splatting as gsp
    kw = dict(default_step_size=1.2, mode="scale_modify", if_dmax=True, dmax_mode="fix", dmax=PT_DMAX)
    p, sm, pts, gout, want = point_case(kind, False)
    pg = p.to(dev).requires_grad_(True)
    if kind == "sampled":
        out = gsp.generate_2D_gaussian_splatting_step(PT_ONE["hw"], pg, PT_ONE["scale"], sm.to(dev), sample_coords=pts.to(dev), **kw)
    else:
        out = gsp.generate_2D_gaussian_splatting_query(PT_ONE["hw"], pg, PT_ONE["scale"], sm.to(dev), pts.to(dev), **kw)
    (out * gout.to(dev)).sum().backward()
    gradbars.check_raw(pg.grad, want, p, 1.0, f"host api {kind} points, one image")
    p, sms, pts, gout, wants = point_case(kind, True)
    pg = p.to(dev).requires_grad_(True)
    coords = dict(sample_coords=pts.to(dev)) if kind == "sampled" else dict(query_coords=pts.to(dev))
    out = gsp.generate_2D_gaussian_splatting_batch(PT_SIZES, pg, PT_SCALES, [s.to(dev) for s in sms], **coords, **kw)
    (out * gout.to(dev)).sum().backward()
    for b in range(len(PT_SIZES)):
        gradbars.check_raw(pg.grad[b], wants[b], p[b], 1.0, f"host api {kind} points, batch/sample {b}")
    gsp.deferred_asserts.flush()


# ---- the fused-loss step: the loss's own grad_img feeds the backward ------------------------------------------------------------
LOSS_WEIGHT = 0.6


def mse_truth(p, hw, sm, dmax, target, batch):
    """d (weight * mean((image - target)^2) / batch) / d p with the float64 image: upstream weights 2 c_b (img64 - target)"""
    from oracle import gs_oracle
    H, W = hw
    a, b, c = kernel_frame(p, hw, sm)
    img = gs_oracle.forward_f64(a, b, c, H, W, dmax)
    dimg = 2.0 * (LOSS_WEIGHT / (3.0 * H * W * batch)) * (img - target.permute(1, 2, 0).double().numpy())
    return chain_rule_f64(p, hw, sm, gs_oracle.backward_f64(a, b, c, dimg.astype(np.float32), dmax))


@functools.lru_cache(maxsize=None)
def loss_case(batched, op):
    if not batched:
        p, hw, sm = parameters(ONE["lr"], ONE["seed"]), ONE["hw"], scale_pair(ONE["scale"])
        target = torch.rand(3, *hw, generator=torch.Generator().manual_seed(5))
        return p, sm, target, mse_truth(p, hw, sm, OPS[op], target, 1)
    B = len(BATCH_SIZES)
    ps = [parameters(BATCH_LR, BATCH_SEED + b) for b in range(B)]
    sms = [scale_pair(s) for s in BATCH_SCALES["heights"]]
    targets = [torch.rand(3, h, w, generator=torch.Generator().manual_seed(50 + b)) for b, (h, w) in enumerate(BATCH_SIZES)]
    wants = [mse_truth(ps[b], BATCH_SIZES[b], sms[b], OPS[op], targets[b], B) for b in range(B)]
    return torch.stack(ps), torch.stack(sms), targets, wants


@pytest.mark.parametrize("op", sorted(OPS))
@pytest.mark.parametrize("kernel", HOST_KERNELS)
def test_fused_mse_step(kernel, op, dev):
    from gsasr_amd import gaussian_splatting as gsp
    kw = dict(dmax=OPS[op]) if OPS[op] is not None else dict(if_dmax=False)
    with forced_backward(kernel):
        p, sm, target, want = loss_case(False, op)
        pg = p.to(dev).requires_grad_(True)
        gsp.generate_2D_gaussian_splatting_loss(ONE["hw"], pg, ONE["scale"], sm.to(dev), target.to(dev), loss="mse",
                                                loss_weight=LOSS_WEIGHT, **kw).backward()
        gradbars.check_raw(pg.grad, want, p, 1.0, f"fused mse, one image/{kernel}/{op}")
        p, sms, targets, wants = loss_case(True, op)
        pg = p.to(dev).requires_grad_(True)
        gsp.generate_2D_gaussian_splatting_batch_loss(BATCH_SIZES, pg, BATCH_SCALES["heights"], [s.to(dev) for s in sms],
                                                      [t.to(dev) for t in targets], loss="mse", loss_weight=LOSS_WEIGHT, **kw).backward()
        for b in range(len(BATCH_SIZES)):
            gradbars.check_raw(pg.grad[b], wants[b], p[b], 1.0, f"fused mse, batch/{kernel}/{op}/sample {b}")
    gsp.deferred_asserts.flush()


# ---- sixteen Gaussians per LR pixel ------------------------------------------------------------------------------------------
DENSE = dict(lr=(12, 12), seed=200, gpp=16, scale=4.0, hw=(48, 48))


@functools.lru_cache(maxsize=None)
def dense_case(op):
    p, sm = parameters(DENSE["lr"], DENSE["seed"], DENSE["gpp"]), scale_pair(DENSE["scale"])
    wgt = weights(*DENSE["hw"], 7)
    return p, sm, wgt, truth(p, DENSE["hw"], sm, wgt, OPS[op])


@pytest.mark.parametrize("op", sorted(OPS))
def test_dense_sample(op, dev):
    """LR 12x12 at 16 per LR pixel: 2304 px are far below the 1024 tiles the library's own rule asks of the home-tile backward
    (splat_common.h: bwd_wants_home), so the default is the Gaussian-stationary kernel here; the home-tile kernel is forced"""
    from gsasr_amd import gaussian_splatting as gsp
    H, W = DENSE["hw"]
    p, sm, wgt, want = dense_case(op)
    assert not (H * W >= 1024 * 512)
    kw = dict(if_dmax=True, dmax_mode="fix", dmax=OPS[op]) if OPS[op] is not None else dict(if_dmax=False)
    for kernel in ("auto", "home"):
        with forced_backward(kernel):
            pg = p.to(dev).requires_grad_(True)
            out = gsp.generate_2D_gaussian_splatting_step((H, W), pg, DENSE["scale"], sm.to(dev), **kw)
            (out * torch.from_numpy(wgt).permute(2, 0, 1).to(dev)).sum().backward()
            gradbars.check_raw(pg.grad, want, p, 1.0, f"dense 16 per LR pixel/{kernel}/{op}")
    gsp.deferred_asserts.flush()


# ---- the chain rule on its own -------------------------------------------------------------------------------------------------
SWEEP = 64


def swept_parameters(seed=9):
    """~450 rows: each of the seven activated columns sweeps -12 .. 12 over 64 rows while the others stay ordinary, plus the
    saturated row of test_fused_prologue_matches_unfused_torch_path"""
    g = torch.Generator().manual_seed(seed)
    n = 7 * SWEEP + 1
    p = 0.5 * torch.randn(n, 9, generator=g)
    p[:, 7:9] = torch.rand(n, 2, generator=g)
    for k in range(7):
        p[k * SWEEP:(k + 1) * SWEEP, k] = torch.linspace(-12.0, 12.0, SWEEP)
    p[-1] = torch.tensor([9.0, -9.0, 6.0, -7.0, 8.0, -8.0, 0.0, 0.3, 0.9])
    return p


def column_ratio(got, want):
    want = np.asarray(want, np.float64)
    err = np.abs(np.asarray(got, np.float64) - want)
    return (err / (np.abs(want) + 1e-6 * np.abs(want).max(axis=0, keepdims=True))).max(axis=0)


@pytest.mark.parametrize("hw", [(60, 84), (33, 2049)], ids=["60x84", "33x2049"])
def test_prologue_backward_alone(hw, dev):
    """gsasr_prologue_backward element by element against float64 autograd of host_ref.prologue.  1 - tanh^2 and s (1 - s) cancel
    in fp32 in any implementation, so the yardstick is torch's fp32 CPU autograd of the same expression, computed here: per
    column r_k = max_i |err| / (|want| + 1e-6 max_i |want|) of the kernel may be 4 r_k of torch fp32 + 1e-6 (device expf / tanhf a
    unit or two in the last place from the host's, the order of the products)."""
    from gsasr_amd import _cabi
    from oracle import host_ref
    p = swept_parameters()
    sm32 = torch.tensor([3.0, 3.0])
    step32 = (1.2 / sm32[0]).reshape(1)                                        # ~0.4, as torch's fp32 forms it
    sm64 = torch.tensor([1.2 / float(step32)] * 2, dtype=torch.float64)      # the same step in double
    g = torch.Generator().manual_seed(21)
    ups = [torch.rand(p.shape[0], c, generator=g) for c in (3, 2, 3)]
    p64 = p.clone().double().requires_grad_(True)
    torch.autograd.backward(list(host_ref.prologue(p64, hw, sm64)[:3]), [u.double() for u in ups])
    p32 = p.clone().requires_grad_(True)
    torch.autograd.backward(list(host_ref.prologue(p32, hw, sm32)[:3]), ups)
    got = _cabi.prologue_backward(p.to(dev), step32.to(dev), hw[0], hw[1], *(u.to(dev) for u in ups)).cpu().numpy()
    assert np.isfinite(got).all()
    want = p64.grad.numpy()
    r_gpu, r_ref = column_ratio(got, want), column_ratio(p32.grad.numpy(), want)
    for k, name in enumerate(gradbars.RAW_NAMES):
        print(f"{hw} column {name}: kernel {r_gpu[k]:.3e}, torch fp32 {r_ref[k]:.3e}")
    for k, name in enumerate(gradbars.RAW_NAMES):
        assert r_gpu[k] <= 4.0 * r_ref[k] + 1e-6, (name, float(r_gpu[k]), float(r_ref[k]))
