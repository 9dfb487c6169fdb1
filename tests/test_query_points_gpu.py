"""GPU parity of queries at fractional pixel positions (gsasr_splat_query_*, GSASR_FLAG_CONTINUOUS): values and gradients.

Yardsticks: the CPU oracle on a refined grid -- a point at (k_r / m, k_c / m) on the H x W grid IS pixel (k_r, k_c) of the
(m (H - 1) + 1) x (m (W - 1) + 1) grid, m a power of two (tests/test_query_points.py) -- and, for positions that lie on no
grid, a float64 evaluation of the definition written here (`_eval64`: float32 positions and box decisions as the kernels take
them, everything else in double, gradients by autograd).  Tolerances are the project's own (tests/test_sampled_pixels.py):
1e-4 per value, gradients 2e-4 of the tensor's max-abs.
"""
import math

import numpy as np
import pytest
import torch

import gradbars

pytestmark = pytest.mark.gpu

IMG_ATOL = 1e-4
GRAD_RTOL = 2e-4
EPS = 1e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the MI355X box)"
    return torch.device("cuda:0")


def _relmax(got, want):
    return float(np.abs(got - want).max() / max(1e-12, np.abs(want).max()))


def _synth(h_lr, w_lr, scale, seed, gpp=1):
    from gsasr_amd import synthetic
    return synthetic.kernel_inputs(h_lr, w_lr, scale, seed=seed, gpp=gpp)


def _plan(sig, xy, col, H, W, dmax, dev, cutoff=0.0, continuous=True):
    from gsasr_amd import _cabi
    a, b, c = (t.to(dev).contiguous() for t in (sig, xy, col))
    return _cabi.plan(a, b, c, H, W, dmax, cutoff=cutoff, flags=_cabi.FLAG_CONTINUOUS if continuous else 0), (a, b, c)


def _query(sig, xy, col, H, W, dmax, pts, gout, dev, cutoff=0.0):
    """query forward + backward through the plan API -> (out [3,S], (g_sigmas, g_coords, g_colors)) as numpy"""
    from gsasr_amd import _cabi
    plan, (a, b, c) = _plan(sig, xy, col, H, W, dmax, dev, cutoff)
    out, state = _cabi.query_forward(plan, pts)
    g = (torch.empty_like(a), torch.empty_like(b), torch.empty_like(c))
    _cabi.query_backward(plan, state, a, b, c, gout, *g, overwrite=True)
    torch.cuda.synchronize()
    return out.cpu().numpy(), tuple(t.cpu().numpy() for t in g)


def _eval64(sig, xy, col, H, W, dmax, pts, gout=None):
    """The definition in float64 (CPU): px = float32(2 c / (W - 1) - 1) formed in double, the box decision from the float32
    dx, dy against the float32 dmax, exponent and sum in double; 0 outside the closed domain.  Returns out [3,S] and, with
    `gout`, the gradients of sum(gout * out) with respect to (sigmas, coords, colors), all numpy float64."""
    sig, xy, col = (t.detach().cpu().double().requires_grad_(gout is not None) for t in (sig, xy, col))
    p = pts.detach().cpu().float()
    r, c = p[:, 0], p[:, 1]
    valid = (r >= 0) & (r <= H - 1) & (c >= 0) & (c <= W - 1)
    r, c = torch.where(valid, r, torch.zeros_like(r)), torch.where(valid, c, torch.zeros_like(c))
    px, py = (2.0 * c.double() / (W - 1) - 1.0).float(), (2.0 * r.double() / (H - 1) - 1.0).float()
    outs = []
    for s0 in range(0, p.shape[0], 512):      # (chunks of points: [512, N] doubles at a time)
        sl = slice(s0, s0 + 512)
        inside = valid[sl, None].expand(-1, sig.shape[0])
        if dmax is not None:
            dxf = px[sl, None] - xy[:, 0].detach().float()[None, :]
            dyf = py[sl, None] - xy[:, 1].detach().float()[None, :]
            dm = torch.tensor(float(dmax), dtype=torch.float32)
            inside = inside & (dxf.abs() <= dm) & (dyf.abs() <= dm)
        dx, dy = px[sl, None].double() - xy[None, :, 0], py[sl, None].double() - xy[None, :, 1]
        sx, sy, rho = sig[None, :, 0], sig[None, :, 1], sig[None, :, 2]
        d = dx * dx / (sx * sx) - 2 * rho * dx * dy / (sx * sy) + dy * dy / (sy * sy)
        v = torch.where(inside, torch.exp(-0.5 / (1 - rho * rho) * d), torch.zeros((), dtype=torch.float64))
        outs.append((v @ col).t())
    out = torch.cat(outs, dim=1)
    if gout is None:
        return out.numpy()
    (out * gout.detach().cpu().double()).sum().backward()
    return out.detach().numpy(), (sig.grad.numpy(), xy.grad.numpy(), col.grad.numpy())


def _check(out, grads, want, gwant, tag="", sig=None, min_share=0.0):
    err = float(np.abs(out - want).max())
    rels = [_relmax(g, w) for g, w in zip(grads, gwant)]
    print(f"{tag}: max |value - reference| = {err:.3e}; gradient rel-max (sigmas, coords, colors) = " + ", ".join(f"{r:.3e}" for r in rels))
    assert err <= IMG_ATOL, tag
    for g, rel, name in zip(grads, rels, ("sigmas", "coords", "colors")):
        assert np.isfinite(g).all(), (tag, name)
        assert rel <= GRAD_RTOL, (tag, name)
    if sig is not None:      # every column to its own bar, element by element (tests/gradbars.py)
        gradbars.check_kernel(grads, gwant, sig, min_share, tag)


_ORACLE = {}


def _refined_oracle(m, dmax):
    """forward_f64 / backward_f64 on the refined grid for the 700 points (k_r / m, k_c / m) of test 1, once per (m, dmax)"""
    from oracle import gs_oracle
    if (m, dmax) not in _ORACLE:
        sig, xy, col, H, W = _synth(48, 40, 4.0, seed=21)
        Hm, Wm = m * (H - 1) + 1, m * (W - 1) + 1
        g = torch.Generator().manual_seed(50 + m)
        k = torch.stack([torch.randint(0, Hm, (700,), generator=g), torch.randint(0, Wm, (700,), generator=g)], dim=1)
        k[5] = k[3]          # repeated points are independent outputs whose gradients add
        k[7] = k[3]
        k[0] = torch.tensor([0, 0])
        k[1] = torch.tensor([Hm - 1, Wm - 1])      # the far corner of the closed domain
        gout = torch.rand(3, 700, generator=torch.Generator().manual_seed(6))
        s, x, c = sig.numpy(), xy.numpy(), col.numpy()
        want = gs_oracle.forward_f64(s, x, c, Hm, Wm, dmax)[k[:, 0].numpy(), k[:, 1].numpy(), :].T
        wgt = torch.zeros(Hm, Wm, 3, dtype=torch.float32)
        wgt.index_put_((k[:, 0], k[:, 1]), gout.t().contiguous(), accumulate=True)
        _ORACLE[(m, dmax)] = (k, gout, want, gs_oracle.backward_f64(s, x, c, wgt.numpy(), dmax))
    return _ORACLE[(m, dmax)]


@pytest.mark.parametrize("cutoff", [0.0, 104.0, -1.0], ids=["adaptive", "tau104", "nocut"])
@pytest.mark.parametrize("dmax", [None, 0.5, 0.1], ids=["unbounded", "dmax0.5", "dmax0.1"])
@pytest.mark.parametrize("m", [2, 4])
def test_query_against_refined_grid_oracle(m, dmax, cutoff, dev):
    sig, xy, col, H, W = _synth(48, 40, 4.0, seed=21)
    k, gout, want, gwant = _refined_oracle(m, dmax)
    pts = (k.to(torch.float32) / m).to(dev)          # exact in float32
    out, grads = _query(sig, xy, col, H, W, dmax, pts, gout.to(dev), dev, cutoff)
    _check(out, grads, want, gwant, f"m={m} dmax={dmax} cutoff={cutoff}", sig, gradbars.SYNTHETIC_SHARE)


def _domain_points(H, W, n, seed):
    """uniform over the closed domain + the four corners + points on every edge"""
    g = torch.Generator().manual_seed(seed)
    p = torch.rand(n, 2, generator=g) * torch.tensor([H - 1.0, W - 1.0])
    p[0:4] = torch.tensor([[0.0, 0.0], [0.0, W - 1.0], [H - 1.0, 0.0], [H - 1.0, W - 1.0]])
    p[4:12, 0] = 0.0
    p[12:20, 0] = H - 1.0
    p[20:28, 1] = 0.0
    p[28:36, 1] = W - 1.0
    p[40] = p[38]
    return p.clamp_(min=0.0).minimum(torch.tensor([H - 1.0, W - 1.0]))


@pytest.mark.parametrize("case", [(48, 40, 4.0, 1, None, 3000), (48, 40, 4.0, 1, 0.1, 3000), (24, 20, 4.0, 16, 0.5, 1500),
                                  (20, 16, 12.0, 1, 0.1, 2000), (24, 40, 2.5, 1, 0.5, 1000)],
                         ids=["x4-unbounded", "x4-dmax0.1", "x4-16-per-lr-px", "x12", "x2.5"])
def test_query_irrational_positions(case, dev):
    h_lr, w_lr, scale, gpp, dmax, n = case
    sig, xy, col, H, W = _synth(h_lr, w_lr, scale, seed=13, gpp=gpp)
    pts = _domain_points(H, W, n, seed=17)
    gout = torch.rand(3, n, generator=torch.Generator().manual_seed(8))
    out, grads = _query(sig, xy, col, H, W, dmax, pts.to(dev), gout.to(dev), dev)
    want, gwant = _eval64(sig, xy, col, H, W, dmax, pts, gout)
    _check(out, grads, want, gwant, f"{case}", sig, gradbars.SYNTHETIC_SHARE)


def _with_small_gaussians():
    """the 1 920 Gaussians of test 1 + 64 with sigma = 0.05 px centred BETWEEN four pixel centres, 20 x 18 px apart"""
    sig, xy, col, H, W = _synth(48, 40, 4.0, seed=21)
    ii = (10 + 20 * torch.arange(8)).repeat_interleave(8)        # rows i: the centre is at (i + 0.5, j + 0.5)
    jj = (8 + 18 * torch.arange(8)).repeat(8)
    cx = (2.0 * (jj.double() + 0.5) / (W - 1) - 1.0).float()
    cy = (2.0 * (ii.double() + 0.5) / (H - 1) - 1.0).float()
    g = torch.Generator().manual_seed(31)
    small_sig = torch.stack([torch.full((64,), 0.05 * 2.0 / (W - 1)), torch.full((64,), 0.05 * 2.0 / (H - 1)), torch.zeros(64)], dim=1)
    small_col = 0.25 + 0.75 * torch.rand(64, 3, generator=g)     # distinct colours
    sig = torch.cat([sig, small_sig]).contiguous()
    xy = torch.cat([xy, torch.stack([cx, cy], dim=1)]).contiguous()
    col = torch.cat([col, small_col]).contiguous()
    centre = torch.stack([ii + 0.5, jj + 0.5], dim=1).float()
    around = torch.cat([torch.stack([ii + a, jj + b], dim=1).float() for a in (0, 1) for b in (0, 1)])
    return sig, xy, col, H, W, torch.cat([centre, around]), small_col


@pytest.mark.parametrize("cutoff", [0.0, 20.0], ids=["adaptive", "tau20"])
@pytest.mark.parametrize("dmax", [None, 0.1], ids=["unbounded", "dmax0.1"])
def test_query_between_the_pixel_centres(dmax, cutoff, dev):
    """Gaussians whose support holds no pixel centre: dead on a plain plan, worth their colour on a continuous one.  An
    implementation that only sorts float points fails here."""
    from gsasr_amd import _cabi
    sig, xy, col, H, W, pts, small_col = _with_small_gaussians()
    n0 = sig.shape[0] - 64
    gout = 0.5 + torch.rand(3, pts.shape[0], generator=torch.Generator().manual_seed(9))
    out, grads = _query(sig, xy, col, H, W, dmax, pts.to(dev), gout.to(dev), dev, cutoff)
    want, gwant = _eval64(sig, xy, col, H, W, dmax, pts, gout)
    _check(out, grads, want, gwant, f"dmax={dmax} cutoff={cutoff}", sig, gradbars.SYNTHETIC_SHARE)
    # the centre is worth the small Gaussian's colour plus the background of the ordinary ones ...
    back = _eval64(sig[:n0], xy[:n0], col[:n0], H, W, dmax, pts[:64])
    assert np.abs(out[:, :64] - (small_col.numpy().T + back)).max() <= IMG_ATOL
    # ... the four pixel centres around it (14 sigma away) see nothing of it ...
    assert np.abs(out[:, 64:] - _eval64(sig[:n0], xy[:n0], col[:n0], H, W, dmax, pts[64:])).max() <= IMG_ATOL
    # ... and its colour gradient is its own grad_out column
    gk = grads[2]
    assert np.abs(gk[n0:] - gout[:, :64].numpy().T).max() <= GRAD_RTOL * np.abs(gk).max()
    # on a plan WITHOUT the flag the same call is refused, never a silently incomplete sum
    plain, (a, b, c) = _plan(sig, xy, col, H, W, dmax, dev, cutoff, continuous=False)
    with pytest.raises(RuntimeError, match="GSASR_FLAG_CONTINUOUS"):
        _cabi.query_forward(plain, pts.to(dev))
    cont, _ = _plan(sig, xy, col, H, W, dmax, dev, cutoff)
    _, st = _cabi.query_forward(cont, pts.to(dev))
    g = (torch.empty_like(a), torch.empty_like(b), torch.empty_like(c))
    with pytest.raises(RuntimeError, match="GSASR_FLAG_CONTINUOUS"):
        _cabi.query_backward(plain, st, a, b, c, gout.to(dev), *g, overwrite=True, resort=True)


@pytest.mark.parametrize("stacked", [1.0, 0.05], ids=["all-on-one-spot", "a-twentieth"])
def test_query_adversarial_stack_keeps_the_error_bound(stacked, dev):
    """the input of tests/test_adaptive_cutoff.py::test_adversarial_stack_keeps_the_error_bound, queried at every half-pixel
    position within 16 px of the stack: the adaptive continuous plan against the tau = 104 one, with that test's own bound"""
    from gsasr_amd import _cabi
    h = w = 192
    n = 8192
    g = np.random.default_rng(5)
    sig, xy, col, _, _ = _synth(48, 48, 4.0, 11, 4)
    sig, xy, col = sig[:n].numpy().copy(), xy[:n].numpy().copy(), col[:n].numpy().copy()
    m = int(n * stacked)
    xy[:m] = np.array([0.113, -0.207], np.float32)
    sig[:m, 0] = 0.02 + 0.002 * g.random(m)
    sig[:m, 1] = 0.02 + 0.002 * g.random(m)
    sig[:m, 2] = 0.0
    col[:m] = 1.0
    dmax = 0.25
    sig, xy, col = (torch.from_numpy(np.ascontiguousarray(t, dtype=np.float32)) for t in (sig, xy, col))
    cx, cy = (0.113 + 1.0) * 0.5 * (w - 1), (-0.207 + 1.0) * 0.5 * (h - 1)
    kr = torch.arange(max(0, math.ceil(2 * (cy - 16))), min(2 * (h - 1), math.floor(2 * (cy + 16))) + 1)
    kc = torch.arange(max(0, math.ceil(2 * (cx - 16))), min(2 * (w - 1), math.floor(2 * (cx + 16))) + 1)
    pts = (torch.stack(torch.meshgrid(kr, kc, indexing="ij"), dim=-1).reshape(-1, 2).float() / 2).to(dev)
    plan, _ = _plan(sig, xy, col, h, w, dmax, dev)
    tau, k = _cabi.plan_cutoff(plan)
    assert tau >= math.log(m / EPS) - 1e-3 and k >= m
    a, _ = _cabi.query_forward(plan, pts)
    exact, _ = _plan(sig, xy, col, h, w, dmax, dev, cutoff=104.0)
    b, _ = _cabi.query_forward(exact, pts)
    a, b = a.cpu().numpy(), b.cpu().numpy()
    err = np.abs(a - b)
    print(f"stacked={stacked}: tau'={tau:.3f} K={k}, {pts.shape[0]} points, max |a - b| = {err.max():.3e}, "
          f"max (|a - b| - 5e-6 |b|) = {(err - 5e-6 * np.abs(b)).max():.3e}")
    assert (err <= EPS * 1.002 + 5e-6 * np.abs(b)).all(), float((err - 5e-6 * np.abs(b)).max())
    assert err.max() > 0.0      # terms ARE skipped


def test_query_integer_points_and_the_integer_path_on_a_continuous_plan(dev):
    from gsasr_amd import _cabi
    sig, xy, col, H, W = _synth(48, 40, 4.0, seed=21)
    g = torch.Generator().manual_seed(5)
    ipts = torch.stack([torch.randint(0, H, (700,), generator=g), torch.randint(0, W, (700,), generator=g)], dim=1).to(dev)
    ipts[5] = ipts[3]
    gout = torch.rand(3, 700, generator=g).to(dev)
    for dmax in (None, 0.1):
        cont, (a, b, c) = _plan(sig, xy, col, H, W, dmax, dev)
        plain, _ = _plan(sig, xy, col, H, W, dmax, dev, continuous=False)

        def run(plan, pts, fwd, bwd):
            out, st = fwd(plan, pts)
            gr = (torch.empty_like(a), torch.empty_like(b), torch.empty_like(c))
            bwd(plan, st, a, b, c, gout, *gr, overwrite=True)
            return out.cpu().numpy(), [t.cpu().numpy() for t in gr]
        oq, gq = run(cont, ipts.float(), _cabi.query_forward, _cabi.query_backward)
        oi, gi = run(cont, ipts, _cabi.sample_forward, _cabi.sample_backward)
        op, gp = run(plain, ipts, _cabi.sample_forward, _cabi.sample_backward)
        # integer-valued float points: the same px, py bit for bit, the same plan, the same kernels
        assert np.abs(oq - oi).max() <= IMG_ATOL
        # the integer path on the two plans: the same terms up to the cutoff, in another order
        assert np.abs(oi - op).max() <= IMG_ATOL
        for x, y, z, name in zip(gq, gi, gp, ("sigmas", "coords", "colors")):
            assert _relmax(x, y) <= GRAD_RTOL and _relmax(y, z) <= GRAD_RTOL, name
        # the image kernels keep out of a continuous plan
        img = torch.empty(H, W, 3, device=dev)
        with pytest.raises(RuntimeError, match="GSASR_FLAG_CONTINUOUS"):
            _cabi.forward(cont, img, overwrite=True)
        with pytest.raises(RuntimeError, match="GSASR_FLAG_CONTINUOUS"):
            _cabi.forward_u8(cont)
        gr = (torch.empty_like(a), torch.empty_like(b), torch.empty_like(c))
        with pytest.raises(RuntimeError, match="GSASR_FLAG_CONTINUOUS"):
            _cabi.backward(cont, a, b, c, img, *gr, overwrite=True)
        # ... and a forward with plain dims finds no plan on that workspace
        d = _cabi.make_dims(sig.shape[0], H, W, dmax, flags=_cabi.FLAG_OVERWRITE_IMAGE)
        rc = _cabi.lib().gsasr_splat_forward(__import__("ctypes").byref(d), cont.workspace.data_ptr(), cont.workspace.numel(),
                                             img.data_ptr(), None)
        assert rc == -3
    torch.cuda.synchronize()


def test_query_large_class_dead_and_invalid_points(dev):
    """large Gaussians (window > 128 px), dead ones (NaN / off-image), out-of-domain and non-finite points (0, no gradient)"""
    g = torch.Generator().manual_seed(4)
    n, H, W, S = 300, 300, 420, 400
    sig = torch.cat([0.02 + 0.9 * torch.rand(n, 2, generator=g), 1.8 * torch.rand(n, 1, generator=g) - 0.9], dim=1)
    xy = 2.4 * torch.rand(n, 2, generator=g) - 1.2
    col = torch.rand(n, 3, generator=g)
    sig[7, 0] = float("nan")
    xy[9] = torch.tensor([30.0, -30.0])
    pts = _domain_points(H, W, S, seed=1)
    bad = torch.tensor([[-0.5, 3.0], [H - 0.5, 3.0], [5.0, -1e-3], [5.0, W - 1 + 1e-3], [float("nan"), 1.0], [2.0, float("inf")],
                        [float("-inf"), 2.0], [-1.0, -1.0]])      # (no wrap-around for floats)
    pts[50:58] = bad
    valid = np.ones(S, bool)
    valid[50:58] = False
    gout = torch.rand(3, S, generator=g)
    live = [i for i in range(n) if i not in (7, 9)]
    for dmax in (None, 0.7):
        out, grads = _query(sig, xy, col, H, W, dmax, pts.to(dev), gout.to(dev), dev)
        want, gwant = _eval64(sig[live], xy[live], col[live], H, W, dmax, pts, gout)
        assert (out[:, ~valid] == 0).all()
        assert np.abs(out - want).max() <= IMG_ATOL
        for got, wnt, name in zip(grads, gwant, ("sigmas", "coords", "colors")):
            assert np.isfinite(got).all(), name
            assert _relmax(got[live], wnt) <= GRAD_RTOL, name
        gradbars.check_kernel([t[live] for t in grads], gwant, sig[live], 1.0, f"query large class dmax {dmax}")
        assert (grads[0][7] == 0).all() and (grads[2][9] == 0).all()
        # invalid points take no part in the backward: the same gradients without them
        vt = torch.from_numpy(valid)
        _, g2 = _query(sig, xy, col, H, W, dmax, pts[vt].to(dev), gout[:, vt].contiguous().to(dev), dev)
        for x, y in zip(grads, g2):
            assert _relmax(x, y) <= 1e-5


def test_query_accumulate_mode_resort_and_no_points(dev):
    """without OVERWRITE_GRADS the backward adds into the caller's buffers; `resort` sorts the points again (points != NULL);
    n = 0: empty output, zero gradient"""
    from gsasr_amd import _cabi
    sig, xy, col, H, W = _synth(32, 32, 4.0, seed=8)
    plan, (a, b, c) = _plan(sig, xy, col, H, W, 0.2, dev)
    pts = _domain_points(H, W, 500, seed=2).to(dev)
    gout = torch.rand(3, 500, device=dev)
    out, state = _cabi.query_forward(plan, pts)
    g0 = (torch.empty_like(a), torch.empty_like(b), torch.empty_like(c))
    _cabi.query_backward(plan, state, a, b, c, gout, *g0, overwrite=True)          # points = NULL: what the forward sorted
    g1 = (torch.ones_like(a), torch.ones_like(b), torch.ones_like(c))
    _cabi.query_backward(plan, state, a, b, c, gout, *g1, overwrite=False, resort=True)
    for x, y in zip(g0, g1):
        assert _relmax((y - 1).cpu().numpy(), x.cpu().numpy()) <= 1e-5
    out0, st0 = _cabi.query_forward(plan, pts[:0])
    assert out0.shape == (3, 0)
    _cabi.query_backward(plan, st0, a, b, c, gout[:, :0].contiguous(), *g1, overwrite=True)
    assert all(float(t.abs().max()) == 0 for t in g1)
    with pytest.raises(RuntimeError, match="points"):
        _cabi.query_forward(plan, torch.zeros(5, 2, dtype=torch.int64, device=dev))
    with pytest.raises(RuntimeError, match="points"):
        _cabi.query_forward(plan, torch.zeros(5, 3, device=dev))


@pytest.mark.parametrize("mode", ["scale_modify", "scale"])
def test_host_api_query_against_the_cpu_path(mode, dev):
    """generate_2D_gaussian_splatting_query on the GPU (fused prologue + continuous plan + query kernels) against its own CPU
    torch path -- which tests/test_query_points.py pins to the oracle -- values and gs_parameters.grad, both step-size modes"""
    from gsasr_amd import gaussian_splatting as gsp
    g = torch.Generator().manual_seed(12)
    n_lr = 24
    raw = 0.5 * torch.randn(n_lr * n_lr * 4, 9, generator=g)
    raw[:, 7:9] = torch.rand(n_lr * n_lr * 4, 2, generator=g)
    H = W = 96
    pts = _domain_points(H, W, 600, seed=3)
    wgt = torch.rand(3, 600, generator=g)
    kw = dict(default_step_size=1.2, mode=mode, if_dmax=True, dmax_mode="fix", dmax=0.3)
    p0 = raw.clone().requires_grad_(True)
    o0 = gsp.generate_2D_gaussian_splatting_query((H, W), p0, 4.0, torch.tensor([4.0, 4.0]), pts, **kw)
    (o0 * wgt).sum().backward()
    for sm in (torch.tensor([4.0, 4.0]), torch.tensor([4.0, 4.0], device=dev)):      # (a device scale_modify: formed by the plan's first kernel)
        p1 = raw.clone().to(dev).requires_grad_(True)
        o1 = gsp.generate_2D_gaussian_splatting_query((H, W), p1, 4.0, sm, pts.to(dev), **kw)
        assert o1.shape == (3, 600) and o1.is_cuda
        (o1 * wgt.to(dev)).sum().backward()
        assert float((o1.detach().cpu() - o0.detach()).abs().max()) <= IMG_ATOL
        assert _relmax(p1.grad.cpu().numpy(), p0.grad.numpy()) <= GRAD_RTOL
    # unbounded op, points given on the host
    p2, p3 = raw.clone().requires_grad_(True), raw.clone().to(dev).requires_grad_(True)
    o2 = gsp.generate_2D_gaussian_splatting_query((H, W), p2, 4.0, torch.tensor([4.0, 4.0]), pts, if_dmax=False, mode=mode)
    o3 = gsp.generate_2D_gaussian_splatting_query((H, W), p3, 4.0, torch.tensor([4.0, 4.0]), pts, if_dmax=False, mode=mode)
    (o2 * wgt).sum().backward()
    (o3 * wgt.to(dev)).sum().backward()
    assert float((o3.detach().cpu() - o2.detach()).abs().max()) <= IMG_ATOL
    assert _relmax(p3.grad.cpu().numpy(), p2.grad.numpy()) <= GRAD_RTOL
    with pytest.raises(ValueError, match="requires_grad"):
        gsp.generate_2D_gaussian_splatting_query((H, W), p1, 4.0, sm, pts.to(dev).requires_grad_(True), **kw)
    with pytest.raises(ValueError, match="sample_coords"):
        gsp.generate_2D_gaussian_splatting_query((H, W), p1, 4.0, sm, pts.to(dev).long(), **kw)


def test_host_api_batched_query_equals_per_sample(dev):
    """[B,N,9] + float [B,S,2] points through the batched canvas == B single-image queries (ragged sizes)"""
    from gsasr_amd import gaussian_splatting as gsp
    g = torch.Generator().manual_seed(5)
    B, n, S = 4, 12 * 12 * 16, 300
    raw = 0.5 * torch.randn(B, n, 9, generator=g)
    raw[:, :, 7:9] = torch.rand(B, n, 2, generator=g)
    sizes = [(48, 48), (40, 48), (48, 36), (33, 47)]
    scales = [4.0, 4.0, 3.0, 2.75]
    pts = torch.stack([_domain_points(h, w, S, seed=20 + i) for i, (h, w) in enumerate(sizes)]).to(dev)
    pts[1, 60] = torch.tensor([39.5, 3.0])        # outside sample 1's own 40 rows, inside its slot: 0
    wgt = torch.rand(B, 3, S, generator=g).to(dev)
    kw = dict(default_step_size=1.2, mode="scale_modify", if_dmax=True, dmax_mode="fix", dmax=0.5)
    p1 = raw.clone().to(dev).requires_grad_(True)
    o1 = gsp.generate_2D_gaussian_splatting_batch(sizes, p1, scales, [torch.tensor([s, s]) for s in scales], query_coords=pts, **kw)
    assert o1.shape == (B, 3, S) and bool((o1[1, :, 60] == 0).all())
    (o1 * wgt).sum().backward()
    p2 = raw.clone().to(dev).requires_grad_(True)
    o2 = torch.stack([gsp.generate_2D_gaussian_splatting_query(sizes[b], p2[b], scales[b], torch.tensor([scales[b]] * 2), pts[b], **kw)
                      for b in range(B)])
    (o2 * wgt).sum().backward()
    assert float((o1 - o2).abs().max()) <= 2e-5
    assert _relmax(p1.grad.cpu().numpy(), p2.grad.cpu().numpy()) <= GRAD_RTOL
    # ... and each sample against the CPU path
    p3 = raw.clone().requires_grad_(True)
    o3 = gsp.generate_2D_gaussian_splatting_batch(sizes, p3, scales, [torch.tensor([s, s]) for s in scales], query_coords=pts.cpu(), **kw)
    (o3 * wgt.cpu()).sum().backward()
    assert float((o1.detach().cpu() - o3.detach()).abs().max()) <= IMG_ATOL
    assert _relmax(p1.grad.cpu().numpy(), p3.grad.numpy()) <= GRAD_RTOL


def test_host_api_query_under_bf16_autocast(dev):
    """AMP configs run the op inside torch.autocast: the query Functions compute in fp32"""
    from gsasr_amd import gaussian_splatting as gsp
    g = torch.Generator().manual_seed(3)
    raw = 0.5 * torch.randn(16 * 16, 9, generator=g)
    raw[:, 7:9] = torch.rand(16 * 16, 2, generator=g)
    pts = _domain_points(64, 64, 200, seed=4).to(dev)
    kw = dict(default_step_size=1.2, mode="scale_modify", if_dmax=True, dmax_mode="fix", dmax=0.4)
    p0 = raw.clone().to(dev).requires_grad_(True)
    ref = gsp.generate_2D_gaussian_splatting_query((64, 64), p0, 4.0, torch.tensor([4.0, 4.0]), pts, **kw)
    ref.sum().backward()
    p1 = raw.clone().to(dev).requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = gsp.generate_2D_gaussian_splatting_query((64, 64), p1.bfloat16().float(), 4.0, torch.tensor([4.0, 4.0]), pts, **kw)
        out2 = gsp.generate_2D_gaussian_splatting_query((64, 64), p1, 4.0, torch.tensor([4.0, 4.0]), pts, **kw)
    assert out.dtype == torch.float32 and out2.dtype == torch.float32
    out2.sum().backward()
    assert float((out2 - ref).abs().max()) <= 2e-6
    assert _relmax(p1.grad.cpu().numpy(), p0.grad.cpu().numpy()) <= 1e-5
