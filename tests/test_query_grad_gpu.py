"""GPU parity of the gradient of a query with respect to its POSITIONS (gsasr_*_query_backward_points, `coords_grad=True`).

Yardsticks: a float64 evaluation of the definition written here (`_pos64`: float32 positions and box decisions as the kernels
take them, everything else in double and in the completed-square form, the positions px, py as autograd leaves); the CPU oracle
through the identity d t / d px = -d t / d x_j (tests/test_query_grad.py); the library's own Gaussian backward through the same
identity summed over the points; and the CPU torch path of the host API.  Tolerance: the project's bar for gradients on this
path (tests/test_sampled_pixels.py, tests/test_query_points_gpu.py): 2e-4 of the reference tensor's max-abs, every component
finite.  No test here leaves out points or Gaussians other than the ones it names as invalid or dead.
"""
import math

import numpy as np
import pytest
import torch

from test_query_grad import fit_shift, identity_points, oracle_point_grads, shift_points
from test_query_points_gpu import _domain_points, _plan, _synth, _with_small_gaussians

pytestmark = pytest.mark.gpu

GRAD_RTOL = 2e-4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the MI355X box)"
    return torch.device("cuda:0")


def _relmax(got, want):
    return float(np.abs(got - want).max() / max(1e-12, np.abs(want).max()))


def _pos64(sig, xy, col, H, W, dmax, pts, gout):
    """The definition in float64 (CPU): px = float32(2 c / (W - 1) - 1) formed in double, the box decision from the float32 dx, dy
    against the float32 dmax; E = -(u^2 + B^2 / (1 - rho^2)) / 2 with B = v - rho u, in double; d sum(gout * out) / d (px, py) by
    autograd with px, py as leaves (neither the box test nor the rounding is differentiated), times (2 / (W - 1), 2 / (H - 1)).
    Returns [S,2] (d/dr, d/dc), zero rows outside the closed domain."""
    sig, xy, col = (t.detach().cpu().double() for t in (sig, xy, col))
    gout = gout.detach().cpu().double()
    p = pts.detach().cpu().float()
    r, c = p[:, 0], p[:, 1]
    valid = (r >= 0) & (r <= H - 1) & (c >= 0) & (c <= W - 1)
    r, c = torch.where(valid, r, torch.zeros_like(r)), torch.where(valid, c, torch.zeros_like(c))
    px32, py32 = (2.0 * c.double() / (W - 1) - 1.0).float(), (2.0 * r.double() / (H - 1) - 1.0).float()
    g = torch.zeros(p.shape[0], 2, dtype=torch.float64)
    sx, sy, rho = sig[None, :, 0], sig[None, :, 1], sig[None, :, 2]
    for s0 in range(0, p.shape[0], 512):      # (chunks of points: [512, N] doubles at a time)
        sl = slice(s0, s0 + 512)
        inside = valid[sl, None].expand(-1, sig.shape[0])
        if dmax is not None:
            dxf = px32[sl, None] - xy[:, 0].float()[None, :]
            dyf = py32[sl, None] - xy[:, 1].float()[None, :]
            dm = torch.tensor(float(dmax), dtype=torch.float32)
            inside = inside & (dxf.abs() <= dm) & (dyf.abs() <= dm)
        px, py = px32[sl].double().requires_grad_(True), py32[sl].double().requires_grad_(True)
        u, v = (px[:, None] - xy[None, :, 0]) / sx, (py[:, None] - xy[None, :, 1]) / sy
        B = v - rho * u
        t = torch.where(inside, torch.exp(-0.5 * (u * u + B * B / (1 - rho * rho))), torch.zeros((), dtype=torch.float64))
        ((t @ col).t() * gout[:, sl]).sum().backward()
        g[sl, 0] = py.grad * (2.0 / (H - 1))
        g[sl, 1] = px.grad * (2.0 / (W - 1))
    g[~valid] = 0.0
    return g.numpy()


def _qgrad(sig, xy, col, H, W, dmax, pts, gout, dev, cutoff=0.0, extra_flags=0):
    """query forward + position backward through the plan API -> [S,2] numpy"""
    from gsasr_amd import _cabi
    a, b, c = (t.to(dev).contiguous() for t in (sig, xy, col))
    plan = _cabi.plan(a, b, c, H, W, dmax, cutoff=cutoff, flags=_cabi.FLAG_CONTINUOUS | extra_flags)
    _, state = _cabi.query_forward(plan, pts.to(dev))
    g = _cabi.query_backward_points(plan, state, gout.to(dev).contiguous())
    torch.cuda.synchronize()
    assert g.shape == (pts.shape[0], 2) and g.dtype == torch.float32
    return g.cpu().numpy()


def _check(got, want, tag):
    rel = _relmax(got, want)
    print(f"{tag}: gradient rel-max = {rel:.3e} (reference max-abs {np.abs(want).max():.3e}, shape {got.shape})")
    assert np.isfinite(got).all(), tag
    assert rel <= GRAD_RTOL, tag


CASES = [(48, 40, 4.0, 1, None, 3000), (48, 40, 4.0, 1, 0.1, 3000), (24, 20, 4.0, 16, 0.5, 1500), (20, 16, 12.0, 1, 0.1, 2000),
         (24, 40, 2.5, 1, 0.5, 1000)]
IDS = ["x4-unbounded", "x4-dmax0.1", "x4-16-per-lr-px", "x12", "x2.5"]
# every case under the adaptive cutoff; the two plain x4 cases also at tau = 104 and without a cutoff
RUNS = [(c, 0.0, f"{i}-adaptive") for c, i in zip(CASES, IDS)] + \
       [(c, t, f"{i}-{n}") for c, i in zip(CASES[:2], IDS[:2]) for t, n in ((104.0, "tau104"), (-1.0, "nocut"))]


@pytest.mark.parametrize("case,cutoff", [(c, t) for c, t, _ in RUNS], ids=[n for _, _, n in RUNS])
def test_position_gradient_at_irrational_positions(case, cutoff, dev):
    """(f) the inputs of test_query_irrational_positions, corners and edge points of `_domain_points` included"""
    h_lr, w_lr, scale, gpp, dmax, n = case
    sig, xy, col, H, W = _synth(h_lr, w_lr, scale, seed=13, gpp=gpp)
    pts = _domain_points(H, W, n, seed=17)
    gout = torch.rand(3, n, generator=torch.Generator().manual_seed(8))
    got = _qgrad(sig, xy, col, H, W, dmax, pts, gout, dev, cutoff)
    _check(got, _pos64(sig, xy, col, H, W, dmax, pts, gout), f"{case} cutoff={cutoff}")


@pytest.mark.parametrize("dmax", [None, 0.1], ids=["unbounded", "dmax0.1"])
def test_position_gradient_against_the_oracle_identity(dmax, dev):
    """(g) one oracle backward per point on the refined grid, m = 2"""
    sig, xy, col, H, W = _synth(48, 40, 4.0, seed=21)
    k, gout = identity_points(H, W, 2, seed=77)
    got = _qgrad(sig, xy, col, H, W, dmax, k.to(torch.float32) / 2, gout, dev)
    _check(got, oracle_point_grads(sig, xy, col, H, W, 2, k, gout, dmax), f"oracle identity dmax={dmax}")


@pytest.mark.parametrize("dmax", [None, 0.1], ids=["unbounded", "dmax0.1"])
def test_sum_identity_against_the_gaussian_backward(dmax, dev):
    """(h) sum_s g_px[s] = -sum_j g_coords[j, 0] (and y) against the library's own query_backward on the same plan, points and
    grad_out.  Both sides are sums of the same S x N float32 terms in two groupings; the scale of the comparison is
    sum_j |g_coords[j, axis]|, the size of what the right-hand side adds up (its terms cancel in the sum)."""
    from gsasr_amd import _cabi
    sig, xy, col, H, W = _synth(48, 40, 4.0, seed=13)
    n = 3000
    pts = _domain_points(H, W, n, seed=17).to(dev)
    gout = torch.rand(3, n, generator=torch.Generator().manual_seed(8)).to(dev)
    plan, (a, b, c) = _plan(sig, xy, col, H, W, dmax, dev)
    _, state = _cabi.query_forward(plan, pts)
    g = (torch.empty_like(a), torch.empty_like(b), torch.empty_like(c))
    _cabi.query_backward(plan, state, a, b, c, gout, *g, overwrite=True)
    gp = _cabi.query_backward_points(plan, state, gout)
    torch.cuda.synchronize()
    gc, gp = g[1].double().cpu().numpy(), gp.double().cpu().numpy()
    for axis, unit, name in ((0, (W - 1) / 2.0, "x"), (1, (H - 1) / 2.0, "y")):
        lhs = gp[:, 1 - axis].sum() * unit          # g_points = (d/dr, d/dc): column 1 is x
        rhs, scale = -gc[:, axis].sum(), np.abs(gc[:, axis]).sum()
        print(f"dmax={dmax} {name}: sum_s g_p = {lhs:.6e}, -sum_j g_coords = {rhs:.6e}, scale {scale:.3e}, ratio {abs(lhs - rhs) / scale:.3e}")
        assert np.isfinite(lhs) and abs(lhs - rhs) <= GRAD_RTOL * scale


@pytest.mark.parametrize("cutoff", [0.0, 20.0], ids=["adaptive", "tau20"])
@pytest.mark.parametrize("dmax", [None, 0.1], ids=["unbounded", "dmax0.1"])
def test_position_gradient_between_the_pixel_centres(dmax, cutoff, dev):
    """(i) 64 Gaussians of sigma = 0.05 px between the pixel centres: points at their centre, on their flank (+-0.05 px in r and
    in c) and at the four surrounding pixel centres.  The flank gradients are about 40 x the others: the two subsets are compared
    separately, each against its own max-abs."""
    from gsasr_amd import _cabi
    sig, xy, col, H, W, base, _ = _with_small_gaussians()
    centre, around = base[:64], base[64:]
    flank = torch.cat([centre + torch.tensor(d) for d in ((0.05, 0.0), (-0.05, 0.0), (0.0, 0.05), (0.0, -0.05))])
    pts = torch.cat([flank, centre, around])
    nf = flank.shape[0]
    gout = 0.5 + torch.rand(3, pts.shape[0], generator=torch.Generator().manual_seed(9))
    got = _qgrad(sig, xy, col, H, W, dmax, pts, gout, dev, cutoff)
    want = _pos64(sig, xy, col, H, W, dmax, pts, gout)
    print(f"flank max-abs {np.abs(want[:nf]).max():.3e}, rest max-abs {np.abs(want[nf:]).max():.3e}")
    _check(got[:nf], want[:nf], f"flank dmax={dmax} cutoff={cutoff}")
    _check(got[nf:], want[nf:], f"centre + pixel centres dmax={dmax} cutoff={cutoff}")
    # a plan WITHOUT the flag is refused by both calls
    plain, _ = _plan(sig, xy, col, H, W, dmax, dev, cutoff, continuous=False)
    cont, _ = _plan(sig, xy, col, H, W, dmax, dev, cutoff)
    _, st = _cabi.query_forward(cont, pts.to(dev))
    with pytest.raises(RuntimeError, match="GSASR_FLAG_CONTINUOUS"):
        _cabi.query_backward_points(plain, st, gout.to(dev), resort=True)
    from gsasr_amd import synthetic
    raw = synthetic.gs_parameters(12, 10, seed=1, device=dev)
    ip = torch.tensor([[3, 4], [20, 30], [47, 39]], device=dev)
    _, splan, sst = _cabi.step_sample_forward(raw, torch.tensor([0.3], device=dev), 48, 40, dmax, ip)      # a step plan of integer points
    with pytest.raises(RuntimeError, match="GSASR_FLAG_CONTINUOUS"):
        _cabi.step_query_backward_points(splan, sst, torch.ones(3, 3, device=dev))
    torch.cuda.synchronize()


def test_position_gradient_large_class_dead_and_invalid_points(dev):
    """(j) the input of test_query_large_class_dead_and_invalid_points: large Gaussians (window > 128 px), dead ones (NaN /
    off-image: they contribute nothing), and its eight invalid points (exact zero rows)"""
    g = torch.Generator().manual_seed(4)
    n, H, W, S = 300, 300, 420, 400
    sig = torch.cat([0.02 + 0.9 * torch.rand(n, 2, generator=g), 1.8 * torch.rand(n, 1, generator=g) - 0.9], dim=1)
    xy = 2.4 * torch.rand(n, 2, generator=g) - 1.2
    col = torch.rand(n, 3, generator=g)
    sig[7, 0] = float("nan")
    xy[9] = torch.tensor([30.0, -30.0])
    pts = _domain_points(H, W, S, seed=1)
    bad = torch.tensor([[-0.5, 3.0], [H - 0.5, 3.0], [5.0, -1e-3], [5.0, W - 1 + 1e-3], [float("nan"), 1.0], [2.0, float("inf")],
                        [float("-inf"), 2.0], [-1.0, -1.0]])
    pts[50:58] = bad
    gout = torch.rand(3, S, generator=g)
    live = [i for i in range(n) if i not in (7, 9)]
    for dmax in (None, 0.7):
        got = _qgrad(sig, xy, col, H, W, dmax, pts, gout, dev)
        assert (got[50:58] == 0).all()
        _check(got, _pos64(sig[live], xy[live], col[live], H, W, dmax, pts, gout), f"large class dmax={dmax}")


def test_points_null_resort_no_points_and_a_forward_only_plan(dev):
    """(k) points = NULL (what the forward sorted) against `resort` (points != NULL): the same sums in another order; S = 0; a
    GSASR_FLAG_FORWARD_ONLY continuous plan is accepted and gives what a full plan gives; the call does not depend on a
    Gaussian backward having run before it"""
    from gsasr_amd import _cabi
    sig, xy, col, H, W = _synth(32, 32, 4.0, seed=8)
    pts = _domain_points(H, W, 500, seed=2).to(dev)
    gout = torch.rand(3, 500, generator=torch.Generator().manual_seed(3)).to(dev)
    plan, (a, b, c) = _plan(sig, xy, col, H, W, 0.2, dev)
    _, state = _cabi.query_forward(plan, pts)
    g0 = _cabi.query_backward_points(plan, state, gout)
    g1 = _cabi.query_backward_points(plan, state, gout, resort=True)
    gg = (torch.empty_like(a), torch.empty_like(b), torch.empty_like(c))
    _cabi.query_backward(plan, state, a, b, c, 2.0 * gout, *gg, overwrite=True)      # leaves ANOTHER gradient gathered in the scratch
    g2 = _cabi.query_backward_points(plan, state, gout)
    fo = _cabi.plan(a, b, c, H, W, 0.2, flags=_cabi.FLAG_CONTINUOUS | _cabi.FLAG_FORWARD_ONLY)
    _, sfo = _cabi.query_forward(fo, pts)
    g3 = _cabi.query_backward_points(fo, sfo, gout)
    torch.cuda.synchronize()
    want = _pos64(sig, xy, col, H, W, 0.2, pts, gout)
    _check(g0.cpu().numpy(), want, "points = NULL")
    for other, name in ((g1, "resort"), (g2, "after a Gaussian backward"), (g3, "forward-only plan")):
        assert _relmax(other.cpu().numpy(), g0.cpu().numpy()) <= 1e-5, name
    out0, st0 = _cabi.query_forward(plan, pts[:0])
    e = _cabi.query_backward_points(plan, st0, gout[:, :0].contiguous())
    assert e.shape == (0, 2)
    with pytest.raises(RuntimeError, match="grad_out"):
        _cabi.query_backward_points(plan, state, gout[:, :10].contiguous())


@pytest.mark.parametrize("stacked", [1.0, 0.05], ids=["all-on-one-spot", "a-twentieth"])
def test_position_gradient_on_the_adversarial_stack(stacked, dev):
    """(l) the input of test_query_adversarial_stack_keeps_the_error_bound: the adaptive continuous plan against the tau = 104
    one, position gradients within 2e-4 of the latter's max-abs"""
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
    pts = torch.stack(torch.meshgrid(kr, kc, indexing="ij"), dim=-1).reshape(-1, 2).float() / 2
    gout = torch.rand(3, pts.shape[0], generator=torch.Generator().manual_seed(2))
    adaptive = _qgrad(sig, xy, col, h, w, dmax, pts, gout, dev)
    exact = _qgrad(sig, xy, col, h, w, dmax, pts, gout, dev, cutoff=104.0)
    _check(adaptive, exact, f"stacked={stacked}: adaptive against tau = 104")


def _host_inputs(seed, n_lr=24):
    g = torch.Generator().manual_seed(seed)
    raw = 0.5 * torch.randn(n_lr * n_lr * 4, 9, generator=g)
    raw[:, 7:9] = torch.rand(n_lr * n_lr * 4, 2, generator=g)
    return raw, g


@pytest.mark.parametrize("mode", ["scale_modify", "scale"])
def test_host_api_both_gradients_against_the_cpu_path(mode, dev):
    """(m) generate_2D_gaussian_splatting_query(coords_grad=True) on the GPU against its own CPU torch path (pinned to the oracle
    by tests/test_query_grad.py): gs_parameters.grad and query_coords.grad, both step-size modes, a device scale_modify, host
    and float64 positions"""
    from gsasr_amd import gaussian_splatting as gsp
    raw, g = _host_inputs(12)
    H = W = 96
    pts = _domain_points(H, W, 600, seed=3)
    wgt = torch.rand(3, 600, generator=g)
    kw = dict(default_step_size=1.2, mode=mode, if_dmax=True, dmax_mode="fix", dmax=0.3, coords_grad=True)
    p0, q0 = raw.clone().requires_grad_(True), pts.clone().requires_grad_(True)
    o0 = gsp.generate_2D_gaussian_splatting_query((H, W), p0, 4.0, torch.tensor([4.0, 4.0]), q0, **kw)
    (o0 * wgt).sum().backward()
    for sm in (torch.tensor([4.0, 4.0]), torch.tensor([4.0, 4.0], device=dev)):      # (a device scale_modify: formed by the plan's first kernel)
        p1, q1 = raw.clone().to(dev).requires_grad_(True), pts.clone().to(dev).requires_grad_(True)
        o1 = gsp.generate_2D_gaussian_splatting_query((H, W), p1, 4.0, sm, q1, **kw)
        (o1 * wgt.to(dev)).sum().backward()
        assert float((o1.detach().cpu() - o0.detach()).abs().max()) <= 1e-4
        assert q1.grad.shape == q1.shape and q1.grad.is_cuda and q1.grad.dtype == torch.float32
        _check(p1.grad.cpu().numpy(), p0.grad.numpy(), f"{mode} gs_parameters.grad")
        _check(q1.grad.cpu().numpy(), q0.grad.numpy(), f"{mode} query_coords.grad")
    # unbounded op, float64 positions on the host
    kw.update(if_dmax=False)
    p2, q2 = raw.clone().requires_grad_(True), pts.clone().double().requires_grad_(True)
    p3, q3 = raw.clone().to(dev).requires_grad_(True), pts.clone().double().requires_grad_(True)
    o2 = gsp.generate_2D_gaussian_splatting_query((H, W), p2, 4.0, torch.tensor([4.0, 4.0]), q2, **kw)
    o3 = gsp.generate_2D_gaussian_splatting_query((H, W), p3, 4.0, torch.tensor([4.0, 4.0]), q3, **kw)
    (o2 * wgt).sum().backward()
    (o3 * wgt.to(dev)).sum().backward()
    assert q3.grad.dtype == torch.float64 and not q3.grad.is_cuda and q3.grad.shape == q3.shape
    _check(p3.grad.cpu().numpy(), p2.grad.numpy(), "unbounded gs_parameters.grad")
    _check(q3.grad.numpy(), q2.grad.numpy(), "unbounded query_coords.grad (float64, host)")
    # without the keyword the guard stands
    with pytest.raises(ValueError, match="requires_grad"):
        gsp.generate_2D_gaussian_splatting_query((H, W), p1, 4.0, sm, pts.to(dev).requires_grad_(True), dmax=0.3)
    # S = 0: an empty result with a graph to both inputs
    pe, qe = raw.clone().to(dev).requires_grad_(True), torch.zeros(0, 2, device=dev, requires_grad=True)
    oe = gsp.generate_2D_gaussian_splatting_query((H, W), pe, 4.0, torch.tensor([4.0, 4.0]), qe, **kw)
    assert oe.shape == (3, 0)
    oe.sum().backward()
    assert qe.grad.shape == (0, 2) and pe.grad.shape == pe.shape


def test_host_api_positions_only_and_gaussians_only(dev, monkeypatch):
    """each of the two backward passes runs only when its input needs a gradient"""
    from gsasr_amd import _cabi, gaussian_splatting as gsp
    raw, g = _host_inputs(7, n_lr=12)
    H = W = 48
    pts = _domain_points(H, W, 200, seed=5).to(dev)
    sm = torch.tensor([4.0, 4.0])
    calls = []
    real_g, real_p = _cabi.step_query_backward, _cabi.step_query_backward_points
    monkeypatch.setattr(_cabi, "step_query_backward", lambda *a, **k: (calls.append("gaussians"), real_g(*a, **k))[1])
    monkeypatch.setattr(_cabi, "step_query_backward_points", lambda *a, **k: (calls.append("points"), real_p(*a, **k))[1])
    p, q = raw.clone().to(dev).requires_grad_(True), pts.clone().requires_grad_(True)
    gsp.generate_2D_gaussian_splatting_query((H, W), p, 4.0, sm, q, dmax=0.3, coords_grad=True).sum().backward()
    assert sorted(calls) == ["gaussians", "points"]
    both = q.grad.clone()
    calls.clear()
    p2, q2 = raw.clone().to(dev), pts.clone().requires_grad_(True)
    gsp.generate_2D_gaussian_splatting_query((H, W), p2, 4.0, sm, q2, dmax=0.3, coords_grad=True).sum().backward()
    assert calls == ["points"] and p2.grad is None
    assert _relmax(q2.grad.cpu().numpy(), both.cpu().numpy()) <= 1e-5
    calls.clear()
    p3, q3 = raw.clone().to(dev).requires_grad_(True), pts.clone()
    gsp.generate_2D_gaussian_splatting_query((H, W), p3, 4.0, sm, q3, dmax=0.3, coords_grad=True).sum().backward()
    assert calls == ["gaussians"] and q3.grad is None
    assert _relmax(p3.grad.cpu().numpy(), p.grad.cpu().numpy()) <= 1e-5


def test_host_api_ragged_batch_against_per_sample_and_the_cpu_path(dev):
    """[B,N,9] + float [B,S,2] points through the batched canvas == B single-image calls == the CPU path, for both gradients; the
    point inside a slot but outside its sample gets a zero row"""
    from gsasr_amd import gaussian_splatting as gsp
    g = torch.Generator().manual_seed(5)
    B, n, S = 4, 12 * 12 * 16, 300
    raw = 0.5 * torch.randn(B, n, 9, generator=g)
    raw[:, :, 7:9] = torch.rand(B, n, 2, generator=g)
    sizes = [(48, 48), (40, 48), (48, 36), (33, 47)]
    scales = [4.0, 4.0, 3.0, 2.75]
    pts = torch.stack([_domain_points(h, w, S, seed=20 + i) for i, (h, w) in enumerate(sizes)])
    pts[1, 60] = torch.tensor([39.5, 3.0])        # outside sample 1's own 40 rows, inside its slot
    wgt = torch.rand(B, 3, S, generator=g)
    sms = [torch.tensor([s, s]) for s in scales]
    kw = dict(default_step_size=1.2, mode="scale_modify", if_dmax=True, dmax_mode="fix", dmax=0.5, coords_grad=True)
    p1, q1 = raw.clone().to(dev).requires_grad_(True), pts.clone().to(dev).requires_grad_(True)
    o1 = gsp.generate_2D_gaussian_splatting_batch(sizes, p1, scales, sms, query_coords=q1, **kw)
    (o1 * wgt.to(dev)).sum().backward()
    assert q1.grad.shape == (B, S, 2) and bool((q1.grad[1, 60] == 0).all())
    p2, q2 = raw.clone().to(dev).requires_grad_(True), pts.clone().to(dev).requires_grad_(True)
    o2 = torch.stack([gsp.generate_2D_gaussian_splatting_query(sizes[b], p2[b], scales[b], sms[b], q2[b], **kw) for b in range(B)])
    (o2 * wgt.to(dev)).sum().backward()
    p3, q3 = raw.clone().requires_grad_(True), pts.clone().requires_grad_(True)
    o3 = gsp.generate_2D_gaussian_splatting_batch(sizes, p3, scales, sms, query_coords=q3, **kw)
    (o3 * wgt).sum().backward()
    assert bool((q3.grad[1, 60] == 0).all())
    _check(p1.grad.cpu().numpy(), p2.grad.cpu().numpy(), "batch against per-sample: gs_parameters.grad")
    _check(q1.grad.cpu().numpy(), q2.grad.cpu().numpy(), "batch against per-sample: query_coords.grad")
    _check(p1.grad.cpu().numpy(), p3.grad.numpy(), "batch against the CPU path: gs_parameters.grad")
    _check(q1.grad.cpu().numpy(), q3.grad.numpy(), "batch against the CPU path: query_coords.grad")
    # positions only, on the canvas
    p4, q4 = raw.clone().to(dev), pts.clone().to(dev).requires_grad_(True)
    (gsp.generate_2D_gaussian_splatting_batch(sizes, p4, scales, sms, query_coords=q4, **kw) * wgt.to(dev)).sum().backward()
    assert _relmax(q4.grad.cpu().numpy(), q1.grad.cpu().numpy()) <= 1e-5


def test_host_api_position_gradient_under_bf16_autocast(dev):
    """AMP configs run the op inside torch.autocast: the query Functions compute in fp32, the positions' gradient too"""
    from gsasr_amd import gaussian_splatting as gsp
    raw, _ = _host_inputs(3, n_lr=8)
    pts = _domain_points(64, 64, 200, seed=4).to(dev)
    kw = dict(default_step_size=1.2, mode="scale_modify", if_dmax=True, dmax_mode="fix", dmax=0.4, coords_grad=True)
    p0, q0 = raw.clone().to(dev).requires_grad_(True), pts.clone().requires_grad_(True)
    gsp.generate_2D_gaussian_splatting_query((64, 64), p0, 4.0, torch.tensor([4.0, 4.0]), q0, **kw).sum().backward()
    p1, q1 = raw.clone().to(dev).requires_grad_(True), pts.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = gsp.generate_2D_gaussian_splatting_query((64, 64), p1, 4.0, torch.tensor([4.0, 4.0]), q1, **kw)
    assert out.dtype == torch.float32
    out.sum().backward()
    assert q1.grad.dtype == torch.float32
    assert _relmax(q1.grad.cpu().numpy(), q0.grad.cpu().numpy()) <= 1e-5
    assert _relmax(p1.grad.cpu().numpy(), p0.grad.cpu().numpy()) <= 1e-5


@pytest.mark.parametrize("use_dmax", [False, True], ids=["unbounded", "dmax0.3"])
def test_fitting_a_shift_on_the_gpu(use_dmax, dev):
    """(e) of tests/test_query_grad.py through the host API on the GPU: the same Gaussians (`synthetic.gs_parameters(24, 20,
    seed=3)` at scale 4 are `kernel_inputs(24, 20, 4.0, seed=3)`), points, optimiser and bound"""
    from gsasr_amd import gaussian_splatting as gsp, synthetic
    raw = synthetic.gs_parameters(24, 20, seed=3, device=dev)
    H, W = 96, 80
    pts = shift_points(H, W, 400, seed=9).to(dev)
    sm = torch.tensor([4.0, 4.0])

    def query(q):
        return gsp.generate_2D_gaussian_splatting_query((H, W), raw, 4.0, sm, q, dmax=0.3, if_dmax=use_dmax, coords_grad=True)
    off, truth = fit_shift(query, pts)
    err = float((off - truth).abs().max())
    print(f"use_dmax={use_dmax}: fitted offset {off.tolist()}, |error| = {err:.2e} px")
    assert err <= 0.01
