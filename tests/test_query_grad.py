"""The gradient of a query with respect to its POSITIONS (`coords_grad=True`, gsasr_*_query_backward_points), without a GPU:
the torch CPU path as the executable statement of the semantics, the argument behaviour of the keyword, and the C ABI's names.

The yardstick is the CPU oracle through one identity.  A term's value depends on the position only through px - x_j, so
d t_sj / d px = -d t_sj / d x_j: for ONE point s, g_px[s] = -sum_j g_coords[j, 0] of a Gaussian backward whose weight image is
that point alone.  A point at (k_r / m, k_c / m) IS pixel (k_r, k_c) of the refined (m (H - 1) + 1) x (m (W - 1) + 1) grid
(tests/test_query_points.py), so one `gs_oracle.backward_f64` per point on that grid gives its position gradient, in units of
px, py; (2 / (W - 1), 2 / (H - 1)) of the point's OWN grid turn it into d/dc, d/dr.  Tolerance: the project's bar for gradients
on this path (tests/test_sampled_pixels.py): 2e-4 of the reference tensor's max-abs, every component finite.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from gsasr_amd import _cabi, gaussian_splatting as gsp, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAD_RTOL = 2e-4
NEW = ("gsasr_splat_query_backward_points", "gsasr_step_query_backward_points")


def _relmax(got, want):
    return float(np.abs(got - want).max() / max(1e-12, np.abs(want).max()))


def oracle_point_grads(sig, xy, col, H, W, m, k, gout, dmax):
    """[S,2] (d/dr, d/dc) of the points (k_r / m, k_c / m) through the identity: one oracle backward per point on the refined grid"""
    from oracle import gs_oracle
    Hm, Wm = m * (H - 1) + 1, m * (W - 1) + 1
    s, x, c = sig.numpy(), xy.numpy(), col.numpy()
    want = np.zeros((k.shape[0], 2))
    for i in range(k.shape[0]):
        wgt = np.zeros((Hm, Wm, 3), np.float32)
        wgt[int(k[i, 0]), int(k[i, 1])] = gout[:, i].numpy()
        _, gc, _ = gs_oracle.backward_f64(s, x, c, wgt, dmax)
        want[i, 0] = -gc[:, 1].sum() * 2.0 / (H - 1)
        want[i, 1] = -gc[:, 0].sum() * 2.0 / (W - 1)
    return want


def identity_points(H, W, m, seed):
    """16 points (k_r / m, k_c / m): 13 random ones, a repeat (with the same grad_out column), and two corners of the closed domain"""
    Hm, Wm = m * (H - 1) + 1, m * (W - 1) + 1
    g = torch.Generator().manual_seed(seed)
    k = torch.stack([torch.randint(0, Hm, (16,), generator=g), torch.randint(0, Wm, (16,), generator=g)], dim=1)
    k[13] = k[2]
    k[14] = torch.tensor([0, 0])
    k[15] = torch.tensor([Hm - 1, Wm - 1])
    gout = 0.25 + torch.rand(3, 16, generator=g)
    gout[:, 13] = gout[:, 2]
    return k, gout


@pytest.mark.parametrize("dmax", [None, 0.1], ids=["unbounded", "dmax0.1"])
def test_cpu_path_position_gradient_against_the_oracle_identity(dmax):
    sig, xy, col, H, W = synthetic.kernel_inputs(48, 40, 4.0, seed=21)
    m = 2
    k, gout = identity_points(H, W, m, seed=77)
    pts = (k.to(torch.float32) / m).requires_grad_(True)          # exact: m is a power of two
    out = gsp.query_dense(sig, xy, col, H, W, dmax, pts)
    (out * gout).sum().backward()
    want = oracle_point_grads(sig, xy, col, H, W, m, k, gout, dmax)
    got = pts.grad.numpy()
    rel = _relmax(got, want)
    print(f"dmax={dmax}: position gradient rel-max against the oracle identity = {rel:.3e} (max-abs {np.abs(want).max():.3e})")
    assert np.isfinite(got).all()
    assert np.abs(want).max() > 1e-3          # the check is not vacuous
    assert rel <= GRAD_RTOL
    assert np.array_equal(got[13], got[2])    # a repeated point is an independent output with the same row


def test_cpu_path_invalid_points_get_zero_rows_and_repeats_equal_rows():
    H, W = 48, 40
    raw = synthetic.gs_parameters(12, 10, seed=2)
    bad = torch.tensor([[-0.25, 3.0], [H - 1 + 0.25, 2.0], [5.0, -1e-3], [5.0, W - 1 + 1e-3], [float("nan"), 1.0],
                        [2.0, float("nan")], [2.0, float("inf")], [float("-inf"), 3.0]])
    ok = torch.tensor([[0.0, 0.0], [H - 1.0, W - 1.0], [10.5, 7.25], [10.5, 7.25], [30.2, 20.9]])
    for use_dmax in (True, False):
        pts = torch.cat([ok, bad]).requires_grad_(True)
        out = gsp.generate_2D_gaussian_splatting_query((H, W), raw, 4.0, torch.tensor([4.0, 4.0]), pts, dmax=0.3, if_dmax=use_dmax,
                                                       coords_grad=True)
        (out * torch.arange(1.0, 4.0)[:, None]).sum().backward()
        g = pts.grad
        assert g.shape == pts.shape and bool((g[5:] == 0).all())
        assert bool(torch.isfinite(g).all()) and float(g[:5].abs().min()) > 0          # edges and corners: the analytic value
        assert torch.equal(g[2], g[3])
        # the valid rows are what they are alone
        alone = ok.clone().requires_grad_(True)
        o2 = gsp.generate_2D_gaussian_splatting_query((H, W), raw, 4.0, torch.tensor([4.0, 4.0]), alone, dmax=0.3, if_dmax=use_dmax,
                                                      coords_grad=True)
        (o2 * torch.arange(1.0, 4.0)[:, None]).sum().backward()
        assert torch.equal(alone.grad, g[:5])


def test_the_keyword_and_which_input_gets_a_gradient():
    raw = synthetic.gs_parameters(6, 6, seed=1)
    sm = torch.tensor([4.0, 4.0])
    pts = torch.tensor([[0.5, 0.25], [23.0, 23.0], [11.3, 4.7]])
    # the default is what it was
    with pytest.raises(ValueError, match="requires_grad"):
        gsp.generate_2D_gaussian_splatting_query((24, 24), raw, 4.0, sm, pts.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="requires_grad"):
        gsp.generate_2D_gaussian_splatting_query((24, 24), raw, 4.0, sm, pts.clone().requires_grad_(True), coords_grad=False)
    # with the keyword: shape and dtype of the coordinates, float64 included; the values do not depend on the keyword
    base = gsp.generate_2D_gaussian_splatting_query((24, 24), raw, 4.0, sm, pts)
    grads = {}
    for dt in (torch.float32, torch.float64):
        q = pts.clone().to(dt).requires_grad_(True)
        p = raw.clone().requires_grad_(True)
        out = gsp.generate_2D_gaussian_splatting_query((24, 24), p, 4.0, sm, q, coords_grad=True)
        assert torch.equal(out.detach(), base)
        out.sum().backward()
        assert q.grad.shape == (3, 2) and q.grad.dtype == dt and float(q.grad.abs().max()) > 0
        assert p.grad is not None and float(p.grad.abs().max()) > 0
        grads[dt] = q.grad
    assert _relmax(grads[torch.float32].numpy(), grads[torch.float64].numpy()) <= 1e-5
    # the keyword without requires_grad: nothing to differentiate, nothing raised
    out = gsp.generate_2D_gaussian_splatting_query((24, 24), raw, 4.0, sm, pts, coords_grad=True)
    assert torch.equal(out, base) and not out.requires_grad
    # positions only / Gaussians only
    q = pts.clone().requires_grad_(True)
    gsp.generate_2D_gaussian_splatting_query((24, 24), raw, 4.0, sm, q, coords_grad=True).sum().backward()
    assert raw.grad is None and _relmax(q.grad.numpy(), grads[torch.float32].numpy()) <= 1e-6
    p = raw.clone().requires_grad_(True)
    q = pts.clone()
    gsp.generate_2D_gaussian_splatting_query((24, 24), p, 4.0, sm, q, coords_grad=True).sum().backward()
    assert q.grad is None and p.grad is not None
    # S = 0: an empty result
    q0 = torch.zeros(0, 2, requires_grad=True)
    o0 = gsp.generate_2D_gaussian_splatting_query((24, 24), raw, 4.0, sm, q0, coords_grad=True)
    assert o0.shape == (3, 0)
    o0.sum().backward()
    assert q0.grad.shape == (0, 2)
    # the batch form on CPU tensors: per-sample dense evaluation, each on its own grid
    rawb = torch.stack([raw, raw])
    sizes, scales, sms = [(24, 24), (24, 20)], [4.0, 4.0], [sm, sm]
    qb = torch.tensor([[[0.5, 0.25], [23.0, 23.0]], [[10.0, 19.0], [3.5, 18.75]]], requires_grad=True)
    with pytest.raises(ValueError, match="requires_grad"):
        gsp.generate_2D_gaussian_splatting_batch(sizes, rawb, scales, sms, query_coords=qb)
    with pytest.raises(ValueError, match="query_coords"):
        gsp.generate_2D_gaussian_splatting_batch(sizes, rawb, scales, sms, coords_grad=True)
    ob = gsp.generate_2D_gaussian_splatting_batch(sizes, rawb, scales, sms, query_coords=qb, coords_grad=True)
    assert ob.shape == (2, 3, 2)
    ob.sum().backward()
    assert qb.grad.shape == (2, 2, 2)
    for b in range(2):
        q1 = qb[b].detach().clone().requires_grad_(True)
        gsp.generate_2D_gaussian_splatting_query(sizes[b], rawb[b], 4.0, sm, q1, coords_grad=True).sum().backward()
        assert torch.equal(qb.grad[b], q1.grad)


def test_new_names_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "gsasr_splat.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(gsasr_[a-z_0-9]+)\s*\(", hdr))
    L = ctypes.CDLL(_cabi.LIB_PATH)
    for name in NEW:
        assert name in declared and name in _cabi.EXPORTS and hasattr(L, name), name
    assert re.search(r"#define\s+GSASR_SPLAT_ABI_VERSION\s+7\b", hdr)
    assert _cabi.lib().gsasr_abi_version() == 7
    assert callable(_cabi.query_backward_points) and callable(_cabi.step_query_backward_points)


def fit_shift(query, pts, steps=120, lr=0.05):
    """Adam on a 2-vector offset against the query at pts + (0.3, -0.2); returns the fitted offset"""
    truth = torch.tensor([0.3, -0.2])
    with torch.no_grad():
        target = query(pts + truth.to(pts))
    off = torch.zeros(2, requires_grad=True)
    opt = torch.optim.Adam([off], lr=lr)
    for _ in range(steps):
        opt.zero_grad()
        loss = ((query(pts + off.to(pts)) - target) ** 2).mean()
        loss.backward()
        opt.step()
    return off.detach(), truth


def shift_points(H, W, n, seed):
    g = torch.Generator().manual_seed(seed)
    return 2.0 + torch.rand(n, 2, generator=g) * torch.tensor([H - 5.0, W - 5.0])      # at least 2 px inside the grid


@pytest.mark.parametrize("dmax", [None, 0.3], ids=["unbounded", "dmax0.3"])
def test_fitting_a_shift_on_the_cpu_path(dmax):
    sig, xy, col, H, W = synthetic.kernel_inputs(24, 20, 4.0, seed=3)
    assert (H, W) == (96, 80)
    pts = shift_points(H, W, 400, seed=9)
    off, truth = fit_shift(lambda q: gsp.query_dense(sig, xy, col, H, W, dmax, q), pts)
    err = float((off - truth).abs().max())
    print(f"dmax={dmax}: fitted offset {off.tolist()}, |error| = {err:.2e} px")
    assert err <= 0.01
