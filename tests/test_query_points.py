"""Queries at fractional pixel positions, without a GPU: the torch CPU path of `generate_2D_gaussian_splatting_query` (the
executable statement of the semantics), its argument errors, and the C ABI's new names and workspace sizes.

The yardstick is the CPU oracle on a REFINED grid: a point at (k_r / m, k_c / m) on the H x W grid is pixel (k_r, k_c) of the
(m (H - 1) + 1) x (m (W - 1) + 1) grid -- the kernel-frame tensors are in normalised units and do not depend on the grid, and
for m a power of two k / m is exact in float32 and both grids' table expressions are the same correctly rounded quotient.  The
kernel-frame tensors come from `oracle.host_ref.prologue`, so the host frame is covered by the oracle's own restatement.
Tolerances are the project's (tests/test_sampled_pixels.py): 1e-4 per value, gradients 2e-4 of the tensor's max-abs.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from gsasr_amd import _cabi, gaussian_splatting as gsp, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMG_ATOL = 1e-4
GRAD_RTOL = 2e-4
NEW = ("gsasr_splat_query_forward", "gsasr_splat_query_backward", "gsasr_step_query_forward", "gsasr_step_query_forward_sm",
       "gsasr_step_query_backward")


def _relmax(got, want):
    return float(np.abs(got - want).max() / max(1e-12, np.abs(want).max()))


def _refined_points(H, W, m, seed):
    """EVERY point (k_r / m, k_c / m) of the closed domain, + a few repeats (independent outputs whose gradients add)"""
    Hm, Wm = m * (H - 1) + 1, m * (W - 1) + 1
    kr, kc = torch.meshgrid(torch.arange(Hm), torch.arange(Wm), indexing="ij")
    k = torch.stack([kr.reshape(-1), kc.reshape(-1)], dim=1)
    g = torch.Generator().manual_seed(seed)
    rep = k[torch.randint(0, k.shape[0], (6,), generator=g)]
    k = torch.cat([k, rep, rep[:2]])
    return k, Hm, Wm


@pytest.mark.parametrize("use_dmax", [True, False], ids=["dmax0.3", "unbounded"])
@pytest.mark.parametrize("m", [1, 2, 4])
def test_cpu_path_against_the_refined_grid_oracle(m, use_dmax):
    from oracle import gs_oracle, host_ref
    H, W, scale = 48, 40, 4.0
    raw = synthetic.gs_parameters(12, 10, seed=7 + m)
    sm = torch.tensor([scale, scale])
    k, Hm, Wm = _refined_points(H, W, m, seed=m)
    pts = k.to(torch.float32) / m                      # exact: m is a power of two
    gout = torch.rand(3, pts.shape[0], generator=torch.Generator().manual_seed(3))
    p = raw.clone().requires_grad_(True)
    out = gsp.generate_2D_gaussian_splatting_query((H, W), p, scale, sm, pts, dmax=0.3, if_dmax=use_dmax)
    assert out.shape == (3, pts.shape[0]) and out.dtype == torch.float32
    (out * gout).sum().backward()
    # the oracle on the refined grid, fed with its own restatement of the host frame
    q = raw.clone().requires_grad_(True)
    sig, xy, col, dmax = host_ref.prologue(q, (H, W), sm, 1.2, 0.3, "fix")
    dm = float(dmax) if use_dmax else None
    s, x, c = sig.detach().numpy(), xy.detach().numpy(), col.detach().numpy()
    ref = gs_oracle.forward_f64(s, x, c, Hm, Wm, dm)
    want = ref[k[:, 0].numpy(), k[:, 1].numpy(), :].T
    err = float(np.abs(out.detach().numpy() - want).max())
    print(f"m={m} dmax={dm}: max |value - oracle| = {err:.3e}")
    assert err <= IMG_ATOL
    # the gradient image the points stand for on the refined grid (repeats accumulated), through the oracle's backward and
    # host_ref's chain rule
    wgt = torch.zeros(Hm, Wm, 3, dtype=torch.float32)
    wgt.index_put_((k[:, 0], k[:, 1]), gout.t().contiguous(), accumulate=True)
    gs, gc, gk = gs_oracle.backward_f64(s, x, c, wgt.numpy(), dm)
    ((sig * torch.from_numpy(gs).float()).sum() + (xy * torch.from_numpy(gc).float()).sum() + (col * torch.from_numpy(gk).float()).sum()).backward()
    rel = _relmax(p.grad.numpy(), q.grad.numpy())
    print(f"m={m} dmax={dm}: gradient rel-max = {rel:.3e}")
    assert np.isfinite(p.grad.numpy()).all()
    assert rel <= GRAD_RTOL


def test_cpu_path_outside_the_domain_and_nan_give_zero_and_no_gradient():
    H, W = 48, 40
    raw = synthetic.gs_parameters(12, 10, seed=2)
    bad = torch.tensor([[-0.25, 3.0], [H - 1 + 0.25, 2.0], [5.0, -1e-3], [5.0, W - 1 + 1e-3], [float("nan"), 1.0],
                        [2.0, float("nan")], [2.0, float("inf")], [float("-inf"), 3.0]])
    for use_dmax in (True, False):
        p = raw.clone().requires_grad_(True)
        out = gsp.generate_2D_gaussian_splatting_query((H, W), p, 4.0, torch.tensor([4.0, 4.0]), bad, dmax=0.3, if_dmax=use_dmax)
        assert out.shape == (3, bad.shape[0]) and bool((out == 0).all())
        out.sum().backward()
        assert bool((p.grad == 0).all())
        # next to valid points: the valid ones are what they are alone, the others 0 and without a share in the gradient
        ok = torch.tensor([[0.0, 0.0], [H - 1.0, W - 1.0], [10.5, 7.25]])
        p1, p2 = raw.clone().requires_grad_(True), raw.clone().requires_grad_(True)
        o1 = gsp.generate_2D_gaussian_splatting_query((H, W), p1, 4.0, torch.tensor([4.0, 4.0]), torch.cat([ok, bad]), dmax=0.3, if_dmax=use_dmax)
        o2 = gsp.generate_2D_gaussian_splatting_query((H, W), p2, 4.0, torch.tensor([4.0, 4.0]), ok, dmax=0.3, if_dmax=use_dmax)
        assert torch.equal(o1[:, :3], o2) and bool((o1[:, 3:] == 0).all()) and float(o2.detach().abs().max()) > 0
        o1.sum().backward()
        o2.sum().backward()
        assert torch.equal(p1.grad, p2.grad) and bool(torch.isfinite(p1.grad).all())


def test_cpu_path_integer_points_are_the_pixels():
    """the value at an integer-valued (r, c) IS pixel (r, c): against the oracle on the plain grid through another door (m = 1
    above), and a half-pixel point differs from both neighbours"""
    H, W = 48, 40
    raw = synthetic.gs_parameters(12, 10, seed=4)
    pts = torch.tensor([[10.0, 7.0], [10.5, 7.0], [11.0, 7.0]])
    o = gsp.generate_2D_gaussian_splatting_query((H, W), raw, 4.0, torch.tensor([4.0, 4.0]), pts, cuda_rendering=False)
    assert not torch.equal(o[:, 1], o[:, 0]) and not torch.equal(o[:, 1], o[:, 2])
    # a nested list is taken like a tensor
    o2 = gsp.generate_2D_gaussian_splatting_query((H, W), raw, 4.0, torch.tensor([4.0, 4.0]), pts.tolist())
    assert torch.equal(o, o2)


def test_new_names_abi_version_and_workspace_sizes():
    hdr = open(os.path.join(ROOT, "include", "gsasr_splat.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(gsasr_[a-z_0-9]+)\s*\(", hdr))
    L = ctypes.CDLL(_cabi.LIB_PATH)
    for name in NEW:
        assert name in declared and name in _cabi.EXPORTS and hasattr(L, name), name
    assert re.search(r"#define\s+GSASR_FLAG_CONTINUOUS\s+65536u", hdr) and _cabi.FLAG_CONTINUOUS == 65536
    assert _cabi.lib().gsasr_abi_version() == 7
    nbytes = _cabi.lib().gsasr_splat_workspace_bytes
    for s, h, w in ((65536, 1024, 1024), (1048576, 1024, 1024)):       # config 2's shape; 16 Gaussians per LR pixel
        cont = nbytes(ctypes.byref(_cabi.make_dims(s, h, w, 0.1, flags=_cabi.FLAG_CONTINUOUS)))
        assert cont > 0 and cont == nbytes(ctypes.byref(_cabi.make_dims(s, h, w, 0.1, list_cap=-1)))
        assert cont == nbytes(ctypes.byref(_cabi.make_dims(s, h, w, 0.1, flags=_cabi.FLAG_CONTINUOUS, list_cap=-1)))
    # not combinable with an explicit list capacity, a row band, a view or a kernel-choice flag: a size of 0
    C = _cabi.FLAG_CONTINUOUS
    assert nbytes(ctypes.byref(_cabi.make_dims(65536, 1024, 1024, 0.1, flags=C, list_cap=100))) == 0
    assert nbytes(ctypes.byref(_cabi.make_dims(65536, 1024, 1024, 0.1, rows=(0, 512), flags=C))) == 0
    d = _cabi.make_dims(65536, 256, 256, 0.1, flags=C)
    v = _cabi.View(1024, 1024, 16, 32)
    assert _cabi.lib().gsasr_splat_workspace_bytes_view(ctypes.byref(d), ctypes.byref(v)) == 0
    assert _cabi.lib().gsasr_step_workspace_bytes_view(ctypes.byref(d), ctypes.byref(v)) == 0
    for f in (_cabi.FLAG_FWD_WIDE, _cabi.FLAG_FWD_NARROW, _cabi.FLAG_BWD_GAUSSIAN, _cabi.FLAG_BWD_TILE, _cabi.FLAG_BWD_ATOMIC,
              _cabi.FLAG_BWD_HOME):
        assert nbytes(ctypes.byref(_cabi.make_dims(65536, 1024, 1024, 0.1, flags=C | f))) == 0
    # the sort's scratch serves both kinds of points
    sb = _cabi.lib().gsasr_sample_workspace_bytes
    assert sb(ctypes.byref(_cabi.make_dims(65536, 1024, 1024, 0.1, flags=C)), 1000) == sb(ctypes.byref(_cabi.make_dims(65536, 1024, 1024, 0.1)), 1000) > 0


def test_argument_errors_of_the_query_functions():
    raw = synthetic.gs_parameters(6, 6, seed=1)
    sm = torch.tensor([4.0, 4.0])
    with pytest.raises(ValueError, match="sample_coords"):
        gsp.generate_2D_gaussian_splatting_query((24, 24), raw, 4.0, sm, torch.zeros(5, 2, dtype=torch.int64))
    with pytest.raises(ValueError, match="sample_coords"):
        gsp.generate_2D_gaussian_splatting_query((24, 24), raw, 4.0, sm, [(0, 0), (3, 7)])
    for shape in ((5, 3), (5,), (2, 5, 2)):
        with pytest.raises(ValueError, match=r"\[S,2\]"):
            gsp.generate_2D_gaussian_splatting_query((24, 24), raw, 4.0, sm, torch.zeros(*shape))
    with pytest.raises(ValueError, match="requires_grad"):
        gsp.generate_2D_gaussian_splatting_query((24, 24), raw, 4.0, sm, torch.zeros(5, 2, requires_grad=True))
    rawb = torch.stack([raw, raw])
    sizes, scales, sms = [(24, 24), (24, 20)], [4.0, 4.0], [sm, sm]
    with pytest.raises(ValueError, match="not both"):
        gsp.generate_2D_gaussian_splatting_batch(sizes, rawb, scales, sms, sample_coords=torch.zeros(2, 5, 2, dtype=torch.int64),
                                                 query_coords=torch.zeros(2, 5, 2))
    with pytest.raises(ValueError, match=r"\[B,S,2\]"):
        gsp.generate_2D_gaussian_splatting_batch(sizes, rawb, scales, sms, query_coords=torch.zeros(5, 2))
    with pytest.raises(ValueError, match=r"\[B,S,2\]"):
        gsp.generate_2D_gaussian_splatting_batch(sizes, rawb, scales, sms, query_coords=torch.zeros(3, 5, 2))
    with pytest.raises(ValueError, match="sample_coords"):
        gsp.generate_2D_gaussian_splatting_batch(sizes, rawb, scales, sms, query_coords=torch.zeros(2, 5, 2, dtype=torch.int32))
    with pytest.raises(ValueError, match="requires_grad"):
        gsp.generate_2D_gaussian_splatting_batch(sizes, rawb, scales, sms, query_coords=torch.zeros(2, 5, 2, requires_grad=True))
    # a float sample_coords tensor keeps falling into the reference's indexing loop and raising there
    with pytest.raises((IndexError, TypeError)):
        gsp.generate_2D_gaussian_splatting_step((24, 24), raw, 4.0, sm, sample_coords=torch.zeros(5, 2), cuda_rendering=False)
    # the batch form on CPU tensors: per-sample dense evaluation, each on its own grid
    pts = torch.tensor([[[0.5, 0.25], [23.0, 23.0]], [[10.0, 19.0], [3.5, 18.75]]])
    ob = gsp.generate_2D_gaussian_splatting_batch(sizes, rawb, scales, sms, query_coords=pts)
    assert ob.shape == (2, 3, 2)
    for b in range(2):
        assert torch.equal(ob[b], gsp.generate_2D_gaussian_splatting_query(sizes[b], rawb[b], 4.0, sm, pts[b]))
