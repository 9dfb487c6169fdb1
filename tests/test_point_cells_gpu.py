"""GPU parity of the sampled-pixel and query kernels on coarse point-cells and crowded blocks (k_pts_*, k_sample_fwd, k_sample_bwd,
k_query_bwd_pts of gsasr_amd/csrc/splat_sampled.hip), on the inputs of tests/point_cases.py.

Every other test of this path stays at or below 1024 x 768 px, the last size whose point-cells are 8 x 8 px, and draws 1.6-16
points per block.  Here: every pair (shx, shy) an image up to 4096^2 or a canvas of 64 crops reaches, blocks holding exactly 24,
25, 28, 29, 49 and 300 points and 1000 copies of one position (one walk of a point-stationary kernel takes 24 resp. 28), 700
invalid points anywhere in the list, Python's negative indices, the corners of the domain.  tests/test_point_cells.py holds the
conditions that make these inputs worth running: every planted point's reference value is above 1e-3.

Yardsticks and bars are the suite's own: the float64 definitions `_eval64` (tests/test_query_points_gpu.py) and `_pos64`
(tests/test_query_grad_gpu.py), evaluated at the points only; 1e-4 per value, gradients 2e-4 of the tensor's max-abs and every
column to its own bar (tests/gradbars.py, every row in scope).  A slip of the index arithmetic drops a term or writes a value to
another point's slot: an error the size of the value itself.

The canvas the error case uses: 64 samples of (496, 3600), 31744 x 3600 px -- 15872 point-cells at the coarsest cell a canvas
allows (shx, shy) = (9, 4).  Its plan (no tile lists) is accepted; the sampled and query calls on it are refused.
"""
import numpy as np
import pytest
import torch

import gradbars
import point_cases as pc
from test_query_grad_gpu import _pos64
from test_query_points_gpu import GRAD_RTOL, IMG_ATOL, _eval64, _relmax

pytestmark = pytest.mark.gpu

CHUNK = 512      # points per call of the float64 reference: one autograd graph of [512, N] doubles at a time


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the MI355X box)"
    return torch.device("cuda:0")


_REF = {}


def _reference(key, sig, xy, col, H, W, dmax, pos, gout, positions):
    """(values [3,T], (g_sigmas, g_coords, g_colors), position gradient [T,2] or None) in float64, once per `key`.  The gradients
    are linear in grad_out, so the sum over chunks of points is the gradient of the whole."""
    if key not in _REF:
        outs, grads = [], None
        for s0 in range(0, pos.shape[0], CHUNK):
            o, g = _eval64(sig, xy, col, H, W, dmax, pos[s0:s0 + CHUNK], gout[:, s0:s0 + CHUNK])
            outs.append(o)
            grads = g if grads is None else tuple(x + y for x, y in zip(grads, g))
        gp = _pos64(sig, xy, col, H, W, dmax, pos, gout) if positions else None
        for a in (*grads, *(() if gp is None else (gp,))):
            a.setflags(write=False)
        want = np.concatenate(outs, axis=1)
        want.setflags(write=False)
        _REF[key] = (want, grads, gp)
    return _REF[key]


def _nan_like(*ts):
    return tuple(torch.full_like(t, float("nan")) for t in ts)


def _check_values(out, want, P, tag, where=""):
    """values within IMG_ATOL at every valid point, exact zeros at the invalid ones; the worst point named with its block"""
    counts = pc.block_counts(P)
    valid = P.valid.numpy()
    err = np.abs(out - want).max(axis=0)
    err = np.where(np.isfinite(err), err, np.inf)
    worst = int(np.argmax(np.where(valid, err, -1.0)))
    print(f"{tag}: max |value - reference| = {err[worst]:.3e}")
    stray = np.nonzero(~valid & ((out != 0).any(axis=0) | ~np.isfinite(out).all(axis=0)))[0]
    assert stray.size == 0, f"{tag}: {stray.size} invalid points with a value, first {where}{pc.describe(P, int(stray[0]), counts)}"
    bad = np.nonzero(valid & ~(err <= IMG_ATOL))[0]
    assert bad.size == 0, (f"{tag}: {bad.size} points beyond {IMG_ATOL}; worst {err[worst]:.3e} (reference "
                           f"{want[:, worst].tolist()}, got {out[:, worst].tolist()}) at {where}{pc.describe(P, worst, counts)}")
    return float(err[worst])


def _check_grads(grads, gwant, sig, tag):
    rels = [_relmax(g, w) for g, w in zip(grads, gwant)]
    print(f"{tag}: gradient rel-max (sigmas, coords, colors) = " + ", ".join(f"{r:.3e}" for r in rels))
    for g, rel, name in zip(grads, rels, ("sigmas", "coords", "colors")):
        rows = np.nonzero(~np.isfinite(g).all(axis=1))[0]
        assert rows.size == 0, f"{tag}: {name}: {rows.size} rows not finite (unwritten?), first Gaussian {int(rows[0])}"
        assert rel <= GRAD_RTOL, f"{tag}: {name}: rel-max {rel:.3e}"
    elem, col = gradbars.check_kernel(grads, gwant, sig, 1.0, tag)
    print(f"{tag}: worst error / element bar = {elem:.3f}, worst error / column bar = {col:.3f}")


def _check_positions(got, want, P, tag, where=""):
    """the position gradient: finite, exact zero rows at the invalid points, rel-max <= GRAD_RTOL (test_query_grad_gpu._check)"""
    counts = pc.block_counts(P)
    valid = P.valid.numpy()
    err = np.abs(got - want).max(axis=1)
    err = np.where(np.isfinite(err), err, np.inf)
    worst = int(np.argmax(err))
    scale = max(1e-12, float(np.abs(want).max()))
    print(f"{tag}: position gradient rel-max = {err[worst] / scale:.3e} (reference max-abs {scale:.3e})")
    stray = np.nonzero(~valid & (got != 0).any(axis=1))[0]
    assert stray.size == 0, f"{tag}: {stray.size} invalid points with a position gradient, first {where}{pc.describe(P, int(stray[0]), counts)}"
    assert np.isfinite(got).all() and err[worst] <= GRAD_RTOL * scale, (
        f"{tag}: position gradient off by {err[worst]:.3e} = {err[worst] / scale:.3e} of the max-abs (reference {want[worst].tolist()}, "
        f"got {got[worst].tolist()}) at {where}{pc.describe(P, worst, counts)}")


def _case_dmax(C, bounded):
    return pc.bounded_dmax(C.H, C.W) if bounded else None


def _tag(C, kind, bounded, cutoff):
    return (f"{kind} {C.H}x{C.W} (shx, shy) = {C.shifts} {'dmax 8 px' if bounded else 'unbounded'}"
            f"{'' if cutoff == 0.0 else f' tau {cutoff:g}'}")


RUNS = [(s, b, 0.0) for s in pc.SHAPES for b in (False, True)] + [((1500, 1500), b, 104.0) for b in (False, True)]
RUN_IDS = [f"{h}x{w}-s{pc.SHAPES[(h, w)][0][0]}x{pc.SHAPES[(h, w)][0][1]}-{'dmax8px' if b else 'unbounded'}-{'adaptive' if t == 0.0 else 'tau104'}"
           for (h, w), b, t in RUNS]


@pytest.mark.parametrize("shape,bounded,cutoff", RUNS, ids=RUN_IDS)
def test_sampled_pixels_on_coarse_cells_and_crowded_blocks(shape, bounded, cutoff, dev):
    from gsasr_amd import _cabi
    C = pc.single(*shape, False)
    P, dmax = C.P, _case_dmax(C, bounded)
    assert pc.pt_cells(C.H, C.W) == C.shifts
    tag = _tag(C, "sampled", bounded, cutoff)
    a, b, c = (t.to(dev) for t in (C.sig, C.xy, C.col))
    plan = _cabi.plan(a, b, c, C.H, C.W, dmax, cutoff=cutoff)
    out, state = _cabi.sample_forward(plan, P.pts.to(dev))
    g = _nan_like(a, b, c)          # an unwritten row shows
    gout = C.gout.to(dev)
    _cabi.sample_backward(plan, state, a, b, c, gout, *g, overwrite=True)
    torch.cuda.synchronize()
    want, gwant, _ = _reference(("single", shape, False, bounded), C.sig, C.xy, C.col, C.H, C.W, dmax, P.pos, C.gout, False)
    _check_values(out.cpu().numpy(), want, P, tag)
    _check_grads(tuple(t.cpu().numpy() for t in g), gwant, C.sig, tag)
    if shape == (1024, 1024) and not bounded:
        # accumulate mode adds to what the buffers hold (the same sorted points, so the same sums in the same order)
        g1 = tuple(torch.ones_like(t) for t in (a, b, c))
        _cabi.sample_backward(plan, state, a, b, c, gout, *g1, overwrite=False)
        torch.cuda.synchronize()
        for x, y, name in zip(g, g1, ("sigmas", "coords", "colors")):
            assert _relmax((y - 1).cpu().numpy(), x.cpu().numpy()) <= 1e-5, f"{tag}: accumulate mode, {name}"


@pytest.mark.parametrize("shape,bounded,cutoff", RUNS, ids=RUN_IDS)
def test_queries_on_coarse_cells_and_crowded_blocks(shape, bounded, cutoff, dev):
    from gsasr_amd import _cabi
    C = pc.single(*shape, True)
    P, dmax = C.P, _case_dmax(C, bounded)
    tag = _tag(C, "query", bounded, cutoff)
    a, b, c = (t.to(dev) for t in (C.sig, C.xy, C.col))
    plan = _cabi.plan(a, b, c, C.H, C.W, dmax, cutoff=cutoff, flags=_cabi.FLAG_CONTINUOUS)
    out, state = _cabi.query_forward(plan, P.pts.to(dev))
    g = _nan_like(a, b, c)
    gout = C.gout.to(dev)
    _cabi.query_backward(plan, state, a, b, c, gout, *g, overwrite=True)
    gp = _cabi.query_backward_points(plan, state, gout)
    torch.cuda.synchronize()
    assert gp.shape == (P.pts.shape[0], 2) and gp.dtype == torch.float32
    want, gwant, pwant = _reference(("single", shape, True, bounded), C.sig, C.xy, C.col, C.H, C.W, dmax, P.pos, C.gout, True)
    _check_values(out.cpu().numpy(), want, P, tag)
    _check_grads(tuple(t.cpu().numpy() for t in g), gwant, C.sig, tag)
    _check_positions(gp.cpu().numpy(), pwant, P, tag)


def _canvas_reference(C, fractional, dmax):
    """per sample, on its own grid with its own Gaussians"""
    refs = [_reference(("canvas", C.name, fractional, dmax, b), s.sig, s.xy, s.col, s.H, s.W, dmax, s.P.pos, s.gout, fractional)
            for b, s in enumerate(C.samples)]
    gwant = tuple(np.concatenate([r[1][k] for r in refs]) for k in range(3))
    return refs, gwant


@pytest.mark.parametrize("bounded", [False, True], ids=["unbounded", "dmax8px"])
@pytest.mark.parametrize("fractional", [False, True], ids=["sampled", "query"])
@pytest.mark.parametrize("name", list(pc.CANVASES))
def test_batched_canvas_with_coarse_cells(name, fractional, bounded, dev):
    from gsasr_amd import _cabi
    C = pc.canvas(name, fractional)
    ch, cw, _ = pc.canvas_hw(C.sizes)
    assert pc.pt_cells(ch, cw, batched=True) == C.shifts
    dmax = C.dmax if bounded else None
    tag = f"{'query' if fractional else 'sampled'} canvas {name} (shx, shy) = {C.shifts} {'dmax' if bounded else 'unbounded'}"
    a, b, c = (t.to(dev) for t in (C.sig, C.xy, C.col))
    plan = _cabi.plan(a, b, c, 0, 0, dmax, flags=_cabi.FLAG_CONTINUOUS if fractional else 0, sizes=C.sizes)
    fwd, bwd = (_cabi.query_forward, _cabi.query_backward) if fractional else (_cabi.sample_forward, _cabi.sample_backward)
    out, state = fwd(plan, C.pts.to(dev))
    g = _nan_like(a, b, c)
    gout = C.gout.to(dev)
    bwd(plan, state, a, b, c, gout, *g, overwrite=True)
    gp = _cabi.query_backward_points(plan, state, gout) if fractional else None
    torch.cuda.synchronize()
    B = len(C.sizes)
    assert out.shape == (B, 3, pc.CANVAS_POINTS)
    refs, gwant = _canvas_reference(C, fractional, dmax)
    out = out.cpu().numpy()
    worst = 0.0
    for k, (s, (want, _, pwant)) in enumerate(zip(C.samples, refs)):      # a point's value lands in its own sample's [k, :, s] slot
        where = f"sample {k} ({s.H} x {s.W}, canvas rows from {k * C.slot}) "
        worst = max(worst, _check_values(out[k], want, s.P, f"{tag} sample {k}", where))
        if fractional:
            _check_positions(gp[k].cpu().numpy(), pwant, s.P, f"{tag} sample {k}", where)
    print(f"{tag}: max |value - reference| over the samples = {worst:.3e}")
    _check_grads(tuple(t.cpu().numpy() for t in g), gwant, C.sig, tag)


def test_canvas_beyond_the_point_cell_table_is_refused(dev):
    """15872 point-cells at (shx, shy) = (9, 4): GSASR_ERR_ARG before any kernel, from every entry point of the path; the process goes on"""
    from gsasr_amd import _cabi
    sizes = pc.TOO_LARGE
    ch, cw, _ = pc.canvas_hw(sizes)
    shx, shy, ncx, ncy = pc.pt_view(ch, cw, batched=True)
    assert ncx * ncy > pc.PT_CELLS
    B = len(sizes)
    sig, xy, col = pc.gaussians(sizes[0][0], sizes[0][1], B, 0, seed=3)
    a, b, c = (t.to(dev) for t in (sig, xy, col))
    ipts = torch.zeros(B, 4, 2, dtype=torch.int64, device=dev)
    match = "too large for the sampled-pixel path"
    plain = _cabi.plan(a, b, c, 0, 0, 0.01, list_cap=-1, sizes=sizes)
    with pytest.raises(RuntimeError, match=match):
        _cabi.sample_forward(plain, ipts)
    cont = _cabi.plan(a, b, c, 0, 0, 0.01, flags=_cabi.FLAG_CONTINUOUS, list_cap=-1, sizes=sizes)
    with pytest.raises(RuntimeError, match=match):
        _cabi.query_forward(cont, ipts.float())
    # the backward entry points refuse it too (a state as a forward would have left it)
    state = (ipts.int().contiguous(), 4, torch.empty(1 << 20, dtype=torch.uint8, device=dev))
    gout = torch.ones(B, 3, 4, device=dev)
    g = tuple(torch.zeros_like(t) for t in (a, b, c))
    with pytest.raises(RuntimeError, match=match):
        _cabi.sample_backward(plain, state, a, b, c, gout, *g, overwrite=True)
    with pytest.raises(RuntimeError, match=match):
        _cabi.query_backward_points(cont, (ipts.float().contiguous(), 4, state[2]), gout)
    assert all(float(t.abs().max()) == 0 for t in g)
    del plain, cont
    # ... and the process goes on: the smallest canvas of this file's regime answers as before
    C = pc.canvas("64x192", False)
    a, b, c = (t.to(dev) for t in (C.sig, C.xy, C.col))
    plan = _cabi.plan(a, b, c, 0, 0, None, sizes=C.sizes)
    out, _ = _cabi.sample_forward(plan, C.pts.to(dev))
    torch.cuda.synchronize()
    s = C.samples[0]
    want, _, _ = _reference(("canvas", C.name, False, None, 0), s.sig, s.xy, s.col, s.H, s.W, None, s.P.pos, s.gout, False)
    _check_values(out[0].cpu().numpy(), want, s.P, "after the refused calls: canvas 64x192 sample 0")
