"""The plan's shortened chain (gsasr_amd/csrc/splat_plan.hip): k_classify hands the largest cell count to k_bin (one atomicMax
per block, beside the dead sub-classes' counters); k_bin's fused scan takes the cutoff's inputs from those words and the extent
lines, every wave for itself, with no block-wide reduction of the histogram.  The cases also cover what was measured and not
kept (groups from runs of equal keys, a DPP scan, block 0 publishing from registers: profiles/plan_chain_ab.txt): the orders
and classes they were built for are inputs any plan must get right.

Bars, by name from tests/test_view_gpu.py: image IMG_ATOL = 1e-4 absolute against oracle.gs_oracle.forward_f64; gradients
GRAD_RTOL = 2e-4 of the tensor's max-abs, `_row_tol` per Gaussian and the per-column bars of tests/gradbars.py against
backward_f64.  Colours are a palette of order 1, well apart: a Gaussian that lost its slot (two Gaussians with one rank: one
record overwritten) shows in the image at 0.1-1, four orders above the bar.

Header words read here (gsasr_amd/csrc/splat_common.h, HDR_WORDS): 0, 1 the normal class' largest half-extents, 2 the largest
cell count, 4 tau', 5 K, 7 the near-dead count, 8, 9 the reach.  The scan-kernel path computes words 2 and 7 from the histogram
itself; which path a plan takes is decided once per process (development switch GSASR_SPLAT_FUSED_MAX), so the other path runs
in a fresh child process: `python tests/test_plan_chain_gpu.py <case> <fused_max>` prints the header of the same input."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))

import gradbars  # noqa: E402

pytestmark = pytest.mark.gpu
IMG_ATOL = 1e-4
GRAD_RTOL = 2e-4
PALETTE = np.array([(1.3, -0.4, 0.9), (0.35, 1.0, 2.5), (-1.0, 0.6, 1.1), (2.0, 0.08, 0.999), (0.7, 1.7, -0.2), (1.05, 0.2, 0.5),
                    (-0.6, -1.2, 1.6)], np.float32)
HDR = ("ext_x", "ext_y", "max_cell", "kc", "tau", "K", "max_block", "near", "reach_x", "reach_y")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the MI355X box)"
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def paint(n, seed=0):
    g = np.random.default_rng(seed)
    return (PALETTE[np.arange(n) % len(PALETTE)] * g.uniform(0.9, 1.0, (n, 1))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def synth(h_lr, w_lr, scale, seed, gpp=1):
    """raster-ordered kernel-frame Gaussians of the package's own prologue, painted with the palette"""
    from gsasr_amd import synthetic
    sig, xy, col, H, W = synthetic.kernel_inputs(h_lr, w_lr, scale, seed=seed, gpp=gpp)
    return sig.numpy().copy(), xy.numpy().copy(), paint(sig.shape[0], seed), H, W


def header(plan):
    torch.cuda.synchronize()
    w = plan.workspace[:40].cpu().numpy().view(np.uint32)
    out = {k: int(v) for k, v in zip(HDR, w)}
    out["tau"] = float(w[4:5].view(np.float32)[0])
    out["kc"] = float(w[3:4].view(np.float32)[0])
    return out


def cell_keys(xy, h, w):
    """k_classify's cell of a centre on the image, in its own fp32 arithmetic (16-px cells, row-major)"""
    f = np.float32
    hx, hy = f(0.5) * f(w - 1), f(0.5) * f(h - 1)
    px = np.clip(np.floor((xy[:, 0].astype(f) + f(1)) * hx), 0, w - 1).astype(np.int64) >> 4
    py = np.clip(np.floor((xy[:, 1].astype(f) + f(1)) * hy), 0, h - 1).astype(np.int64) >> 4
    return py * ((w + 15) // 16) + px


def _row_tol(want, sig):
    kappa = np.maximum(1.0 - np.asarray(sig)[:, 2].astype(np.float64) ** 2, 1e-12)[:, None]
    return (5e-4 + 5e-6 / np.sqrt(kappa)) * np.abs(want).max(axis=1, keepdims=True) + 1e-5 * np.abs(want).max() + 1e-30


def check_grads(got, want, sig, what, column_bar=True):
    for g, w, name in zip(got, want, ("sigmas", "coords", "colors")):
        g, w = np.asarray(g, np.float64), np.asarray(w, np.float64)
        assert np.isfinite(g).all(), (what, name)
        rel = float(np.abs(g - w).max() / max(1e-12, np.abs(w).max()))
        print(f"{what} grad {name}: rel err {rel:.3e}")
        assert rel <= GRAD_RTOL, (what, name, rel)
        bad = np.abs(g - w) > _row_tol(w, sig)
        assert not bad.any(), (what, name, int(np.argwhere(bad)[0][0]), float(np.abs(g - w)[bad].max()), float(np.abs(w).max()))
    gradbars.check_kernel(got, want, sig, 0.0, what, column_bar)


def gradients(plan, ts, wgt):
    from gsasr_amd import _cabi
    out = [torch.full_like(t, float("nan")) for t in ts]
    _cabi.backward(plan, *ts, wgt.contiguous(), *out, overwrite=True)
    return [t.cpu().numpy() for t in out]


def check_rendered(sig, xy, col, H, W, dmax, dev, what, rows=None, cutoff=0.0, view=None, column_bar=True):
    """plan (whole image, a row band or a window (y0, x0, h, w) of the grid), forward and backward against the f64 oracle"""
    from gsasr_amd import _cabi
    from oracle import gs_oracle
    ts = [_t(a, dev) for a in (sig, xy, col)]
    if view is not None:
        y0, x0, h, w = view
        plan = _cabi.plan(*ts, h, w, dmax, cutoff=cutoff, view=(H, W, y0, x0))
        band = (y0, y0 + h)
    else:
        x0, w, band = 0, W, rows or (0, H)
        h = band[1] - band[0]
        plan = _cabi.plan(*ts, H, W, dmax, rows=rows, cutoff=cutoff)
    img = torch.full((h, w, 3), float("nan"), device=dev)
    _cabi.forward(plan, img, overwrite=True)
    img = img.cpu().numpy()
    ref = gs_oracle.forward_f64(sig, xy, col, H, W, dmax, rows=band)[:, x0:x0 + w]
    err = float(np.abs(img - ref).max())
    print(f"{what}: image max|err| {err:.3e} (largest value {np.abs(ref).max():.3f})")
    assert np.isfinite(img).all() and err <= IMG_ATOL, (what, err)
    wgt = torch.rand(h, w, 3, generator=torch.Generator().manual_seed(17))
    pad = np.zeros((h, W, 3), np.float32)
    pad[:, x0:x0 + w] = wgt.numpy()
    want = gs_oracle.backward_f64(sig, xy, col, pad, dmax, h=H, rows=band)
    check_grads(gradients(plan, ts, wgt.to(dev)), want, sig, what, column_bar)
    return plan


# ---- inputs shared with the child process ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stacked_input():
    """20 480 Gaussians (80 k_classify blocks, three extent groups) on 256^2, every seventh on one point: that cell's atomics
    come from every block and group"""
    sig, xy, col, H, W = synth(64, 64, 4.0, 5, gpp=5)
    xy, col = xy.copy(), col.copy()
    xy[::7] = np.array([0.3137, -0.1871], np.float32)
    col[::7] /= 256.0      # 2 926 of them on one pixel: the image stays of order 10, where fp32 still resolves the 1e-4 bar; one lost is 4e-3
    return sig, xy, col, H, W


@functools.lru_cache(maxsize=None)
def groups_input():
    """2 049 k_classify blocks = 65 extent groups of tiny Gaussians on 96 x 80: the wave-level reduction of k_bin loops"""
    n = 2049 * 256 - 3
    g = np.random.default_rng(11)
    H, W = 80, 96
    xy = g.uniform(-0.98, 0.98, (n, 2)).astype(np.float32)
    sig = np.stack([g.uniform(0.4, 0.9, n) * 2 / (W - 1), g.uniform(0.4, 0.9, n) * 2 / (H - 1), g.uniform(-0.3, 0.3, n)], 1).astype(np.float32)
    # the widest one in the LAST group only, the fullest cell fed by the last blocks: a reduction that stops at 64 groups misses both
    sig[-5, 0] = 3.0 * 2 / (W - 1)
    sig[-9, 1] = 2.5 * 2 / (H - 1)
    xy[-4000:] = np.array([-0.52, 0.41], np.float32)
    return sig, xy, paint(n, 3), H, W


CASES = {"stacked": (stacked_input, 0.1), "groups": (groups_input, 0.5)}


def plan_header(case, dev):
    from gsasr_amd import _cabi
    make, dmax = CASES[case]
    sig, xy, col, H, W = make()
    plan = _cabi.plan(*[_t(a, dev) for a in (sig, xy, col)], H, W, dmax)
    tau, k = _cabi.plan_cutoff(plan)
    hd = header(plan)
    assert abs(hd["tau"] - tau) <= 1e-6 * tau and hd["K"] == k
    return hd, plan


def other_path(case, fused_max):
    """the header of `case` planned in a fresh process whose k_bin takes the other path (fused up to `fused_max` blocks)"""
    env = dict(os.environ, GSASR_SPLAT_DEV="1", GSASR_SPLAT_FUSED_MAX=str(fused_max))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), case], capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


# ---- (1) the running maximum across blocks -----------------------------------------------------------------------------------
def test_largest_cell_count_across_blocks_and_groups(dev):
    sig, xy, col, H, W = stacked_input()
    assert sig.shape[0] == 20480
    hd, _ = plan_header("stacked", dev)                       # 80 k_bin blocks: the fused scan
    want = int(np.bincount(cell_keys(xy, H, W)).max())
    assert want >= sig.shape[0] // 7
    assert hd["max_cell"] == want, (hd, want)
    scan = other_path("stacked", 0)                            # the same input through k_scan
    print("fused", hd, "scan", scan)
    assert scan["max_cell"] == want
    assert (hd["tau"], hd["K"]) == (scan["tau"], scan["K"]), (hd, scan)
    for word in ("ext_x", "ext_y", "near", "reach_x", "reach_y", "kc"):
        assert hd[word] == scan[word], (word, hd, scan)
    check_rendered(sig, xy, col, H, W, 0.1, dev, "stacked")


# ---- (2) more than 64 extent groups ------------------------------------------------------------------------------------------
def test_more_than_64_extent_groups(dev):
    sig, xy, col, H, W = groups_input()
    assert (sig.shape[0] + 255) // 256 == 2049
    scan, _ = plan_header("groups", dev)                      # 2 049 blocks: past the fused limit, the scan kernel
    fused = other_path("groups", 1 << 20)                      # ... and every block scanning for itself
    want = int(np.bincount(cell_keys(xy, H, W)).max())
    print("fused", fused, "scan", scan)
    assert scan["max_cell"] == want and fused["max_cell"] == want
    for word in ("tau", "K", "kc", "ext_x", "ext_y", "near", "reach_x", "reach_y"):
        assert fused[word] == scan[word], (word, fused, scan)
    # the widest Gaussians sit in group 64 (3 and 2.5 px under tau ~ 25; the others stay below 0.9 px: at most 9)
    assert fused["ext_x"] >= 15 and fused["ext_y"] >= 15


# ---- (3) key orders inside a wave ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lattice():
    """64 x 64 LR pixels at x4 in raster order, centres within 1.2 px of their LR pixel's centre (2 px from the nearest cell edge):
    a wave is one LR row, 16 cells, 16 runs of four"""
    sig, _, col, H, W = synth(64, 64, 4.0, 9)
    g = np.random.default_rng(8)
    jj, ii = np.meshgrid(np.arange(64), np.arange(64), indexing="xy")
    px = (jj.ravel() + 0.5) * 4.0 + g.uniform(-1.2, 1.2, 4096)
    py = (ii.ravel() + 0.5) * 4.0 + g.uniform(-1.2, 1.2, 4096)
    xy = np.stack([px * 2 / (W - 1) - 1, py * 2 / (H - 1) - 1], 1).astype(np.float32)
    return sig, xy, col, H, W


def alternating(period):
    """the raster set with the first wave's first 32 lanes taken by the Gaussians of two cells, `period` of one, then `period` of
    the other: runs of one key apart from each other (several atomics on one counter); period 1 alternates lane by lane"""
    sig, xy, col, H, W = lattice()
    keys = cell_keys(xy, H, W)
    a = np.flatnonzero(keys == keys[40 * 64 + 20])[:16]
    b = np.flatnonzero(keys == keys[40 * 64 + 30])[:16]
    assert len(a) == 16 and len(b) == 16 and keys[a[0]] != keys[b[0]]
    front = np.stack([a.reshape(-1, period), b.reshape(-1, period)], 1).reshape(-1)
    rest = np.setdiff1d(np.arange(sig.shape[0]), front)
    order = np.concatenate([front, rest])
    heads = 1 + int(np.count_nonzero(np.diff(cell_keys(xy[order[:64]], H, W))))
    return order, heads


def runs_case(name):
    if name == "gpp16-jittered":
        sig, xy, col, H, W = synth(48, 48, 4.0, 21, gpp=16)
        g = np.random.default_rng(4)
        xy = (xy + g.uniform(-8.0, 8.0, xy.shape).astype(np.float32) * np.float32(2.0 / (W - 1))).astype(np.float32)
        return sig, xy, col, H, W, 0.1
    sig, xy, col, H, W = lattice()
    n = sig.shape[0]
    if name == "raster":
        order = np.arange(n)
        runs = [1 + int(np.count_nonzero(np.diff(cell_keys(xy[k:k + 64], H, W)))) for k in range(0, n, 64)]
        assert max(runs) == 16, max(runs)                       # every wave: sixteen runs, sixteen distinct cells
    elif name == "shuffled":
        order = np.random.default_rng(2).permutation(n)
        runs = [1 + int(np.count_nonzero(np.diff(cell_keys(xy[order[k:k + 64]], H, W)))) for k in range(0, n, 64)]
        assert min(runs) > 24, min(runs)                        # every wave: keys in no order
    elif name == "two-cells-runs":
        order, heads = alternating(4)
        assert 8 <= heads <= 24, heads
    else:
        order, heads = alternating(1)
        assert heads > 24, heads
    return sig[order], xy[order], col[order], H, W, 0.1


@pytest.mark.parametrize("name", ["raster", "shuffled", "two-cells-runs", "two-cells-loop", "gpp16-jittered"])
def test_key_orders_inside_a_wave(name, dev):
    sig, xy, col, H, W, dmax = runs_case(name)
    plan = check_rendered(sig, xy, col, H, W, dmax, dev, name)
    assert header(plan)["max_cell"] == int(np.bincount(cell_keys(xy, H, W)).max())


# ---- (4) classes and edges ---------------------------------------------------------------------------------------------------
def test_row_band_with_dead_near_dead_and_large(dev):
    import math
    from gsasr_amd import _cabi
    sig, xy, col, H, W = synth(48, 48, 4.0, 33)
    rows = (64, 136)
    dmax = 1.6                                  # the box reaches 153 px: the wide Gaussians below are of the large class
    n = sig.shape[0]
    hx = 0.5 * (W - 1)
    tau_c = _cabi.resolve_cutoff(0.0, n + 40)
    m = 32                                      # near-dead: support under the conservative cutoff stops just short of column 0
    s2, x2 = np.zeros((m, 3), np.float32), np.zeros((m, 2), np.float32)
    s2[:, 0] = s2[:, 1] = 3.0 / hx
    x2[:, 0] = -1.0 - (math.sqrt(2.0 * tau_c) * 3.0 * 1.000002 + 0.05) / hx
    x2[:, 1] = np.linspace(-0.2, 0.3, m)
    s3, x3 = np.zeros((8, 3), np.float32), np.zeros((8, 2), np.float32)      # large: half-extent beyond 128 px
    s3[:, 0] = 30.0 / hx
    s3[:, 1] = np.linspace(24.0, 34.0, 8) / hx
    s3[:, 2] = np.linspace(-0.5, 0.5, 8)
    x3[:] = np.random.default_rng(6).uniform(-0.6, 0.6, (8, 2))
    sig2, xy2 = np.concatenate([sig, s2, s3]), np.concatenate([xy, x2, x3])
    col2 = np.concatenate([col, paint(m + 8, 1)])
    col2[n + m:] *= 0.05                        # (a wide Gaussian covers 10^4 pixels: keep the image of order 1)
    plan = check_rendered(sig2, xy2, col2, H, W, dmax, dev, "band", rows=rows)
    hd = header(plan)
    assert hd["near"] >= m, hd                  # counted (the band's own near-dead come on top)
    ys = (xy[:, 1].astype(np.float64) + 1.0) * 0.5 * (H - 1)
    assert np.count_nonzero((ys < rows[0] - 40) | (ys > rows[1] + 40)) >= 400      # dead for this band (its support is far shorter than 40 px)


@pytest.mark.parametrize("n", [1, 63, 65, 257, 1023])
def test_ragged_counts(n, dev):
    sig, xy, col, H, W = synth(32, 32, 4.0, 12)
    pick = np.linspace(0, sig.shape[0] - 1, n).astype(np.int64)      # in raster order, spread over the image
    check_rendered(sig[pick], xy[pick], col[pick], H, W, 0.1, dev, f"n={n}", column_bar=n > 1)


def test_unbounded_op(dev):
    sig, xy, col, H, W = synth(24, 24, 4.0, 14)
    check_rendered(sig, xy, col, H, W, None, dev, "unbounded")


def test_one_window(dev):
    sig, xy, col, H, W = synth(48, 40, 4.0, 15)
    plan = check_rendered(sig, xy, col, H, W, 0.1, dev, "window", view=(37, 22, 90, 101))
    assert header(plan)["K"] > 0               # (adaptive: the window's own counts)


def test_canvas_of_three_unequal_samples(dev):
    from gsasr_amd import _cabi
    from oracle import gs_oracle
    samples = [synth(20, 28, 4.0, 41), synth(28, 20, 4.0, 42), synth(24, 24, 2.0, 43)]
    n_per = max(s[0].shape[0] for s in samples)
    parts = []
    for sig, xy, col, _, _ in samples:          # NaN records (dead to every plan) pad a sample to n_per
        fill = n_per - sig.shape[0]
        parts.append([np.concatenate([a, np.full((fill, a.shape[1]), np.nan, np.float32)]) for a in (sig, xy, col)])
    ts = [_t(np.concatenate([p[k] for p in parts]), dev) for k in range(3)]
    sizes = [(H, W) for _, _, _, H, W in samples]
    plan = _cabi.plan(*ts, 0, 0, 0.1, sizes=sizes)
    d = plan.dims
    img = torch.full((d.h, d.w, 3), float("nan"), device=dev)
    _cabi.forward(plan, img, overwrite=True)
    img = img.cpu().numpy()
    grad = torch.full((d.h, d.w, 3), 7.0, device=dev)              # (junk in the padding: the backward must not read it)
    wgts = [torch.rand(H, W, 3, generator=torch.Generator().manual_seed(50 + b)) for b, (H, W) in enumerate(sizes)]
    for b, wgt in enumerate(wgts):
        grad[b * d.slot: b * d.slot + wgt.shape[0], : wgt.shape[1]] = wgt.to(dev)
    got = gradients(plan, ts, grad)
    for b, (sig, xy, col, H, W) in enumerate(samples):
        ref = gs_oracle.forward_f64(sig, xy, col, H, W, 0.1)
        err = float(np.abs(img[b * d.slot: b * d.slot + H, :W] - ref).max())
        print(f"canvas sample {b}: image max|err| {err:.3e}")
        assert err <= IMG_ATOL, (b, err)
        want = gs_oracle.backward_f64(sig, xy, col, wgts[b].numpy(), 0.1)
        n = sig.shape[0]
        check_grads([g[b * n_per: b * n_per + n] for g in got], want, sig, f"canvas sample {b}")
        assert all(not g[b * n_per + n: (b + 1) * n_per].any() for g in got)


# ---- (5) a plan that does not adapt ------------------------------------------------------------------------------------------
def test_explicit_cutoff_publishes_the_extents(dev):
    import math
    sig, xy, col, H, W = synth(48, 40, 4.0, 18)
    tau, dmax = 32.0, 0.1
    plan = check_rendered(sig, xy, col, H, W, dmax, dev, "tau32", cutoff=tau)
    hd = header(plan)
    assert abs(hd["tau"] - tau) <= 1e-4 * tau and hd["K"] == 0, hd
    # every Gaussian of this set is of the normal class (centre on the image, half-extent <= the box: 8 / 10 px)
    k = math.sqrt(2.0 * tau)
    ex = np.ceil(np.minimum(dmax, k * np.abs(sig[:, 0].astype(np.float64))) * 0.5 * (W - 1)).max() + 2
    ey = np.ceil(np.minimum(dmax, k * np.abs(sig[:, 1].astype(np.float64))) * 0.5 * (H - 1)).max() + 2
    assert abs(hd["ext_x"] - ex) <= 1 and abs(hd["ext_y"] - ey) <= 1, (hd, ex, ey)      # (the half-extent is rounded to fp32 before the ceil)
    assert (hd["reach_x"], hd["reach_y"]) == (hd["ext_x"], hd["ext_y"]), hd             # no smaller cutoff: the reach is the extent


if __name__ == "__main__":
    hd, _ = plan_header(sys.argv[1], torch.device("cuda:0"))
    print(json.dumps(hd))
