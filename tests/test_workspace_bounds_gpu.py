"""The plan, step and sample workspaces at exactly their declared size, between guards, on garbage (tests/wsguard.py).

The size of a workspace (`make_layout`, `make_step_layout`, `make_pt_layout`: gsasr_amd/csrc/splat_common.h, splat_step.hip,
splat_sampled.hip) and the kernels that index it are separate code, kept in agreement by hand.  Every other test takes its workspace
from `torch.empty(nbytes)`, which the caching allocator rounds up and carves from a larger segment: a write past the end is not
seen, and the memory is whatever the allocator had -- often zeros.  Here every workspace is the middle of a `GuardedBytes`: the
library is told `workspace_bytes == n` exactly, 64 KiB of guard on either side must not change, and guards and workspace start
from 0xFF bytes, from zeros and from seeded random bytes (what a pooled workspace holds: the last step's data).

One case per branch of the layout (CASES below: the smallest shape that reaches the branch; <= 128 x 128 px, a few hundred
Gaussians).  Per case and fill: plan, forward and backward, the guards checked after every call, and

  image      <= IMG_ATOL = 1e-4 absolute against oracle.gs_oracle.forward_f64          (tests/test_hip_parity.py)
  gradients  tests/gradbars.py::check_kernel against backward_f64 (every column and element to its own bar)
  raw-parameter gradients of the step entry points: gradbars.check_raw against tests/test_param_grad_columns_gpu.py's truth
  sampled / queried values <= IMG_ATOL, their gradients <= GRAD_RTOL = 2e-4 of the tensor's max-abs + check_kernel
                                                        (tests/test_sampled_pixels.py, test_query_points_gpu.py, test_query_grad_gpu.py)
  8-bit pixels: the oracle's rint(clamp(v, 0, 1) * 255) within one level, exact further than 0.05 levels from a rounding boundary
                                                        (tests/test_store_policy_gpu.py)

Across fills the results agree to ORDER_RTOL = 2e-5 * max(1, max|value|) (tests/test_view_gpu.py: the same sums in another order)
-- the image always (a pixel's sum follows wave timing), the gradients of the Gaussian-stationary kernel, of the atomic path of the
tile-stationary one (BT_WIDE: more tiles than slots) and of the sampled / query backward (float atomics) -- and BIT FOR BIT where
include/gsasr_splat.h documents the kernel as deterministic:
  GSASR_FLAG_BWD_TILE   "deterministic partial-gradient slots + gather"                       (the flag's comment, line 80)
  GSASR_FLAG_BWD_HOME   "no slots, no gather, no atomics, deterministic"                      (the flag's comment, lines 91-92)
  8-bit output of non-overlapping terms is not claimed: <= 1 level.

Every case prints its branch, n, the slack `n - 1 - highest byte written` (how much room an overrun of this case would have to
hide in: the tail of the last array that the case does not write) and its worst errors next to their bars; one run is kept in
profiles/workspace_bounds.txt.

A workspace one byte short is refused before anything is written: GSASR_ERR_WORKSPACE (-2, include/gsasr_splat.h: "workspace too
small or misaligned"), gsasr_last_error() names the workspace, guards and middle keep every byte.
"""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import gradbars
from wsguard import FILLS, GuardedBytes

pytestmark = pytest.mark.gpu

IMG_ATOL = 1e-4         # tests/test_hip_parity.py
GRAD_RTOL = 2e-4        # tests/test_sampled_pixels.py, test_query_points_gpu.py, test_query_grad_gpu.py
ORDER_RTOL = 2e-5       # tests/test_view_gpu.py
ERR_WORKSPACE = -2      # GSASR_ERR_WORKSPACE
HDR_BYTES = 64 * 4      # HDR_WORDS * 4 (gsasr_amd/csrc/splat_common.h): the counter arrays follow the plan header
ENTRY_BYTES = 8         # one tile-list entry (uint2)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the MI355X box)"
    return torch.device("cuda:0")


# ---- scenes: kernel-frame Gaussians as float32 numpy ------------------------------------------------------------------------
class Sample:
    """Gaussians on the H x W grid; `win` = (y0, x0, h, w): the window of it that is rendered (None: all of it)"""

    def __init__(self, sig, xy, col, H, W, win=None):
        self.sig, self.xy, self.col = (np.ascontiguousarray(a, dtype=np.float32) for a in (sig, xy, col))
        self.H, self.W, self.win = H, W, win

    @property
    def hw(self):
        return (self.H, self.W) if self.win is None else tuple(self.win[2:])

    @property
    def origin(self):
        return (0, 0) if self.win is None else tuple(self.win[:2])


def lr_scene(H, W, seed, step=4, gpp=1, win=None):
    """one Gaussian (`gpp`: several) per `step` x `step` pixels in jittered raster order, 0.2 - 1 LR pixels in size, |rho| < 0.8"""
    rng = np.random.default_rng(seed + 1000 * H + W)
    lh, lw = math.ceil(H / step), math.ceil(W / step)
    n = lh * lw * gpp
    jj, ii = np.meshgrid(np.arange(lw), np.arange(lh), indexing="xy")
    cx = np.repeat((jj.ravel() + 0.5) / lw, gpp) + rng.uniform(-0.5, 0.5, n) / lw
    cy = np.repeat((ii.ravel() + 0.5) / lh, gpp) + rng.uniform(-0.5, 0.5, n) / lh
    xy = np.stack([cx, cy], 1) * 2.0 - 1.0
    s = rng.uniform(0.2, 1.0, (n, 2)) * step / 1.2 * 2.0 / np.array([W - 1, H - 1])
    sig = np.concatenate([s, rng.uniform(-0.8, 0.8, (n, 1))], 1)
    col = rng.uniform(0.05, 0.6, (n, 3))
    return Sample(sig, xy, col, H, W, win)


def px_scene(H, W, cx, cy, std, seed, colour=(0.02, 0.2)):
    """Gaussians centred at pixels (cx, cy) (arrays) with stds `std` [n, 2] in pixels"""
    rng = np.random.default_rng(seed)
    n = len(cx)
    xy = np.stack([np.asarray(cx) * 2.0 / (W - 1) - 1.0, np.asarray(cy) * 2.0 / (H - 1) - 1.0], 1)
    sig = np.concatenate([np.asarray(std) * 2.0 / np.array([W - 1, H - 1]), rng.uniform(-0.6, 0.6, (n, 1))], 1)
    return Sample(sig, xy, rng.uniform(*colour, (n, 3)), H, W)


def tile_scene(H, W, tile_h, per_tile, seed):
    """`per_tile` small Gaussians centred inside every 32 x `tile_h`-px tile of the image, the last tile of the last tile row
    included: with per_tile above the list capacity every tile's list overflows"""
    rng = np.random.default_rng(seed)
    cx, cy = [], []
    for ty in range(math.ceil(H / tile_h)):
        for tx in range(math.ceil(W / 32)):
            x1, y1 = min(32 * tx + 32, W), min(tile_h * ty + tile_h, H)
            cx.append(rng.uniform(32 * tx + 0.5, x1 - 1.5, per_tile))
            cy.append(rng.uniform(tile_h * ty + 0.5, y1 - 1.5, per_tile))
    cx, cy = np.concatenate(cx), np.concatenate(cy)
    order = rng.permutation(len(cx))         # (a wave of k_bin then holds Gaussians of several tiles)
    return px_scene(H, W, cx[order], cy[order], rng.uniform(0.6, 1.4, (len(cx), 2)), seed + 1)


def with_wide(smp, seed):
    """the scene with two Gaussians of ~8 px std added: under the unbounded op their windows cover the whole image -- more
    tiles than a plan has slots per Gaussian (BT_WIDE: the tile-stationary backward adds them into `sums` with atomics)"""
    wide = px_scene(smp.H, smp.W, [0.4 * smp.W, 0.7 * smp.W], [0.6 * smp.H, 0.3 * smp.H], [[8.0, 7.0], [6.5, 8.5]], seed, colour=(0.05, 0.3))
    k = smp.sig.shape[0] // 2
    join = lambda a, b: np.concatenate([a[:k], b, a[k:]])
    return Sample(join(smp.sig, wide.sig), join(smp.xy, wide.xy), join(smp.col, wide.col), smp.H, smp.W, smp.win)


def padded(smp, n_per):
    """NaN records (dead to every plan) behind the sample's own, up to `n_per`"""
    fill = n_per - smp.sig.shape[0]
    assert fill >= 0
    pad = lambda a: np.concatenate([a, np.full((fill, a.shape[1]), np.nan, np.float32)])
    out = Sample(pad(smp.sig), pad(smp.xy), pad(smp.col), smp.H, smp.W, smp.win)
    out.live = smp.sig.shape[0]
    return out


def empty_scene(H, W, s, seed=0):
    smp = lr_scene(H, W, seed, step=16)
    return Sample(smp.sig[40:40 + s], smp.xy[40:40 + s], smp.col[40:40 + s], H, W)


# ---- the branch table -----------------------------------------------------------------------------------------------------
def F(name):
    from gsasr_amd import _cabi
    return getattr(_cabi, "FLAG_" + name)


class Case:
    def __init__(self, branch, samples, dmax=0.1, flags=(), fwd=(), list_cap=-1, rows=None, backward=True, bitwise=False,
                 last_entry=False):
        self.branch, self.make_samples, self.dmax, self.flag_names, self.fwd_names = branch, samples, dmax, tuple(flags), tuple(fwd)
        self.list_cap, self.rows, self.backward, self.bitwise, self.last_entry = list_cap, rows, backward, bitwise, last_entry

    @functools.cached_property
    def samples(self):
        smps = self.make_samples()
        if len(smps) > 1:
            n_per = max(s.sig.shape[0] for s in smps)
            smps = [padded(s, n_per) for s in smps]
        return smps

    @property
    def flags(self):
        return sum(F(n) for n in self.flag_names)

    @property
    def fwd_flags(self):
        return sum(F(n) for n in self.fwd_names)

    @property
    def viewed(self):
        return any(s.win is not None for s in self.samples)


CANVAS = [(40, 56), (33, 47), (24, 30)]
CANVAS_GRIDS = [(64, 80, (10, 12, 40, 56)), (48, 60, (7, 5, 33, 47)), (56, 56, (20, 18, 24, 30))]      # H, W, (y0, x0, h, w)

# name -> the branch of make_layout (gsasr_amd/csrc/splat_common.h) it reaches.  list_cap -1: no tile lists unless the row says so
CASES = {
    "plain": Case("no slots, no lists: off_win is the last array; Gaussian-stationary backward",
                  lambda: [lr_scene(70, 50, 1)], flags=["BWD_GAUSSIAN"]),
    "plain-unbounded": Case("the same under the unbounded op (windows from the support, not the dmax box)",
                            lambda: [lr_scene(70, 50, 2)], dmax=None, flags=["BWD_GAUSSIAN"]),
    "bwd-tile": Case("GSASR_FLAG_BWD_TILE: part (32 * part_k bytes per Gaussian) and qspan present, qspan last",
                     lambda: [lr_scene(70, 50, 3)], flags=["BWD_TILE"], bitwise=True),
    "bwd-tile-wide": Case("... with Gaussians whose windows span more tiles than part_k (BT_WIDE: atomics into sums)",
                          lambda: [with_wide(lr_scene(70, 50, 4), 5)], dmax=None, flags=["BWD_TILE"]),
    "bwd-home": Case("GSASR_FLAG_BWD_HOME: the Gaussian-stationary layout, home-tile backward",
                     lambda: [lr_scene(70, 50, 6)], flags=["BWD_HOME"], bitwise=True),
    "forward-only": Case("GSASR_FLAG_FORWARD_ONLY: no fin / sums / done; bbox and win follow rec",
                         lambda: [lr_scene(70, 50, 7)], flags=["FORWARD_ONLY"], backward=False),
    "lists-h4-overflow": Case("tile lists of 32 x 16-px tiles (tl_hlog 4), capacity 64, 72 and more per tile: every list overflows, "
                              "the entries are the last array",
                              lambda: [tile_scene(30, 60, 16, 72, 8)], flags=["FORWARD_ONLY", "FWD_NARROW"], fwd=["FWD_NARROW"],
                              list_cap=64, backward=False, last_entry=True),
    "lists-h5-overflow": Case("tile lists of 32 x 32-px tiles (tl_hlog 5: the wide forward), capacity 64, every list overflows",
                              lambda: [tile_scene(60, 60, 32, 72, 9)], flags=["FORWARD_ONLY", "FWD_WIDE"], fwd=["FWD_WIDE"],
                              list_cap=64, backward=False, last_entry=True),
    "lists-h4-tile-backward": Case("lists and slots: the tile-stationary backward reads the overflowing lists' tiles by the walk",
                                   lambda: [tile_scene(30, 60, 16, 72, 10)], flags=["BWD_TILE", "FWD_NARROW"], fwd=["FWD_NARROW"],
                                   list_cap=64, last_entry=True, bitwise=True),
    "row-band": Case("rows 9 .. 62 of 70 (53 rows: not a multiple of the tile height; tl_ntiles follows the band), lists",
                     lambda: [lr_scene(70, 50, 11)], flags=["BWD_GAUSSIAN", "FWD_NARROW"], fwd=["FWD_NARROW"], list_cap=64, rows=(9, 62)),
    "canvas-3": Case("batched canvas: batch 3, unequal sample_hw, px table x batch, geo table",
                     lambda: [lr_scene(h, w, 12 + b) for b, (h, w) in enumerate(CANVAS)], flags=["BWD_GAUSSIAN"]),
    "canvas-3-tile": Case("... with slots (16-row tiles on a canvas)",
                          lambda: [lr_scene(h, w, 15 + b) for b, (h, w) in enumerate(CANVAS)], flags=["BWD_TILE"], bitwise=True),
    "canvas-3-views": Case("the canvas with one view per sample: off_vtab is the last array",
                           lambda: [lr_scene(H, W, 18 + b, win=win) for b, (H, W, win) in enumerate(CANVAS_GRIDS)], flags=["BWD_GAUSSIAN"]),
    "single-view": Case("one image with a view (gsasr_splat_workspace_bytes_view): a 50 x 70 window of 96 x 112",
                        lambda: [lr_scene(96, 112, 21, step=6, win=(21, 30, 50, 70))], flags=["BWD_GAUSSIAN"]),
    "s0": Case("s == 0 on 128 x 128: one k_classify block zeroes all counters and cursors; the image is zero",
               lambda: [empty_scene(128, 128, 0)], flags=["BWD_GAUSSIAN"]),
    "s1": Case("s == 1 on 128 x 128", lambda: [empty_scene(128, 128, 1)], flags=["BWD_GAUSSIAN"]),
}


def case_dims(case, extra_flags=0):
    from gsasr_amd import _cabi
    smps = case.samples
    flags = case.flags | extra_flags
    if len(smps) == 1:
        h, w = smps[0].hw
        d = _cabi.make_dims(smps[0].sig.shape[0], h, w, case.dmax, case.rows, 0.0, flags, case.list_cap)
        return _cabi.make_view(d, (smps[0].H, smps[0].W, *smps[0].origin) if case.viewed else None)
    sizes = [s.hw for s in smps]
    d = _cabi.make_batch_dims(smps[0].sig.shape[0], sizes, max(w for _, w in sizes), max(h for h, _ in sizes), case.dmax, 0.0, flags)
    d.list_cap = case.list_cap
    return _cabi.make_view(d, [(s.H, s.W, *s.origin) for s in smps] if case.viewed else None)


def rows_of(case, smp):
    return case.rows or (0, smp.hw[0])


@functools.lru_cache(maxsize=None)
def oracle(name):
    """per sample: (image [rows, w, 3], upstream weights [rows, w, 3], gradients) in float64; once per case, never written"""
    from oracle import gs_oracle
    case = CASES[name]
    out = []
    for b, smp in enumerate(case.samples):
        live = getattr(smp, "live", smp.sig.shape[0])
        a, c, k = smp.sig[:live], smp.xy[:live], smp.col[:live]
        (y0, x0), (h, w), (r0, r1) = smp.origin, smp.hw, rows_of(case, smp)
        wgt = np.random.default_rng(100 + b).uniform(-1.0, 1.0, (r1 - r0, w, 3)).astype(np.float32)
        if live == 0:
            out.append((np.zeros((r1 - r0, w, 3)), wgt, None))
            continue
        img = gs_oracle.forward_f64(a, c, k, smp.H, smp.W, case.dmax, rows=(y0 + r0, y0 + r1))[:, x0:x0 + w]
        grads = None
        if case.backward:
            pad = np.zeros((r1 - r0, smp.W, 3), np.float32)
            pad[:, x0:x0 + w] = wgt
            grads = gs_oracle.backward_f64(a, c, k, pad, case.dmax, h=smp.H, rows=(y0 + r0, y0 + r1))
        out.append((img, wgt, grads))
    if name not in ("s0", "s1"):
        assert all(float(np.abs(o[0]).max()) > 0.05 for o in out), name
    return out


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def case_inputs(case, dev):
    return tuple(_t(np.concatenate([getattr(s, k) for s in case.samples]), dev) for k in ("sig", "xy", "col"))


def plan_call(d, inputs, ws, nbytes, dev):
    """gsasr_splat_plan[_view] on `ws` (a uint8 tensor: its address is passed) with workspace_bytes = `nbytes`; the status"""
    from gsasr_amd import _cabi
    fn, _, dargs = _cabi._vcall("gsasr_splat_plan", d)
    return fn(*(t.data_ptr() if t.numel() else None for t in inputs), *dargs, ws.data_ptr(), nbytes, _cabi._stream(dev))


def workspace_bytes(d):
    from gsasr_amd import _cabi
    fn, _, dargs = _cabi._vcall("gsasr_splat_workspace_bytes", d)
    n = int(fn(*dargs))
    assert n > 0, _cabi.lib().gsasr_last_error()
    return n


def last_error():
    from gsasr_amd import _cabi
    return _cabi.lib().gsasr_last_error().decode(errors="replace")


def refused(call, g, what):
    """`call()` must fail with GSASR_ERR_WORKSPACE, the message naming the workspace, and change no byte of guards or middle"""
    before = g.buf.clone()
    try:
        rc = call()
        msg = last_error()
    except RuntimeError as e:       # (the ctypes wrappers raise: "... failed (status -2): message")
        rc, msg = (ERR_WORKSPACE if f"(status {ERR_WORKSPACE})" in str(e) else 0), str(e)
    torch.cuda.synchronize()
    assert rc == ERR_WORKSPACE and "workspace" in msg, (what, rc, msg)
    assert torch.equal(g.buf, before), f"{what}: a refused call wrote"


def canvas_of(case, d, per_sample, dev, fill):
    """the samples' [rows, w, 3] arrays in their slots of a canvas [B * slot, w_max, 3] that holds `fill` elsewhere"""
    if len(case.samples) == 1:
        return _t(per_sample[0], dev)
    t = torch.full((d.h, d.w, 3), float(fill), device=dev)
    for b, a in enumerate(per_sample):
        t[b * d.slot: b * d.slot + a.shape[0], :a.shape[1]] = _t(a, dev)
    return t


def run_case(name, fill, dev, ws=None, nbytes=None, checks=True):
    """plan, forward and backward of case `name` on a workspace that starts from `fill`, through the C ABI with
    workspace_bytes == n exactly.  Returns (the GuardedBytes, per-sample images, gradients or None)"""
    from gsasr_amd import _cabi
    case = CASES[name]
    d = case_dims(case)
    n = workspace_bytes(d)
    inputs = case_inputs(case, dev)
    g = ws if ws is not None else GuardedBytes(n, dev, fill, seed=len(name))
    mid = g.mid if nbytes is None else g.span(nbytes)
    if checks:
        refused(lambda: plan_call(d, inputs, mid, n - 1, dev), g, f"{name} plan, one byte short")
    rc = plan_call(d, inputs, mid, mid.numel(), dev)
    assert rc == 0, (name, rc, last_error())
    torch.cuda.synchronize()
    if checks:
        g.check(f"{name}/{fill} plan")
    plan = _cabi.Plan(d, mid, dev)
    rows = d.row1 - d.row0
    img = torch.full((rows, d.w, 3), float("nan"), device=dev)
    _cabi.forward(plan, img, overwrite=True, flags=case.fwd_flags)
    torch.cuda.synchronize()
    if checks:
        g.check(f"{name}/{fill} forward")
    img = img.cpu().numpy().astype(np.float64)
    slot = d.slot if d.batch > 1 else 0
    images = []
    for b, smp in enumerate(case.samples):
        r0, r1 = rows_of(case, smp)
        images.append(img[b * slot: b * slot + (r1 - r0), :smp.hw[1]])
        if d.batch > 1:     # the padding of a slot: exactly zero under GSASR_FLAG_OVERWRITE_IMAGE
            assert not img[b * slot + smp.hw[0]: (b + 1) * slot].any() and not img[b * slot: (b + 1) * slot, smp.hw[1]:].any(), (name, b)
    grads = None
    if case.backward:
        wgt = canvas_of(case, d, [o[1] for o in oracle(name)], dev, 7.0)     # (junk in the padding: never read)
        out = [torch.full_like(t, float("nan")) for t in inputs]
        _cabi.backward(plan, *inputs, wgt, *out, overwrite=True)
        torch.cuda.synchronize()
        if checks:
            g.check(f"{name}/{fill} backward")
        grads = [t.cpu().numpy() for t in out]
    if checks:
        short = _cabi.Plan(d, mid[:n - 1], dev)
        refused(lambda: _cabi.forward(short, torch.empty(rows, d.w, 3, device=dev), overwrite=True, flags=case.fwd_flags), g,
                f"{name} forward, one byte short")
        if case.backward:
            refused(lambda: _cabi.backward(short, *inputs, wgt, *[torch.empty_like(t) for t in inputs], overwrite=True), g,
                    f"{name} backward, one byte short")
    return g, images, grads


def check_against_oracle(name, images, grads, what):
    """-> (worst image error, worst gradient error / element bar, ... / column bar)"""
    case = CASES[name]
    img_err, elem, col = 0.0, 0.0, 0.0
    n_per = case.samples[0].sig.shape[0]
    for b, (smp, (ref, _, gref)) in enumerate(zip(case.samples, oracle(name))):
        assert np.isfinite(images[b]).all(), (what, b)
        err = float(np.abs(images[b] - ref).max()) if ref.size else 0.0
        img_err = max(img_err, err)
        assert err <= IMG_ATOL, f"{what} sample {b}: image max|err| {err:.3e} > {IMG_ATOL}"
        if grads is None or gref is None:
            continue
        live = getattr(smp, "live", n_per)
        mine = [g[b * n_per: b * n_per + live] for g in grads]
        e, c = gradbars.check_kernel(mine, gref, smp.sig[:live], 1.0, f"{what} sample {b}")
        elem, col = max(elem, e), max(col, c)
        assert all(not g[b * n_per + live: (b + 1) * n_per].any() for g in grads), (what, b)       # NaN records: exactly zero
    return img_err, elem, col


def order_bar(a):
    return ORDER_RTOL * max(1.0, float(np.abs(a).max()) if a.size else 0.0)


def check_across_fills(name, base, other, what, bitwise):
    (img0, g0), (img1, g1) = base, other
    for b, (x, y) in enumerate(zip(img0, img1)):
        assert float(np.abs(x - y).max()) <= order_bar(x) if x.size else True, (what, "image", b)
    if g0 is None:
        return
    for x, y, t in zip(g0, g1, ("sigmas", "coords", "colors")):
        if bitwise:
            assert np.array_equal(x, y), f"{what}: gradient {t} differs in {int((x != y).sum())} elements, max {np.abs(x - y).max():.3e}"
        elif x.size:
            assert float(np.abs(x - y).max()) <= order_bar(x), (what, t, float(np.abs(x - y).max()), order_bar(x))


@pytest.mark.parametrize("name", list(CASES))
def test_layout_branch(name, dev):
    case = CASES[name]
    runs = {fill: run_case(name, fill, dev) for fill in FILLS}
    n = runs[FILLS[0]][0].n
    highest = max(runs[a][0].highest_written(runs[b][0]) for a in FILLS for b in FILLS if a != b)
    slack = n - 1 - highest
    print(f"\n{name}: {case.branch}\n{name}: n = {n}, slack = {slack} bytes behind the highest byte written")
    for fill in FILLS:
        _, images, grads = runs[fill]
        img_err, elem, col = check_against_oracle(name, images, grads, f"{name}/{fill}")
        print(f"{name}/{fill}: image max|err| {img_err:.3e} (bar {IMG_ATOL:.0e}); gradient worst error / element bar {elem:.3f}, "
              f"/ column bar {col:.3f} (bars 1)" + ("" if case.backward else " -- no backward"))
    for fill in FILLS[1:]:
        check_across_fills(name, runs[FILLS[0]][1:], runs[fill][1:], f"{name}: {FILLS[0]} against {fill}", case.bitwise)
    assert 0 <= slack < n
    if case.last_entry:      # the cap check ran on the last slot of the last tile: the workspace's final eight bytes
        assert slack < ENTRY_BYTES, f"{name}: the last entry slot of the workspace was not written (slack {slack})"
    if name == "s0":
        assert all(not im.any() for im in runs[FILLS[0]][1])
    if name == "bwd-tile-wide":
        wide_path_is_reached(case)


def wide_path_is_reached(case):
    """the BT_WIDE row stays one: the plan's slots per Gaussian (part_k, read off the workspace size: the plan with slots carries
    align256(32 s part_k) + align256(16 s) bytes more than the one without) are fewer than the 32 x 16-px tiles that the window
    of a wide Gaussian covers -- the whole image under the unbounded op; 16-row tiles: h w < 64 s (bt_tall, splat_common.h)"""
    from gsasr_amd import _cabi
    smp = case.samples[0]
    s, (h, w) = smp.sig.shape[0], smp.hw
    size = lambda flag: workspace_bytes(_cabi.make_dims(s, h, w, case.dmax, None, 0.0, F(flag), case.list_cap))      # noqa: E731
    up = lambda v: (v + 255) // 256 * 256      # noqa: E731
    extra = size("BWD_TILE") - size("BWD_GAUSSIAN")
    part_k = [k for k in (8, 16) if up(32 * s * k) + up(16 * s) == extra]
    assert len(part_k) == 1, (extra, s)
    assert case.dmax is None and h * w < 64 * s
    tiles = ((w + 31) // 32) * ((h + 15) // 16)
    px = (np.abs(smp.sig[:, :2]) * np.array([w - 1, h - 1]) / 2.0).min(axis=1)        # the smaller std in pixels
    assert (px > 6.0).sum() == 2 and tiles > part_k[0], (tiles, part_k)       # 4 std of the two wide Gaussians reaches every tile


def test_the_guard_reports_a_write_that_the_layout_allows(dev):
    """Can this file fail?  The same plan with workspace_bytes = n, but the helper is told that the region ends 256 bytes earlier:
    what the library may write there is a write into the guard for the helper -- all of it inside the helper's own allocation --
    and it must say so.  The case is one whose last 256 bytes are written (its highest_written)."""
    name = "lists-h4-overflow"
    d = case_dims(CASES[name])
    n = workspace_bytes(d)
    a, b = (run_case(name, fill, dev, checks=False)[0] for fill in ("ff", "zero"))
    assert a.intact() and b.intact()
    tail = (a.written() | b.written())[n - 256:]
    assert a.highest_written(b) >= n - ENTRY_BYTES and tail.mean() > 0.5
    for fill in FILLS:
        g = GuardedBytes(n - 256, dev, fill, seed=3)
        _, images, _ = run_case(name, fill, dev, ws=g, nbytes=n, checks=False)
        c = g.intact()
        print(f"{name}/{fill} with the guard 256 bytes early: {c!r}")
        assert not c and n - 256 <= c.first <= c.last <= n - 1, repr(c)
        check_against_oracle(name, images, None, f"{name}/{fill} short guard")


# ---- reuse: four plans in a row on one workspace, parity alternating ----------------------------------------------------------
REUSE_HW = (72, 56)
REUSE_S = 252       # 18 x 14 LR pixels


@functools.lru_cache(maxsize=None)
def reuse_inputs():
    """four scenes of REUSE_S Gaussians on 72 x 56 under the unbounded op: LR-pixel sized; mostly dead (NaN, or support off the
    image) and large (half-extent beyond 128 px: std 1.5 - 2 in grid units); all in one 16 x 16-px cell; LR-pixel sized again"""
    from oracle import gs_oracle
    H, W = REUSE_HW
    first, last = lr_scene(H, W, 31), lr_scene(H, W, 34)
    assert first.sig.shape[0] == REUSE_S
    rng = np.random.default_rng(32)
    mixed = lr_scene(H, W, 33)
    kind = rng.permutation(REUSE_S)
    nan, off, large = kind[:90], kind[90:150], kind[150:215]
    mixed.sig[nan], mixed.xy[nan], mixed.col[nan] = np.nan, np.nan, np.nan
    mixed.xy[off] = mixed.xy[off] + np.where(rng.uniform(size=(60, 1)) < 0.5, 7.0, -7.0)       # far outside [-1, 1]
    mixed.sig[large, :2] = rng.uniform(1.5, 2.0, (65, 2))      # std 41 .. 71 px: half-extent far beyond 128 px at any tau >= 16
    mixed.col[large] = rng.uniform(0.005, 0.02, (65, 3))
    cell = px_scene(H, W, rng.uniform(33.0, 46.0, REUSE_S), rng.uniform(17.0, 30.0, REUSE_S), rng.uniform(0.7, 1.5, (REUSE_S, 2)), 35,
                    colour=(0.005, 0.05))
    out = []
    for k, smp in enumerate((first, mixed, cell, last)):
        wgt = np.random.default_rng(40 + k).uniform(-1.0, 1.0, (H, W, 3)).astype(np.float32)
        live = np.isfinite(smp.sig).all(axis=1)
        img = gs_oracle.forward_f64(smp.sig[live], smp.xy[live], smp.col[live], H, W, None)
        grads = gs_oracle.backward_f64(smp.sig[live], smp.xy[live], smp.col[live], wgt, None)
        out.append((smp, wgt, live, img, grads))
    return out


@pytest.mark.parametrize("kernel", ["BWD_GAUSSIAN", "BWD_TILE", "BWD_HOME"])
def test_four_plans_on_one_workspace(kernel, dev):
    """plan 1 without GSASR_FLAG_COUNTERS_CLEAN on seeded garbage, plans 2 - 4 with it and the alternating GSASR_FLAG_PARITY, as
    the workspace pool of gsasr_amd/_cabi.py and gsasr_autograd.cpp use a workspace; every plan against the oracle, and after every
    plan the OTHER parity's whole counter array (cells, extent groups, dead-class lines) is zero: the next plan's promise"""
    from gsasr_amd import _cabi
    H, W = REUSE_HW
    base = _cabi.make_dims(REUSE_S, H, W, None, None, 0.0, F(kernel), -1)
    n = workspace_bytes(base)
    count_bytes = int(_cabi.lib().gsasr_splat_counter_bytes(ctypes.byref(base)))
    assert count_bytes > 0 and count_bytes % 256 == 0 and HDR_BYTES + 2 * count_bytes < n
    g = GuardedBytes(n, dev, "seeded", seed=17)
    for k, (smp, wgt, live, ref, gref) in enumerate(reuse_inputs()):
        parity = k & 1
        flags = F(kernel) | (F("COUNTERS_CLEAN") if k else 0) | (F("PARITY") if parity else 0)
        d = _cabi.make_dims(REUSE_S, H, W, None, None, 0.0, flags, -1)
        assert workspace_bytes(d) == n
        inputs = tuple(_t(a, dev) for a in (smp.sig, smp.xy, smp.col))
        assert plan_call(d, inputs, g.mid, n, dev) == 0, last_error()
        torch.cuda.synchronize()
        g.check(f"plan {k + 1}")
        other = HDR_BYTES + (1 - parity) * count_bytes
        assert not g.mid[other: other + count_bytes].any(), f"plan {k + 1} ({kernel}): the counters of parity {1 - parity} are not zero"
        plan = _cabi.Plan(d, g.mid, dev)
        img = torch.full((H, W, 3), float("nan"), device=dev)
        _cabi.forward(plan, img, overwrite=True)
        out = [torch.full_like(t, float("nan")) for t in inputs]
        _cabi.backward(plan, *inputs, _t(wgt, dev), *out, overwrite=True)
        torch.cuda.synchronize()
        g.check(f"plan {k + 1}: forward and backward")
        assert not g.mid[other: other + count_bytes].any(), f"plan {k + 1} ({kernel}): forward / backward touched the clean counters"
        img = img.cpu().numpy().astype(np.float64)
        err = float(np.abs(img - ref).max())
        grads = [t.cpu().numpy() for t in out]
        assert all(not a[~live].any() for a in grads), k        # dead records: exactly zero
        elem, col = gradbars.check_kernel([a[live] for a in grads], gref, smp.sig[live], 1.0, f"{kernel} plan {k + 1}")
        print(f"{kernel} plan {k + 1} (parity {parity}): image max|err| {err:.3e} (bar {IMG_ATOL:.0e}, largest value {np.abs(ref).max():.2f}); "
              f"gradient worst error / element bar {elem:.3f}, / column bar {col:.3f}")
        assert np.isfinite(img).all() and err <= IMG_ATOL, (kernel, k, err)


# ---- the sample workspace (make_pt_layout) behind a GSASR_FLAG_CONTINUOUS plan ---------------------------------------------------
PT_SIZES = {1: [(44, 52)], 3: [(44, 52), (33, 47), (40, 36)]}
PT_DMAX = 0.3


@functools.lru_cache(maxsize=None)
def point_case(batch, n_points):
    """per sample: the scene, integer points, fractional points, grad_out, and the float64 values and gradients of both"""
    from oracle import gs_oracle
    from test_query_grad_gpu import _pos64
    from test_query_points_gpu import _eval64
    out = []
    for b, (H, W) in enumerate(PT_SIZES[batch]):
        smp = lr_scene(H, W, 50 + b)
        g = torch.Generator().manual_seed(1000 * n_points + b)
        ipts = torch.stack([torch.randint(0, H, (n_points,), generator=g), torch.randint(0, W, (n_points,), generator=g)], dim=1)
        fpts = torch.rand(n_points, 2, generator=g) * torch.tensor([H - 1.0, W - 1.0])
        if n_points > 8:
            ipts[5] = ipts[7] = ipts[3]         # repeated points are independent outputs whose gradients add
            fpts[0], fpts[1] = torch.tensor([0.0, 0.0]), torch.tensor([H - 1.0, W - 1.0])       # corners of the closed domain
        gout = torch.rand(3, n_points, generator=g)
        a, c, k = smp.sig, smp.xy, smp.col
        ref = gs_oracle.forward_f64(a, c, k, H, W, PT_DMAX)
        ival = ref[ipts[:, 0].numpy(), ipts[:, 1].numpy(), :].T
        wgt = torch.zeros(H, W, 3)
        wgt.index_put_((ipts[:, 0], ipts[:, 1]), gout.t().contiguous(), accumulate=True)
        igrads = gs_oracle.backward_f64(a, c, k, wgt.numpy(), PT_DMAX)
        ts = tuple(torch.from_numpy(t) for t in (a, c, k))
        fval, fgrads = _eval64(*ts, H, W, PT_DMAX, fpts, gout)
        fpos = _pos64(*ts, H, W, PT_DMAX, fpts, gout)
        out.append(dict(smp=smp, ipts=ipts, fpts=fpts, gout=gout, ival=ival, igrads=igrads, fval=fval, fgrads=fgrads, fpos=fpos))
    return out


def relmax(got, want):
    return float(np.abs(got - want).max() / max(1e-12, np.abs(want).max()))


def run_points(batch, n_points, fill, dev):
    """a GSASR_FLAG_CONTINUOUS plan and, on it, the sampled forward / backward and the query forward / backward / position
    backward, each with its own guarded sample workspace.  Returns ({name: per-sample arrays}, slack of the sample workspace)"""
    from gsasr_amd import _cabi
    per = point_case(batch, n_points)
    sizes = PT_SIZES[batch]
    n_per = per[0]["smp"].sig.shape[0] if batch == 1 else max(p["smp"].sig.shape[0] for p in per)
    smps = [p["smp"] if batch == 1 else padded(p["smp"], n_per) for p in per]
    if batch == 1:
        d = _cabi.make_dims(n_per, *sizes[0], PT_DMAX, None, 0.0, F("CONTINUOUS"), -1)
    else:
        d = _cabi.make_batch_dims(n_per, sizes, max(w for _, w in sizes), max(h for h, _ in sizes), PT_DMAX, 0.0, F("CONTINUOUS"))
        d.list_cap = -1
    n = workspace_bytes(d)
    inputs = tuple(_t(np.concatenate([getattr(s, k) for s in smps]), dev) for k in ("sig", "xy", "col"))
    g = GuardedBytes(n, dev, fill, seed=n_points)
    refused(lambda: plan_call(d, inputs, g.mid, n - 1, dev), g, "continuous plan, one byte short")
    assert plan_call(d, inputs, g.mid, n, dev) == 0, last_error()
    plan = _cabi.Plan(d, g.mid, dev)
    L, st = _cabi.lib(), _cabi._stream(dev)
    n_sws = int(L.gsasr_sample_workspace_bytes(ctypes.byref(d), n_points))
    assert n_sws > 0
    stack = lambda key: (per[0][key] if batch == 1 else torch.stack([p[key] for p in per])).to(dev).contiguous()
    gout = stack("gout")
    res, guards = {}, []
    for kind, pts in (("sampled", stack("ipts")), ("query", stack("fpts"))):
        sws = GuardedBytes(n_sws, dev, fill, seed=n_points + 7)
        guards.append(sws)
        fwd, bwd = (_cabi.sample_forward, _cabi.sample_backward) if kind == "sampled" else (_cabi.query_forward, _cabi.query_backward)
        name = "gsasr_splat_sample_forward" if kind == "sampled" else "gsasr_splat_query_forward"
        dpts = pts.to(torch.int32) if kind == "sampled" else pts
        scratch_out = torch.empty(batch * 3 * n_points, device=dev)
        refused(lambda: getattr(L, name)(ctypes.byref(d), g.mid.data_ptr(), n, dpts.data_ptr(), n_points, scratch_out.data_ptr(),
                                         sws.mid.data_ptr(), n_sws - 1, st), sws, f"{name}, sample workspace one byte short")
        refused(lambda: getattr(L, name)(ctypes.byref(d), g.mid.data_ptr(), n - 1, dpts.data_ptr(), n_points, scratch_out.data_ptr(),
                                         sws.mid.data_ptr(), n_sws, st), g, f"{name}, plan workspace one byte short")
        out, state = fwd(plan, pts, sample_ws=sws.mid)
        torch.cuda.synchronize()
        sws.check(f"{kind} forward: sample workspace"), g.check(f"{kind} forward: plan workspace")
        grads = [torch.full_like(t, float("nan")) for t in inputs]
        bwd(plan, state, *inputs, gout, *grads, overwrite=True)
        torch.cuda.synchronize()
        sws.check(f"{kind} backward: sample workspace"), g.check(f"{kind} backward: plan workspace")
        res[kind] = out.cpu().numpy().reshape(batch, 3, n_points)
        res[kind + "-grads"] = [t.cpu().numpy().reshape(batch, n_per, -1) for t in grads]
        # the backward with the plan workspace, then the sample workspace, one byte short (the wrappers pass the tensors' sizes)
        short_plan, short_state = _cabi.Plan(d, g.mid[:n - 1], dev), (state[0], state[1], sws.mid[:n_sws - 1])
        junk = [torch.empty_like(t) for t in inputs]
        refused(lambda: bwd(short_plan, state, *inputs, gout, *junk, overwrite=True), g, f"{kind} backward, plan workspace one byte short")
        refused(lambda: bwd(plan, short_state, *inputs, gout, *junk, overwrite=True), sws, f"{kind} backward, sample workspace one byte short")
        sws.check(f"{kind} refused backwards: sample workspace"), g.check(f"{kind} refused backwards: plan workspace")
        if kind == "query":
            gp = _cabi.query_backward_points(plan, state, gout)
            torch.cuda.synchronize()
            sws.check("position backward: sample workspace"), g.check("position backward: plan workspace")
            res["query-pos"] = gp.cpu().numpy().reshape(batch, n_points, 2)
            refused(lambda: _cabi.query_backward_points(short_plan, state, gout), g, "position backward, plan workspace one byte short")
            refused(lambda: _cabi.query_backward_points(plan, short_state, gout), sws, "position backward, sample workspace one byte short")
            sws.check("refused position backwards: sample workspace"), g.check("refused position backwards: plan workspace")
    return res, per, g, guards


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("n_points", [1, 255, 257, 1025])
def test_sample_workspace(n_points, batch, dev):
    """n_points either side of k_pts_count's 256-thread blocks and of k_pts_scan's 1024"""
    runs = {fill: run_points(batch, n_points, fill, dev) for fill in FILLS}
    sws = [runs[f][3] for f in FILLS]
    n_sws = sws[0][0].n
    slack = n_sws - 1 - max(sws[i][k].highest_written(sws[j][k]) for k in (0, 1) for i in range(3) for j in range(3) if i != j)
    n = runs[FILLS[0]][2].n
    slack_plan = n - 1 - max(runs[a][2].highest_written(runs[b][2]) for a in FILLS for b in FILLS if a != b)
    print(f"\npoints-{n_points}-batch-{batch}: make_pt_layout for {n_points * batch} points behind a GSASR_FLAG_CONTINUOUS plan\n"
          f"points-{n_points}-batch-{batch}: sample workspace n = {n_sws}, slack = {slack}; plan workspace n = {n}, slack = {slack_plan}")
    for fill in FILLS:
        res, per, _, _ = runs[fill]
        worst = dict(value=0.0, grad=0.0, pos=0.0)
        for b, p in enumerate(per):
            live = p["smp"].sig.shape[0]
            for kind, val, gref in (("sampled", p["ival"], p["igrads"]), ("query", p["fval"], p["fgrads"])):
                what = f"{kind} {n_points} points batch {batch} sample {b} fill {fill}"
                got = res[kind][b]
                err = float(np.abs(got - val).max())
                worst["value"] = max(worst["value"], err)
                assert np.isfinite(got).all() and err <= IMG_ATOL, (what, err)
                mine = [a[b][:live] for a in res[kind + "-grads"]]
                for x, y, t in zip(mine, gref, ("sigmas", "coords", "colors")):
                    assert np.isfinite(x).all(), (what, t)
                    worst["grad"] = max(worst["grad"], relmax(x, y))
                    assert relmax(x, y) <= GRAD_RTOL, (what, t, relmax(x, y))
                gradbars.check_kernel(mine, gref, p["smp"].sig, 1.0, what)
                assert all(not a[b][live:].any() for a in res[kind + "-grads"]), what
            rel = relmax(res["query-pos"][b], p["fpos"])
            worst["pos"] = max(worst["pos"], rel)
            assert np.isfinite(res["query-pos"][b]).all() and rel <= GRAD_RTOL, (n_points, batch, b, fill, rel)
        print(f"points-{n_points}-batch-{batch}/{fill}: values max|err| {worst['value']:.3e} (bar {IMG_ATOL:.0e}); gradients rel-max "
              f"{worst['grad']:.3e}, positions {worst['pos']:.3e} (bar {GRAD_RTOL:.0e})")
    base = runs[FILLS[0]][0]
    for fill in FILLS[1:]:
        for key, val in runs[fill][0].items():
            for x, y in zip(base[key] if isinstance(val, list) else [base[key]], val if isinstance(val, list) else [val]):
                assert float(np.abs(x - y).max()) <= order_bar(x), (key, fill, float(np.abs(x - y).max()), order_bar(x))
    assert 0 <= slack < n_sws and 0 <= slack_plan < n


# ---- the step entry points and the host API: every workspace the Python layer acquires is a GuardedBytes -------------------------
class GuardedPool:
    """stands in for `_cabi._POOL.take` and for the three places where gsasr_amd/_cabi.py makes a workspace or scratch of its own
    for a step call: each request gets the middle of a fresh GuardedBytes of exactly the bytes asked for"""

    def __init__(self, dev, fill):
        self.dev, self.fill, self.guards = dev, fill, []

    def bytes(self, nbytes, dev=None):
        g = GuardedBytes(nbytes, self.dev, self.fill, seed=len(self.guards))
        self.guards.append(g)
        return g.mid

    def take(self, key, nbytes, dev):
        return self.bytes(nbytes), 0, False

    def check(self, what, at_least=1):
        torch.cuda.synchronize()
        assert len(self.guards) >= at_least, (what, len(self.guards))
        for k, g in enumerate(self.guards):
            g.check(f"{what}: workspace {k} of {len(self.guards)}")


@pytest.fixture
def guarded(monkeypatch, dev):
    from gsasr_amd import _cabi, _cpp_node

    real = {name: getattr(_cabi, name) for name in ("_image_shape", "_canvas_shape")}

    def install(fill, short=0):
        """`short`: every plan / step workspace is acquired, and declared to the library, `short` bytes below its size"""
        pool = GuardedPool(dev, fill)
        for name, fn in real.items():
            monkeypatch.setattr(_cabi, name, (lambda fn: lambda *a, **k: (lambda hit: (hit[0], hit[1] - short))(fn(*a, **k)))(fn))
        monkeypatch.setattr(_cabi._POOL, "take", pool.take)
        monkeypatch.setattr(_cabi._POOL, "give", lambda key, ws, parity: None)      # (a guarded workspace is not pooled)
        monkeypatch.setattr(_cabi, "_fresh_ws", lambda nbytes, d: pool.bytes(nbytes))
        monkeypatch.setattr(_cabi, "_sample_ws", lambda d, n_points, dv: pool.bytes(
            int(_cabi.lib().gsasr_sample_workspace_bytes(ctypes.byref(d), n_points))))
        monkeypatch.setattr(_cabi, "_loss_scratch_of", lambda nbytes, d: pool.bytes(nbytes).view(torch.float32))
        monkeypatch.setattr(_cpp_node, "load", lambda: None)        # (the Python nodes, which take from that pool)
        return pool
    return install


def step_forward_refused(guarded, call, what):
    """the step forward `call()` with its workspace one byte short, on seeded garbage: GSASR_ERR_WORKSPACE, the message names
    the workspace, and no byte of any guarded region (the workspace, a loss scratch, a sample workspace) or guard changed"""
    pool = guarded("seeded", short=1)
    with pytest.raises(RuntimeError, match=rf"\(status {ERR_WORKSPACE}\): .*workspace"):
        call()
    torch.cuda.synchronize()
    assert pool.guards, what
    for g in pool.guards:
        assert g.intact() and not g.written().any(), f"{what}: a refused call wrote"


def tpg():
    import test_param_grad_columns_gpu
    return test_param_grad_columns_gpu


def step_image_truth(p, hw, sm, dmax, window=None):
    from oracle import gs_oracle
    a, b, c = tpg().kernel_frame(p, hw, sm)
    if window is None:
        return gs_oracle.forward_f64(a, b, c, hw[0], hw[1], dmax)
    y0, x0, h, w = window
    return gs_oracle.forward_f64(a, b, c, hw[0], hw[1], dmax, rows=(y0, y0 + h))[:, x0:x0 + w]


def check_planar(img, ref, what):
    got = img.detach().permute(1, 2, 0).cpu().numpy().astype(np.float64)
    err = float(np.abs(got - ref).max())
    assert np.isfinite(got).all() and err <= IMG_ATOL, (what, err)
    return err


STEP_FORMS = [("gsasr_step_forward", "one", "step_size"), ("gsasr_step_forward_sm", "one", "scale_modify"),
              ("gsasr_step_forward_view", "window", "step_size"), ("gsasr_step_forward_sm_view", "window", "scale_modify")]


@pytest.mark.parametrize("kernel", ["gaussian", "tile", "home"])
@pytest.mark.parametrize("form,which,source", STEP_FORMS, ids=[f[0] for f in STEP_FORMS])
def test_step_workspace_single(form, which, source, kernel, guarded, dev):
    """make_step_layout: six arrays behind the plan, off_ghwc (the interleaved copy of the planar upstream gradient that the
    Gaussian-stationary and home-tile backward read) the last; gsasr_step_forward[_sm][_view] + gsasr_step_backward[_view]"""
    from gsasr_amd import _cabi
    t = tpg()
    op = "bounded"
    p, hw, sm, wgt, window, want = t.one_image_case(which, op)
    ref = step_image_truth(p, hw, sm, t.OPS[op], window)
    h, w = hw if window is None else window[2:]
    view = None if window is None else (hw[0], hw[1], window[0], window[1])
    results = []
    for fill in FILLS:
        pool = guarded(fill)
        pg = p.to(dev)
        step, sm_dev = t.step_source(source, sm, dev)
        img, plan = _cabi.step_forward(pg, step, h, w, t.OPS[op], t.kernel_flag(kernel), scale_modify=sm_dev, view=view)
        pool.check(f"{form}/{kernel}/{fill} forward")
        grad = torch.from_numpy(wgt).permute(2, 0, 1).contiguous().to(dev)
        got = _cabi.step_backward(plan, pg, step, grad, chw=True)
        pool.check(f"{form}/{kernel}/{fill} backward")
        assert len(pool.guards) == 1 and plan.workspace.numel() == pool.guards[0].n
        err = check_planar(img, ref, f"{form}/{kernel}/{fill}")
        elem, col = gradbars.check_raw(got, want, p, 1.0, f"{form}/{kernel}/{fill}")
        results.append((pool.guards[0], img.cpu().numpy(), got.cpu().numpy()))
        print(f"{form}/{kernel}/{fill}: n = {pool.guards[0].n}; image max|err| {err:.3e} (bar {IMG_ATOL:.0e}); raw gradient worst error / "
              f"element bar {elem:.3f}, / column bar {col:.3f}")
        short = _cabi.Plan(plan.dims, plan.workspace[:-1], dev)
        refused(lambda: _cabi.step_backward(short, pg, step, grad, chw=True), pool.guards[0], f"{form} backward, one byte short")
    step, sm_dev = t.step_source(source, sm, dev)
    step_forward_refused(guarded, lambda: _cabi.step_forward(p.to(dev), step, h, w, t.OPS[op], t.kernel_flag(kernel), scale_modify=sm_dev,
                                                             view=view), f"{form}/{kernel}, one byte short")
    n = results[0][0].n
    slack = n - 1 - max(results[i][0].highest_written(results[j][0]) for i in range(3) for j in range(3) if i != j)
    print(f"{form}/{kernel}: step workspace n = {n}, slack = {slack}")
    for _, img, got in results[1:]:
        assert float(np.abs(img - results[0][1]).max()) <= order_bar(results[0][1])
        if kernel in ("tile", "home"):       # documented as deterministic (see the module's docstring)
            assert np.array_equal(got, results[0][2]), (form, kernel)
        else:
            assert float(np.abs(got - results[0][2]).max()) <= order_bar(results[0][2])


@pytest.mark.parametrize("kernel", ["gaussian", "tile", "home"])
@pytest.mark.parametrize("source", ["step_size", "scale_modify"])
@pytest.mark.parametrize("windows", [False, True], ids=["canvas", "canvas-of-views"])
def test_step_workspace_batched(windows, source, kernel, guarded, dev):
    """the batched step: planar upstream gradient [B, 3, rows, w] with more rows than a slot needs (k_chw_to_hwc leaves the rows
    past grad_rows alone), the ragged batch of tests/test_param_grad_columns_gpu.py with and without a window per sample"""
    from gsasr_amd import _cabi
    t = tpg()
    scales_by = "heights"
    p, sms, own, wgts, wins, wants = t.batch_case(scales_by, windows)
    dmax = t.BATCH_DMAX[scales_by]
    refs = [step_image_truth(p[b], t.BATCH_SIZES[b], sms[b], dmax, wins[b]) for b in range(len(own))]
    views = [(hw[0], hw[1], wn[0], wn[1]) for hw, wn in zip(t.BATCH_SIZES, wins)] if windows else None
    hm, wm = max(h for h, _ in own), max(w for _, w in own)
    grad = torch.full((len(own), 3, hm + 3, wm), 7.0)          # (whatever lies outside a sample's own pixels is never read)
    for b, (h, w) in enumerate(own):
        grad[b, :, :h, :w] = torch.from_numpy(wgts[b]).permute(2, 0, 1)
    results = []
    for fill in FILLS:
        pool = guarded(fill)
        pg = p.to(dev)
        steps, sm_dev = t.step_source(source, sms, dev)
        img, plan = _cabi.batch_forward(pg, steps, own, dmax, t.kernel_flag(kernel), scale_modify=sm_dev, views=views)
        pool.check(f"batch/{kernel}/{fill} forward")
        got = _cabi.batch_backward(plan, pg, steps, grad.to(dev), chw=True)
        pool.check(f"batch/{kernel}/{fill} backward")
        assert len(pool.guards) == 1
        worst = [0.0, 0.0, 0.0]
        for b, (h, w) in enumerate(own):
            worst[0] = max(worst[0], check_planar(img[b, :, :h, :w], refs[b], f"batch sample {b}/{kernel}/{fill}"))
            e, c = gradbars.check_raw(got[b], wants[b], p[b], 1.0, f"batch windows={windows}/{kernel}/{fill}/sample {b}")
            worst[1], worst[2] = max(worst[1], e), max(worst[2], c)
        print(f"batch windows={windows}/{kernel}/{fill}: n = {pool.guards[0].n}; image max|err| {worst[0]:.3e} (bar {IMG_ATOL:.0e}); raw "
              f"gradient worst error / element bar {worst[1]:.3f}, / column bar {worst[2]:.3f}")
        results.append((pool.guards[0], img.cpu().numpy(), got.cpu().numpy()))
        short = _cabi.Plan(plan.dims, plan.workspace[:-1], dev)
        refused(lambda: _cabi.batch_backward(short, pg, steps, grad.to(dev), chw=True), pool.guards[0], "batched backward, one byte short")
    steps, sm_dev = t.step_source(source, sms, dev)
    step_forward_refused(guarded, lambda: _cabi.batch_forward(p.to(dev), steps, own, dmax, t.kernel_flag(kernel), scale_modify=sm_dev,
                                                              views=views), f"batched forward/{kernel}, one byte short")
    n = results[0][0].n
    slack = n - 1 - max(results[i][0].highest_written(results[j][0]) for i in range(3) for j in range(3) if i != j)
    print(f"batch windows={windows}/{source}/{kernel}: step workspace n = {n}, slack = {slack}")
    for _, img, got in results[1:]:
        assert float(np.abs(img - results[0][1]).max()) <= order_bar(results[0][1])
        if kernel in ("tile", "home"):       # documented as deterministic (see the module's docstring)
            assert np.array_equal(got, results[0][2]), (windows, source, kernel, int((got != results[0][2]).sum()))
        else:
            assert float(np.abs(got - results[0][2]).max()) <= order_bar(results[0][2])


def check_u8(px, ref, what):
    """tests/test_store_policy_gpu.py: the oracle's quantised pixels, exact away from the rounding boundaries"""
    v = np.clip(ref, 0.0, 1.0) * 255.0
    want = np.rint(v).astype(np.int64)
    px = px.astype(np.int64)
    assert int(np.abs(px - want).max()) <= 1, what
    safe = np.abs(v - np.floor(v) - 0.5) > 0.05
    assert safe.mean() > 0.8 and (px[safe] == want[safe]).all(), what
    assert int(px.max()) > 30, what


@pytest.mark.parametrize("which,source", [("one", "step_size"), ("one", "scale_modify"), ("window", "step_size")],
                         ids=["gsasr_step_forward_u8", "gsasr_step_forward_sm_u8", "gsasr_step_forward_u8_view"])
def test_step_workspace_u8(which, source, guarded, dev):
    """the forward-only step layout (no backward arrays, no gradient scratch) behind the 8-bit store"""
    from gsasr_amd import _cabi
    t = tpg()
    p, hw, sm, _, window, _ = t.one_image_case(which, "bounded")
    ref = step_image_truth(p, hw, sm, t.OPS["bounded"], window)
    h, w = hw if window is None else window[2:]
    view = None if window is None else (hw[0], hw[1], window[0], window[1])
    first = None
    for fill in FILLS:
        pool = guarded(fill)
        step, sm_dev = t.step_source(source, sm, dev)
        out, plan = _cabi.step_forward_u8(p.to(dev), step, h, w, t.OPS["bounded"], scale_modify=sm_dev, view=view)
        pool.check(f"u8 {which}/{source}/{fill}")
        assert len(pool.guards) == 1
        px = out.cpu().numpy()
        check_u8(px, ref, f"u8 {which}/{source}/{fill}")
        print(f"u8 {which}/{source}/{fill}: n = {pool.guards[0].n}, written up to byte {int(np.nonzero(pool.guards[0].written())[0][-1])}")
        first = px if first is None else first
        assert int(np.abs(px.astype(np.int64) - first.astype(np.int64)).max()) <= 1
    step, sm_dev = t.step_source(source, sm, dev)
    step_forward_refused(guarded, lambda: _cabi.step_forward_u8(p.to(dev), step, h, w, t.OPS["bounded"], scale_modify=sm_dev, view=view),
                         f"u8 {which}/{source}, one byte short")


@pytest.mark.parametrize("kernel", ["gaussian", "tile", "home"])
@pytest.mark.parametrize("batched", [False, True], ids=["one-image", "batch"])
def test_step_workspace_loss(batched, kernel, guarded, dev):
    """gsasr_step_forward_loss (its plan workspace AND its loss scratch guarded) + gsasr_step_backward on the gradient it stored:
    the fused MSE case of tests/test_param_grad_columns_gpu.py"""
    from gsasr_amd import _cabi
    t = tpg()
    op = "bounded"
    flags = t.kernel_flag(kernel)
    first = None
    for fill in FILLS:
        pool = guarded(fill)
        if not batched:
            p, sm, target, want = t.loss_case(False, op)
            pg = p.to(dev)
            step, _ = t.step_source("step_size", sm, dev)
            loss, grad, img, plan = _cabi.step_forward_loss(pg, step, *t.ONE["hw"], t.OPS[op], target.to(dev), _cabi.LOSS_KINDS["mse"],
                                                            weight=t.LOSS_WEIGHT, extra_flags=flags, want_image=True)
            pool.check(f"loss/{kernel}/{fill} forward", at_least=2)
            got = _cabi.step_backward(plan, pg, None, grad, chw=True)
            refs, imgs, gots, wants, ps = [step_image_truth(p, t.ONE["hw"], sm, t.OPS[op])], [img], [got], [want], [p]
        else:
            p, sms, targets, wants = t.loss_case(True, op)
            pg = p.to(dev)
            steps, _ = t.step_source("step_size", sms, dev)
            hm, wm = max(h for h, _ in t.BATCH_SIZES), max(w for _, w in t.BATCH_SIZES)
            tgt = torch.zeros(len(targets), 3, hm, wm)
            for b, x in enumerate(targets):
                tgt[b, :, :x.shape[1], :x.shape[2]] = x
            loss, grad, img, plan = _cabi.batch_forward_loss(pg, steps, t.BATCH_SIZES, t.OPS[op], tgt.to(dev), _cabi.LOSS_KINDS["mse"],
                                                             weight=t.LOSS_WEIGHT, extra_flags=flags, want_image=True)
            pool.check(f"batch loss/{kernel}/{fill} forward", at_least=2)
            got = _cabi.batch_backward(plan, pg, None, grad, chw=True)
            refs = [step_image_truth(p[b], t.BATCH_SIZES[b], sms[b], t.OPS[op]) for b in range(len(targets))]
            imgs = [img[b, :, :h, :w] for b, (h, w) in enumerate(t.BATCH_SIZES)]
            gots, ps = list(got), list(p)
        pool.check(f"loss/{kernel}/{fill} backward", at_least=2)
        assert len(pool.guards) == 2        # the step workspace and the loss scratch
        worst = [0.0, 0.0, 0.0]
        for b in range(len(refs)):
            worst[0] = max(worst[0], check_planar(imgs[b], refs[b], f"loss sample {b}/{kernel}/{fill}"))
            e, c = gradbars.check_raw(gots[b], wants[b], ps[b], 1.0, f"fused mse batched={batched}/{kernel}/{fill}/sample {b}")
            worst[1], worst[2] = max(worst[1], e), max(worst[2], c)
        sizes = [g.n for g in pool.guards]
        print(f"fused mse batched={batched}/{kernel}/{fill}: workspace and scratch n = {sizes}; image max|err| {worst[0]:.3e}; raw gradient "
              f"worst error / element bar {worst[1]:.3f}, / column bar {worst[2]:.3f}")
        res = (loss.cpu().numpy(), got.cpu().numpy())
        first = first or res
        # (another plan each time: the same sums in another order.  "Two calls on ONE plan give the same bits" is held in
        # tests/test_scratch_bounds_gpu.py, where one plan runs on three fills of the loss scratch)
        assert float(np.abs(res[0] - first[0]).max()) <= order_bar(first[0])
        assert float(np.abs(res[1] - first[1]).max()) <= order_bar(first[1])
    if not batched:
        step_forward_refused(guarded, lambda: _cabi.step_forward_loss(pg, step, *t.ONE["hw"], t.OPS[op], target.to(dev), _cabi.LOSS_KINDS["mse"],
                                                                      weight=t.LOSS_WEIGHT, extra_flags=flags), "step loss, one byte short")
    else:
        step_forward_refused(guarded, lambda: _cabi.batch_forward_loss(pg, steps, t.BATCH_SIZES, t.OPS[op], tgt.to(dev), _cabi.LOSS_KINDS["mse"],
                                                                       weight=t.LOSS_WEIGHT, extra_flags=flags), "batch loss, one byte short")


# ---- the host API: the Python layer's own idea of nbytes (_image_shape, _canvas_shape, _acquire) ---------------------------------
def host_calls(dev):
    """name -> a function that runs one forward + backward of a host entry point and returns its results as numpy arrays"""
    from gsasr_amd import gaussian_splatting as gsp
    t = tpg()
    kw = dict(if_dmax=True, dmax_mode="fix", dmax=t.OPS["bounded"])

    def finish(out, pg, wgt):
        (out * wgt).sum().backward()
        return [out.detach().cpu().numpy(), pg.grad.cpu().numpy()]

    def step():
        p, hw, sm, wgt, _, _ = t.one_image_case("one", "bounded")
        pg = p.to(dev).requires_grad_(True)
        return finish(gsp.generate_2D_gaussian_splatting_step(hw, pg, float(sm[0]), sm.to(dev), **kw), pg,
                      torch.from_numpy(wgt).permute(2, 0, 1).to(dev))

    def view():
        p, hw, sm, wgt, window, _ = t.one_image_case("window", "bounded")
        pg = p.to(dev).requires_grad_(True)
        return finish(gsp.generate_2D_gaussian_splatting_view(hw, pg, float(sm[0]), sm.to(dev), window, **kw), pg,
                      torch.from_numpy(wgt).permute(2, 0, 1).to(dev))

    def batch(windows):
        p, sms, own, wgts, wins, _ = t.batch_case("heights", windows)
        pg = p.to(dev).requires_grad_(True)
        out = gsp.generate_2D_gaussian_splatting_batch(t.BATCH_SIZES, pg, t.BATCH_SCALES["heights"], [s.to(dev) for s in sms],
                                                       windows=t.BATCH_WINDOWS if windows else None, dmax=t.BATCH_DMAX["heights"])
        wgt = torch.zeros_like(out)
        for b, (h, w) in enumerate(own):
            wgt[b, :, :h, :w] = torch.from_numpy(wgts[b]).permute(2, 0, 1).to(dev)
        return finish(out, pg, wgt)

    def batch_loss():
        p, sms, targets, _ = t.loss_case(True, "bounded")
        pg = p.to(dev).requires_grad_(True)
        loss = gsp.generate_2D_gaussian_splatting_batch_loss(t.BATCH_SIZES, pg, t.BATCH_SCALES["heights"], [s.to(dev) for s in sms],
                                                             [x.to(dev) for x in targets], loss="mse", loss_weight=t.LOSS_WEIGHT,
                                                             dmax=t.OPS["bounded"])
        loss.backward()
        return [loss.detach().cpu().numpy().reshape(1), pg.grad.cpu().numpy()]

    def step_uint8():
        p, hw, sm, _, _, _ = t.one_image_case("one", "bounded")
        return [gsp.generate_2D_gaussian_splatting_step_uint8(hw, p.to(dev), float(sm[0]), sm.to(dev), **kw).cpu().numpy()]

    def points(kind):
        pkw = dict(default_step_size=1.2, mode="scale_modify", if_dmax=True, dmax_mode="fix", dmax=t.PT_DMAX)
        p, sm, pts, gout, _ = t.point_case(kind, False)
        pg = p.to(dev).requires_grad_(True)
        if kind == "sampled":
            out = gsp.generate_2D_gaussian_splatting_step(t.PT_ONE["hw"], pg, t.PT_ONE["scale"], sm.to(dev), sample_coords=pts.to(dev), **pkw)
        else:
            out = gsp.generate_2D_gaussian_splatting_query(t.PT_ONE["hw"], pg, t.PT_ONE["scale"], sm.to(dev), pts.to(dev), **pkw)
        return finish(out, pg, gout.to(dev))

    return {"step": step, "view": view, "batch": lambda: batch(False), "batch-windows": lambda: batch(True), "batch-loss": batch_loss,
            "step-uint8": step_uint8, "sampled": lambda: points("sampled"), "query": lambda: points("query")}


HOST = ["step", "view", "batch", "batch-windows", "batch-loss", "step-uint8", "sampled", "query"]


@pytest.mark.parametrize("name", HOST)
def test_host_api_on_guarded_workspaces(name, guarded, dev):
    """one forward + backward of a host entry point with every workspace it acquires guarded and seeded with garbage: the guards
    stay intact, and the results are those of the same call on the allocator's memory, to the bar for sums in another order"""
    from gsasr_amd import gaussian_splatting as gsp
    call = host_calls(dev)[name]
    plain = call()
    pool = guarded("seeded")
    got = call()
    pool.check(f"host {name}")
    gsp.deferred_asserts.flush()
    print(f"host {name}: {len(pool.guards)} guarded workspaces of {[g.n for g in pool.guards]} bytes")
    assert len(plain) == len(got)
    for x, y in zip(got, plain):
        assert x.shape == y.shape and np.isfinite(x.astype(np.float64)).all()
        if x.dtype == np.uint8:
            assert int(np.abs(x.astype(np.int64) - y.astype(np.int64)).max()) <= 1        # (a pixel on a rounding boundary)
        else:
            assert float(np.abs(x - y).max()) <= order_bar(y), (name, float(np.abs(x - y).max()), order_bar(y))
