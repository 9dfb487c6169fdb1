"""The dmax box edge through every kernel, against the float64 oracle (tests/edge_lattice.py, tests/test_box_edge.py).

The library takes the decision |dx| <= dmax, |dy| <= dmax in three places -- the plan's double-precision window, the cell / tile-list
/ span bookkeeping built from it, and the float test inside the kernels, which exists in some thirty copies -- and random centres
never put a pixel on the edge.  The inputs here hold, per axis and sign, exact ties (kept), pairs one float step inside (kept) and
one and two steps outside (dropped), mid-unit and as the only pixel of a 32-, 16- and 8-px unit that the box reaches, on the first
and last row and column of the grid, of a row band and of a window, and just outside them.  A wrong kept or dropped pair is an
error of 0.2 to 0.9 against a bar of 1e-4 (tests/test_box_edge.py measures it on every case), so a failure names the pair.

Bars: image IMG_ATOL = 1e-4 * max(1, max|ref|) against oracle.gs_oracle.forward_f64; gradients tests/gradbars.py, every row in
scope (min_share 1.0), column bar on, against backward_f64 with an upstream gradient on the planted pixels and their four
neighbours.  Cutoffs: the adaptive default and none (cutoff = -1) unless a test says otherwise.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import edge_lattice as el
import gradbars
from test_box_edge import IMG_ATOL, QUERY_CANVAS, img_bar, query_case, query_points
from test_u8_output_gpu import KERNELS, within_one_level

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CUTOFFS = [0.0, -1.0]
CUT_IDS = ["adaptive", "nocut"]
SHAPE_CASE = {(512, 512): "512", (1024, 512): "1024x512", (256, 256): "256", (512, 256): "512x256", (768, 1024): "768x1024",
              (250, 300): "250x300"}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the MI355X box)"
    return torch.device("cuda:0")


def tensors(c, dev):
    return tuple(torch.from_numpy(np.array(c[k])).to(dev) for k in ("sig", "xy", "col"))


def plan_of(c, dev, flags=0, cap=0, cutoff=0.0, rows=None):
    """the plan of case dict `c` (a window: through its view) and its three input tensors"""
    from gsasr_amd import _cabi
    a, b, k = tensors(c, dev)
    view = (c["fh"], c["fw"], c["y0"], c["x0"]) if (c["fh"], c["fw"]) != (c["H"], c["W"]) else None
    return _cabi.plan(a, b, k, c["H"], c["W"], float(c["dmax"]), rows=rows, cutoff=cutoff, flags=flags, list_cap=cap, view=view), (a, b, k)


def check_image(name, got_hwc, ref, what, rows=None):
    got = got_hwc.detach().cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all(), what
    err = np.abs(got - ref)
    print(f"{what}: image error {err.max():.3e}, bar {img_bar(ref):.3e}")
    assert err.max() <= img_bar(ref), f"{what}: {el.blame(name, err, rows)}"


def check_grads(name, got, c, gref, what):
    """the gradients of the live records against the truth; the NaN records (dead Gaussians) get a stored gradient of exactly zero"""
    idx = el.live(c["sig"], c["xy"], c["col"])[3]
    got = [g.detach().cpu().numpy() for g in got]
    live = [g[idx] for g in got]
    dead = np.ones(got[0].shape[0], bool)
    dead[idx] = False
    assert dead.any() and all((g[dead] == 0.0).all() for g in got), f"{what}: a NaN record's gradient is not zero"
    try:
        worst = gradbars.check_kernel(live, gref, c["sig"][idx], 1.0, what)
    except AssertionError as e:
        raise AssertionError(f"{e}\n{el.blame_gradient(name, live, gref)}") from None
    print(f"{what}: worst gradient error / element bar {worst[0]:.3f}, / column bar {worst[1]:.3f}")


def render(plan, dev, flag=0, chw=False, into=None):
    from gsasr_amd import _cabi
    d = plan.dims
    rows = d.row1 - d.row0
    if into is not None:
        return _cabi.forward(plan, into, overwrite=False, chw=chw, flags=flag)
    img = torch.full((3, rows, d.w) if chw else (rows, d.w, 3), float("nan"), device=dev)
    return _cabi.forward(plan, img, overwrite=True, chw=chw, flags=flag)


# ---- every forward kernel ---------------------------------------------------------------------------------------------------------
def forward_plan(kernel, dev, cutoff, name=None, rows=None, forward_only=True):
    """the plan that selects forward kernel `kernel` of tests/test_u8_output_gpu.py KERNELS (same shape, record count, width flag and
    list capacity), on the edge lattice of that shape"""
    from gsasr_amd import _cabi
    H, W, s_total, width, cap = KERNELS[kernel]
    name = name or SHAPE_CASE[(H, W)]
    c = el.case(name, records=s_total)
    assert (c["H"], c["W"]) == (H, W) and c["sig"].shape[0] >= s_total
    flag = _cabi.FLAG_FWD_WIDE if width == "wide" else _cabi.FLAG_FWD_NARROW
    plan, abk = plan_of(c, dev, flag | (_cabi.FLAG_FORWARD_ONLY if forward_only else 0), cap, cutoff, rows)
    assert _cabi.forward_subtile_width(plan, flag) == (16 if width == "wide" else 8)
    return name, c, plan, flag


ACCUMULATE = ("fwd2-parts2", "dense-default", "fwd16-list")


@pytest.mark.parametrize("cutoff", CUTOFFS, ids=CUT_IDS)
@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_every_forward_kernel(kernel, cutoff, dev):
    name, c, plan, flag = forward_plan(kernel, dev, cutoff, forward_only=(len(kernel) % 2 == 0))
    ref = el.reference(name)[0]
    check_image(name, render(plan, dev, flag), ref, f"{kernel} {name} HWC")
    check_image(name, render(plan, dev, flag, chw=True).permute(1, 2, 0), ref, f"{kernel} {name} CHW")
    if kernel in ACCUMULATE:
        base = torch.rand(c["H"], c["W"], 3, generator=torch.Generator().manual_seed(3)).to(dev) - 0.5
        img = render(plan, dev, flag, into=base.clone())
        check_image(name, img - base, ref, f"{kernel} {name} accumulated")     # (|base| <= 0.5: the sum rounds at 6e-8)


def test_the_fine_forward():
    """k_render_fwd8 sits behind a development switch that is read once per process: a child process runs the 512^2 case"""
    env = dict(os.environ, GSASR_SPLAT_DEV="1", GSASR_SPLAT_FWD8="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "fwd8"], capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert r.returncode == 0 and "fwd8 box edge ok" in r.stdout, (r.stdout[-1500:], r.stderr[-1500:])


# ---- row bands ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cutoff", CUTOFFS, ids=CUT_IDS)
@pytest.mark.parametrize("kernel", ["fwd2-parts2", "list-persub", "fwd16", "fwd16-list", "split-pairs"])
@pytest.mark.parametrize("band", [(37, 203), (16, None)], ids=["rows37-203", "rows16-end"])
def test_row_bands(kernel, band, cutoff, dev):
    """ties on the band's first and last row (37 and 202; 16) as the first / last row of a box inside the band, and on the rows just
    outside it (36 and 203; 15) as the last / first row of a box outside it"""
    H = KERNELS[kernel][0]
    rows = (band[0], band[1] or H)
    name = f"{H}-band{band[0]}"
    name, c, plan, flag = forward_plan(kernel, dev, cutoff, name=name, rows=rows)
    check_image(name, render(plan, dev, flag), el.reference(name, rows)[0], f"{kernel} {name} rows {rows}", rows)


# ---- the large class ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cutoff", CUTOFFS, ids=CUT_IDS)
@pytest.mark.parametrize("width", ["narrow", "wide"])
def test_large_class(width, cutoff, dev):
    """reach 140 px > RCAP_PX = 128: these Gaussians are the large-class segment that every tile scans, not cells or lists"""
    from gsasr_amd import _cabi
    c = el.case("large-class")
    flag = _cabi.FLAG_FWD_WIDE if width == "wide" else _cabi.FLAG_FWD_NARROW
    plan, (a, b, k) = plan_of(c, dev, flag, 256, cutoff)
    ref, gref, up = el.reference("large-class")
    check_image("large-class", render(plan, dev, flag), ref, f"large class {width}")
    g = _cabi.backward_new(plan, a, b, k, torch.from_numpy(np.array(up)).to(dev))
    check_grads("large-class", g, c, gref, f"large class {width} backward")


# ---- every backward kernel ----------------------------------------------------------------------------------------------------------
G, T, A, HOME = "GAUSSIAN", "TILE", "ATOMIC", "HOME"


def launcher_choice(H, W, s, kind, cap, wide):
    """the instantiation launch_backward (gsasr_amd/csrc/splat_backward.hip) picks for a whole H x W image of `s` RECORDS, restated
    from its rules and those of splat_common.h (bt_tall, tl_dense, tl_hlog_for, launch_bwd_home's variant).  The library exposes
    none of this on a plan, so the table below is held to this restatement: an entry whose shape no longer meets the rule it
    quotes fails here, not silently on another kernel."""
    px = H * W
    if kind == G:
        return ("gaussian", "unrolled" if px >= 32.0 * s else "plain")             # BWD_UNROLL_MIN = 32
    if kind == HOME:
        ncx, ncy = (W + 15) // 16, (H + 15) // 16                                    # CELL = 16
        per_cell = s / (ncx * ncy)
        variant = 0 if per_cell >= 64.0 else 1 if per_cell >= 24.0 else 2
        n0 = ((ncx + 1) // 2) * ncy
        if variant == 0 and n0 > 512 and n0 % 512 != 0 and n0 % 512 <= 384:
            variant = 3
        return ("home", variant)
    tall = kind == T and px >= 64.0 * s                                              # bt_tall (plans with slots)
    sparse = px >= 32.0 * s
    nsub = ((W + 7) // 8) * ((H + 15) // 16)
    tl_hlog = 0 if cap < 0 else 5 if wide else 4 if (cap > 0 or nsub >= 2048) else 0   # tl_hlog_for with an explicit capacity
    lists = tl_hlog != 0 and tl_hlog == (5 if tall else 4)
    four = lists and not sparse and not tall and 4.0 * s >= px                       # tl_dense
    return ("atomic" if kind == A else "tile", 32 if tall else 16, "sparse" if sparse else "dense", "lists" if lists else "search",
            "four-waves" if four else "two-waves")


# name -> (case, records, backward flag, list_cap, wide forward on the plan, the instantiation): the shape that selects each backward
# instantiation.  The launcher's rules read dims.s, the RECORD count: the live Gaussians + the NaN record 1, or `records` if larger
# (the 256 case: 144 + 1 = 145).
BACKWARDS = {
    # "unroll = rows * w >= BWD_UNROLL_MIN (32) * s": 65 536 px over 145 records
    "gaussian-unrolled": ("256", 0, G, -1, False, ("gaussian", "unrolled")),
    # ... and without: 16 px per record
    "gaussian-plain": ("256", 4096, G, -1, False, ("gaussian", "plain")),
    # bt_tall: "h * w >= 64 * s" -> 32-row tiles; "sparse = rows * w >= 32 * s"; list_cap < 0: no lists, the search
    "tile32-search": ("256", 0, T, -1, False, ("tile", 32, "sparse", "search", "two-waves")),
    # "lists = tl_ok && tl_hlog == bt_hlog": tl_hlog_for gives 5 where the forward is the wide kernel
    "tile32-lists": ("256", 0, T, 256, True, ("tile", 32, "sparse", "lists", "two-waves")),
    # 32 * 1400 <= 65 536 < 64 * 1400: 16-row tiles, sparse
    "tile16-sparse-search": ("256", 1400, T, -1, False, ("tile", 16, "sparse", "search", "two-waves")),
    "tile16-sparse-lists": ("256", 1400, T, 256, False, ("tile", 16, "sparse", "lists", "two-waves")),
    # 16 px per record: not sparse (BT_CHUNKS 8 / BT_WAVES), and not tl_dense (4 * s < w * rows)
    "tile16-search": ("256", 4096, T, -1, False, ("tile", 16, "dense", "search", "two-waves")),
    "tile16-lists": ("256", 4096, T, 256, False, ("tile", 16, "dense", "lists", "two-waves")),
    # "lists && !sparse && bt_hlog == 4 && tl_dense": four waves per tile
    "tile16-lists-four-waves": ("256", 16384, T, 256, False, ("tile", 16, "dense", "lists", "four-waves")),
    "atomic": ("256", 0, A, -1, False, ("atomic", 16, "sparse", "search", "two-waves")),
    "atomic-dense-lists": ("256", 16384, A, 256, False, ("atomic", 16, "dense", "lists", "four-waves")),
    # launch_bwd_home: "variant = per_cell >= 64 ? 0 : per_cell >= 24 ? 1 : 2", per_cell = s / ncells, 256 cells of 16 px
    "home-2": ("256", 4096, HOME, 0, False, ("home", 2)),
    "home-1": ("256", 8192, HOME, 0, False, ("home", 1)),
    "home-0": ("256", 16384, HOME, 0, False, ("home", 0)),           # n0 = 8 * 16 = 128 tiles <= 512: stays 0
    # "n0 > 512 && over != 0 && over <= 384 -> 3": 640 x 512 has 32 x 40 cells, n0 = 16 * 40 = 640, over = 128; 64 records per cell
    "home-3": ("640x512", 81920, HOME, 0, False, ("home", 3)),
}
# the forms that are not whole images of the table: (case, records, backward flag, list_cap, wide forward)
BAND_ENTRY = {kind: (None, 4096, kind, 256 if kind == T else -1, False) for kind in (G, T, A, HOME)}


def test_backwards_table_meets_the_rules_it_quotes():
    seen = set()
    for entry, (name, records, kind, cap, wide, want) in BACKWARDS.items():
        c = el.case(name, records=records)
        got = launcher_choice(c["H"], c["W"], c["sig"].shape[0], kind, cap, wide)
        assert got == want, (entry, got, want)
        seen.add(got)
    assert len(seen) == len(BACKWARDS)          # no two entries reach the same instantiation
    assert {g[1] for g in seen if g[0] == "home"} == {0, 1, 2, 3}


def backward_case(entry, dev, cutoff, chw_grad=False, rows=None, name=None):
    from gsasr_amd import _cabi
    case, records, kind, cap, wide = BACKWARDS[entry][:5] if isinstance(entry, str) else entry
    name = name or case
    if not isinstance(entry, str):
        entry = f"{kind.lower()} {'lists' if cap > 0 else 'search'}"
    c = el.case(name, records=records)
    flags = getattr(_cabi, "FLAG_BWD_" + kind) | (_cabi.FLAG_FWD_WIDE if wide else 0)
    plan, (a, b, k) = plan_of(c, dev, flags, cap, cutoff, rows)
    ref, gref, up = el.reference(name, rows)
    what = f"{entry} {name} cutoff {cutoff}" + (f" rows {rows}" if rows else "") + (" planar gradient" if chw_grad else "")
    check_image(name, render(plan, dev), ref, what, rows)
    gimg = torch.from_numpy(np.array(up)).to(dev)
    if chw_grad:
        g = [torch.full_like(t, float("nan")) for t in (a, b, k)]
        gimg = gimg.permute(2, 0, 1).contiguous()
        _cabi._splat_backward(plan, tuple(t.data_ptr() for t in (a, b, k, gimg, *g)), _cabi.FLAG_CHW_GRAD | _cabi.FLAG_OVERWRITE_GRADS)
    else:
        g = _cabi.backward_new(plan, a, b, k, gimg)
    torch.cuda.synchronize()
    check_grads(name, g, c, gref, what)


@pytest.mark.parametrize("cutoff", CUTOFFS, ids=CUT_IDS)
@pytest.mark.parametrize("entry", sorted(BACKWARDS))
def test_every_backward_kernel(entry, cutoff, dev):
    backward_case(entry, dev, cutoff)


@pytest.mark.parametrize("entry", ["tile32-search", "tile16-lists-four-waves", "atomic"])
def test_planar_gradient(entry, dev):
    backward_case(entry, dev, 0.0, chw_grad=True)


@pytest.mark.parametrize("kind", [G, T, A, HOME])
@pytest.mark.parametrize("band", [(37, 203), (16, 256)], ids=["rows37-203", "rows16-end"])
def test_backward_row_band(kind, band, dev):
    backward_case(BAND_ENTRY[kind], dev, 0.0, rows=band, name=f"256-band{band[0]}")


def test_eight_gaussians_per_wave():
    """k_render_bwd8 behind GSASR_SPLAT_BWD8=1 (read once per process): a child process, as tests/test_rows_vs_oracle.py runs it"""
    env = dict(os.environ, GSASR_SPLAT_DEV="1", GSASR_SPLAT_BWD8="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "bwd8"], capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert r.returncode == 0 and "bwd8 box edge ok" in r.stdout, (r.stdout[-1500:], r.stderr[-1500:])


# ---- windows and canvases -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [G, T, A])
@pytest.mark.parametrize("cap", [-1, 256], ids=["search", "lists"])
def test_window(cap, kind, dev):
    """the window (19, 7, 70, 61) of 128 x 96: ties on its border rows and columns from inside, on the ones just outside from outside"""
    for cutoff in CUTOFFS:
        backward_case(("window", 0, kind, cap, False), dev, cutoff)


CANVAS = ["canvas-0", "canvas-1", "canvas-2"]
CANVAS_WINDOWS = ["canvas-window-0", "canvas-window-1", "canvas-window-2"]


def canvas_records(names):
    """records per sample: the largest sample's live records + the NaN record 1 + one more; every sample is padded with NaN records"""
    return max(len(el.case(n)["table"]) for n in names) + 2


def canvas_inputs(names, dev):
    n_per = canvas_records(names)
    cs = [el.case(n, records=n_per) for n in names]
    assert all(c["sig"].shape[0] == n_per for c in cs)
    abk = tuple(torch.cat([torch.from_numpy(np.array(c[key])) for c in cs]).to(dev) for key in ("sig", "xy", "col"))
    windows = cs[0]["fh"] != cs[0]["H"]
    return cs, abk, n_per, [(c["H"], c["W"]) for c in cs], ([(c["fh"], c["fw"], c["y0"], c["x0"]) for c in cs] if windows else None)


@pytest.mark.parametrize("kind", [G, T, A])
@pytest.mark.parametrize("cap", [-1, 256], ids=["search", "lists"])
@pytest.mark.parametrize("names", [CANVAS, CANVAS_WINDOWS], ids=["samples", "windows"])
def test_ragged_canvas(names, cap, kind, dev):
    """three samples (40, 56), (64, 64), (33, 47), each with a lattice on its own grid; and one window of each of those grids, batched.
    A canvas has one dmax and every sample's lattice its own (2 * reach / (its longer side - 1)): the canvas is planned once per
    sample, with that sample's dmax, and that sample is checked (the others then render boxes that are not theirs)"""
    from gsasr_amd import _cabi
    cs, (a, b, k), n_per, sizes, views = canvas_inputs(names, dev)
    for cutoff in CUTOFFS:
        for bi, c in enumerate(cs):
            what = f"canvas {names[bi]} {kind} cap {cap} cutoff {cutoff}"
            plan = _cabi.plan(a, b, k, 0, 0, float(c["dmax"]), cutoff=cutoff, flags=getattr(_cabi, "FLAG_BWD_" + kind), list_cap=cap,
                              sizes=sizes, views=views)
            d = plan.dims
            img = torch.full((d.batch * d.slot, d.w, 3), float("nan"), device=dev)
            _cabi.forward(plan, img, overwrite=True)
            ref, gref, up = el.reference(names[bi])
            check_image(names[bi], img[bi * d.slot: bi * d.slot + c["H"], : c["W"]], ref, what)
            gimg = torch.zeros(d.batch * d.slot, d.w, 3, device=dev)
            gimg[bi * d.slot: bi * d.slot + c["H"], : c["W"]] = torch.from_numpy(np.array(up)).to(dev)
            g = _cabi.backward_new(plan, a, b, k, gimg)
            check_grads(names[bi], [t[bi * n_per: (bi + 1) * n_per] for t in g], c, gref, what)


def test_sampled_pixels_on_the_ragged_canvas(dev):
    """sample_forward / sample_backward on the canvas: the first S planted points of every sample, S the smallest sample's count"""
    from gsasr_amd import _cabi
    from oracle import gs_oracle
    cs, (a, b, k), n_per, sizes, _ = canvas_inputs(CANVAS, dev)
    pts = [el.planted_points(c["table"], c["fh"], c["fw"]) for c in cs]
    S = min(len(p) for p in pts)
    pts = np.stack([p[:: max(1, len(p) // S)][:S] for p in pts])
    gout = np.random.RandomState(9).uniform(0.25, 1.0, (len(cs), 3, S)).astype(np.float32)
    for bi, c in enumerate(cs):
        plan = _cabi.plan(a, b, k, 0, 0, float(c["dmax"]), sizes=sizes)
        out, state = _cabi.sample_forward(plan, torch.from_numpy(pts).to(dev))
        want = el.reference(CANVAS[bi])[0][pts[bi, :, 0], pts[bi, :, 1]].T
        err = np.abs(out[bi].cpu().numpy() - want).max(axis=0)
        i = int(np.argmax(err))
        assert err.max() <= IMG_ATOL * max(1.0, np.abs(want).max()), \
            f"sample {bi} point {pts[bi, i]}: error {err[i]:.3e}; {el.describe(c['table'], pts[bi, i][0], pts[bi, i][1], c['reach'])}"
        g = [torch.full_like(t, float("nan")) for t in (a, b, k)]
        _cabi.sample_backward(plan, state, a, b, k, torch.from_numpy(gout).to(dev), *g, overwrite=True)
        s, x, k_, _ = el.live(c["sig"], c["xy"], c["col"])
        wgt = np.zeros((c["H"], c["W"], 3), np.float32)
        np.add.at(wgt, (pts[bi, :, 0], pts[bi, :, 1]), gout[bi].T)
        gref = gs_oracle.backward_f64(s, x, k_, wgt, float(c["dmax"]))
        check_grads(CANVAS[bi], [t[bi * n_per: (bi + 1) * n_per] for t in g], c, gref, f"sampled pixels, canvas sample {bi}")


# ---- points -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["256", "512", "large-class"])
def test_sampled_pixels(name, dev):
    """sample_forward / sample_backward at every planted pixel and its four neighbours"""
    from gsasr_amd import _cabi
    from oracle import gs_oracle
    c = el.case(name)
    pts = el.planted_points(c["table"], c["fh"], c["fw"])
    s, x, k_, idx = el.live(c["sig"], c["xy"], c["col"])
    gout = np.random.RandomState(5).uniform(0.25, 1.0, (3, len(pts))).astype(np.float32)
    wgt = np.zeros((c["H"], c["W"], 3), np.float32)
    wgt[pts[:, 0], pts[:, 1]] = gout.T
    gref = gs_oracle.backward_f64(s, x, k_, wgt, float(c["dmax"]))
    want = el.reference(name)[0][pts[:, 0], pts[:, 1]].T
    for cutoff in CUTOFFS:
        plan, (a, b, k) = plan_of(c, dev, 0, 0, cutoff)
        out, state = _cabi.sample_forward(plan, torch.from_numpy(pts).to(dev))
        err = np.abs(out.cpu().numpy() - want).max(axis=0)
        print(f"{name} cutoff {cutoff}: {len(pts)} points, value error {err.max():.3e}")
        i = int(np.argmax(err))
        assert err.max() <= IMG_ATOL * max(1.0, np.abs(want).max()), \
            f"point {pts[i]}: error {err[i]:.3e}; {el.describe(c['table'], pts[i][0], pts[i][1], c['reach'])}"
        g = [torch.full_like(t, float("nan")) for t in (a, b, k)]
        _cabi.sample_backward(plan, state, a, b, k, torch.from_numpy(gout).to(dev), *g, overwrite=True)
        check_grads(name, g, c, gref, f"sampled pixels {name} cutoff {cutoff}")


@pytest.mark.parametrize("m", [2, 4])
def test_queries_at_refined_grid_ties(m, dev):
    """query_forward / query_backward / query_backward_points on a continuous plan at ties planted between the pixel centres; the
    truth is the oracle on the refined grid (tests/test_query_points_gpu.py), the position gradient through the oracle identity
    and the sum identity of tests/test_query_grad_gpu.py"""
    from gsasr_amd import _cabi
    from oracle import gs_oracle
    from test_query_grad import oracle_point_grads
    q = query_case(m)
    t, H, W, Hm, Wm = q["table"], q["H"], q["W"], q["Hm"], q["Wm"]
    s, x, k_, idx = el.live(q["sig"], q["xy"], q["col"])
    kk = query_points(q)
    dmax = float(q["dmax"])
    gout = np.random.RandomState(7).uniform(0.25, 1.0, (3, len(kk))).astype(np.float32)
    want = gs_oracle.forward_f64(s, x, k_, Hm, Wm, dmax)[kk[:, 0], kk[:, 1]].T
    wgt = np.zeros((Hm, Wm, 3), np.float32)
    wgt[kk[:, 0], kk[:, 1]] = gout.T
    gref = gs_oracle.backward_f64(s, x, k_, wgt, dmax)
    sub = np.arange(0, len(kk), max(1, len(kk) // 48))       # the identity costs one oracle backward per point
    pwant = oracle_point_grads(torch.from_numpy(s), torch.from_numpy(x), torch.from_numpy(k_), H, W, m, kk[sub], torch.from_numpy(gout[:, sub]), dmax)
    a, b, k = (torch.from_numpy(np.array(q[key])).to(dev) for key in ("sig", "xy", "col"))
    pts = torch.from_numpy(kk.astype(np.float32) / m).to(dev)
    c = dict(q, fh=Hm, fw=Wm)
    for cutoff in CUTOFFS:
        plan = _cabi.plan(a, b, k, H, W, dmax, cutoff=cutoff, flags=_cabi.FLAG_CONTINUOUS)
        out, state = _cabi.query_forward(plan, pts)
        err = np.abs(out.cpu().numpy() - want).max(axis=0)
        i = int(np.argmax(err))
        print(f"m={m} cutoff {cutoff}: {len(kk)} points, value error {err.max():.3e}")
        assert err.max() <= IMG_ATOL * max(1.0, np.abs(want).max()), \
            f"refined pixel {kk[i]}: error {err[i]:.3e}; {el.describe(t, kk[i][0], kk[i][1], 6 * m)}"
        g = [torch.full_like(v, float("nan")) for v in (a, b, k)]
        go = torch.from_numpy(gout).to(dev)
        _cabi.query_backward(plan, state, a, b, k, go, *g, overwrite=True)
        live = [v.cpu().numpy()[idx] for v in g]
        print(gradbars.check_kernel(live, gref, s, 1.0, f"query m={m} cutoff {cutoff}"))
        gp = _cabi.query_backward_points(plan, state, go).double().cpu().numpy()
        rel = np.abs(gp[sub] - pwant).max() / np.abs(pwant).max()
        print(f"m={m} cutoff {cutoff}: position gradient against the oracle identity {rel:.3e}")
        assert np.isfinite(gp).all() and rel <= 2e-4
        gc = np.nan_to_num(g[1].double().cpu().numpy())
        for axis, unit in ((0, (W - 1) / 2.0), (1, (H - 1) / 2.0)):       # sum_s g_p = -sum_j g_coords, in pixels
            lhs, rhs, scale = gp[:, 1 - axis].sum() * unit, -gc[idx, axis].sum(), np.abs(gc[idx, axis]).sum()
            assert abs(lhs - rhs) <= 2e-4 * scale, (axis, lhs, rhs, scale)


def test_queries_on_the_ragged_canvas(dev):
    """query_forward / query_backward / query_backward_points on a continuous plan of the canvas (40, 56), (64, 64), (33, 47): every
    sample has its own lattice of ties between its pixel centres (m = 2) and, like test_ragged_canvas, its own dmax, so the canvas
    is planned once per sample with that sample's dmax and that sample is checked: values against the refined-grid oracle, the
    Gaussians' gradients to tests/gradbars.py, the position gradient through the sum identity of tests/test_query_grad_gpu.py
    and, on a few points, the oracle identity"""
    from gsasr_amd import _cabi
    from oracle import gs_oracle
    from test_query_grad import oracle_point_grads
    m = 2
    n_per = max(len(query_case(m, b)["table"]) for b in QUERY_CANVAS) + 2
    qs = [query_case(m, b, records=n_per) for b in QUERY_CANVAS]
    assert all(q["sig"].shape[0] == n_per for q in qs)
    a, b, k = (torch.cat([torch.from_numpy(np.array(q[key])) for q in qs]).to(dev) for key in ("sig", "xy", "col"))
    sizes = [(q["H"], q["W"]) for q in qs]
    kks = [query_points(q) for q in qs]
    S = min(len(kk) for kk in kks)
    kks = [kk[:: max(1, len(kk) // S)][:S] for kk in kks]
    pts = torch.from_numpy(np.stack(kks).astype(np.float32) / m).to(dev)
    gout = np.random.RandomState(13).uniform(0.25, 1.0, (len(qs), 3, S)).astype(np.float32)
    go = torch.from_numpy(gout).to(dev)
    for bi, q in enumerate(qs):
        H, W, Hm, Wm, dmax, kk, t = q["H"], q["W"], q["Hm"], q["Wm"], float(q["dmax"]), kks[bi], q["table"]
        s, x, k_, idx = el.live(q["sig"], q["xy"], q["col"])
        want = gs_oracle.forward_f64(s, x, k_, Hm, Wm, dmax)[kk[:, 0], kk[:, 1]].T
        wgt = np.zeros((Hm, Wm, 3), np.float32)
        wgt[kk[:, 0], kk[:, 1]] = gout[bi].T
        gref = gs_oracle.backward_f64(s, x, k_, wgt, dmax)
        sub = np.arange(0, S, max(1, S // 12))
        pwant = oracle_point_grads(torch.from_numpy(s), torch.from_numpy(x), torch.from_numpy(k_), H, W, m, kk[sub],
                                   torch.from_numpy(gout[bi][:, sub]), dmax)
        for cutoff in CUTOFFS:
            what = f"canvas queries sample {bi} cutoff {cutoff}"
            plan = _cabi.plan(a, b, k, 0, 0, dmax, cutoff=cutoff, flags=_cabi.FLAG_CONTINUOUS, sizes=sizes)
            out, state = _cabi.query_forward(plan, pts)
            err = np.abs(out[bi].cpu().numpy() - want).max(axis=0)
            i = int(np.argmax(err))
            print(f"{what}: {S} points, value error {err.max():.3e}")
            assert err.max() <= IMG_ATOL * max(1.0, np.abs(want).max()), \
                f"{what}: refined pixel {kk[i]}: error {err[i]:.3e}; {el.describe(t, kk[i][0], kk[i][1], 8)}"
            g = [torch.full_like(v, float("nan")) for v in (a, b, k)]
            _cabi.query_backward(plan, state, a, b, k, go, *g, overwrite=True)
            mine = [v[bi * n_per: (bi + 1) * n_per].cpu().numpy() for v in g]
            live = [v[idx] for v in mine]
            worst = gradbars.check_kernel(live, gref, s, 1.0, what)
            print(f"{what}: worst gradient error / element bar {worst[0]:.3f}, / column bar {worst[1]:.3f}")
            gp = _cabi.query_backward_points(plan, state, go).double().cpu().numpy()[bi]
            rel = np.abs(gp[sub] - pwant).max() / np.abs(pwant).max()
            print(f"{what}: position gradient against the oracle identity {rel:.3e}")
            assert np.isfinite(gp).all() and rel <= 2e-4, what
            for axis, unit in ((0, (W - 1) / 2.0), (1, (H - 1) / 2.0)):       # sum_s g_p = -sum_j g_coords, in pixels
                lhs, rhs, scale = gp[:, 1 - axis].sum() * unit, -live[1][:, axis].astype(np.float64).sum(), np.abs(live[1][:, axis]).sum()
                assert abs(lhs - rhs) <= 2e-4 * scale, (what, axis, lhs, rhs, scale)


# ---- fused forms, once each ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["fwd2-parts2", "fwd16"])
def test_fused_mse_and_u8(kernel, dev):
    """the fused MSE forward (loss, image gradient, image) and the 8-bit forward on the 512^2 lattice, narrow and wide"""
    from gsasr_amd import _cabi
    name, c, plan, flag = forward_plan(kernel, dev, 0.0)
    ref = el.reference(name)[0]
    target = torch.rand(c["H"], c["W"], 3, generator=torch.Generator().manual_seed(11))
    loss, grad, img = _cabi.forward_loss(plan, target.to(dev), _cabi.LOSS_KINDS["mse"], want_image=True, flags=flag)
    check_image(name, img, ref, f"fused mse {kernel} image")
    diff = ref - target.numpy().astype(np.float64)
    want_loss = float((diff ** 2).mean())
    assert abs(float(loss[0]) - want_loss) <= 1e-4 * want_loss, (float(loss[0]), want_loss)
    gerr = np.abs(grad.cpu().numpy() - 2.0 * diff / diff.size)
    assert gerr.max() <= 2.0 / diff.size * img_bar(ref), el.blame(name, gerr)
    got = _cabi.forward_u8(plan, flags=flag).cpu().numpy()
    # tests/test_u8_output_gpu.py test_dense_input_against_the_own_float_image's rule, with the ORACLE image as the float image
    ok, share = within_one_level(got, ref.astype(np.float32), 255 * 2e-5)
    if not ok:
        want = (np.clip(ref, 0, 1) * 255.0).round()
        raise AssertionError(el.blame(name, np.abs(got.astype(np.float64) - want) / 255.0))
    assert share <= 0.03, share


def _child(which):
    sys.path.insert(0, ROOT)
    device = torch.device("cuda:0")
    if which == "fwd8":
        for cutoff in CUTOFFS:
            name, c, plan, flag = forward_plan("fwd2-parts2", device, cutoff)
            check_image(name, render(plan, device, flag), el.reference(name)[0], f"fwd8 cutoff {cutoff}")
        print("fwd8 box edge ok")
    else:
        for entry in ("gaussian-unrolled", "gaussian-plain"):
            backward_case(entry, device, 0.0)
        print("bwd8 box edge ok")


if __name__ == "__main__":
    _child(sys.argv[1])
