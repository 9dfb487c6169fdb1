"""The dmax box edge on the CPU: the input of tests/edge_lattice.py holds what it promises, the oracle agrees with itself on it,
and a box test that is wrong by one comparison or one float step is far outside every bar on it.

The bars are the suite's: image 1e-4 * max(1, max|ref|) against oracle.gs_oracle.forward_f64 (tests/test_hip_parity.py: IMG_ATOL),
gradients tests/gradbars.py with every row in scope (|rho| <= 0.4: kappa >= 0.84).  `restated_*` below are the project's own
formulas (oracle/gs_ref.c) written out in numpy with the comparison as a parameter.
"""
import numpy as np
import pytest
import torch

import edge_lattice as el
import gradbars

IMG_ATOL = 1e-4
# the package's CPU definitions take dx = px - x in double from the float32 px; the oracle promotes the float32 DIFFERENCE (one more
# rounding, 6e-8 of dx): the two agree to ~1e-7 of a term, a thousandth of the image bar
CPU_RTOL = 1e-6
GPU_CASES = sorted(el.CASES)
CANVAS = ["canvas-0", "canvas-1", "canvas-2"]
CANVAS_WINDOWS = ["canvas-window-0", "canvas-window-1", "canvas-window-2"]
# A third of the pairs of an axis aligned: on every grid of 250 pixels and more a side.  The samples of the ragged canvas, their windows
# and the window of 128 x 96 are 33 to 128 pixels a side: two to four aligned pixels per sign and axis against a slot every one to
# eight pixels; they hold the >= 4 aligned kept pairs per sign and axis like every other case.
SMALL = CANVAS + CANVAS_WINDOWS + ["window"]
# `spacing >= 2 * reach + 8` (separate boxes, a planted pixel owned by one Gaussian) holds where sixteen boxes fit a side; the others
# let their boxes overlap, and a failure message then names the nearest planted pair, not the only one
SEPARATE = [n for n in GPU_CASES if not el.CASES[n][4].get("overlap")]


def img_bar(ref):
    return IMG_ATOL * max(1.0, float(np.abs(ref).max()))


def restated(c, keep, upstream=None):
    """forward [fh, fw, 3] (float64) of the live Gaussians of case dict `c` with the box test `keep(|d|, dmax) -> bool` on the
    float32 differences; with `upstream` [fh, fw, 3] also d/d colours [n, 3]"""
    sig, xy, col, _ = el.live(c["sig"], c["xy"], c["col"])
    fh, fw, dmax = c["fh"], c["fw"], c["dmax"]
    px, py = el.pixel_coords(fw), el.pixel_coords(fh)
    img = np.zeros((fh, fw, 3))
    gcol = np.zeros((sig.shape[0], 3))
    for j in range(sig.shape[0]):
        dxf, dyf = px - xy[j, 0], py - xy[j, 1]                 # float32, as the reference forms them
        cols = np.nonzero(keep(np.abs(dxf), dmax))[0]
        rows = np.nonzero(keep(np.abs(dyf), dmax))[0]
        if not len(cols) or not len(rows):
            continue
        sx, sy, rho = (float(v) for v in sig[j])
        dx, dy = dxf[cols].astype(np.float64)[None, :], dyf[rows].astype(np.float64)[:, None]
        d = dx * dx / (sx * sx) - 2 * rho * dx * dy / (sx * sy) + dy * dy / (sy * sy)
        v = np.exp(-0.5 / (1 - rho * rho) * d)
        img[np.ix_(rows, cols)] += v[:, :, None] * col[j].astype(np.float64)
        if upstream is not None:
            gcol[j] = (v[:, :, None] * upstream[np.ix_(rows, cols)]).sum(axis=(0, 1))
    return img, gcol


INCLUSIVE = lambda a, dmax: a <= dmax                               # the op
STRICT = lambda a, dmax: a < dmax                                   # a `<` for the `<=`
ONE_ULP_WIDE = lambda a, dmax: a <= el.step(dmax, 1)                # a dmax one float step too large


def window_of(c, full):
    return full[c["y0"]: c["y0"] + c["H"], c["x0"]: c["x0"] + c["W"]]


# ---- the counts: conditions on every case the GPU file uses ---------------------------------------------------------------------
def float_counts(c):
    """the categories from the oracle's float arithmetic alone: px[X] - x against dmax, never the constructor's table"""
    sig, xy, col, _ = el.live(c["sig"], c["xy"], c["col"])
    t = c["table"]
    out = {}
    for axis, n, idx, k in (("x", c["fw"], t["X"], 0), ("y", c["fh"], t["Y"], 1)):
        d = el.pixel_coords(n)[idx] - xy[:, k]
        ulps = el.ulps_out(d, c["dmax"])
        kept = np.abs(d) <= c["dmax"]
        assert np.array_equal(kept, ulps <= 0)
        aligned = np.where(d > 0, idx % 32 == 0, idx % 32 == 31)
        for s in (1, -1):
            m = np.sign(d) == s
            out[(axis, s)] = dict(exact=int((m & (ulps == 0)).sum()), inside=int((m & (ulps == -1)).sum()),
                                  outside=int((m & (ulps == 1)).sum()), outside2=int((m & (ulps == 2)).sum()),
                                  aligned_kept=int((m & aligned & np.isin(ulps, (0, -1))).sum()),
                                  aligned=int((m & aligned).sum()), all=int(m.sum()))
    return out


def add_counts(a, b):
    return {k: {f: a[k][f] + b[k][f] for f in a[k]} for k in a}


@pytest.mark.parametrize("name", GPU_CASES)
def test_counts(name):
    """per axis and per sign, in EVERY case (each sample of the canvas and each of its windows alone): >= 4 exact ties, >= 4 one ulp
    inside, >= 4 one ulp outside, >= 1 two ulp outside, >= 4 kept pairs whose pixel is the only one of its 32-px unit (so of its 16-
    and 8-px unit) that the box reaches; a third of the pairs of an axis aligned except on the SMALL grids"""
    cnt = float_counts(el.case(name))
    print(name, cnt)
    for (axis, s), c in cnt.items():
        for what in ("exact", "inside", "outside", "aligned_kept"):
            assert c[what] >= 4, (name, axis, s, what, c)
        assert c["outside2"] >= 1, (name, axis, s, c)
    for axis in "xy" if name not in SMALL else "":
        assert 3 * (cnt[(axis, 1)]["aligned"] + cnt[(axis, -1)]["aligned"]) >= cnt[(axis, 1)]["all"] + cnt[(axis, -1)]["all"], (name, axis)
    t = el.case(name)["table"]       # the two axes are independent: kept x kept, kept x dropped, dropped x dropped corners
    kx, ky = t["k_x"] <= 0, t["k_y"] <= 0
    assert (kx & ky).any() and (kx & ~ky).any() and (~kx & ky).any() and (~kx & ~ky).any()


def test_separate_boxes():
    """the cases that keep `spacing >= 2 * reach + 8`: no pixel lies in the boxes of two Gaussians"""
    assert {"512", "512-band16", "1024x512", "512x256", "768x1024", "640x512"} <= set(SEPARATE)
    for name in SEPARATE:
        c = el.case(name)
        s, x, k, _ = el.live(c["sig"], c["xy"], c["col"])
        inx = np.abs(el.pixel_coords(c["fw"])[None, :] - x[:, 0:1]) <= c["dmax"]
        iny = np.abs(el.pixel_coords(c["fh"])[None, :] - x[:, 1:2]) <= c["dmax"]
        cover = np.einsum("jr,jc->rc", iny.astype(np.int32), inx.astype(np.int32))
        assert cover.max() == 1, name


def test_parameters_and_edges():
    for name in GPU_CASES:
        c = el.case(name)
        sig, xy, col, _ = el.live(c["sig"], c["xy"], c["col"])
        dm = float(c["dmax"])
        assert c["dmax"] == np.float32(2.0 * c["reach"] / (max(c["fh"], c["fw"]) - 1))
        assert (sig[:, :2] >= 1.6 * dm * (1 - 1e-6)).all() and (sig[:, :2] <= 2.4 * dm * (1 + 1e-6)).all()
        assert (np.abs(sig[:, 2]) <= 0.4).all() and (col >= 0.3).all() and (col <= 1.0).all()
        assert np.isnan(c["sig"][1]).all()
        t = c["table"]
        # (row 0 as a box's first row needs rows 0-32; in 512-band16 the forced box that ends on row 15 and the one that starts on row
        # 16 take them -- the one case whose boxes are separate and whose row 0 is not planted)
        assert 0 in t["X"] and c["fw"] - 1 in t["X"] and c["fh"] - 1 in t["Y"] and (0 in t["Y"] or name == "512-band16"), name
    assert {36, 37, 202, 203} <= set(el.case("512-band37")["table"]["Y"].tolist())
    assert {15, 16} <= set(el.case("512-band16")["table"]["Y"].tolist())
    c = el.case("window")
    assert {c["y0"], c["y0"] + c["H"] - 1, c["y0"] - 1, c["y0"] + c["H"]} <= set(c["table"]["Y"].tolist())
    assert {c["x0"], c["x0"] + c["W"] - 1, c["x0"] - 1, c["x0"] + c["W"]} <= set(c["table"]["X"].tolist())
    padded = el.case("256", records=16384)
    assert padded["sig"].shape[0] == 16384 and np.array_equal(el.live(padded["sig"], padded["xy"], padded["col"])[0],
                                                              el.live(el.case("256")["sig"], el.case("256")["xy"], el.case("256")["col"])[0])
    for a, b in ((2, 20), (40, 60)):        # the regular cases keep their boxes apart
        with pytest.raises(AssertionError):
            el.edge_lattice(128, 128, a, b - 17)


# ---- the reference alone passes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GPU_CASES)
def test_the_reference_alone_passes(name):
    from oracle import gs_oracle
    c = el.case(name)
    ref, gref, up = el.reference(name)
    s, x, k, _ = el.live(c["sig"], c["xy"], c["col"])
    dm, rows = float(c["dmax"]), (c["y0"], c["y0"] + c["H"])
    pad = np.zeros((c["H"], c["fw"], 3), np.float32)
    pad[:, c["x0"]: c["x0"] + c["W"]] = up
    for fma in (False, True):
        img = gs_oracle.forward_f32(s, x, k, c["fh"], c["fw"], dm, use_fma=fma, rows=rows)[:, c["x0"]: c["x0"] + c["W"]]
        err = np.abs(img - ref)
        print(f"{name} fma={fma}: image error {err.max():.3e}, bar {img_bar(ref):.3e}")
        assert err.max() <= img_bar(ref), el.blame(name, err)
        g = gs_oracle.backward_f32(s, x, k, pad, dm, use_fma=fma, h=c["fh"], rows=rows)
        print(name, fma, gradbars.check_kernel(g, gref, s, 1.0, f"{name} backward_f32 fma={fma}"))


# ---- the input discriminates ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GPU_CASES)
def test_a_wrong_comparison_is_far_outside_the_bars(name):
    c = el.case(name)
    ref, gref, up = el.reference(name)
    full_up = np.zeros((c["fh"], c["fw"], 3))
    full_up[c["y0"]: c["y0"] + c["H"], c["x0"]: c["x0"] + c["W"]] = up
    assert (np.abs(el.upstream(c, seed=len(name))[tuple(el.planted_points(c["table"], c["fh"], c["fw"]).T)]).min(axis=1) > 0).all()
    s = el.live(c["sig"], c["xy"], c["col"])[0]
    right, gright = restated(c, INCLUSIVE, full_up)
    assert np.abs(window_of(c, right) - ref).max() <= 1e-9 * max(1.0, np.abs(ref).max())      # the restatement is the op
    assert np.abs(gright - gref[2]).max() <= 1e-9 * np.abs(gref[2]).max()
    t = c["table"]
    for keep, k_hit, what in ((STRICT, 0, "strict"), (ONE_ULP_WIDE, 1, "one ulp wide")):
        wrong, gwrong = restated(c, keep, full_up)
        diff = np.abs(wrong - right).max(axis=2)
        inside = np.abs(window_of(c, wrong) - ref).max()
        print(f"{name} {what}: image off by {inside:.3f} = {inside / img_bar(ref):.0f} bars")
        assert inside >= 1000 * img_bar(ref), (name, what)
        # every planted pair of the category this variant gets wrong, individually: its pixel on the centre's row (column)
        hit_x, hit_y = t["k_x"] == k_hit, t["k_y"] == k_hit
        assert hit_x.sum() >= 8 and hit_y.sum() >= 8
        assert (diff[t["row_c"][hit_x], t["X"][hit_x]] > 0.1).all(), (name, what, "x")
        assert (diff[t["Y"][hit_y], t["col_c"][hit_y]] > 0.1).all(), (name, what, "y")
        elem, col_ = gradbars.ratios(gwrong, gref[2], s[:, 2], gradbars.KERNEL_GROUPS["colors"])[:2]
        print(f"{name} {what}: d/d colours {elem.max():.1f} element bars, {col_.max():.1f} column bars")
        assert elem.min() > 1.0 and col_.min() > 1.0, (name, what)


# ---- our CPU path ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GPU_CASES)
def test_the_cpu_path_at_the_planted_pixels(name):
    """gsasr_amd.gaussian_splatting.query_dense (the package's definition of the op off the GPU) at every planted pixel and its
    four neighbours, NaN records included in its input as zero-colour records cannot be: it is given the live ones"""
    from gsasr_amd import gaussian_splatting as gsp
    from oracle import gs_oracle
    c = el.case(name)
    s, x, k, _ = el.live(c["sig"], c["xy"], c["col"])
    full = gs_oracle.forward_f64(s, x, k, c["fh"], c["fw"], float(c["dmax"]))
    pts = el.planted_points(c["table"], c["fh"], c["fw"])
    got = gsp.query_dense(torch.from_numpy(s).double(), torch.from_numpy(x).double(), torch.from_numpy(k).double(), c["fh"], c["fw"],
                          float(c["dmax"]), torch.from_numpy(pts).float())
    want = full[pts[:, 0], pts[:, 1]].T
    err = np.abs(got.numpy() - want).max()
    print(name, len(pts), err)
    assert err <= CPU_RTOL * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("name", ["window", "canvas-0", "canvas-2"])
def test_the_cpu_render_and_its_gradients(name):
    """oracle.host_ref.autograd_render (dense, double): image and all three gradients"""
    from oracle import host_ref
    c = el.case(name)
    ref, gref, up = el.reference(name)
    s, x, k = (torch.from_numpy(a).double().requires_grad_(True) for a in el.live(c["sig"], c["xy"], c["col"])[:3])
    img = host_ref.autograd_render(s, x, k, c["fh"], c["fw"], float(c["dmax"]))[c["y0"]: c["y0"] + c["H"], c["x0"]: c["x0"] + c["W"]]
    assert np.abs(img.detach().numpy() - ref).max() <= CPU_RTOL * max(1.0, np.abs(ref).max())
    (img * torch.from_numpy(up.copy()).double()).sum().backward()
    for g, w in zip((s.grad, x.grad, k.grad), gref):
        assert np.abs(g.numpy() - w).max() <= 10 * CPU_RTOL * np.abs(w).max()


# ---- queries: ties on a refined grid ---------------------------------------------------------------------------------------------
QUERY_BASE = (96, 80, 6, 20)        # H, W, reach, spacing of the grid the queries are made on: dmax = 12 / 95
# ... and of the three samples of the ragged canvas (overlapping boxes, like their pixel lattices)
QUERY_CANVAS = [(40, 56, 4, 2), (64, 64, 4, 2), (33, 47, 3.375, 1)]
_QUERY = {}


def query_case(m, base=QUERY_BASE, records=0):
    """(built once per argument list) the lattice on the refined grid (m (H - 1) + 1) x (m (W - 1) + 1) with planted indices that are no multiples of m, and the
    planted positions as points k / m of the H x W grid, kept where the kernels' own expression of the point's coordinate gives the
    refined grid's float.  -> dict(sig, xy, col, dmax, table, keep_x, keep_y, H, W, Hm, Wm)"""
    if (m, base, records) in _QUERY:
        return _QUERY[(m, base, records)]
    H, W, reach, spacing = base
    Hm, Wm = m * (H - 1) + 1, m * (W - 1) + 1
    sig, xy, col, dmax, table = el.edge_lattice(Hm, Wm, reach * m, spacing * m, seed=m, refine=m, records=records, overlap=base != QUERY_BASE)
    assert dmax == np.float32(2.0 * reach / (max(H, W) - 1))       # the same box on both grids
    keep = {}
    for axis, n, nm, idx in (("x", W, Wm, table["X"]), ("y", H, Hm, table["Y"])):
        pos = (idx.astype(np.float32) / np.float32(m)).astype(np.float32)                  # k / m, exact in float
        as_kernels = (2.0 * pos.astype(np.float64) / (n - 1) - 1.0).astype(np.float32)
        keep[axis] = (as_kernels == el.pixel_coords(nm)[idx]) & (idx % m != 0)
    q = dict(sig=sig, xy=xy, col=col, dmax=dmax, table=table, keep_x=keep["x"], keep_y=keep["y"], H=H, W=W, Hm=Hm, Wm=Wm, m=m)
    _QUERY[(m, base, records)] = q
    return q


def query_points(q):
    """the refined-grid pixels [S, 2] of a query case that hold a planted tie: column X on the centre's row, row Y on the centre's
    column and the corner (Y, X), of the positions kept"""
    t = q["table"]
    kk = np.concatenate([np.stack([t["row_c"], t["X"]], 1)[q["keep_x"]], np.stack([t["Y"], t["col_c"]], 1)[q["keep_y"]],
                         np.stack([t["Y"], t["X"]], 1)[q["keep_x"] & q["keep_y"]]])
    return np.unique(kk, axis=0)


@pytest.mark.parametrize("m,base", [(2, QUERY_BASE), (4, QUERY_BASE)] + [(2, b) for b in QUERY_CANVAS],
                         ids=["m2", "m4", "canvas-0", "canvas-1", "canvas-2"])
def test_query_ties_between_the_pixel_centres(m, base):
    q = query_case(m, base)
    t = q["table"]
    assert (t["X"] % m != 0).all() and (t["Y"] % m != 0).all()
    for axis, keep in (("x", q["keep_x"]), ("y", q["keep_y"])):
        for s in (1, -1):
            n = int((keep & (t["sign_" + axis] == s) & (np.abs(t["k_" + axis]) <= 2)).sum())
            ties = int((keep & (t["sign_" + axis] == s) & (t["k_" + axis] == 0)).sum())
            print(f"m={m} {axis} sign {s}: {n} positions within 2 ulp of the edge, {ties} exact ties")
            assert n >= 4, (m, axis, s)
