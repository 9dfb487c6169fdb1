"""Gaussians whose dmax box edge falls ON a pixel, or one or two float steps beside it (numpy only; a plain module like gradbars).

The bounded op keeps a term only if |dx| <= dmax and |dy| <= dmax, decided in float32 on the pixel coordinates
px[i] = (float)(2.0 * i / (n - 1) - 1.0) and the float difference dx = px[X] - x (oracle/gs_ref.c: grid_coord and the box tests).
Random centres never meet that edge.  Here every Gaussian gets one PLANTED column X and one planted row Y, and its centre is the
float for which fl(px[X] - x) is, in units of the float spacing of dmax ("ulp"),

    category  0   exactly +-dmax              kept
             -1   one ulp inside              kept
             +1   one ulp outside             dropped
             +2   two ulp outside             dropped

The SIGN of a pair is the sign of that difference: +1 = the planted pixel is the box's last column (row), -1 = its first.

What a pixel admits.  dx is a difference of floats of size |x| <= 1 and lands on a lattice of spacing ulp(x), up to 8 times the
spacing of dmax's own floats: for |x| >= 1/2 only one of eight consecutive ulp offsets can be reached at a given pixel, for
|x| < 1/8 all of them.  So the CATEGORY FOLLOWS THE PIXEL: `admits` lists, by trying the candidate centres, which of the four a
pixel can carry, slots are chosen among the pixels that admit what is still missing, and a pixel that admits none of the four
takes the nearest reachable offset (its `k` in the table says which, e.g. -5 or +3; such pairs count for nothing).

Layout.  One list of slots per axis, Gaussians on their cross product, so that the two axes are independent (kept x kept,
kept x dropped and dropped x dropped corners all occur) and a Gaussian's box [c - reach, c + reach] shares no pixel with another's:
slots keep a pitch of at least `spacing` >= 2 * reach + 8 (forced slots, see below, and the few slots placed for a scarce
category keep only their boxes 3 px apart; `overlap=True` gives the boxes up altogether: the large class, tiny grids).  Every other slot
is ALIGNED: its planted pixel is the only column (row) of its 32-px unit that the box reaches -- sign +1 on an index = 0 (mod 32),
sign -1 on 31 (mod 32), which is also 0 / 15 (mod 16) and 0 / 7 (mod 8): 16-px plan cells, 8- and 16-px sub-tiles and 32 x 16 /
32 x 32 tiles at once.  The rest sit mid-unit.  Forced slots put planted pixels on the first and last index of the grid, on the
border of a window or row band and just outside it.
"""
import math

import numpy as np

CATEGORIES = (0, -1, 1, 2)          # ulps outward of +-dmax
KEPT = (0, -1)
F32 = np.float32


def pixel_coords(n):
    """the reference's pixel coordinates: a double expression rounded once to float"""
    return (2.0 * np.arange(n, dtype=np.float64) / (n - 1) - 1.0).astype(np.float32)


def step(v, k):
    """the float32 `k` steps away from `v` in magnitude (k > 0: larger)"""
    v = F32(v)
    for _ in range(abs(int(k))):
        v = np.nextafter(v, F32(math.copysign(np.inf, v)) if k > 0 else F32(0.0))
    return v


def ulps_out(d, dmax):
    """how many float32 steps |d| lies beyond dmax (negative: inside), from the bit patterns"""
    a = np.abs(np.asarray(d, dtype=np.float32)).view(np.int32).astype(np.int64)
    return a - int(np.asarray(dmax, dtype=np.float32).view(np.int32))


def centre_for(p, sign, k, dmax):
    """the float32 centre x with fl(p - x) == sign * step(dmax, k), or None if no float gives it"""
    want = F32(sign) * step(dmax, k)
    x = F32(np.float64(p) - np.float64(want))
    for cand in (x, np.nextafter(x, F32(np.inf)), np.nextafter(x, F32(-np.inf)),
                 np.nextafter(np.nextafter(x, F32(np.inf)), F32(np.inf)), np.nextafter(np.nextafter(x, F32(-np.inf)), F32(-np.inf))):
        if F32(p) - cand == want:
            return cand
    return None


def nearest_centre(p, sign, dmax):
    """for a pixel that admits none of the four categories: the centre whose difference is the closest reachable one"""
    x = F32(np.float64(p) - np.float64(F32(sign) * F32(dmax)))
    return x, int(ulps_out(F32(p) - x, dmax))


def admits(p, sign, dmax):
    return tuple(k for k in CATEGORIES if centre_for(p, sign, k, dmax) is not None)


class Slot:
    __slots__ = ("X", "sign", "aligned", "forced", "cats")

    def __init__(self, X, sign, aligned, forced, cats):
        self.X, self.sign, self.aligned, self.forced, self.cats = int(X), int(sign), bool(aligned), bool(forced), tuple(cats)


def _box(X, sign, reach):
    """the pixels a box with planted index X may reach: [lo, hi] (the planted pixel itself included)"""
    r = int(math.ceil(reach))
    return (X - 2 * r, X) if sign > 0 else (X, X + 2 * r)


def _is_aligned(X, sign, unit=32):
    return X % unit == (0 if sign > 0 else unit - 1)


WANTED = {0: 4, -1: 4, 1: 4, 2: 2}      # pairs per sign and axis that a case should hold at the least


def assign(slots, others):
    """the categories of the `others` Gaussians of every slot: whatever is missing most (per sign) among those the slot's pixel
    admits, the slots that admit least first.  -> ([categories] per slot, {(sign, category) or ("aligned", sign): still missing})"""
    left = {(s, k): float(w) for s in (1, -1) for k, w in WANTED.items()}
    left.update({("aligned", 1): 4.0, ("aligned", -1): 4.0})
    out = [None] * len(slots)
    for i in sorted(range(len(slots)), key=lambda i: (len(slots[i].cats), slots[i].X)):
        sl, out[i] = slots[i], []
        for _ in range(others if sl.cats else 0):
            def want(k):
                w = left[(sl.sign, k)]
                if sl.aligned and k in KEPT:
                    w = max(w, left[("aligned", sl.sign)])
                return w
            k = max(sl.cats, key=want)
            out[i].append(k)
            left[(sl.sign, k)] -= 1
            if sl.aligned and k in KEPT:
                left[("aligned", sl.sign)] -= 1
    return out, left


def axis_slots(n, dmax, spacing, forced=(), others=8, refine=1, overlap=False):
    """slots along one axis of `n` pixels.  `forced` = [(X, sign)].  `others`: how many Gaussians share a slot (the slots of the
    other axis), for the running count of what is still missing.  `refine` = m > 1: planted indices are no multiples of m (points of
    a refined grid that are no pixel centres) and alignment is to units of 32 * m"""
    px = pixel_coords(n)
    reach = float(dmax) * (n - 1) / 2.0
    r = int(math.ceil(reach))
    half = spacing / 2.0
    unit = 32 * refine
    slots, boxes = [], []
    for X, sign in forced:
        if 0 <= X < n and (refine == 1 or X % refine):
            lo, hi = _box(X, sign, reach)
            if overlap or all(hi < a or lo > b for a, b in boxes):      # (a forced box may leave the grid: row 15 as a last row)
                slots.append(Slot(X, sign, _is_aligned(X, sign, unit), True, admits(px[X], sign, dmax)))
                boxes.append((lo, hi))
    def missing():
        return assign(slots, others)[1]

    def free(X, sign, pitch=True):
        """the box inside the grid and at least 3 px from every other box; with `pitch`, the centre `spacing` from the others"""
        c = X - sign * reach
        if c - r < 0 or c + r > n - 1:
            return False
        lo, hi = _box(X, sign, reach)
        for s, (a, b) in zip(slots, boxes):
            if not (hi + 3 <= a or lo - 3 >= b) and not overlap:
                return False
            if (pitch and not s.forced and abs(s.X - s.sign * reach - c) < spacing) or (s.X, s.sign) == (X, sign):
                return False
        return True

    cache = {}

    def adm(X, sign):
        if (X, sign) not in cache:
            cache[(X, sign)] = admits(px[X], sign, dmax)
        return cache[(X, sign)]

    def place(slot):
        slots.append(slot)
        boxes.append(_box(slot.X, slot.sign, reach))

    # Two passes over one list `slots` (with `boxes` beside it).  Invariants of both: a slot is (planted index, sign) and is placed
    # once; its box lies inside the grid (forced slots excepted) and, unless `overlap`, at least 3 px from every other box; `missing()`
    # replays `assign` on the slots so far and says what the counts still lack.  Pass 1 is driven by that: it takes the requirement
    # fewest pixels can carry and the outermost free pixel that carries it, and closes a requirement that no free pixel helps.  Pass 2
    # fills what is left at the pitch `spacing`, keeping a third of all slots aligned.  Neither pass is trusted: the categories are
    # recomputed from the float differences when the table is built, and tests/test_box_edge.py counts them again.
    # first what is scarce: slots that carry a category (or an aligned kept pair) that is still missing, wherever they are.
    # A box with sign +1 extends to the left of its planted pixel, so the leftmost candidate leaves most room, and vice versa.
    closed = set()

    def carries(q, X):
        sign = q[1] if q[0] == "aligned" else q[0]
        if refine > 1 and X % refine == 0:
            return False
        if q[0] == "aligned":
            return _is_aligned(X, sign, unit) and bool(set(adm(X, sign)) & set(KEPT))
        return q[1] in adm(X, sign)

    rare = {q: sum(carries(q, X) for X in range(n)) for q in missing()}      # the fewer pixels carry it, the earlier its turn
    while True:
        left = {q: v for q, v in missing().items() if q not in closed and v > 0}
        if not left:
            break
        q = min(left, key=lambda t: (t[1] != 2, rare[t], str(t)))
        sign = q[1] if q[0] == "aligned" else q[0]
        best = None
        order = list(range(n) if sign > 0 else range(n - 1, -1, -1))
        # an aligned pixel if one carries it; for the two-ulp pairs first a pixel that carries nothing else (those lie beside the
        # strip in the middle that all the other scarce categories compete for)
        first = [X for X in order if adm(X, sign) == (2,)] if q[1] == 2 else [X for X in order if _is_aligned(X, sign, unit)]
        for X in first + order:
            if carries(q, X) and free(X, sign, pitch=False):
                best = Slot(X, sign, _is_aligned(X, sign, unit), False, adm(X, sign))
                break
        if best is None:
            closed.add(q)           # this grid cannot give it
            continue
        place(best)
        if missing().get(q, 0) >= left[q]:
            closed.add(q)

    # then the gaps, left to right, aligned and mid-unit slots in turn
    cmin, j = float(r), 0          # the smallest centre the next slot may have
    while cmin + r <= n - 1:
        want_aligned = 2 * sum(sl.aligned for sl in slots) <= len(slots)       # half of the slots, forced ones counted
        sign = 1 if (j // 2) % 2 == 0 else -1
        first = int(math.ceil(cmin + sign * reach))         # the planted index of the first box centred at `cmin` or later
        best, score = None, -1.0
        for X in range(first, min(n, first + (unit if want_aligned else 12 * refine))):
            al = _is_aligned(X, sign, unit)
            if al != want_aligned or (refine > 1 and X % refine == 0) or not free(X, sign):
                continue
            if not al and X % unit in (0, unit - 1, unit // 2 - 1, unit // 2):
                continue
            cats = adm(X, sign)
            sc = len(cats)
            if sc > score:
                best, score = Slot(X, sign, al, False, cats), sc
        j += 1
        if best is None and want_aligned and 3 * sum(sl.aligned for sl in slots) >= len(slots) + 1:
            # no aligned pixel free within a unit: a mid-unit one, if any, as long as a third of the slots stay aligned
            for X in range(first, min(n, first + 12 * refine)):
                if not _is_aligned(X, sign, unit) and not (refine > 1 and X % refine == 0) and free(X, sign):
                    best = Slot(X, sign, False, False, adm(X, sign))
                    break
        if best is None:        # nothing free here: a slot is in the way, or the grid ends
            cmin += 4.0
            continue
        place(best)
        cmin = cmin + 4.0
    order = np.argsort([s.X - s.sign * reach for s in slots])
    return [slots[i] for i in order]


TABLE_DTYPE = np.dtype([("record", np.int32), ("X", np.int32), ("Y", np.int32), ("sign_x", np.int8), ("sign_y", np.int8),
                        ("k_x", np.int32), ("k_y", np.int32), ("aligned_x", np.bool_), ("aligned_y", np.bool_),
                        ("forced_x", np.bool_), ("forced_y", np.bool_), ("row_c", np.int32), ("col_c", np.int32)])


def edge_lattice(H, W, reach_px, spacing, records=0, seed=0, grid=None, forced_rows=(), forced_cols=(), refine=1, overlap=False):
    """-> sigmas [s,3], coords [s,2], colors [s,3] (float32 numpy), dmax (np.float32), table (TABLE_DTYPE, one entry per live
    Gaussian).  `grid` = (fh, fw, y0, x0): the lattice is built on the fh x fw grid and H x W is the window at (y0, x0); X, Y,
    row_c, col_c are indices of the FULL grid then.  `row_c` / `col_c`: the pixel nearest the centre.  k_x / k_y: the category
    actually reached, computed from the float difference.  `records`: NaN records pad the list to that count (record 1 is one
    always), as tests/test_u8_output_gpu.py `separated` does."""
    assert overlap or spacing >= 2 * reach_px + 8
    fh, fw, y0, x0 = (H, W, 0, 0) if grid is None else grid
    nmax = max(fh, fw)
    dmax = F32(2.0 * reach_px / (nmax - 1))
    rows_f = list(forced_rows) + [(0, -1), (fh - 1, 1)]
    cols_f = list(forced_cols) + [(0, -1), (fw - 1, 1)]
    if grid is not None:    # the window's border rows / columns as box edges from inside, and the ones just outside from outside
        rows_f += [(y0, -1), (y0 + H - 1, 1), (y0 - 1, 1), (y0 + H, -1)]
        cols_f += [(x0, -1), (x0 + W - 1, 1), (x0 - 1, 1), (x0 + W, -1)]
    def pitch(n):      # `spacing` is in pixels of the longer axis; the shorter one has the same pitch in coordinates
        p = int(round(spacing * (n - 1) / (nmax - 1)))
        return max(p, 1) if overlap else max(p, int(math.ceil(float(dmax) * (n - 1))) + 8)

    guess = max(2, nmax // spacing)
    xs = axis_slots(fw, dmax, pitch(fw), cols_f, others=guess, refine=refine, overlap=overlap)
    ys = axis_slots(fh, dmax, pitch(fh), rows_f, others=len(xs), refine=refine, overlap=overlap)
    xs = axis_slots(fw, dmax, pitch(fw), cols_f, others=len(ys), refine=refine, overlap=overlap)
    cat_x, cat_y = assign(xs, len(ys))[0], assign(ys, len(xs))[0]
    px, py = pixel_coords(fw), pixel_coords(fh)
    rng = np.random.RandomState(seed)
    recs, tab = [], []
    for iy, sy in enumerate(ys):
        for ix, sx in enumerate(xs):
            kx = cat_x[ix][iy] if sx.cats else None
            ky = cat_y[iy][ix] if sy.cats else None
            x, kx = (centre_for(px[sx.X], sx.sign, kx, dmax), kx) if kx is not None else nearest_centre(px[sx.X], sx.sign, dmax)
            y, ky = (centre_for(py[sy.X], sy.sign, ky, dmax), ky) if ky is not None else nearest_centre(py[sy.X], sy.sign, dmax)
            sig = (rng.uniform(1.6, 2.4) * dmax, rng.uniform(1.6, 2.4) * dmax, rng.uniform(-0.4, 0.4))
            col = rng.uniform(0.3, 1.0, 3)
            recs.append([sig[0], sig[1], sig[2], x, y, col[0], col[1], col[2]])
            col_c = int(np.clip(round((float(x) + 1.0) * 0.5 * (fw - 1)), 0, fw - 1))
            row_c = int(np.clip(round((float(y) + 1.0) * 0.5 * (fh - 1)), 0, fh - 1))
            tab.append((0, sx.X, sy.X, sx.sign, sy.sign, kx, ky, sx.aligned, sy.aligned, sx.forced, sy.forced, row_c, col_c))
    rec = np.asarray(recs, dtype=np.float32)
    n = rec.shape[0]
    total = max(n + 1, records)
    out = np.full((total, 8), np.nan, np.float32)
    out[0] = rec[0]
    out[2: n + 1] = rec[1:]
    table = np.array(tab, dtype=TABLE_DTYPE)
    table["record"] = np.concatenate([[0], np.arange(2, n + 1)])
    # the categories as the oracle's own float arithmetic sees them
    dx = px[table["X"]] - out[table["record"], 3]
    dy = py[table["Y"]] - out[table["record"], 4]
    assert np.array_equal(np.sign(dx), table["sign_x"]) and np.array_equal(np.sign(dy), table["sign_y"])
    assert np.array_equal(ulps_out(dx, dmax), table["k_x"]) and np.array_equal(ulps_out(dy, dmax), table["k_y"])
    return (np.ascontiguousarray(out[:, 0:3]), np.ascontiguousarray(out[:, 3:5]), np.ascontiguousarray(out[:, 5:8]), dmax, table)


def live(sigmas, coords, colors):
    """the records that are no NaN records (dead by the header's contract): what the CPU side is given"""
    ok = np.isfinite(sigmas).all(1) & np.isfinite(coords).all(1) & np.isfinite(colors).all(1)
    return sigmas[ok], coords[ok], colors[ok], np.nonzero(ok)[0]


def counts(table, axis):
    """{(sign, what): number of pairs} on `axis` ("x" / "y"): what = 0, -1, 1, 2, "aligned_kept", "aligned", "all" """
    out = {}
    k, sg, al = table["k_" + axis], table["sign_" + axis], table["aligned_" + axis]
    for s in (1, -1):
        m = sg == s
        for c in CATEGORIES:
            out[(s, c)] = int((m & (k == c)).sum())
        out[(s, "aligned_kept")] = int((m & al & np.isin(k, KEPT)).sum())
        out[(s, "aligned")] = int((m & al).sum())
        out[(s, "all")] = int(m.sum())
    return out


def planted_points(table, fh, fw, neighbours=True):
    """(row, col) of every planted pixel of the table -- column X at the centre's row and row Y at the centre's column, and the
    corner (Y, X) -- with their four neighbours, inside the grid, unique"""
    pts = set()
    for t in table:
        for r, c in ((t["row_c"], t["X"]), (t["Y"], t["col_c"]), (t["Y"], t["X"])):
            for dr, dc in ((0, 0), (1, 0), (-1, 0), (0, 1), (0, -1)) if neighbours else ((0, 0),):
                if 0 <= r + dr < fh and 0 <= c + dc < fw:
                    pts.add((int(r + dr), int(c + dc)))
    return np.array(sorted(pts), dtype=np.int64)


def describe(table, row, col, reach):
    """the planted pair nearest to pixel (row, col) of the full grid, for a failure message"""
    best = None
    for t in table:
        for axis, idx, other, oc in (("x", t["X"], row, t["row_c"]), ("y", t["Y"], col, t["col_c"])):
            at = col if axis == "x" else row
            if abs(other - oc) <= reach + 2:
                d = abs(int(at) - int(idx))
                if best is None or d < best[0]:
                    best = (d, f"Gaussian {int(t['record'])}: planted {'column' if axis == 'x' else 'row'} {int(idx)}, sign "
                               f"{int(t['sign_' + axis])}, category {int(t['k_' + axis])} ulp "
                               f"({'kept' if t['k_' + axis] <= 0 else 'dropped'}), {'aligned' if t['aligned_' + axis] else 'mid-unit'}"
                               f"{', forced' if t['forced_' + axis] else ''}; {d} px from the failing pixel")
    return best[1] if best else "no planted pair near this pixel"


# ---- the cases of tests/test_box_edge.py (CPU) and tests/test_box_edge_gpu.py -------------------------------------------------
# name -> (H, W, reach_px, spacing, keywords).  The reach is chosen so that dmax = 2 reach / (n - 1) lies just above a power of
# two: all four categories can be reached only where ulp(x) <= ulp(dmax), i.e. |x| < 2^(e+1) for dmax in [2^e, 2^(e+1)) -- a strip
# of one to two boxes' width in the middle of the grid, widest for dmax at the bottom of its binade (512 px: reach 16, 32 / 511).
CASES = {
    "512": (512, 512, 16, 40, {}),
    # row bands (37, 203) and (16, None): their first and last rows as box edges from inside, the rows just outside from outside
    # (the box forced below row 203 covers the strip in the middle of the grid where alone a pixel admits all four categories, and
    # leaves no room there for a separate box of either sign: this case lets its boxes overlap)
    "512-band37": (512, 512, 16, 40, dict(overlap=True, forced_rows=[(37, -1), (202, 1), (36, 1), (203, -1)])),
    "512-band16": (512, 512, 16, 40, dict(forced_rows=[(16, -1), (15, 1)])),
    "256-band37": (256, 256, 8, 16, dict(overlap=True, forced_rows=[(37, -1), (202, 1), (36, 1), (203, -1)])),
    "256-band16": (256, 256, 8, 16, dict(overlap=True, forced_rows=[(16, -1), (15, 1)])),
    "1024x512": (1024, 512, 32, 72, {}),
    "512x256": (512, 256, 16, 40, {}),
    "768x1024": (768, 1024, 32, 72, {}),
    "640x512": (640, 512, 20, 48, {}),
    # grids too small for sixteen separate boxes a side: the boxes overlap (a pixel then sums several Gaussians, as in real input)
    "256": (256, 256, 8, 16, dict(overlap=True)),
    "250x300": (250, 300, 10, 12, dict(overlap=True)),
    "large-class": (512, 384, 140, 40, dict(overlap=True)),             # reach above RCAP_PX = 128: the large-class segment
    "window": (70, 61, 4, 8, dict(grid=(128, 96, 19, 7), overlap=True)),
    "canvas-0": (40, 56, 4, 2, dict(overlap=True)),
    "canvas-1": (64, 64, 4, 2, dict(overlap=True)),
    # 33 rows: the only aligned rows are 32 (a box's last row) and 31 (the first row of a box that leaves the grid), both forced; reach
    # 3.375 px = 0.1467 is one at which both rows admit an exact tie
    "canvas-2": (33, 47, 3.375, 1, dict(overlap=True, forced_rows=[(32, 1), (31, -1)])),
    # ... and one window of each of those grids: batched windows
    "canvas-window-0": (24, 40, 4, 2, dict(grid=(40, 56, 9, 7), overlap=True)),
    "canvas-window-1": (40, 33, 4, 2, dict(grid=(64, 64, 11, 20), overlap=True)),
    "canvas-window-2": (20, 30, 3.375, 1, dict(grid=(33, 47, 6, 9), overlap=True, forced_rows=[(32, 1), (31, -1)])),
}
_BUILT = {}


def case(name, records=0):
    """edge_lattice of CASES[name] -> dict(sig, xy, col, dmax, table, H, W, fh, fw, y0, x0, reach); built once per (name, records)"""
    if (name, records) not in _BUILT:
        H, W, reach, spacing, kw = CASES[name]
        sig, xy, col, dmax, table = edge_lattice(H, W, reach, spacing, records=records, seed=len(name), **kw)
        fh, fw, y0, x0 = kw.get("grid", (H, W, 0, 0))
        for a in (sig, xy, col, table):
            a.setflags(write=False)
        _BUILT[(name, records)] = dict(sig=sig, xy=xy, col=col, dmax=dmax, table=table, H=H, W=W, fh=fh, fw=fw, y0=y0, x0=x0, reach=reach)
    return _BUILT[(name, records)]


def upstream(c, seed=0):
    """an image gradient [fh, fw, 3] of case dict `c`: uniform in [0.25, 1] on every planted pixel (column X on the centre's row, row
    Y on the centre's column, the corner (Y, X)) and its four neighbours, zero elsewhere -- the sums of a gradient then hold the
    terms the box decides on and few others, so that float32 summation (the reference's own included) stays inside the bars even
    for the 281 x 211-px boxes of the large class"""
    up = np.zeros((c["fh"], c["fw"], 3), np.float32)
    pts = planted_points(c["table"], c["fh"], c["fw"])
    up[pts[:, 0], pts[:, 1]] = np.random.RandomState(1000 + seed).uniform(0.25, 1.0, (len(pts), 3)).astype(np.float32)
    return up


_REF = {}


def reference(name, rows=None):
    """(forward_f64 image, backward_f64 gradients for `upstream`, the upstream gradient) of case `name` -- for a window: of the
    window, with the oracle rendering the rows of the FULL grid and the upstream zero outside the window's columns.  `rows`: a row
    band of the (full) image.  Rows of the gradients follow the LIVE records (`live`).  Computed once, never written to."""
    key = (name, rows)
    if key not in _REF:
        from oracle import gs_oracle
        c = case(name)
        s, x, k, _ = live(c["sig"], c["xy"], c["col"])
        r0, r1 = (c["y0"], c["y0"] + c["H"]) if rows is None else rows
        dm = float(c["dmax"])
        img = gs_oracle.forward_f64(s, x, k, c["fh"], c["fw"], dm, rows=(r0, r1))[:, c["x0"]: c["x0"] + c["W"]]
        up = upstream(c, seed=len(name))[r0:r1, c["x0"]: c["x0"] + c["W"]].copy()
        pad = np.zeros((r1 - r0, c["fw"], 3), np.float32)
        pad[:, c["x0"]: c["x0"] + c["W"]] = up
        grads = gs_oracle.backward_f64(s, x, k, pad, dm, h=c["fh"], rows=(r0, r1))
        for a in (img, up) + tuple(grads):
            a.setflags(write=False)
        _REF[key] = (img, grads, up)
    return _REF[key]


def blame(name, err_hw, rows=None):
    """for a failure message: the worst pixel of an error image [rows, W] (or [rows, W, 3]) of case `name` and the planted pair
    next to it"""
    c = case(name)
    e = np.asarray(err_hw)
    e = e.max(axis=2) if e.ndim == 3 else e
    r, q = np.unravel_index(int(np.argmax(e)), e.shape)
    r0 = c["y0"] if rows is None else rows[0]
    return (f"worst pixel (row {r + r0}, column {q + c['x0']}) of the full grid, error {e[r, q]:.3e}: "
            + describe(c["table"], r + r0, q + c["x0"], c["reach"]))


def blame_gradient(name, got, want):
    """the Gaussian whose gradient row is worst, with its planted pairs"""
    c = case(name)
    worst, where = 0.0, 0
    for g, w in zip(got, want):
        g, w = np.asarray(g, np.float64), np.asarray(w, np.float64)
        e = np.abs(g - w).max(axis=1) / (np.abs(w).max() + 1e-30)
        if e.max() > worst:
            worst, where = float(e.max()), int(np.argmax(e))
    t = c["table"][where]
    return (f"worst live Gaussian {where} (record {int(t['record'])}), error {worst:.3e} of the tensor's largest value: planted column "
            f"{int(t['X'])} (sign {int(t['sign_x'])}, {int(t['k_x'])} ulp), planted row {int(t['Y'])} (sign {int(t['sign_y'])}, {int(t['k_y'])} ulp)")
