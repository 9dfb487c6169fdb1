"""An independent float64 reference of the row-band selection (a plain module, like gradbars: `import bandref`), and the
geometries the band tests share.

The window is written here from its documentation alone ("Support cutoff tau", and the dmax box), never from
the library's footprint code: pixel row R sits at 2R/(H-1) - 1, so a Gaussian centred at y has its centre on row
cyp = (y+1)(H-1)/2 and reaches min(dmax, sqrt(2 tau) |sy|) (H-1)/2 rows to either side (tau <= 0: the box alone; no box and no tau:
every row).  Its rows are the integers of [cyp - ey, cyp + ey] on the grid, its columns likewise; a record with a non-finite
sigma or centre, or with no row or no column on the grid, is dead.  Against a band [band0, band1) with `rows_above` / `rows_below`
rows of neighbours, a live Gaussian goes UP when its first row is above band0, DOWN when its last row is at or below band1, and
is FAR when it reaches past the neighbour on a side it goes to.

The kernel takes the same window 0.02 px wider, so the two can differ on a Gaussian whose window edge is that close to a row
that decides something.  `nudge` moves such Gaussians (by 0.2 px, none is dropped) until every edge keeps 0.05 px from the
deciding rows; after that the comparison is exact set equality.
"""
import math

import numpy as np

EDGE_CLEAR = 0.05      # px every window edge keeps from a deciding row after `nudge` (the kernel widens by 0.02)
NUDGE = 0.2            # px a Gaussian is moved by
ERROR_BOUND = 1e-5     # the plan's documented image error under the default cutoff

# geometries of the multi-rank tests: 24 x 12 LR x4 = 96 x 48 HR, 288 Gaussians (96 per rank of three: no multiple of 64)
H_LR, W_LR, SCALE = 24, 12, 4.0
GRAD_SEED = 61
# "adjacent": footprints reach a few rows into the neighbour.  "thin": at three ranks (32-row bands) Gaussians centred in the
# middle band reach BOTH neighbours without reaching past them.  Under the adaptive default tau = ln(N / 1e-5) = 17.2 a
# synthetic Gaussian (sigma <= 2.7 px) spans at most 15.6 rows to a side, and 16.5 are needed from the middle of a 32-row
# band: the thin geometry therefore runs with the explicit tau = 104 (the reference's exact set of fp32 terms), under which the
# 23.75-row dmax box is what bounds nearly every window.
GEOMETRIES = {
    "adjacent": dict(seed=62, dmax=0.2, cutoff=0.0, cap=96),
    "thin": dict(seed=62, dmax=0.5, cutoff=104.0, cap=96),
}


def row_band(h, rank, world):
    return (rank * h) // world, ((rank + 1) * h) // world


def neighbours(h, rank, world):
    """(rows_above, rows_below): the heights of the adjacent bands, 0 at the ends of the split"""
    span = lambda r: row_band(h, r, world)[1] - row_band(h, r, world)[0]
    return (span(rank - 1) if rank > 0 else 0), (span(rank + 1) if rank < world - 1 else 0)


def default_tau(s):
    """the documented adaptive default: ln(s / 1e-5) within [16, 104], as a float32"""
    return float(np.float32(min(max(math.log(max(int(s), 1) / 1e-5), 16.0), 104.0)))


def _extent(sigma, n, dmax, tau):
    ext = np.full(sigma.shape, np.inf if dmax is None else float(np.float32(dmax)))
    if tau > 0.0:
        ext = np.minimum(ext, math.sqrt(2.0 * tau) * np.abs(sigma))
    return ext * 0.5 * (n - 1)


def edges(rec, h, dmax, tau):
    """(lo, hi) of the row window in pixel units, unclipped and unrounded; float64 [n] each"""
    rec = np.asarray(rec, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        cyp = (rec[:, 4] + 1.0) * 0.5 * (h - 1)
        ey = _extent(rec[:, 1], h, dmax, tau)
        return cyp - ey, cyp + ey


def window(rec, h, w, dmax, tau):
    """(r0, r1, live): the inclusive row window on the grid of every record [n, 8] {sx sy rho x y r g b}, and which have one"""
    rec = np.asarray(rec, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        lo, hi = edges(rec, h, dmax, tau)
        cxp = (rec[:, 3] + 1.0) * 0.5 * (w - 1)
        ex = _extent(rec[:, 0], w, dmax, tau)
        finite = np.isfinite(rec[:, [0, 1, 3, 4]]).all(axis=1)
        r0, r1 = np.maximum(np.ceil(lo), 0.0), np.minimum(np.floor(hi), h - 1.0)
        c0, c1 = np.maximum(np.ceil(cxp - ex), 0.0), np.minimum(np.floor(cxp + ex), w - 1.0)
        live = finite & (r0 <= r1) & (c0 <= c1)
    return r0, r1, live


def select(rec, h, w, dmax, tau, rank, world):
    """the reference selection of `rec` as the own set of `rank`: dict of index arrays up / down / far (ascending)"""
    band0, band1 = row_band(h, rank, world)
    above, below = neighbours(h, rank, world)
    r0, r1, live = window(rec, h, w, dmax, tau)
    up = live & (above > 0) & (r0 < band0)
    down = live & (below > 0) & (r1 >= band1)
    far = (up & (r0 < band0 - above)) | (down & (r1 >= band1 + below))
    return dict(up=np.flatnonzero(up), down=np.flatnonzero(down), far=np.flatnonzero(far), live=live)


def deciding_rows(h, rank, world):
    """the four rows the selection compares a window with.  A first row r0 = ceil(lo) is `< d` exactly when lo <= d - 1, a last
    row r1 = floor(hi) is `>= d` exactly when hi >= d: so an edge decides at d - 1 or at d, and both are kept clear"""
    band0, band1 = row_band(h, rank, world)
    above, below = neighbours(h, rank, world)
    four = (band0, band1, band0 - above, band1 + below)
    return four, sorted({d + k for d in four for k in (-1, 0)} | {-1, 0, h - 1, h})     # (... and where the grid clips it dead)


def near_edge(rec, h, dmax, tau, rank, world):
    """which records have a window edge within EDGE_CLEAR px of a deciding row"""
    lo, hi = edges(rec, h, dmax, tau)
    _, rows = deciding_rows(h, rank, world)
    rows = np.asarray(rows, dtype=np.float64)[None, :]
    with np.errstate(invalid="ignore"):
        return (np.abs(lo[:, None] - rows) < EDGE_CLEAR).any(axis=1) | (np.abs(hi[:, None] - rows) < EDGE_CLEAR).any(axis=1)


def nudge(rec, h, dmax, tau, rank, world):
    """float32 copy of `rec` with every Gaussian that `near_edge` names moved down by NUDGE px (again while it still is: both edges
    move together, and five steps of 0.2 px cannot all be within 0.05 px of a row for either edge); returns (records, moved)"""
    rec = np.array(rec, dtype=np.float32)
    moved = np.zeros(rec.shape[0], dtype=bool)
    for _ in range(5):
        near = near_edge(rec, h, dmax, tau, rank, world)
        if not near.any():
            break
        moved |= near
        rec[near, 4] = (rec[near, 4].astype(np.float64) + NUDGE / (0.5 * (h - 1))).astype(np.float32)
    assert not near_edge(rec, h, dmax, tau, rank, world).any()
    return rec, moved


def reaches(rec, h, w, dmax, rows, threshold):
    """which records put more than `threshold` on some pixel of `rows`, by the float64 oracle's own image of each Gaussian alone
    (the operation itself: no window formula behind it); records with a non-finite or zero sigma or centre are left out"""
    from oracle import gs_oracle
    rec = np.asarray(rec, dtype=np.float32)
    out = np.zeros(rec.shape[0], dtype=bool)
    if rows[1] <= rows[0]:
        return out
    ok = np.isfinite(rec).all(axis=1) & (rec[:, 0] != 0) & (rec[:, 1] != 0)
    for i in np.flatnonzero(ok):
        one = rec[i: i + 1]
        img = gs_oracle.forward_f64(one[:, 0:3], one[:, 3:5], one[:, 5:8], h, w, dmax, rows=rows)
        out[i] = np.abs(img).max() > threshold
    return out


def lower_bound(rec, h, w, dmax, tau, rank, world):
    """(must_up, must_down): Gaussians whose own image exceeds the error bound on a neighbour's rows.  Every term the window skips
    is below exp(-tau) |colour|; the default tau keeps all of them together below 1e-5, an explicit smaller tau is the caller's
    own bound, so the threshold is the larger of the two"""
    band0, band1 = row_band(h, rank, world)
    above, below = neighbours(h, rank, world)
    rec = np.asarray(rec, dtype=np.float32)
    cmax = float(np.nanmax(np.abs(np.where(np.isfinite(rec[:, 5:8]), rec[:, 5:8], 0.0)), initial=0.0))
    thr = max(ERROR_BOUND, (math.exp(-tau) if tau > 0.0 else 0.0) * max(1.0, cmax))
    return (reaches(rec, h, w, dmax, (band0 - above, band0), thr), reaches(rec, h, w, dmax, (band1, band1 + below), thr))


def geometry(name, world):
    """(records [288, 8] float32, H, W, dmax, tau passed to BandExchange, cap, [(a, b) own slice per rank]) of a named geometry:
    rank r owns the Gaussians of its LR rows, as a sharded decoder would produce them"""
    import torch
    from gsasr_amd import synthetic
    g = GEOMETRIES[name]
    sig, xy, col, H, W = synthetic.kernel_inputs(H_LR, W_LR, SCALE, seed=g["seed"])
    rec = torch.cat([sig, xy, col], dim=1).contiguous().numpy()
    own = [tuple(v * W_LR for v in row_band(H_LR, r, world)) for r in range(world)]
    return rec, H, W, g["dmax"], g["cutoff"], g["cap"], own


def exchange_tau(cutoff, n_local, cap):
    """tau a BandExchange resolves `cutoff` to (0 = the adaptive default over own + halo records)"""
    return float(cutoff) if cutoff != 0.0 else default_tau(n_local + 2 * cap)
