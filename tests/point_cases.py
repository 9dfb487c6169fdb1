"""Inputs that take the sampled-pixel and query kernels into coarse point-cells and crowded blocks (a plain module like gradbars
and edge_lattice: import it, `import point_cases`).

The kernels of gsasr_amd/csrc/splat_sampled.hip sort the points into point-cells of (1 << shx) x (1 << shy) px and hand a BLOCK of
(1 << max(shx, 4)) columns x (1 << max(shy, 4)) rows to one workgroup.  shx = shy = 3 up to 786 432 px; `pt_cells` transcribes how
they grow above that (`make_pt_view`).  It is a GUARD that a shape is in the regime its case names -- tests/test_point_cells.py pins
its value for every shape here, so a change of the rule asks for new shapes -- and it says which block a point falls in, for the
planting below and for failure messages.  It is never the expected value of a kernel output.

What a case holds:

  Gaussians   `gaussians`: sigma uniform in [0.8, 5] px (the first `n_large` in [40, 80] px: the large class of the unbounded op),
              rho uniform in [-0.9, 0.9] (kappa >= 0.19: every row is in scope of gradbars), centres uniform in [-1, 1]^2, colours
              uniform in [0, 1].
  blocks      `planted_blocks`: whole blocks at least one block away from every border, chosen from the seed.  `lay_lattice` moves
              Gaussians INTO each of them: one centre every 8 px (0.3 px off the pixel centre), sigma = 4 px, |rho| <= 0.5, colour
              >= 0.25.  Every position within half a pixel of a pixel of the block is then at most 4.8 px per axis from a centre, and
              that Gaussian alone is worth exp(-(u^2 + v^2 + 2 |rho| u v) / (2 (1 - rho^2))) * 0.25 >= exp(-2.9) * 0.25 = 0.014 there
              (u, v <= 1.2), inside every dmax box used here (>= 8 px).  So EVERY planted point has a value far above the bar of 1e-4,
              whichever walk of its block evaluates it: a walk that drops, repeats or misplaces a point shows.
  points      `points`: uniform ones (a random Gaussian's centre pixel + an offset in [-4, 4]^2, clamped; none inside a planted
              block), the planted counts PLANTED drawn with replacement from the pixels of one block each (24 = one walk of the
              forward, 25 = one point in the second, 28 / 29 the same for the position backward, 49 = a third walk of one point, 300),
              COPIES copies of one position in a block of its own, the corners of the closed domain, and N_INVALID points outside it.
              The list is shuffled, so invalid points and the members of a block lie anywhere in it.  Integer points carry Python's
              negative indices on three of every eight uniform points.  Fractional points (queries) add a uniform fraction in
              (-0.49, 0.49) per axis: the nearest pixel is the one drawn.
"""
import functools
from types import SimpleNamespace

import torch

# constants of gsasr_amd/csrc/splat_sampled.hip and splat_common.h (tests/test_point_cells.py reads them back from the source)
PT_CELLS = 12288
PT_MIN_SHIFT, PT_MAX_SHIFT = 3, 9
CELL_SHIFT = 4
RCAP_PX = 128
SAMPLE_BLOCK = 24
QGRAD_BLOCK = 28

PLANTED = (24, 25, 28, 29, 49, 300)
COPIES = 1000
N_INVALID = 700
N_UNIFORM = 3000
N_LARGE = 8
LATTICE_PX = 8
LATTICE_SIGMA = 4.0
LATTICE_OFF = 0.3
VALUE_FLOOR = 1e-3          # "has something to check": ten times the bar on a value

UNIFORM, BLOCK, COPY, CORNER, INVALID = range(5)

# (H, W) -> ((shx, shy), Gaussians)
SHAPES = {
    (1024, 1024): ((3, 4), 4096),
    (776, 1024): ((4, 3), 4096),
    (300, 9000): ((5, 3), 4096),
    (9000, 300): ((3, 5), 4096),
    (1500, 1500): ((4, 4), 4096),
    (2048, 2048): ((4, 5), 8192),
    (3000, 3000): ((5, 5), 8192),
    (4096, 4096): ((5, 6), 8192),
}

# batched canvases: name -> (sizes of the 64 samples, (shx, shy))
CANVASES = {
    "64x192": ([(192, 192)] * 64, (4, 4)),
    "64xragged": ([((256, 256), (200, 256), (256, 180), (177, 203))[b % 4] for b in range(64)], (5, 4)),
}
CANVAS_GAUSSIANS, CANVAS_LARGE = 256, 2
CANVAS_UNIFORM, CANVAS_PLANTED, CANVAS_INVALID, CANVAS_POINTS = 120, 30, 3, 160

# a canvas whose point-cells do not fit the table even at the coarsest cell a canvas allows (512 x 16 px)
TOO_LARGE = [(496, 3600)] * 64


def canvas_hw(sizes):
    """(rows, columns) of the canvas of `sizes`: one slot of whole 16-row tiles per sample"""
    slot = (max(h for h, _ in sizes) + 15) // 16 * 16
    return slot * len(sizes), max(w for _, w in sizes), slot


def pt_view(h, w, batched=False):
    """`make_pt_view`: (shx, shy, ncx, ncy) for an h x w image, or canvas when `batched`"""
    shx = shy = PT_MIN_SHIFT
    max_shy = CELL_SHIFT if batched else PT_MAX_SHIFT
    while True:
        ncx, ncy = ((w - 1) >> shx) + 1, ((h - 1) >> shy) + 1
        if ncx * ncy <= PT_CELLS or (shx >= PT_MAX_SHIFT and shy >= max_shy):
            return shx, shy, ncx, ncy
        if (ncy >= ncx or shx >= PT_MAX_SHIFT) and shy < max_shy:
            shy += 1
        else:
            shx += 1


def pt_cells(h, w, batched=False):
    return pt_view(h, w, batched)[:2]


def block_shifts(shifts):
    """(fsx, fsy): a workgroup's block is 1 << fsy rows by 1 << fsx columns"""
    return max(shifts[0], CELL_SHIFT), max(shifts[1], CELL_SHIFT)


def gaussians(H, W, n, n_large, seed):
    """(sigmas [n,3], coords [n,2], colors [n,3]) float32 in the kernel frame"""
    g = torch.Generator().manual_seed(seed)
    spx = 0.8 + 4.2 * torch.rand(n, 2, generator=g)
    spx[:n_large] = 40.0 + 40.0 * torch.rand(n_large, 2, generator=g)
    rho = 1.8 * torch.rand(n, 1, generator=g) - 0.9
    sig = torch.cat([spx[:, 0:1] / ((W - 1) / 2.0), spx[:, 1:2] / ((H - 1) / 2.0), rho], dim=1).float().contiguous()
    xy = (2.0 * torch.rand(n, 2, generator=g) - 1.0).float().contiguous()
    col = torch.rand(n, 3, generator=g).float().contiguous()
    return sig, xy, col


def planted_blocks(H, W, shifts, m, seed):
    """`m` distinct blocks (by, bx), whole and with at least one block between them and every border"""
    fsx, fsy = block_shifts(shifts)
    ny, nx = (H >> fsy) - 2, (W >> fsx) - 2          # by in 1 .. ny, bx in 1 .. nx
    assert ny >= 1 and nx >= 1 and ny * nx >= m, (H, W, shifts)
    k = torch.randperm(ny * nx, generator=torch.Generator().manual_seed(seed))[:m]
    return [(1 + int(v) // nx, 1 + int(v) % nx) for v in k]


def lay_lattice(H, W, shifts, sig, xy, col, blocks, first):
    """Gaussians first, first + 1, ... become the lattice of `blocks` (module docstring); returns new tensors and how many moved"""
    fsx, fsy = block_shifts(shifts)
    sig, xy, col = sig.clone(), xy.clone(), col.clone()
    j = first
    for by, bx in blocks:
        for r in range((by << fsy) + LATTICE_PX // 2, (by + 1) << fsy, LATTICE_PX):
            for c in range((bx << fsx) + LATTICE_PX // 2, (bx + 1) << fsx, LATTICE_PX):
                xy[j, 0] = 2.0 * (c + LATTICE_OFF) / (W - 1) - 1.0
                xy[j, 1] = 2.0 * (r + LATTICE_OFF) / (H - 1) - 1.0
                sig[j, 0] = LATTICE_SIGMA / ((W - 1) / 2.0)
                sig[j, 1] = LATTICE_SIGMA / ((H - 1) / 2.0)
                sig[j, 2] *= 5.0 / 9.0
                col[j] = 0.25 + 0.75 * col[j]
                j += 1
    assert j <= sig.shape[0]
    return sig, xy, col, j - first


def points(H, W, xy, S, seed, fractional, shifts=None, counts=PLANTED, copies=COPIES, n_invalid=N_INVALID, corners=True,
           anchors=None):
    """The points of one image (module docstring).  `shifts`: the point-cell shifts of what the image is part of (default: its
    own); `anchors`: the Gaussians a uniform point may be drawn around (default: all).  Returns a namespace:
      pts     [T,2] what the kernel is given: int64 (row, column), or float32 when `fractional`
      pos     [T,2] float32 positions for the float64 references: the wrapped index, or the position itself; (-1, -1) if invalid
      pix     [T,2] int64 nearest pixel, (-1, -1) if invalid;  valid [T] bool;  kind [T] (UNIFORM .. INVALID)
      member  [T] index into `blocks` of a planted point (the copies: the last block), else -1
      blocks  [(by, bx)] the planted blocks, counts + the block of the copies;  planted: the counts in the same order"""
    shifts = pt_cells(H, W) if shifts is None else shifts
    fsx, fsy = block_shifts(shifts)
    planted = tuple(counts) + ((copies,) if copies else ())
    blocks = planted_blocks(H, W, shifts, len(planted), seed)
    g = torch.Generator().manual_seed(seed + 1)
    anchors = torch.arange(xy.shape[0]) if anchors is None else anchors
    hw = torch.tensor([H - 1, W - 1])

    def in_blocks(rc):
        hit = torch.zeros(rc.shape[0], dtype=torch.bool)
        for by, bx in blocks:
            hit |= ((rc[:, 0] >> fsy) == by) & ((rc[:, 1] >> fsx) == bx)
        return hit

    # uniform: twice as many candidates as needed, the ones inside a planted block left out, the first S kept
    j = anchors[torch.randint(0, anchors.shape[0], (2 * S,), generator=g)]
    centre = torch.stack([(xy[j, 1].double() + 1.0) * 0.5 * (H - 1), (xy[j, 0].double() + 1.0) * 0.5 * (W - 1)], dim=1).round().long()
    uni = (centre + torch.randint(-4, 5, (2 * S, 2), generator=g)).clamp_(min=0).minimum(hw)
    uni = uni[~in_blocks(uni)][:S]
    assert uni.shape[0] == S
    pix, kind, member = [uni], [torch.full((S,), UNIFORM)], [torch.full((S,), -1)]
    for k, ((by, bx), m) in enumerate(zip(blocks, planted)):
        one = copies and k == len(planted) - 1
        r = (by << fsy) + torch.randint(0, 1 << fsy, (1 if one else m,), generator=g)
        c = (bx << fsx) + torch.randint(0, 1 << fsx, (1 if one else m,), generator=g)
        pix.append(torch.stack([r, c], dim=1).expand(m, 2) if one else torch.stack([r, c], dim=1))
        kind.append(torch.full((m,), COPY if one else BLOCK))
        member.append(torch.full((m,), k))
    if corners:
        pix.append(torch.tensor([[0, 0], [0, W - 1], [H - 1, 0], [H - 1, W - 1]]))
        kind.append(torch.full((4,), CORNER))
        member.append(torch.full((4,), -1))
    pix, kind, member = torch.cat(pix), torch.cat(kind), torch.cat(member)
    nv = pix.shape[0]
    if fractional:
        frac = 0.98 * torch.rand(nv, 2, generator=g) - 0.49
        if copies:
            frac[kind == COPY] = frac[kind == COPY][:1]          # copies of one POSITION
        frac[kind == CORNER] = 0.0
        pts = (pix.double() + frac.double()).float().clamp_(min=0.0).minimum(hw.float())
        assert bool((pts.round().long() == pix).all())
        pos = pts.clone()
        other = torch.stack([torch.rand(n_invalid, generator=g) * (H - 1), torch.rand(n_invalid, generator=g) * (W - 1)], dim=1).float()
        bad = other.clone()
        for i in range(n_invalid):      # -0.01, H - 1 + 0.01, W - 1 + 0.01, nan, inf in turn
            axis, v = ((0, -0.01), (0, H - 1 + 0.01), (1, W - 1 + 0.01), (0, float("nan")), (1, float("inf")))[i % 5]
            bad[i, axis] = v
    else:
        pts = pix.clone()
        wrap = torch.arange(nv) % 8
        un = kind == UNIFORM
        pts[un & ((wrap == 0) | (wrap == 2)), 0] -= H          # Python's negative indices: the same pixel
        pts[un & ((wrap == 1) | (wrap == 2)), 1] -= W
        pos = pix.float()
        bad = torch.stack([torch.randint(0, H, (n_invalid,), generator=g), torch.randint(0, W, (n_invalid,), generator=g)], dim=1)
        for i in range(n_invalid):      # row H, row -H - 1, column W, column -W - 1 in turn
            axis, v = ((0, H), (0, -H - 1), (1, W), (1, -W - 1))[i % 4]
            bad[i, axis] = v
    T = nv + n_invalid
    perm = torch.randperm(T, generator=g)
    minus = torch.full((n_invalid, 2), -1)
    return SimpleNamespace(
        pts=torch.cat([pts, bad])[perm].contiguous(), pos=torch.cat([pos, minus.float()])[perm].contiguous(),
        pix=torch.cat([pix, minus])[perm].contiguous(), valid=(torch.arange(T) < nv)[perm],
        kind=torch.cat([kind, torch.full((n_invalid,), INVALID)])[perm], member=torch.cat([member, minus[:, 0]])[perm],
        blocks=blocks, planted=planted, shifts=tuple(shifts), H=H, W=W)


def block_counts(P):
    """{(by, bx): valid points whose nearest pixel lies in that block}"""
    fsx, fsy = block_shifts(P.shifts)
    v = P.pix[P.valid]
    key, n = torch.unique((v[:, 0] >> fsy) * (1 << 20) + (v[:, 1] >> fsx), return_counts=True)
    return {(int(k) >> 20, int(k) & ((1 << 20) - 1)): int(c) for k, c in zip(key, n)}


def describe(P, i, counts=None):
    """point i for a failure message: its pixel, its block, the block's point count and the shifts"""
    fsx, fsy = block_shifts(P.shifts)
    if not bool(P.valid[i]):
        return f"point {i} (invalid: {P.pts[i].tolist()}), (shx, shy) = {P.shifts}"
    r, c = (int(v) for v in P.pix[i])
    blk = (r >> fsy, c >> fsx)
    counts = block_counts(P) if counts is None else counts
    return (f"point {i} at {P.pts[i].tolist()}, pixel ({r}, {c}), block {blk} of {1 << fsy} x {1 << fsx} px holding {counts[blk]} points, "
            f"(shx, shy) = {P.shifts}")


def bounded_dmax(H, W):
    """the dmax of the bounded runs: a box of 8 px along the shorter side"""
    return 16.0 / (min(H, W) - 1)


@functools.lru_cache(maxsize=None)
def single(H, W, fractional):
    """the case of one shape of SHAPES: Gaussians with the lattices laid, points, grad_out [3,T]"""
    shifts, n = SHAPES[(H, W)]
    assert pt_cells(H, W) == shifts, (H, W, pt_cells(H, W))
    seed = 7 * H + W
    sig, xy, col = gaussians(H, W, n, N_LARGE, seed)
    blocks = planted_blocks(H, W, shifts, len(PLANTED) + 1, seed + 50)
    sig, xy, col, moved = lay_lattice(H, W, shifts, sig, xy, col, blocks, N_LARGE)
    anchors = torch.cat([torch.arange(N_LARGE), torch.arange(N_LARGE + moved, n)])
    P = points(H, W, xy, N_UNIFORM, seed + 50, fractional, anchors=anchors)
    assert P.blocks == blocks
    gout = torch.rand(3, P.pts.shape[0], generator=torch.Generator().manual_seed(seed + 99)).contiguous()
    return SimpleNamespace(H=H, W=W, shifts=shifts, sig=sig, xy=xy, col=col, P=P, gout=gout, n_large=N_LARGE, lattice=moved)


@functools.lru_cache(maxsize=None)
def canvas(name, fractional):
    """the case of one canvas of CANVASES: per sample its Gaussians, points and grad_out; and everything stacked for the call"""
    sizes, shifts = CANVASES[name]
    ch, cw, slot = canvas_hw(sizes)
    assert pt_cells(ch, cw, batched=True) == shifts, (name, pt_cells(ch, cw, True))
    samples = []
    for b, (h, w) in enumerate(sizes):
        seed = 100000 + 97 * b + (1 if name == "64x192" else 2)
        sig, xy, col = gaussians(h, w, CANVAS_GAUSSIANS, CANVAS_LARGE, seed)
        blocks = planted_blocks(h, w, shifts, 2, seed + 50)
        sig, xy, col, moved = lay_lattice(h, w, shifts, sig, xy, col, blocks, CANVAS_LARGE)
        anchors = torch.cat([torch.arange(CANVAS_LARGE), torch.arange(CANVAS_LARGE + moved, CANVAS_GAUSSIANS)])
        copies = CANVAS_POINTS - CANVAS_UNIFORM - CANVAS_PLANTED - CANVAS_INVALID
        P = points(h, w, xy, CANVAS_UNIFORM, seed + 50, fractional, shifts=shifts, counts=(CANVAS_PLANTED,), copies=copies,
                   n_invalid=CANVAS_INVALID, corners=False, anchors=anchors)
        assert P.blocks == blocks and P.pts.shape[0] == CANVAS_POINTS
        gout = torch.rand(3, CANVAS_POINTS, generator=torch.Generator().manual_seed(seed + 99))
        samples.append(SimpleNamespace(H=h, W=w, sig=sig, xy=xy, col=col, P=P, gout=gout))
    return SimpleNamespace(
        name=name, sizes=sizes, shifts=shifts, slot=slot, samples=samples,
        sig=torch.cat([s.sig for s in samples]).contiguous(), xy=torch.cat([s.xy for s in samples]).contiguous(),
        col=torch.cat([s.col for s in samples]).contiguous(), pts=torch.stack([s.P.pts for s in samples]).contiguous(),
        gout=torch.stack([s.gout for s in samples]).contiguous(), dmax=16.0 / (min(min(h, w) for h, w in sizes) - 1))
