"""The conditions the inputs of tests/point_cases.py must meet, checked on the CPU and on the float64 reference alone, so that
tests/test_point_cells_gpu.py cannot pass by having nothing to check.

The reference values are taken under the bounded op: every term is >= 0 (colours in [0, 1]), so the unbounded op's value at a
point is at least the bounded one's, and a floor that holds with the dmax box holds without it.
"""
import math
import os
import re

import numpy as np
import pytest
import torch

import gradbars
import point_cases as pc
from test_query_points_gpu import _eval64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = list(pc.SHAPES)
SHAPE_IDS = [f"{h}x{w}" for h, w in SHAPES]
KINDS = [False, True]
KIND_IDS = ["integer", "fractional"]


def test_constants_are_the_library_s():
    """the transcribed constants against the source they were read from"""
    src = open(os.path.join(ROOT, "gsasr_amd", "csrc", "splat_sampled.hip")).read()
    common = open(os.path.join(ROOT, "gsasr_amd", "csrc", "splat_common.h")).read()

    def const(text, name):
        m = re.search(r"constexpr int [^;]*\b" + name + r" = (\d+)", text)
        assert m, name
        return int(m.group(1))
    assert const(src, "PT_CELLS") == pc.PT_CELLS
    assert (const(src, "PT_MIN_SHIFT"), const(src, "PT_MAX_SHIFT")) == (pc.PT_MIN_SHIFT, pc.PT_MAX_SHIFT)
    assert const(src, "SAMPLE_BLOCK") == pc.SAMPLE_BLOCK and const(src, "QGRAD_BLOCK") == pc.QGRAD_BLOCK
    assert const(common, "CELL_SHIFT") == pc.CELL_SHIFT and const(common, "RCAP_PX") == pc.RCAP_PX
    # the planted counts sit on both sides of a walk's capacity in both point-stationary kernels
    for cap in (pc.SAMPLE_BLOCK, pc.QGRAD_BLOCK):
        assert cap in pc.PLANTED and cap + 1 in pc.PLANTED
    assert 2 * pc.SAMPLE_BLOCK + 1 in pc.PLANTED and max(pc.PLANTED) > 10 * pc.QGRAD_BLOCK


def test_every_shape_is_in_the_regime_it_names():
    assert pc.pt_cells(768, 1024) == (3, 3) and pc.pt_cells(1024, 768) == (3, 3)      # the largest size the suite had: still 8 x 8 px
    for (h, w), (shifts, _) in pc.SHAPES.items():
        shx, shy, ncx, ncy = pc.pt_view(h, w)
        assert (shx, shy) == shifts and ncx * ncy <= pc.PT_CELLS, (h, w, shx, shy)
    seen = {s for s, _ in pc.SHAPES.values()}
    assert len(seen) == len(pc.SHAPES)
    assert {x for x, _ in seen} == {3, 4, 5} and {y for _, y in seen} == {3, 4, 5, 6}
    for name, (sizes, shifts) in pc.CANVASES.items():
        ch, cw, slot = pc.canvas_hw(sizes)
        shx, shy, ncx, ncy = pc.pt_view(ch, cw, batched=True)
        assert (shx, shy) == shifts and ncx * ncy <= pc.PT_CELLS and slot % (1 << shy) == 0, name
    ch, cw, _ = pc.canvas_hw(pc.TOO_LARGE)
    shx, shy, ncx, ncy = pc.pt_view(ch, cw, batched=True)
    assert (shx, shy) == (pc.PT_MAX_SHIFT, pc.CELL_SHIFT) and ncx * ncy == 15872 > pc.PT_CELLS and ch <= 32767


def _check_points(P, H, W, fractional, counts, n_uniform, n_invalid):
    """what `points` promises, from its output alone"""
    fsx, fsy = pc.block_shifts(P.shifts)
    T = P.pts.shape[0]
    assert int((P.kind == pc.UNIFORM).sum()) == n_uniform and int((~P.valid).sum()) == n_invalid
    assert bool(((P.kind == pc.INVALID) == ~P.valid).all())
    # the invalid points are spread through the list: every eighth of it holds some (no run of them at the end)
    if n_invalid >= 64:
        per = [int((~P.valid[k * T // 8:(k + 1) * T // 8]).sum()) for k in range(8)]
        assert min(per) >= n_invalid // 16, per
    v = P.valid
    assert bool(((P.pix[v] >= 0).all())) and bool((P.pix[v, 0] < H).all()) and bool((P.pix[v, 1] < W).all())
    if fractional:
        assert P.pts.dtype == torch.float32
        p = P.pts
        inside = (p[:, 0] >= 0) & (p[:, 0] <= H - 1) & (p[:, 1] >= 0) & (p[:, 1] <= W - 1)      # (NaN fails every comparison)
        assert bool((inside == v).all())
        assert bool((p[v].round().long() == P.pix[v]).all())
        assert float((p[v] - P.pix[v].float()).abs().max()) < 0.4901
        bad = p[~v]
        if n_invalid >= 5:
            assert bool(torch.isnan(bad).any()) and bool(torch.isinf(bad).any()) and bool((bad < 0).any())
            assert bool((bad[:, 0] > H - 1).any()) and bool((bad[:, 1] > W - 1).any())
    else:
        assert not P.pts.dtype.is_floating_point
        r, c = P.pts[:, 0], P.pts[:, 1]
        wr, wc = torch.where(r < 0, r + H, r), torch.where(c < 0, c + W, c)
        inside = (wr >= 0) & (wr < H) & (wc >= 0) & (wc < W)
        assert bool((inside == v).all())
        assert bool((torch.stack([wr, wc], 1)[v] == P.pix[v]).all())
        if n_uniform >= 64:
            assert int(((r < 0) & v).sum()) >= n_uniform // 8 and int(((c < 0) & v).sum()) >= n_uniform // 8      # wrapping indices
        bad = P.pts[~v]
        if n_invalid >= 4:
            for axis, n in ((0, H), (1, W)):
                assert bool((bad[:, axis] == n).any()) and bool((bad[:, axis] == -n - 1).any())
    # every planted count is present in ONE block, exactly: no uniform point fell into it
    have = pc.block_counts(P)
    for k, (blk, m) in enumerate(zip(P.blocks, P.planted)):
        by, bx = blk
        assert 1 <= by and (by + 2) << fsy <= H and 1 <= bx and (bx + 2) << fsx <= W, blk
        assert have[blk] == m == int((P.member == k).sum()), (blk, m, have[blk])
        mine = P.pix[P.member == k]
        assert bool(((mine[:, 0] >> fsy) == by).all()) and bool(((mine[:, 1] >> fsx) == bx).all())
    assert list(P.planted[:len(counts)]) == list(counts)
    copy = P.pts[P.kind == pc.COPY]
    assert copy.shape[0] == P.planted[-1] and bool((copy == copy[0]).all())
    # where a block is two rows of point-cells (shy = 3), each planted block has points in both: a walk crosses from one to the other
    if P.shifts[1] == 3:
        for k in range(len(counts)):
            rows = set((P.pix[P.member == k][:, 0] >> 3).tolist())
            assert len(rows) == 2, (P.blocks[k], rows)


def _check_gaussians(sig, H, W, n_large, cutoffs):
    rho = sig[:, 2].double().numpy()
    assert float((1.0 - rho * rho).min()) >= gradbars.KAPPA_MIN
    assert float(gradbars.kappa_of(rho).min()) >= 0.19 - 1e-6
    # under dmax = None the wide Gaussians are the large class: half-extent sqrt(2 tau) sigma above RCAP_PX on some axis (here: both)
    from gsasr_amd import _cabi
    for cutoff in cutoffs:
        tau = _cabi.resolve_cutoff(cutoff, sig.shape[0])
        assert 16.0 <= tau <= 104.0
        ext = math.sqrt(2.0 * tau) * sig[:n_large, :2].double() * torch.tensor([(W - 1) / 2.0, (H - 1) / 2.0])
        assert float(ext.min()) > pc.RCAP_PX, (cutoff, tau, float(ext.min()))
    px = sig[n_large:, :2].double() * torch.tensor([(W - 1) / 2.0, (H - 1) / 2.0])
    assert 0.8 - 1e-4 <= float(px.min()) and float(px.max()) <= 5.0 + 1e-4


@pytest.mark.parametrize("fractional", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_single_image_case_has_something_to_check(shape, fractional):
    H, W = shape
    C = pc.single(H, W, fractional)
    P = C.P
    assert pc.pt_cells(H, W) == C.shifts == P.shifts
    _check_points(P, H, W, fractional, pc.PLANTED, pc.N_UNIFORM, pc.N_INVALID)
    corner = P.pix[P.kind == pc.CORNER].tolist()
    assert [H - 1, W - 1] in corner and [0, 0] in corner and [0, W - 1] in corner and [H - 1, 0] in corner
    _check_gaussians(C.sig, H, W, C.n_large, (0.0, 104.0) if shape == (1500, 1500) else (0.0,))
    want = _eval64(C.sig, C.xy, C.col, H, W, pc.bounded_dmax(H, W), P.pos)
    top = want.max(axis=0)
    valid = P.valid.numpy()
    assert (top[~valid] == 0).all()
    share = float((top[valid] > pc.VALUE_FLOOR).mean())
    planted = (P.member >= 0).numpy()
    print(f"{H}x{W} {'fractional' if fractional else 'integer'}: {int(valid.sum())} valid points, {share:.3f} of them above {pc.VALUE_FLOOR}; "
          f"smallest planted value {top[planted].min():.3e}")
    assert share >= 0.8
    assert top[planted].min() > pc.VALUE_FLOOR        # every planted point, whichever walk of its block takes it


@pytest.mark.parametrize("fractional", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("name", list(pc.CANVASES))
def test_canvas_case_has_something_to_check(name, fractional):
    C = pc.canvas(name, fractional)
    assert C.pts.shape == (64, pc.CANVAS_POINTS, 2) and C.sig.shape[0] == 64 * pc.CANVAS_GAUSSIANS
    assert C.slot % (1 << pc.block_shifts(C.shifts)[1]) == 0      # a sample's blocks are the canvas' blocks
    above = total = 0
    for s in C.samples:
        _check_points(s.P, s.H, s.W, fractional, (pc.CANVAS_PLANTED,), pc.CANVAS_UNIFORM, pc.CANVAS_INVALID)
        _check_gaussians(s.sig, s.H, s.W, pc.CANVAS_LARGE, ())
        top = _eval64(s.sig, s.xy, s.col, s.H, s.W, C.dmax, s.P.pos).max(axis=0)
        valid = s.P.valid.numpy()
        above += int((top[valid] > pc.VALUE_FLOOR).sum())
        total += int(valid.sum())
        assert top[(s.P.member >= 0).numpy()].min() > pc.VALUE_FLOOR
    # (the large class of a canvas: tau is resolved for all its Gaussians)
    from gsasr_amd import _cabi
    tau = _cabi.resolve_cutoff(0.0, C.sig.shape[0])
    assert math.sqrt(2.0 * tau) * 40.0 > pc.RCAP_PX
    print(f"{name}: {above} of {total} valid points above {pc.VALUE_FLOOR}")
    assert above >= 0.8 * total


def test_describe_names_pixel_block_count_and_shifts():
    C = pc.single(776, 1024, True)
    i = int(torch.nonzero(C.P.member == 5)[0])
    text = pc.describe(C.P, i)
    by, bx = C.P.blocks[5]
    assert f"block ({by}, {bx})" in text and "holding 300 points" in text and "(shx, shy) = (4, 3)" in text and "pixel (" in text
    j = int(torch.nonzero(~C.P.valid)[0])
    assert "invalid" in pc.describe(C.P, j)
