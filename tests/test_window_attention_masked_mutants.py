"""Why rows A and B of tests/test_window_attention_masked_dispatch_gpu.py can fail for the defect they name -- on the CPU, without
a kernel: the float64 torch form against deliberately wrong variants of itself, at those rows' shapes (W, nq, nk, H, d, nW) and
with their cases.  A row is vacuous for a defect if the defect moves a quantity the row checks by less than the row's bar, so every
mutant must move EVERY such quantity (out, g_q, g_k, g_v, g_table) by at least 10 bars (4 x e + 1e-6 x max-abs, e the error of
torch's own fp32 / bf16 evaluation; the factor is a condition on the shape, not a measurement; where a shape misses it the shape
changes, not the factor).  Under fp32's bar every shape passes by 5e4 or more.  bf16's bar is some 1e4 times as high, and at 258
windows the slot mutant has only the windows 256 and 257 wrong: of the table's gradient, a sum over all 258 whose bf16 error grows
with them, that is 8.2 (nW 3) and 8.7 (nW 258) bars, and 9.3 of g_q (nW 3) -- seen, but not by ten.  So row A also runs
(300, 9, 9, 2, 5, 3), where 44 windows are wrong, and bf16's condition is asserted there.

    the slot's mask   window w reads mask[(w % 256) % nW], as a k_attn_bwd_q that indexed the mask by its workgroup's slot would
                      (row A).  At (280, 9, 9, 6, 30, nW 4), the shape that stood for "the masks of a slot's windows differ",
                      256 % 4 == 0 and this mutant IS the torch form: every quantity moves by exactly 0 (asserted: the record
                      of why row A has 256 % nW != 0).
    transposed        mask[m][j][i] for mask[m][i][j], as a k_attn_bwd_kv (the key is on the lane there) with query and key
                      swapped would read (row B's nq == nk shape).
    clamped tail      the row's last four entries all mask[.., nk - 4], as a scalar load clamped to nk - 4 (the 16-byte load's
                      start) instead of nk - 1 would read in the partial last tile (row B, nk = 20).

(Adding k's mask before the bias instead of after it is rounding only and no mutant.)"""
import functools

import pytest
import torch

import test_window_attention_masked_bf16_gpu as mbf
import test_window_attention_masked_dispatch_gpu as rows
import test_window_attention_masked_gpu as m32
from gsasr_amd import attention as att
from test_window_attention import bar

NAMES = m32.NAMES
WALK, WALK_OWN, WALK_MANY = rows.WALK, rows.WALK_OWN, rows.WALK_MANY
OLD_WALK = (280, 9, 9, 6, 30, 4)
SQUARE = (2, 20, 20, 2, 30, 2)
PARTIAL = (2, 23, 20, 2, 30, 2)
assert (WALK, WALK_OWN, WALK_MANY) == ((258, 9, 9, 2, 5, 3), (258, 9, 9, 2, 5, 258), (300, 9, 9, 2, 5, 3))
assert SQUARE in rows.MASK_LOADS and PARTIAL in rows.MASK_LOADS


def slot_mask(mask, W):
    """[W, nq, nk]: window w with the mask of its slot"""
    return mask[(torch.arange(W) % 256) % mask.shape[0]]


def transposed(mask, W):
    return mask.transpose(1, 2)[torch.arange(W) % mask.shape[0]]


def clamped_tail(mask, W):
    out = mask.clone()
    out[..., -4:] = mask[..., -4:-3]
    return out[torch.arange(W) % mask.shape[0]]


def f64(case, per_window):
    """the float64 torch form of `case` with one mask per window `[W, nq, nk]`"""
    q, k, v, table, index, _, wgt = case
    return m32.evaluate(lambda *a, mask: att.window_attention_torch(*a, None, mask), q, k, v, table, index, per_window, wgt, dtype=torch.float64)


@functools.lru_cache(maxsize=None)
def bars(kind, shape):
    """(the row's case, its bar per quantity) from the yardsticks of the row's own files"""
    if kind == "fp32":
        case, want, e = m32.yardsticks(shape)
    else:
        (acts, table, index, mask, wgt), want, e = mbf.yardsticks(shape)
        case = (*acts, table, index, mask, wgt)
    return case, [bar(err, float(w.abs().max())) for err, w in zip(e, want)]


def moved(case, mutant):
    W, mask = case[0].shape[0], case[5]
    right = f64(case, mask[torch.arange(W) % mask.shape[0]])
    wrong = f64(case, mutant(mask, W))
    return [float((a - b).abs().max()) for a, b in zip(right, wrong)]


def ratios(shape, mutant, kind):
    case, b = bars(kind, shape)
    move = moved(case, mutant)
    for name, m, limit in zip(NAMES, move, b):
        print(f"{mutant.__name__} {shape} {kind} {name}: moved {m:.3e}, bar {limit:.3e}, ratio {m / limit:.3g}")
    return [m / limit for m, limit in zip(move, b)]


MUTANTS = [(WALK, slot_mask), (WALK_OWN, slot_mask), (WALK_MANY, slot_mask), (SQUARE, transposed), (PARTIAL, clamped_tail)]
IDS = ["slot 258x3", "slot 258x258", "slot 300x3", "transposed", "clamped tail"]


@pytest.mark.parametrize("shape,mutant", MUTANTS, ids=IDS)
def test_a_mutant_moves_every_checked_quantity_by_ten_fp32_bars(shape, mutant):
    assert all(r >= 10 for r in ratios(shape, mutant, "fp32"))


@pytest.mark.parametrize("shape,mutant", MUTANTS[2:], ids=IDS[2:])
def test_a_mutant_moves_every_checked_quantity_by_ten_bf16_bars(shape, mutant):
    assert all(r >= 10 for r in ratios(shape, mutant, "bf16"))


@pytest.mark.parametrize("shape", [WALK, WALK_OWN], ids=IDS[:2])
def test_two_wrong_windows_of_258_under_the_bf16_bar(shape):
    """the ten-bar condition is asserted at WALK_MANY (the module's docstring says why); here only what needs no factor: more
    than 2 bars, past which a result within one bar of the mutant cannot be within one bar of the truth"""
    assert all(x > 2 for x in ratios(shape, slot_mask, "bf16"))


def test_the_slot_mutant_is_invisible_where_256_is_a_multiple_of_nW():
    assert OLD_WALK in m32.SLOTS and 256 % OLD_WALK[5] == 0
    case = m32.yardsticks(OLD_WALK)[0]
    assert moved(case, slot_mask) == [0.0] * 5
    # and the masks it would have confused do differ
    assert not torch.equal(case[5][0], case[5][1])
