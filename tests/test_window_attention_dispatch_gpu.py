"""The host code of the window-attention kernels (gsasr_window_attn_forward / _backward and their _rope twins in
csrc/splat_attn.hip) chooses between code paths by arithmetic on the shape.  tests/test_window_attention_gpu.py and
tests/test_window_attention_rope_gpu.py have the numerics; this file has one row per value of every such decision, with their
cases, yardsticks and bar (4 x e32 + 1e-6 x max-abs against the float64 torch expression, e32 the fp32 torch expression's own
error on the same input).  Every check prints its ratio.  Shapes are (W, nq, nk, H, d); tiles are 16 rows.

    A  wslots = min(W, ATT_TAB_WG = 256): above it a workgroup of k_attn_bwd_q walks the windows slot, slot + 256, ... and
       re-stages K and V between two barriers.  W = 257 (slot 0 two windows), 260, 300, 513 (slot 0 three), with 1 / 2 / 5 / 9
       query tiles (the 4-wave deal with unequal trips around the walk's barriers, and the 3-wave one); the walk under TAB = 1
       (partial columns), TAB = 2 (5000 rows: global atomics) and TAB = 0 (no table gradient).
    B  vec = nk % 4 == 0 and a 16-byte aligned index.  nk = 4, 20, 52, 148 are multiples of 4 and not of 16, so the last key
       tile is partial and the 16-byte load's clamp min(j0, nk - 4) fires; the same nk with an index one element into its
       buffer take the scalar loads.
    C  MAXT of k_attn_fwd by nt = ceil(nk / 16): 3 (nk = 33, 48), 9 (49, 137), 16 (145, 150), each with STATS false and
       true; attn_waves(n) = 3 when the tile count divides by 3 and not by 4, else 4: 5, 6 and 7 tiles for nq (forward,
       k_attn_bwd_q) and for nk (k_attn_bwd_kv), 3 / 4 / 9 / 10 tiles for nk.
    D  the columns' split c16 < d and c16 + 16 < d: d = 15, 16, 17 (rotary: 14, 16, 18).
    E  the launches by gradient: k_attn_bwd_q with a null g_q (table only), without a table gradient (TAB = 0);
       k_attn_bwd_kv with only g_k or only g_v.
    F  TLDS = table_rows <= ATT_TAB_LDS = 4096: 4096 rows with nk = 256 is the largest dynamic-LDS request of the library
       (106 496 bytes in k_attn_bwd_q), 4097 the first table on the atomic path.
    G  achunk = max(8, ceil(W / 64)) windows per slice of k_attn_angle_grad: W = 600 (chunk 10, 60 slices) and 520 (chunk 9,
       58 slices, the last of 7 windows).

The next change to that host code extends the row of the decision it touches."""
import pytest
import torch

import test_window_attention_gpu as biased
import test_window_attention_rope_gpu as rope
from gsasr_amd import _cabi
from gsasr_amd import attention as att
from test_window_attention import held

pytestmark = pytest.mark.gpu
WALK = (257, 9, 9, 2, 5)
SUBSETS = (2, 17, 33, 3, 30)


def ident(shape):
    return "x".join(map(str, shape))


def run_biased(case, need=(True, True, True, True), device=None):
    """(out, g_q, g_k, g_v, g_table) of the biased op for `case` = (q, k, v, table, index, wgt), None where `need` is False"""
    q, k, v, table, index, wgt = case
    device = biased.dev() if device is None else device
    idx = index.to(device)
    # rope.evaluate is the one of the two evaluate()s with a `need`: it only asks for four leaves, so the table rides in its
    # `angles` slot and the closure supplies the index
    return rope.evaluate(lambda *a: att.window_attention(*a, idx), q, k, v, table, wgt, device=device, need=need)


def custom_yardsticks(case):
    """(float64 results, e32 per quantity) of a case whose table and index are not make_case's"""
    want = biased.evaluate(att.window_attention_torch, *case, dtype=torch.float64)
    f32 = biased.evaluate(att.window_attention_torch, *case)
    return want, [float((a.double() - b).abs().max()) for a, b in zip(f32, want)]


def hold_all(what, got, want, e32, names=biased.NAMES):
    ok = True
    for name, g, w, e in zip(names, got, want, e32):
        ok &= held(f"{what} {name}", g, w, e)
    return ok


def same_bits(a, b, what):
    for name, x, y in zip(biased.NAMES, a, b):
        assert torch.equal(x, y), f"{what}: {name} differs"


# ---- A: the window walk of k_attn_bwd_q ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [WALK, (513, 17, 33, 3, 30), (260, 144, 144, 1, 30), (300, 70, 20, 1, 6)], ids=ident)
def test_a_walk_forward_and_gradients(shape):
    biased.check_case(shape)


def test_a_walk_on_the_atomic_path():
    """TAB == 2: the walk with a 5000-row table, its gradient by global atomics.  A row's sum has 257 x 9 terms in no fixed
    order: added in fp32 it was 0.68 ... 1.80 of the bar from run to run, added in double and rounded once 0.228 every time"""
    q, k, v, _, index, wgt = biased.make_case(WALK)
    table = 0.5 * torch.randn(5000, 2, generator=torch.Generator().manual_seed(1))
    case = (q, k, v, table, index * 290, wgt)
    want, e32 = custom_yardsticks(case)
    got = biased.evaluate(att.window_attention, *case, device=biased.dev())
    assert hold_all(f"{WALK} T 5000", got, want, e32)
    used = torch.zeros(5000, dtype=torch.bool)
    used[case[4].flatten()] = True
    assert int(used.sum()) == 17 and bool((got[4].cpu()[~used] == 0).all()), "table rows no (i, j) uses must get exactly 0"


def test_a_walk_without_a_table_gradient():
    """TAB == 0: g_q, g_k, g_v have the bits of the run that also binned the table's gradient"""
    case, want, e32 = biased.yardsticks(WALK)
    full = run_biased(case)
    some = run_biased(case, need=(True, True, True, False))
    assert some[4] is None
    same_bits(some[:4], full[:4], "without the table's gradient")
    assert hold_all(f"{WALK} without the table's gradient", some[:4], want, e32)


def test_a_walked_window_is_independent_of_the_walk():
    """window 256 is the second of slot 0: its results are bitwise those of a call on that window alone"""
    case, want, e32 = biased.yardsticks(WALK)
    q, k, v, table, index, wgt = case
    full = run_biased(case)
    one = (q[256:257], k[256:257], v[256:257], table, index, wgt[256:257])
    alone = run_biased(one)
    same_bits([t[256:257] for t in full[:4]], alone[:4], "window 256 alone")
    want, e32 = custom_yardsticks(one)      # (that window's own e32, not the largest of the 257)
    assert hold_all(f"{WALK} window 256 alone", alone[:4], want, e32)


def test_a_walk_gives_the_same_bits_twice():
    shape = (513, 17, 33, 3, 30)
    case, want, e32 = biased.yardsticks(shape)
    a, b = (run_biased(case) for _ in range(2))
    same_bits(a[:4], b[:4], "two runs at W = 513")
    assert hold_all(f"{shape} second run", b, want, e32)      # (the same wrong bits twice would not do)


# ---- B: the index loads -----------------------------------------------------------------------------------------------
INDEX_SHAPES = [(2, 23, nk, 2, 30) for nk in (4, 20, 52, 148)]


@pytest.mark.parametrize("shape", INDEX_SHAPES, ids=ident)
def test_b_vector_index_load(shape):
    biased.check_case(shape)


def through_the_abi(case, index):
    """(out, stats, g_q, g_k, g_v, g_table) of gsasr_window_attn_forward / _backward with this int32 `index` on the device"""
    d = biased.dev()
    q, k, v, table, wgt = (t.to(d).contiguous() for t in (case[0], case[1], case[2], case[3], case[5]))
    scale = float((q.shape[2] // table.shape[1]) ** -0.5)
    out, stats = _cabi.window_attn_forward(q, k, v, table, index, scale, want_stats=True)
    return (out, stats, *_cabi.window_attn_backward(q, k, v, table, index, scale, out, stats, wgt))


@pytest.mark.parametrize("shape", INDEX_SHAPES, ids=ident)
def test_b_scalar_index_load_of_a_misaligned_index(shape):
    case, want, e32 = biased.yardsticks(shape)
    W, nq, nk, H, d = shape
    index = case[4].to(device=biased.dev(), dtype=torch.int32).contiguous()
    buf = torch.zeros(nq * nk + 8, dtype=torch.int32, device=biased.dev())
    shifted = buf[1:1 + nq * nk].view(nq, nk)
    shifted.copy_(index)
    assert index.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 != 0 and shifted.data_ptr() % 4 == 0 and shifted.is_contiguous()
    vec = through_the_abi(case, index)
    scalar = through_the_abi(case, shifted)
    picked = [0, 2, 3, 4, 5]        # (all but the statistic)
    ok = hold_all(f"{shape} scalar index", [scalar[i] for i in picked], want, e32)
    ok &= held(f"{shape} vector index through the ABI g_table", vec[5], want[4], e32[4])
    assert bool((scalar[5][-3:] == 0).all()), "table rows no (i, j) uses must get exactly 0"
    for name, a, b in zip(("out", "stats", "g_q", "g_k", "g_v"), vec, scalar):
        assert torch.equal(a, b), f"{name}: the 16-byte and the scalar index loads differ"
    assert ok


# ---- C: tile counts and the waves' deal ------------------------------------------------------------------------------
TILES = [(2, 23, 48, 2, 30), (2, 23, 49, 2, 30), (2, 23, 137, 2, 30), (2, 23, 145, 2, 30),
         (2, 70, 90, 2, 30), (2, 90, 100, 2, 30), (2, 100, 70, 2, 30)]


@pytest.mark.parametrize("shape", TILES, ids=ident)
def test_c_tiles_biased(shape):
    biased.check_case(shape)


@pytest.mark.parametrize("shape", TILES, ids=ident)
def test_c_tiles_rope(shape):
    rope.check_case(shape)


@pytest.mark.parametrize("nk", [33, 137, 150])
def test_c_forward_without_the_statistic(nk):
    """STATS false against true under every MAXT: the no_grad forward has the training forward's bits, and those are right"""
    shape, d = (2, 23, nk, 2, 30), biased.dev()
    (q, k, v, table, index, wgt), want, e32 = biased.yardsticks(shape)
    with torch.no_grad():
        plain = att.window_attention(q.to(d), k.to(d), v.to(d), table.to(d), index.to(d))
    assert torch.equal(plain, run_biased((q, k, v, table, index, wgt))[0])
    ok = held(f"{shape} no_grad out", plain, want[0], e32[0])
    (q, k, v, angles, wgt), want, e32 = rope.yardsticks(shape)
    with torch.no_grad():
        plain = att.window_attention_rope(q.to(d), k.to(d), v.to(d), angles.to(d))
    assert torch.equal(plain, rope.evaluate(att.window_attention_rope, q, k, v, angles, wgt, device=d)[0])
    assert ok & held(f"rope {shape} no_grad out", plain, want[0], e32[0])


# ---- D: the head dimension around 16 ---------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [15, 16, 17])
def test_d_head_dimension_biased(d):
    biased.check_case((2, 20, 20, 2, d))


@pytest.mark.parametrize("d", [14, 16, 18])
def test_d_head_dimension_rope(d):
    rope.check_case((2, 20, 20, 2, d))


# ---- E: gradient subsets -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", range(4), ids=biased.NAMES[1:])
def test_e_one_gradient_biased(which):
    case, want, e32 = biased.yardsticks(SUBSETS)
    full = run_biased(case)
    need = tuple(i == which for i in range(4))
    got = run_biased(case, need=need)
    assert all((g is None) != n for g, n in zip(got[1:], need)), "a gradient for exactly the tensor that requires one"
    assert torch.equal(got[0], full[0])
    name = biased.NAMES[1 + which]
    assert held(f"{SUBSETS} only {name}", got[1 + which], want[1 + which], e32[1 + which])
    if which < 3:
        assert torch.equal(got[1 + which], full[1 + which]), f"{name} alone differs from {name} of the run with all four"
    else:
        assert bool((got[4][-3:] == 0).all()), "table rows no (i, j) uses must get exactly 0"


@pytest.mark.parametrize("which", [1, 2], ids=["g_k", "g_v"])
def test_e_one_gradient_rope(which):
    (q, k, v, angles, wgt), want, e32 = rope.yardsticks(SUBSETS)
    d = biased.dev()
    full = rope.evaluate(att.window_attention_rope, q, k, v, angles, wgt, device=d)
    need = tuple(i == which for i in range(4))
    got = rope.evaluate(att.window_attention_rope, q, k, v, angles, wgt, device=d, need=need)
    assert all((g is None) != n for g, n in zip(got[1:], need)), "a gradient for exactly the tensor that requires one"
    assert torch.equal(got[0], full[0]) and torch.equal(got[1 + which], full[1 + which])
    assert held(f"rope {SUBSETS} only {rope.NAMES[1 + which]}", got[1 + which], want[1 + which], e32[1 + which])


# ---- F: the largest table binned in LDS, and the first that is not --------------------------------------------------
@pytest.mark.parametrize("rows", [4096, 4097])
def test_f_table_rows_at_the_lds_ceiling(rows):
    shape = (1, 256, 256, 1, 32)
    q, k, v, _, index, wgt = biased.make_case(shape)
    table = 0.5 * torch.randn(rows, 1, generator=torch.Generator().manual_seed(rows))
    case = (q, k, v, table, index, wgt)
    assert int(index.min()) == 0 and int(index.max()) == 510
    want, e32 = custom_yardsticks(case)
    got = biased.evaluate(att.window_attention, *case, device=biased.dev())
    assert hold_all(f"{shape} T {rows}", got, want, e32)
    assert bool((got[4][511:] == 0).all()) and bool((got[4][:511] != 0).all()), "table rows no (i, j) uses must get exactly 0"


# ---- G: the angle gradient's slices ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(600, 5, 7, 1, 4), (520, 5, 7, 1, 4)], ids=ident)
def test_g_angle_slices(shape):
    case, got, want, e32 = rope.check_case(shape)
    assert held(f"rope {shape} g_angles rows past 5", got[4][:, 5:], want[4][:, 5:], e32[4])
    again = rope.evaluate(att.window_attention_rope, *case, device=biased.dev())
    assert torch.equal(again[4], got[4]) and torch.equal(again[0], got[0])
    case, got, want, e32 = rope.check_case(shape, "extra rows")
    assert got[4].shape[1] == 10 and bool((got[4][:, 7:] == 0).all()) and bool((got[4][:, :7] != 0).any())
