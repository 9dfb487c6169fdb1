"""The host code of the masked family (gsasr_window_attn_masked / _masked_bf16 in csrc/splat_attn.hip: AttnMasked::fill, attn_args,
attn_forward, attn_backward) chooses between code paths by arithmetic on the shape, the pointers and the pitches.
tests/test_window_attention_masked_gpu.py and tests/test_window_attention_masked_bf16_gpu.py have the numerics; this file has one
row per value of every such decision, with their cases, yardsticks and bars: fp32 4 x e32 + 1e-6 x max-abs against the float64 torch
form, e32 the fp32 torch form's own error on the same input; bf16 the same bar with e the error of torch's own bf16 evaluation
(SDPA on bf16 q, k, v with bias + mask as the bf16 attn_mask).  Every check prints its ratio.  Shapes are (W, nq, nk, H, d, nW);
tiles are 16 rows; C = H d.  Every row runs for fp32 and bf16 unless it says otherwise.  tests/test_window_attention_masked_mutants.py
shows on the CPU that rows A and B can fail for the defect they name.

    A  the window walk: wslots = min(W, 256), so a workgroup of k_attn_bwd_q serves the windows slot, slot + 256 and must read the
       mask of the WINDOW (w % nW), not of the slot.  (258, 9, 9, 2, 5, nW 3) and (.., nW 258): 256 % nW != 0, the two windows of
       slot 0 have different masks (asserted), and (300, 9, 9, 2, 5, 3), where 44 windows are second in their slot (under bf16's
       bar two wrong windows of 258 move g_table by less than ten bars: the mutants file).  TAB 1; the first shape under TAB 2
       (5000 rows, index x 290) and TAB 0 (no table gradient: the bits of the TAB 1 run); window 256 alone with its own mask has
       its bits of the full call (fp32).
    B  mvec = nk % 4 == 0 and a 16-byte aligned mask, vec = the same of the index: two flags.  nk = 4, 20, 52, 148 (multiples of 4
       and not of 16: the 16-byte load's clamp min(j0, nk - 4) fires in a partial last tile) and (2, 20, 20, 2, 30, 2) (nq == nk, where
       a transposed read is possible), each with aligned | shifted index x aligned | shifted mask (shifted: contiguous, one element
       into a larger buffer; the mask's buffer is NaN around it).  The four combinations give the same bits.  (As in row D, results
       are pinned and not the load that was taken: where the hardware serves an unaligned 16-byte load, a wrong flag alone is silent.)
    C  six pitches: (3, 17, 33, 3, 30, 3) with q, k, v the column blocks [..., :C] of three buffers with rows of C + 1, C + 4, 2 C
       (padding NaN) and g_q, g_k, g_v written into rows of 2 C, C + 3, C + 8 (padding a sentinel that must survive): the bits of
       the dense call.  (3, 17, 17, 3, 30, 3): q, k, v packed with three dense gradients, and dense q, k, v with a packed gradient.
    D  the bf16 forward's load width (bf16 only, forward only): d = 8, C = 16, (2, 17, 33, 2, 8, 2) with pitch rows (16, 16, 16),
       (24, 24, 24) [16 bytes]; (18, 16, 16), (16, 20, 16), (16, 16, 18) [4 bytes]; (17, 16, 16), (16, 17, 16), (16, 16, 17)
       [2 bytes]; q two elements into its buffer [4 bytes], one element [2 bytes]; d = 6: (12, 12, 12) [4 bytes], (13, 12, 12)
       [2 bytes].  Padding is NaN.  A kernel cannot report the width it took: this row pins RESULTS (the bits of the dense call,
       which a load wider than the alignment or into the padding would change), not the choice.
    E  the launches by gradient, (2, 17, 33, 3, 30, 2): exactly one of g_q, g_k, g_v, g_table.
    F  TLDS = table_rows <= 4096: (2, 17, 33, 2, 30, 2) with 4097 rows -- k_attn_fwd<3, STATS 0 | 1, TLDS 0, MK>, its bf16 twin,
       k_attn_bwd_q<TAB 2, MK> and k_attn_bwd_kv<TLDS 0, MK>, each for both element types (their first launches by any test).
    G  STATS = false under each MAXT of this family, 3 | 4 | 9 | 16: nk = 33, 64, 65, 145 at (2, 23, nk, 2, 30, 2).

Wherever "the same bits" is asked, g_table is held to the bar instead: its sums are LDS or global atomics in no fixed order.

Recorded on an MI355X, the largest ratio to the bar per row (fp32 | bf16):
    A  0.28 (g_q) | 0.47 (g_table)
    B  0.46 (g_table) | 0.51 (g_k)
    C  0.33 (g_k) | 0.27 (g_k)
    D  -- | 0.15 (out)
    E  0.21 (g_v, g_table) | 0.19 (g_k)
    F  0.27 (g_v) | 0.11 (g_v)
    G  0.18 (out) | 0.07 (out)
Every bitwise comparison of rows A to G held.

The next change to that host code extends the row of the decision it touches."""
import functools

import pytest
import torch

import test_window_attention_masked_bf16_gpu as mbf
import test_window_attention_masked_gpu as m32
from gsasr_amd import _cabi
from gsasr_amd import attention as att
from test_window_attention import held

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
KINDS = ("fp32", "bf16")
DTYPE = {"fp32": torch.float32, "bf16": BF}
NAMES = m32.NAMES
NAN = float("nan")
WALK = (258, 9, 9, 2, 5, 3)
WALK_OWN = (258, 9, 9, 2, 5, 258)
WALK_MANY = (300, 9, 9, 2, 5, 3)
MASK_LOADS = [(2, 23, nk, 2, 30, 2) for nk in (4, 20, 52, 148)] + [(2, 20, 20, 2, 30, 2)]
PITCHES = (3, 17, 33, 3, 30, 3)
PACKED = (3, 17, 17, 3, 30, 3)
WIDTHS = (2, 17, 33, 2, 8, 2)
WIDTHS_D6 = (2, 17, 33, 2, 6, 2)
SUBSETS = (2, 17, 33, 3, 30, 2)
GLOBAL_TABLE = (2, 17, 33, 2, 30, 2)
NO_STATS = [(2, 23, nk, 2, 30, 2) for nk in (33, 64, 65, 145)]


def dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def yardsticks(kind, shape, rows=0, mul=1):
    """((q, k, v, table, index, mask, wgt), the float64 results, e per quantity) of make_case(shape) and its random mask -- once
    on the CPU, shared and left unchanged.  bf16: q, k, v and wgt rounded to bf16.  `rows`: a random table of that many rows
    in place of make_case's, with the index times `mul`"""
    if rows == 0 and kind == "fp32":
        return m32.yardsticks(shape)
    if rows == 0:
        (acts, table, index, mask, wgt), want, e = mbf.yardsticks(shape)
        return (*acts, table, index, mask, wgt), want, e
    q, k, v, _, index, mask, wgt = m32.make_case(shape)
    table = 0.5 * torch.randn(rows, shape[3], generator=torch.Generator().manual_seed(rows))
    index = index * mul
    assert int(index.max()) < rows
    if kind == "fp32":
        form = lambda *a, mask: att.window_attention_torch(*a, None, mask)        # noqa: E731
        want = m32.evaluate(form, q, k, v, table, index, mask, wgt, dtype=torch.float64)
        own = m32.evaluate(form, q, k, v, table, index, mask, wgt)
    else:
        q, k, v, wgt = (t.to(BF).float() for t in (q, k, v, wgt))
        form = lambda q, k, v, t, i, m: att.window_attention_torch(q, k, v, t, i, None, m)        # noqa: E731
        want = mbf.evaluate(form, (q, k, v), table, index, mask, wgt, act_dtype=torch.float64, table_dtype=torch.float64)
        own = mbf.evaluate(mbf.sdpa_masked, (q, k, v), table, index, mask, wgt, act_dtype=BF)
    return (q, k, v, table, index, mask, wgt), want, [float((a.double() - b).abs().max()) for a, b in zip(own, want)]


def run_op(kind, case, need=(True, True, True, True)):
    """(out, g_q, g_k, g_v, g_table) of window_attention(..., mask=) in `kind`, None where `need` is False"""
    q, k, v, table, index, mask, wgt = (t.detach() for t in case)       # (the fp32 yardsticks' evaluate marks its inputs as leaves)
    D, dt = dev(), DTYPE[kind]
    leaves = [t.to(D, dt).requires_grad_(n) for t, n in zip((q, k, v), need)] + [table.to(D).requires_grad_(need[3])]
    out = att.window_attention(*leaves, index.to(D), compute=kind, mask=mask.to(D))
    assert out.dtype == dt
    grads = iter(torch.autograd.grad(out, [t for t, n in zip(leaves, need) if n], wgt.to(D, dt)))
    return (out.detach(), *[next(grads) if n else None for n in need])


def forward_only(kind, case):
    q, k, v, table, index, mask, wgt = case
    D, dt = dev(), DTYPE[kind]
    with torch.no_grad():
        return att.window_attention(q.to(D, dt), k.to(D, dt), v.to(D, dt), table.to(D), index.to(D), compute=kind, mask=mask.to(D))


def hold(row, kind, what, got, want, e, names=NAMES):
    """every quantity of `got` that is not None under its bar; `row` and `kind` lead the printed line (the docstring's ratios)"""
    ok = True
    for name, g, w, err in zip(names, got, want, e):
        if g is not None:
            ok &= held(f"[{row} {kind}] {what} {name}", g, w, err)
    return ok


def same_bits(a, b, what, names=NAMES):
    for name, x, y in zip(names, a, b):
        assert x.shape == y.shape and torch.equal(x, y), f"{what}: {name} differs"


def unused_rows_are_zero(g_table, index):
    used = torch.zeros(g_table.shape[0], dtype=torch.bool)
    used[index.flatten()] = True
    assert bool((g_table.cpu()[~used] == 0).all()), "table rows no (i, j) uses must get exactly 0"
    return int(used.sum())


# ---- through the C ABI: the descriptor's pointers and pitches as the test sets them -------------------------------------
ABI_NAMES = ("out", "stats", "g_q", "g_k", "g_v", "g_table")


def on_device(kind, case):
    q, k, v, table, index, mask, wgt = (t.detach() for t in case)
    D, dt = dev(), DTYPE[kind]
    c = dict(q=q.to(D, dt).contiguous(), k=k.to(D, dt).contiguous(), v=v.to(D, dt).contiguous(), table=table.to(D).contiguous(),
             index=index.to(D, torch.int32).contiguous(), mask=mask.to(D).contiguous(), wgt=wgt.to(D, dt).contiguous())
    c["scale"] = float((q.shape[2] // table.shape[1]) ** -0.5)
    return c


def abi_forward(c, **over):
    c = dict(c, **over)
    return _cabi.window_attn_masked_forward(c["q"], c["k"], c["v"], c["table"], c["index"], c["mask"], c["scale"], want_stats=True)


def abi(c, grads=None, **over):
    """(out, stats, g_q, g_k, g_v, g_table) of gsasr_window_attn_masked_forward / _backward on the tensors of `c`, `over` in
    place of some; `grads`: the caller's own g_q, g_k, g_v"""
    c = dict(c, **over)
    out, stats = abi_forward(c)
    g = _cabi.window_attn_masked_backward(c["q"], c["k"], c["v"], c["table"], c["index"], c["mask"], c["scale"], out, stats, c["wgt"], grads=grads)
    return (out, stats, *g)


def hold_abi(row, kind, what, got, want, e):
    """(out, stats, g_q, g_k, g_v, g_table) of `abi` under the bars of (out, g_q, g_k, g_v, g_table)"""
    return hold(row, kind, what, [got[0], *got[2:]], want, e)


def at_offset(t, off, fill):
    """`t` contiguous, `off` elements into a larger buffer of `fill`"""
    buf = torch.full((t.numel() + 8,), fill, dtype=t.dtype, device=t.device)
    view = buf[off:off + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous()
    return view


def in_rows(t, pitch, fill=NAN):
    """`t` `[W,n,C]` as the column block [..., :C] of a buffer with rows of `pitch` elements, `fill` in the padding"""
    W, n, C = t.shape
    buf = torch.full((W, n, pitch), fill, dtype=t.dtype, device=t.device)
    buf[..., :C] = t
    return buf[..., :C]


SENTINEL = {torch.float32: (torch.int32, 0x5A5A5A5A), BF: (torch.int16, 0x5A5A)}


def sentinel_rows(like, pitch):
    """(a buffer `[W,n,pitch]` of like's dtype whose every element has the sentinel's bits, its column block [..., :C])"""
    W, n, C = like.shape
    buf = torch.empty(W, n, pitch, dtype=like.dtype, device=like.device)
    as_int, bits = SENTINEL[like.dtype]
    buf.view(as_int).fill_(bits)
    return buf, buf[..., :C]


def padding_kept(buf, C):
    as_int, bits = SENTINEL[buf.dtype]
    return bool((buf.view(as_int)[..., C:] == bits).all())


# ---- A: the walk with masks that differ inside a slot ----------------------------------------------------------------------
def differing_masks(shape, mask):
    nW = shape[5]
    assert shape[0] > 256 and 256 % nW != 0 and not torch.equal(mask[256 % nW], mask[0]), "slot 0's two windows need two masks"


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", [WALK, WALK_OWN, WALK_MANY], ids=m32.ident)
def test_a_walk_forward_and_gradients(shape, kind):
    case, want, e = yardsticks(kind, shape)
    differing_masks(shape, case[5])
    got = run_op(kind, case)
    assert hold("A", kind, f"{shape}", got, want, e)
    assert bool((got[4][-3:] == 0).all()), "table rows no (i, j) uses must get exactly 0"


@pytest.mark.parametrize("kind", KINDS)
def test_a_walk_on_the_atomic_path(kind):
    """TAB == 2: the walk with a 5000-row table, its gradient by global atomics in double"""
    case, want, e = yardsticks(kind, WALK, rows=5000, mul=290)
    differing_masks(WALK, case[5])
    got = run_op(kind, case)
    assert hold("A", kind, f"{WALK} T 5000", got, want, e)
    assert unused_rows_are_zero(got[4], case[4]) == 17


@pytest.mark.parametrize("kind", KINDS)
def test_a_walk_without_a_table_gradient(kind):
    """TAB == 0: g_q, g_k, g_v have the bits of the run that also binned the table's gradient"""
    case, want, e = yardsticks(kind, WALK)
    full = run_op(kind, case)
    some = run_op(kind, case, need=(True, True, True, False))
    assert some[4] is None
    same_bits(some[:4], full[:4], "without the table's gradient")
    assert hold("A", kind, f"{WALK} without the table's gradient", some, want, e)


def test_a_walked_window_is_independent_of_the_walk():
    """window 256 is the second of slot 0: with its own mask, alone, it has its bits of the full call"""
    case, _, _ = yardsticks("fp32", WALK)
    q, k, v, table, index, mask, wgt = case
    differing_masks(WALK, mask)
    full = run_op("fp32", case)
    m = 256 % WALK[5]
    alone = run_op("fp32", (q[256:257], k[256:257], v[256:257], table, index, mask[m:m + 1], wgt[256:257]))
    same_bits([t[256:257] for t in full[:4]], alone[:4], "window 256 alone")


# ---- B: the mask loads ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", MASK_LOADS, ids=m32.ident)
def test_b_mask_and_index_loads(shape, kind):
    case, want, e = yardsticks(kind, shape)
    c = on_device(kind, case)
    index = {"aligned": at_offset(c["index"], 4, 0), "shifted": at_offset(c["index"], 1, 0)}
    mask = {"aligned": at_offset(c["mask"], 4, NAN), "shifted": at_offset(c["mask"], 1, NAN)}
    for t in (index, mask):
        assert t["aligned"].data_ptr() % 16 == 0 and t["shifted"].data_ptr() % 16 != 0 and t["shifted"].data_ptr() % 4 == 0
    runs = {(i, m): abi(c, index=index[i], mask=mask[m]) for i in index for m in mask}
    first = runs["aligned", "aligned"]
    for key, run in runs.items():
        same_bits(run[:5], first[:5], f"{key[0]} index, {key[1]} mask against both aligned", ABI_NAMES)
    ok = hold_abi("B", kind, f"{shape} aligned", first, want, e)
    ok &= held(f"[B {kind}] {shape} shifted g_table", runs["shifted", "shifted"][5], want[4], e[4])
    assert bool((first[5][-3:] == 0).all()), "table rows no (i, j) uses must get exactly 0"
    if shape[1] == shape[2]:
        assert not torch.equal(case[5], case[5].transpose(1, 2))
    assert ok


# ---- C: the six pitches -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_c_six_pitches(kind):
    case, want, e = yardsticks(kind, PITCHES)
    c = on_device(kind, case)
    C = c["q"].shape[2]
    dense = abi(c)
    views = dict(q=in_rows(c["q"], C + 1), k=in_rows(c["k"], C + 4), v=in_rows(c["v"], 2 * C))
    bufs, grads = zip(sentinel_rows(c["q"], 2 * C), sentinel_rows(c["k"], C + 3), sentinel_rows(c["v"], C + 8))
    assert [t.stride(1) for t in (*views.values(), *grads)] == [C + 1, C + 4, 2 * C, 2 * C, C + 3, C + 8]
    got = abi(c, grads=grads, **views)
    assert all(a is b for a, b in zip(got[2:5], grads)), "the caller's tensors are written in place and returned"
    same_bits(got[:5], dense[:5], "six pitches against the dense call", ABI_NAMES)
    assert all(padding_kept(b, C) for b in bufs), "a gradient row's padding was written"
    ok = hold_abi("C", kind, f"{PITCHES} dense", dense, want, e)
    assert ok & held(f"[C {kind}] {PITCHES} six pitches g_table", got[5], want[4], e[4])


@pytest.mark.parametrize("kind", KINDS)
def test_c_packed_on_one_side_only(kind):
    case, want, e = yardsticks(kind, PACKED)
    c = on_device(kind, case)
    C = c["q"].shape[2]
    dense = abi(c)
    qkv = torch.cat([c["q"], c["k"], c["v"]], dim=-1)
    q, k, v = att._split_qkv(qkv)
    read_packed = abi(c, q=q, k=k, v=v)                    # g_q, g_k, g_v: three dense tensors
    assert all(g.is_contiguous() for g in read_packed[2:5])
    same_bits(read_packed[:5], dense[:5], "packed q, k, v with dense gradients", ABI_NAMES)
    whole, _ = sentinel_rows(qkv, 3 * C)
    write_packed = abi(c, grads=att._split_qkv(whole))      # dense q, k, v
    same_bits(write_packed[:5], dense[:5], "dense q, k, v with a packed gradient", ABI_NAMES)
    assert torch.equal(whole, torch.cat(dense[2:5], dim=-1))
    ok = hold_abi("C", kind, f"{PACKED} dense", dense, want, e)
    ok &= held(f"[C {kind}] {PACKED} packed q, k, v g_table", read_packed[5], want[4], e[4])
    assert ok & held(f"[C {kind}] {PACKED} packed gradient g_table", write_packed[5], want[4], e[4])


def test_c_the_callers_gradients_are_checked():
    c = on_device("fp32", yardsticks("fp32", PACKED)[0])
    out, stats = abi_forward(c)
    back = lambda **kw: _cabi.window_attn_masked_backward(c["q"], c["k"], c["v"], c["table"], c["index"], c["mask"], c["scale"],        # noqa: E731
                                                          out, stats, c["wgt"], **kw)
    g = [torch.empty_like(c[n]) for n in "qkv"]
    only_k = back(grads=(None, g[1], None), need=(True, True, True, False))
    assert only_k[0] is None and only_k[1] is g[1] and only_k[2] is None and only_k[3] is None
    assert torch.equal(g[1], back()[1])
    for bad in [(g[0], g[1]), (g[0], g[1][:, :5], g[2]), (g[0], g[1].double(), g[2]), (g[0], g[1].transpose(0, 1), g[2]), (g[0], g[1][..., ::2], g[2])]:
        with pytest.raises(RuntimeError):
            back(grads=bad)
    with pytest.raises(RuntimeError):
        back(grads=g, packed=True)


# ---- D: the bf16 forward's load width -----------------------------------------------------------------------------------
def widths_check(shape, variants):
    case, want, e = yardsticks("bf16", shape)
    c = on_device("bf16", case)
    dense = abi_forward(c)
    for what, over in variants(c):
        got = abi_forward(c, **over)
        same_bits(got, dense, f"{shape} {what}", ("out", "stats"))
    assert held(f"[D bf16] {shape} dense out", dense[0], want[0], e[0])


def test_d_load_width_by_pitch_and_base():
    def variants(c):
        for pitches in [(16, 16, 16), (24, 24, 24), (18, 16, 16), (16, 20, 16), (16, 16, 18), (17, 16, 16), (16, 17, 16), (16, 16, 17)]:
            views = {n: in_rows(c[n], p) for n, p in zip("qkv", pitches)}
            assert tuple(t.stride(1) for t in views.values()) == pitches and all(t.data_ptr() % 16 == 0 for t in views.values())
            yield f"pitches {pitches}", views
        for off, rem in ((2, 4), (1, 2)):
            q = at_offset(c["q"], off, NAN)
            assert q.data_ptr() % 16 == rem
            yield f"q {off} elements into its buffer", dict(q=q)
    assert WIDTHS[3] * WIDTHS[4] == 16
    widths_check(WIDTHS, variants)


def test_d_load_width_of_an_even_head_dimension():
    def variants(c):
        for pitches in [(12, 12, 12), (13, 12, 12)]:
            views = {n: in_rows(c[n], p) for n, p in zip("qkv", pitches)}
            assert tuple(t.stride(1) for t in views.values()) == pitches
            yield f"pitches {pitches}", views
    assert WIDTHS_D6[3] * WIDTHS_D6[4] == 12
    widths_check(WIDTHS_D6, variants)


# ---- E: gradient subsets ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("which", range(4), ids=NAMES[1:])
def test_e_one_gradient(which, kind):
    case, want, e = yardsticks(kind, SUBSETS)
    full = run_op(kind, case)
    need = tuple(i == which for i in range(4))
    got = run_op(kind, case, need=need)
    assert all((g is None) != n for g, n in zip(got[1:], need)), "a gradient for exactly the tensor that requires one"
    assert torch.equal(got[0], full[0])
    assert hold("E", kind, f"{SUBSETS} only {NAMES[1 + which]}", got, want, e)
    if which < 3:
        assert torch.equal(got[1 + which], full[1 + which]), f"{NAMES[1 + which]} alone differs from that of the run with all four"
    else:
        assert bool((got[4][-3:] == 0).all()), "table rows no (i, j) uses must get exactly 0"


# ---- F: a table that is not in LDS ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_f_table_past_the_lds_ceiling(kind):
    case, want, e = yardsticks(kind, GLOBAL_TABLE, rows=4097)
    got = run_op(kind, case)
    assert hold("F", kind, f"{GLOBAL_TABLE} T 4097", got, want, e)
    assert unused_rows_are_zero(got[4], case[4]) == 17 + 33 - 1 and bool((got[4][49:] == 0).all())
    assert torch.equal(forward_only(kind, case), got[0]), "the no_grad forward differs from the training forward"


# ---- G: the forward without the statistic ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", NO_STATS, ids=m32.ident)
def test_g_forward_without_the_statistic(shape, kind):
    case, want, e = yardsticks(kind, shape)
    plain = forward_only(kind, case)
    assert torch.equal(plain, run_op(kind, case)[0]), "the no_grad forward differs from the training forward"
    assert held(f"[G {kind}] {shape} no_grad out", plain, want[0], e[0])
