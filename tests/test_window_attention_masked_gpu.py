"""The masked family's kernels on the GPU (csrc/splat_attn.hip with MK behind gsasr_amd.window_attention(..., mask=) and
window_attention_qkv): forward and the four gradients against the float64 evaluation of the torch form, under the bar of
tests/test_window_attention.py (4 x e32 + 1e-6 x max-abs, e32 the fp32 torch form's own error on the same input).  Every check
prints its ratio.

Shapes are (W, nq, nk, H, d, nW).  The shipped one carries the real mask of a shifted Swin block (the golden's); the tails of
every tile, one mask broadcast over all windows, nW = W, the limits 255 / 256, both sides of every key-tile threshold between two
forward instantiations, and more than 256 windows per head with a table gradient, so that one workgroup of k_attn_bwd_q serves the
windows slot, slot + 256: 280 windows with nW = 4 (256 % 4 == 0: the two windows of a slot read the SAME mask) and 258 with nW = 3
(their masks differ; tests/test_window_attention_masked_dispatch_gpu.py row A has the rest of the walk).  Every shape runs with a
random ASYMMETRIC mask (3 randn): Swin's own masks are symmetric in (i, j) and cannot show a transposed read in k_attn_bwd_kv,
where the key is on the lane.  The index is relative over nq + nk - 1 rows of a table that has three more: unused rows must come
back exactly 0.

Recorded on an MI355X (largest ratio to the bar per quantity over all shapes, masks and variants): out 0.27, g_q 0.68, g_k 0.39,
g_v 0.39, g_table 0.57; through the switched modules 0.13-0.33.  "one key" (see one_key_bounds): g_q 1.1e-6 and g_table 3.1e-6
absolute against bounds of 9.8e-5 and 1.1e-2, g_k 6.7e-41."""
import copy
import functools

import pytest
import torch

from gsasr_amd import attention as att
from test_window_attention import held
from test_window_attention_masked import SWIN_CASES, golden_yardsticks, load_golden, run_case

pytestmark = pytest.mark.gpu
NAMES = ("out", "g_q", "g_k", "g_v", "g_table")
SHIPPED = [(8, 64, 64, 6, 30, 4)]
TAILS = [(2, 9, 9, 2, 5, 2), (6, 17, 33, 3, 30, 3), (2, 33, 17, 1, 32, 1), (2, 2, 2, 1, 1, 2)]
LIMITS = [(2, 255, 256, 2, 31, 2), (2, 256, 255, 2, 1, 1)]
SLOTS = [(280, 9, 9, 6, 30, 4), (258, 9, 9, 2, 5, 3)]
# the forward's instantiations by key tiles (3 | 4 | up to 9 | up to 16), both sides of every threshold; d = 8 and 32 with a packed
# pitch that is a multiple of 8 take the bf16 forward's 16-byte loads, d = 30 its 4-byte ones, an odd d (TAILS) the 2-byte ones
DISPATCH = [(2, 48, 48, 2, 8, 2), (2, 49, 49, 2, 32, 2), (2, 65, 65, 3, 30, 1), (2, 144, 144, 2, 32, 2), (2, 145, 145, 1, 30, 2)]
SWIN_PATTERN = SHIPPED + [(6, 17, 33, 3, 30, 3)] + SLOTS
NUMERIC = (2, 40, 50, 2, 30, 2)


def dev():
    return torch.device("cuda:0")


def ident(s):
    return "x".join(map(str, s))


def pattern_mask(nW, nq, nk, g):
    """0 / -100 by random group labels, as a shifted window's regions; every row keeps a 0 (key i % nk)"""
    lq, lk = torch.randint(0, 3, (nW, nq), generator=g), torch.randint(0, 3, (nW, nk), generator=g)
    mask = torch.where(lq[:, :, None] == lk[:, None, :], 0.0, -100.0)
    mask[:, torch.arange(nq), torch.arange(nq) % nk] = 0.0
    return mask


def make_case(shape, variant="random"):
    """(q, k, v, table, index, mask, wgt)"""
    W, nq, nk, H, d, nW = shape
    g = torch.Generator().manual_seed(17 * sum(shape) + len(variant))
    q, k, v = torch.randn(W, nq, H * d, generator=g), torch.randn(W, nk, H * d, generator=g), torch.randn(W, nk, H * d, generator=g)
    T = nq + nk - 1 + 3
    table = 0.5 * torch.randn(T, H, generator=g)
    index = torch.arange(nq)[:, None] - torch.arange(nk)[None, :] + nk - 1
    wgt = torch.randn(W, nq, H * d, generator=g)
    mask = 3 * torch.randn(nW, nq, nk, generator=g)
    if variant == "swin":
        mask = load_golden("swin_8_shift")[2] if shape == SHIPPED[0] else pattern_mask(nW, nq, nk, g)
    elif variant == "saturated":
        q = q * 30
    elif variant == "table 50":         # against a -100 mask: a masked score can exceed an unmasked one
        table = torch.where(torch.rand(T, H, generator=g) < 0.5, -50.0, 50.0)
        mask = pattern_mask(nW, nq, nk, g)
    elif variant == "one key":          # -100 everywhere except one key per row
        mask = torch.full((nW, nq, nk), -100.0)
        mask.scatter_(2, torch.randint(0, nk, (nW, nq, 1), generator=g), 0.0)
    return q, k, v, table, index, mask, wgt


def evaluate(fn, q, k, v, table, index, mask, wgt, device="cpu", dtype=torch.float32):
    a = [t.to(device=device, dtype=dtype).requires_grad_(True) for t in (q, k, v, table)]
    out = fn(*a, index.to(device), mask=None if mask is None else mask.to(device=device, dtype=dtype))
    return (out.detach(), *torch.autograd.grad((out * wgt.to(device=device, dtype=dtype)).sum(), a))


def evaluate_qkv(q, k, v, table, index, mask, wgt, device):
    """the packed op on cat(q, k, v) -> (out, the [W,n,3C] gradient, g_table)"""
    qkv = torch.cat([q, k, v], dim=-1).to(device).requires_grad_(True)
    tab = table.to(device).requires_grad_(True)
    out = att.window_attention_qkv(qkv, tab, index.to(device), mask=None if mask is None else mask.to(device))
    return (out.detach(), *torch.autograd.grad((out * wgt.to(device)).sum(), [qkv, tab]))


@functools.lru_cache(maxsize=None)
def yardsticks(shape, variant="random"):
    """(the case, its float64 results, e32 per quantity) -- computed once on the CPU and shared"""
    case = make_case(shape, variant)
    torch_form = lambda *a, mask: att.window_attention_torch(*a, None, mask)        # noqa: E731
    want = evaluate(torch_form, *case, dtype=torch.float64)
    f32 = evaluate(torch_form, *case)
    return case, want, [float((a.double() - b).abs().max()) for a, b in zip(f32, want)]


def one_key_bounds(q, k, v, mask, wgt, shape):
    """The "one key" variant: P is one-hot, so dS = P (dP - delta) is exactly 0 at the row's key in exact arithmetic and g_q, g_k,
    g_table are of the order of exp(-100).  torch's softmax backward forms P dP - P sum(P dP) and cancels exactly (e32 is 1e-44);
    the kernels form delta = sum_c dO_c O_c and dP = sum_c dO_c v_c as two fp32 sums of d products in different orders, each
    within d 2^-24 sum_c |dO_c v_c| of the exact value.  So |dS| <= E = 2 d 2^-24 max sum_c |dO_c| |v_c| (the row's key's v), and
    g_q <= scale E max|k|, g_k <= scale E max|q| times the rows that chose one key, g_table <= E times the W nq pairs that can
    share a table row -> absolute bounds for these three quantities from the number format, on top of the bar"""
    W, nq, nk, H, d, nW = shape
    key = mask.argmax(-1)                                                # [nW, nq]
    vsel = torch.stack([v[w][key[w % nW]] for w in range(W)])            # [W, nq, H * d]
    E = 2 * d * 2.0 ** -24 * float((wgt.detach().abs() * vsel.detach().abs()).view(W, nq, H, d).sum(-1).max())
    rows_per_key = max(int(torch.bincount(key[m], minlength=nk).max()) for m in range(nW))
    scale = d ** -0.5
    return {"g_q": scale * E * float(k.abs().max()), "g_k": scale * E * rows_per_key * float(q.abs().max()), "g_table": E * W * nq}


def held_or_bounded(what, got, want, e, bound):
    """`held`, with an absolute `bound` (one_key_bounds) added to the bar when there is one"""
    if bound is None:
        return held(what, got, want, e)
    err = float((got.detach().cpu().double() - want).abs().max())
    print(f"{what}: err {err:.3e}, e32 {e:.3e}, format bound {bound:.3e}, ratio {err / bound:.3f}")
    return err <= bound + 4.0 * e + 1e-6 * float(want.abs().max())


def check_case(shape, variant="random"):
    case, want, e32 = yardsticks(shape, variant)
    got = evaluate(att.window_attention, *case, device=dev())
    bounds = one_key_bounds(case[0], case[1], case[2], case[5], case[6], shape) if variant == "one key" else {}
    ok = True
    for name, g, w, e in zip(NAMES, got, want, e32):
        ok &= held_or_bounded(f"masked {shape} {variant} {name}", g, w, e, bounds.get(name))
    assert bool((got[4][-3:] == 0).all()), "table rows no (i, j) uses must get exactly 0"
    if shape[1] == shape[2]:        # the packed form: the same bits as the split form on contiguous copies
        out, g_qkv, g_table = evaluate_qkv(*case, device=dev())
        assert g_qkv.shape == (shape[0], shape[1], 3 * shape[3] * shape[4])
        assert torch.equal(out, got[0]) and torch.equal(g_qkv, torch.cat(got[1:4], dim=-1))
        ok &= held_or_bounded(f"masked {shape} {variant} packed g_table", g_table, want[4], e32[4], bounds.get("g_table"))
        assert bool((g_table[-3:] == 0).all())
    assert ok
    return case, got


@pytest.mark.parametrize("shape", SHIPPED + TAILS + LIMITS + SLOTS + DISPATCH, ids=ident)
def test_forward_and_gradients_with_an_asymmetric_mask(shape):
    case, _ = check_case(shape)
    assert not torch.equal(case[5], case[5].transpose(1, 2)) if shape[1] == shape[2] and shape[1] > 1 else True


@pytest.mark.parametrize("shape", SWIN_PATTERN, ids=ident)
def test_forward_and_gradients_with_a_swin_mask(shape):
    case, _ = check_case(shape, "swin")
    assert sorted(case[5].unique().tolist()) == [-100.0, 0.0] and bool((case[5].max(-1).values == 0).all())


@pytest.mark.parametrize("variant", ["saturated", "table 50", "one key"])
def test_numerics(variant):
    case, got = check_case(NUMERIC, variant)
    if variant == "one key":        # every row returns its one key's value row
        W, nq, nk, H, d, nW = NUMERIC
        key = case[5].argmax(-1)                                                 # [nW, nq]
        want = torch.stack([case[2][w][key[w % nW]] for w in range(W)])          # [W, nq, H * d]
        assert float((got[0].cpu() - want).abs().max()) <= 1e-6


def test_a_zero_mask_gives_the_bits_of_no_mask():
    shape = (6, 17, 33, 3, 30, 3)
    q, k, v, table, index, mask, wgt = yardsticks(shape)[0]
    _, want, e32 = yardsticks_unmasked(shape)
    plain = evaluate(att.window_attention, q, k, v, table, index, None, wgt, device=dev())
    zero = evaluate(att.window_attention, q, k, v, table, index, torch.zeros_like(mask), wgt, device=dev())
    for name, a, b in zip(NAMES[:4], zero, plain):
        assert torch.equal(a, b), name
    assert held("zero mask g_table", zero[4], want[4], e32[4]) and held("no mask g_table", plain[4], want[4], e32[4])
    # the packed op without a mask takes the masked family too: the bits of the split op on contiguous copies
    shape = (2, 9, 9, 2, 5, 2)
    q, k, v, table, index, mask, wgt = yardsticks(shape)[0]
    plain = evaluate(att.window_attention, q, k, v, table, index, None, wgt, device=dev())
    out, g_qkv, _ = evaluate_qkv(q, k, v, table, index, None, wgt, dev())
    assert torch.equal(out, plain[0]) and torch.equal(g_qkv, torch.cat(plain[1:4], dim=-1))


@functools.lru_cache(maxsize=None)
def yardsticks_unmasked(shape):
    q, k, v, table, index, _, wgt = yardsticks(shape)[0]
    torch_form = lambda *a, mask: att.window_attention_torch(*a)        # noqa: E731
    want = evaluate(torch_form, q, k, v, table, index, None, wgt, dtype=torch.float64)
    f32 = evaluate(torch_form, q, k, v, table, index, None, wgt)
    return None, want, [float((a.double() - b).abs().max()) for a, b in zip(f32, want)]


def test_plumbing():
    shape = (6, 17, 33, 3, 30, 3)
    case, want, e32 = yardsticks(shape)
    q, k, v, table, index, mask, wgt = case
    d = dev()
    # two identical calls: the same out, g_q, g_k, g_v; no_grad forward == training forward
    runs = [evaluate(att.window_attention, *case, device=d) for _ in range(2)]
    for a, b in zip(runs[0][:4], runs[1][:4]):
        assert torch.equal(a, b)
    with torch.no_grad():
        assert torch.equal(att.window_attention(q.to(d), k.to(d), v.to(d), table.to(d), index.to(d), mask=mask.to(d)), runs[0][0])
    # a mask that is not contiguous fp32 is cast: float64, bf16-representable values in bf16, a strided view
    wide = torch.zeros(3, 17, 40, device=d)
    wide[:, :, :33] = mask.to(d)
    with torch.no_grad():
        args = (q.to(d), k.to(d), v.to(d), table.to(d), index.to(d))
        assert torch.equal(att.window_attention(*args, mask=wide[:, :, :33]), runs[0][0])
        assert torch.equal(att.window_attention(*args, mask=mask.to(d).double()), runs[0][0])
        mb = mask.to(torch.bfloat16)
        assert torch.equal(att.window_attention(*args, mask=mb.to(d)), att.window_attention(*args, mask=mb.float().to(d)))
    # only the table requires a gradient / the table does not
    leaves = [t.to(d).requires_grad_(True) for t in (q, k, v)]
    out = att.window_attention(*leaves, table.to(d), index.to(d), mask=mask.to(d))
    for x, y in zip(torch.autograd.grad(out, leaves, wgt.to(d)), runs[0][1:4]):
        assert torch.equal(x, y)
    tab = table.to(d).requires_grad_(True)
    out = att.window_attention(q.to(d), k.to(d), v.to(d), tab, index.to(d), mask=mask.to(d))
    assert held("only g_table", torch.autograd.grad(out, tab, wgt.to(d))[0], want[4], e32[4])
    # the packed op on a non-contiguous qkv, and under autocast (fp32 boundary)
    shape = (2, 9, 9, 2, 5, 2)
    q, k, v, table, index, mask, wgt = yardsticks(shape)[0]
    ref = evaluate_qkv(q, k, v, table, index, mask, wgt, d)
    qkv = torch.cat([q, k, v], dim=-1).to(d)
    with torch.no_grad():
        strided = torch.zeros(2, 9, 40, device=d)
        strided[..., :30] = qkv
        assert torch.equal(att.window_attention_qkv(strided[..., :30], table.to(d), index.to(d), mask=mask.to(d)), ref[0])
        with torch.autocast("cuda", dtype=torch.bfloat16):
            cast = att.window_attention_qkv(qkv, table.to(d), index.to(d), mask=mask.to(d))
        assert cast.dtype == torch.float32 and torch.equal(cast, ref[0])
    # errors on device tensors come before any launch
    with pytest.raises(ValueError):
        att.window_attention_qkv(qkv, table.to(d), index.to(d), mask=mask)              # the mask on another device
    with pytest.raises(ValueError):
        att.window_attention_qkv(qkv, table.to(d), index.to(d), mask=mask.to(d)[:, :8])


@pytest.mark.parametrize("name", list(SWIN_CASES))
def test_goldens_through_use_hip_attention(name):
    m, data, mask, want, e32 = golden_yardsticks(name)
    sw = copy.deepcopy(m)
    assert att.use_hip_attention(sw) == 1
    got = run_case(sw, SWIN_CASES[name], mask, device=dev())
    assert all([held(f"{name} gpu {k}", got[k], want[k], e32[k]) for k in want])
