"""The window-attention kernels (csrc/splat_attn.hip behind gsasr_amd.window_attention) on the GPU: forward and the four
gradients against the float64 evaluation of the torch expression, under the bar of tests/test_window_attention.py
(4 x e32 + 1e-6 x max-abs, e32 the fp32 torch expression's own error on the same input).  Every check prints its ratio.

Shapes are (W, nq, nk, H, d).  Besides the shipped ones: extents of 1, tails of every tile (16 queries / keys, 16 columns of
the head), the limits 255 / 256 with d = 31 and d = 1, and 420 workgroups with 70 partial tables for the second-stage sum.
The index of a case is relative (i - j shifted) over nq + nk - 1 rows of a table that has three more, so unused rows exist
everywhere and must come back exactly 0."""
import copy
import functools
import os
import sys

import numpy as np
import pytest
import torch

from gsasr_amd import attention as att
from test_window_attention import GOLDEN_CASES, golden_yardsticks, held, run_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("out", "g_q", "g_k", "g_v", "g_table")
SHIPPED = [(3, 144, 144, 6, 30), (2, 256, 256, 6, 32)]
TAILS = [(1, 1, 1, 1, 1), (2, 9, 9, 2, 5), (2, 17, 33, 3, 30), (2, 33, 17, 1, 32), (1, 255, 256, 2, 31), (1, 256, 255, 2, 1)]
MANY = [(70, 9, 9, 6, 30)]
NUMERIC = (2, 40, 50, 2, 30)


def dev():
    return torch.device("cuda:0")


def make_case(shape, variant="plain"):
    W, nq, nk, H, d = shape
    g = torch.Generator().manual_seed(17 * sum(shape) + len(variant))
    q, k, v = torch.randn(W, nq, H * d, generator=g), torch.randn(W, nk, H * d, generator=g), torch.randn(W, nk, H * d, generator=g)
    T = nq + nk - 1 + 3
    table = 0.5 * torch.randn(T, H, generator=g)
    index = torch.arange(nq)[:, None] - torch.arange(nk)[None, :] + nk - 1
    wgt = torch.randn(W, nq, H * d, generator=g)
    if variant == "saturated":          # rows go one-hot: the maximum subtraction carries the softmax
        q = q * 30
    elif variant == "table 50":
        table = torch.where(torch.rand(T, H, generator=g) < 0.5, -50.0, 50.0)
    elif variant == "zero q":           # uniform rows (up to the bias)
        q = torch.zeros_like(q)
        table = torch.zeros_like(table)
    elif variant == "zero v":
        v[1] = 0
    return q, k, v, table, index, wgt


def evaluate(fn, q, k, v, table, index, wgt, device="cpu", dtype=torch.float32):
    a = [t.to(device=device, dtype=dtype).requires_grad_(True) for t in (q, k, v, table)]
    out = fn(*a, index.to(device))
    return (out.detach(), *torch.autograd.grad((out * wgt.to(device=device, dtype=dtype)).sum(), a))


@functools.lru_cache(maxsize=None)
def yardsticks(shape, variant="plain"):
    """(the case, its float64 results, e32 per quantity) -- computed once on the CPU and shared"""
    case = make_case(shape, variant)
    want = evaluate(att.window_attention_torch, *case, dtype=torch.float64)
    f32 = evaluate(att.window_attention_torch, *case)
    return case, want, [float((a.double() - b).abs().max()) for a, b in zip(f32, want)]


def check_case(shape, variant="plain"):
    case, want, e32 = yardsticks(shape, variant)
    got = evaluate(att.window_attention, *case, device=dev())
    ok = True
    for name, g, w, e in zip(NAMES, got, want, e32):
        ok &= held(f"{shape} {variant} {name}", g, w, e)
    assert bool((got[4][-3:] == 0).all()), "table rows no (i, j) uses must get exactly 0"
    assert ok
    return case, got


@pytest.mark.parametrize("shape", SHIPPED + TAILS + MANY, ids=lambda s: "x".join(map(str, s)))
def test_forward_and_gradients(shape):
    check_case(shape)


@pytest.mark.parametrize("variant", ["saturated", "table 50", "zero q", "zero v"])
def test_numerics(variant):
    case, got = check_case(NUMERIC, variant)
    if variant == "zero v":
        assert bool((got[0][1] == 0).all()) and bool((got[1][1] == 0).all()) and bool((got[2][1] == 0).all())
    if variant == "zero q":
        want = case[2].view(2, 50, 2, 30).mean(1)       # uniform rows: every query returns the mean value
        assert float((got[0].detach().cpu().view(2, 40, 2, 30) - want[:, None]).abs().max()) <= 1e-6


def test_large_table_takes_the_atomic_path():
    """above 4096 table rows the table gradient is not binned in LDS"""
    q, k, v, _, index, wgt = make_case((2, 9, 9, 2, 5))
    g = torch.Generator().manual_seed(1)
    table = 0.5 * torch.randn(5000, 2, generator=g)
    index = index * 290
    want = evaluate(att.window_attention_torch, q, k, v, table, index, wgt, dtype=torch.float64)
    f32 = evaluate(att.window_attention_torch, q, k, v, table, index, wgt)
    got = evaluate(att.window_attention, q, k, v, table, index, wgt, device=dev())
    assert all([held(f"T 5000 {n}", a, w, float((f.double() - w).abs().max())) for n, a, w, f in zip(NAMES, got, want, f32)])
    used = torch.zeros(5000, dtype=torch.bool)
    used[index.flatten()] = True
    assert bool((got[4].cpu()[~used] == 0).all())
    # ... and without a table gradient the other three come out the same, bit for bit
    d = dev()
    leaves = [t.to(d).requires_grad_(True) for t in (q, k, v)]
    out = att.window_attention(*leaves, table.to(d), index.to(d))
    for x, y in zip(torch.autograd.grad(out, leaves, wgt.to(d)), got[1:4]):
        assert torch.equal(x, y)


def test_cross_index_leaves_unused_rows_exactly_zero():
    data = np.load(os.path.join(ROOT, "tests", "golden", "attention_cross_12.npz"))
    index = torch.from_numpy(data["index"].astype(np.int64))
    g = torch.Generator().manual_seed(2)
    q, k, v, wgt = (torch.randn(2, 144, 60, generator=g) for _ in range(4))
    table = torch.from_numpy(data["table"])
    want = evaluate(att.window_attention_torch, q, k, v, table, index, wgt, dtype=torch.float64)
    f32 = evaluate(att.window_attention_torch, q, k, v, table, index, wgt)
    got = evaluate(att.window_attention, q, k, v, table, index, wgt, device=dev())
    assert all([held(f"cross index {n}", a, w, float((f.double() - w).abs().max())) for n, a, w, f in zip(NAMES, got, want, f32)])
    assert int(index.max()) == 506 and table.shape[0] == 529
    assert bool((got[4][507:] == 0).all()) and bool((got[4][:507] != 0).any())


def test_plumbing():
    shape = (2, 17, 33, 3, 30)
    (q, k, v, table, index, wgt), want, e32 = yardsticks(shape)
    d = dev()
    # q / k / v as views of one fused tensor, grad_out non-contiguous, the table without a gradient
    nq, nk, C = 17, 33, 90
    fused = torch.zeros(2, nk, 3 * C, device=d)
    fused[:, :nq, :C], fused[:, :, C:2 * C], fused[:, :, 2 * C:] = q.to(d), k.to(d), v.to(d)
    fused.requires_grad_(True)
    tq, tk, tv = fused[:, :nq, :C], fused[:, :, C:2 * C], fused[:, :, 2 * C:]
    assert not tq.is_contiguous() and not tk.is_contiguous()
    tab = table.to(d)
    out = att.window_attention(tq, tk, tv, tab, index.to(d))
    gout = wgt.to(d).transpose(0, 1).contiguous().transpose(0, 1)
    assert not gout.is_contiguous()
    (gf,) = torch.autograd.grad(out, fused, gout)
    ok = held("views out", out, want[0], e32[0])
    ok &= held("views g_q", gf[:, :nq, :C], want[1], e32[1]) & held("views g_k", gf[:, :, C:2 * C], want[2], e32[2])
    ok &= held("views g_v", gf[:, :, 2 * C:], want[3], e32[3])
    assert ok and float(gf[:, nq:, :C].abs().max()) == 0.0
    # no_grad forward == training forward, bitwise; dq, dk, dv bitwise equal across two runs
    runs = [evaluate(att.window_attention, q, k, v, table, index, wgt, device=d) for _ in range(2)]
    with torch.no_grad():
        plain = att.window_attention(q.to(d), k.to(d), v.to(d), tab, index.to(d))
    assert torch.equal(plain, runs[0][0]) and torch.equal(plain, out)
    for a, b in zip(runs[0][:4], runs[1][:4]):
        assert torch.equal(a, b)
    # a non-default current stream
    s = torch.cuda.Stream(device=d)
    s.wait_stream(torch.cuda.current_stream(d))
    with torch.cuda.stream(s):
        on_s = evaluate(att.window_attention, q, k, v, table, index, wgt, device=d)
    s.synchronize()
    for a, b in zip(on_s[:4], runs[0][:4]):
        assert torch.equal(a, b)
    assert held("stream g_table", on_s[4], want[4], e32[4])
    # an out-of-range index on the device is a ValueError before any launch
    bad = index.to(d).clone()
    bad[3, 4] = table.shape[0]
    with pytest.raises(ValueError):
        att.window_attention(q.to(d), k.to(d), v.to(d), tab, bad)


@pytest.mark.parametrize("name", list(GOLDEN_CASES))
def test_goldens_through_use_hip_attention(name):
    m, data, want, e32 = golden_yardsticks(name)
    sw = copy.deepcopy(m)
    assert att.use_hip_attention(sw) == 1
    got = run_case(sw, GOLDEN_CASES[name], device=dev())
    assert all([held(f"{name} gpu {k}", got[k], want[k], e32[k]) for k in want])


def test_decoder_modes_agree():
    """tools/c5_models.Fea2GSDecoder(attention="hip", scale_attention="constant") against the default decoder with the same
    weights, feat [2, 64, 24, 12]: output and the gradients in seed, feat and one table; e32 from the default decoder in fp32
    against itself in float64.  Shipped width (180 channels, 6 heads, 12 x 12 windows) with one cross block of 2 layers and
    one self block of 2 layers: every kind of layer (cross / self, plain / shifted) once, so that the float64 yardstick
    takes a second on the CPU and the comparison is not one of two fp32 nets 38 layers deep."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import c5_models
    torch.manual_seed(0)
    kw = dict(cross_layers=2, self_blocks=1, self_layers=2)
    base = c5_models.Fea2GSDecoder(**kw)
    feat, scale = torch.randn(2, 64, 24, 12), torch.tensor([2.0, 3.5])
    wgt = torch.randn(2, 16 * 24 * 12, 9)

    def run(net, device="cpu", dtype=torch.float32):
        net = net.to(device=device, dtype=dtype)
        f = feat.to(device=device, dtype=dtype).requires_grad_(True)
        out = net(f, scale.to(device=device, dtype=dtype))
        table = net.cross[0].layers[1].attn.bias
        gs = torch.autograd.grad((out * wgt.to(device=device, dtype=dtype)).sum(), [net.seed, f, table])
        return (out.detach(), *gs)

    want = run(copy.deepcopy(base), dtype=torch.float64)
    f32 = run(copy.deepcopy(base))
    hip = c5_models.Fea2GSDecoder(**kw, attention="hip", scale_attention="constant")
    hip.load_state_dict(base.state_dict())
    got = run(hip, device=dev())
    assert all([held(f"decoder {n}", g, w, float((f.double() - w).abs().max())) for n, g, w, f in zip(("out", "g_seed", "g_feat", "g_table"), got, want, f32)])
