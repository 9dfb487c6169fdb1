"""The rotary window-attention kernels (the ROPE variants of csrc/splat_attn.hip behind gsasr_amd.window_attention_rope) on the
GPU: forward and the four gradients (q, k, v, angles) against the float64 evaluation of the torch expression, under the bar of
tests/test_window_attention.py (4 x e32 + 1e-6 x max-abs, e32 the fp32 torch expression's own error on the same input).  Every
check prints its ratio.

Shapes are (W, nq, nk, H, d); angles are 6 randn(H, N, d/2) unless a case says otherwise.  Besides the shipped shapes: extents of
1, tails of every tile, the limits 255 / 256 with d = 30 and d = 2, many windows for the angle gradient's two-stage sum (70 and
300: 9 and 38 slices), and angle rows past max(nq, nk), which must come back exactly 0."""
import copy
import functools
import os
import sys

import pytest
import torch

from gsasr_amd import attention as att
from test_window_attention import held
from test_window_attention_rope import GOLDEN_CASES, golden_yardsticks, run_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("out", "g_q", "g_k", "g_v", "g_angles")
SHIPPED = [(3, 144, 144, 6, 32), (2, 256, 256, 6, 32)]
TAILS = [(1, 1, 1, 1, 2), (2, 9, 9, 2, 6), (2, 17, 33, 3, 30), (2, 33, 17, 1, 32), (1, 255, 256, 2, 30), (1, 256, 255, 2, 2)]
MANY = [(70, 9, 9, 6, 32), (300, 5, 7, 1, 4)]
NUMERIC = (2, 40, 50, 2, 30)


def dev():
    return torch.device("cuda:0")


def make_case(shape, variant="plain"):
    W, nq, nk, H, d = shape
    g = torch.Generator().manual_seed(19 * sum(shape) + len(variant))
    q, k, v = torch.randn(W, nq, H * d, generator=g), torch.randn(W, nk, H * d, generator=g), torch.randn(W, nk, H * d, generator=g)
    N = max(nq, nk) + (3 if variant == "extra rows" else 0)
    angles = 6 * torch.randn(H, N, d // 2, generator=g)
    wgt = torch.randn(W, nq, H * d, generator=g)
    if variant == "saturated":          # rows go one-hot: the maximum subtraction carries the softmax
        q = q * 30
    elif variant == "zero angles":
        angles = torch.zeros_like(angles)
    elif variant == "angles 30":        # the range of the shipped 16 x 16 grids
        angles = 60 * torch.rand(H, N, d // 2, generator=g) - 30
    elif variant == "zero q":           # uniform rows
        q = torch.zeros_like(q)
    elif variant == "zero v":
        v[1] = 0
    return q, k, v, angles, wgt


def evaluate(fn, q, k, v, angles, wgt, device="cpu", dtype=torch.float32, need=(True, True, True, True)):
    a = [t.detach().to(device=device, dtype=dtype, copy=True).requires_grad_(n) for t, n in zip((q, k, v, angles), need)]      # (the case is shared: left unchanged)
    out = fn(*a)
    grads = iter(torch.autograd.grad((out * wgt.to(device=device, dtype=dtype)).sum(), [t for t, n in zip(a, need) if n]))
    return (out.detach(), *[next(grads) if n else None for n in need])


@functools.lru_cache(maxsize=None)
def yardsticks(shape, variant="plain"):
    """(the case, its float64 results, e32 per quantity) -- computed once on the CPU and shared"""
    case = make_case(shape, variant)
    want = evaluate(att.window_attention_rope_torch, *case, dtype=torch.float64)
    f32 = evaluate(att.window_attention_rope_torch, *case)
    return case, want, [float((a.double() - b).abs().max()) for a, b in zip(f32, want)]


def check_case(shape, variant="plain"):
    case, want, e32 = yardsticks(shape, variant)
    got = evaluate(att.window_attention_rope, *case, device=dev())
    ok = True
    for name, g, w, e in zip(NAMES, got, want, e32):
        ok &= held(f"rope {shape} {variant} {name}", g, w, e)
    assert ok
    return case, got, want, e32


@pytest.mark.parametrize("shape", SHIPPED + TAILS + MANY, ids=lambda s: "x".join(map(str, s)))
def test_forward_and_gradients(shape):
    case, got, want, e32 = check_case(shape)
    W, nq, nk, H, d = shape
    if nq != nk:        # the rows past min(nq, nk) get only q's part or only k's: against float64 like the rest, on their own
        lo = min(nq, nk)
        assert float(want[4][:, lo:].abs().max()) > 0
        assert held(f"rope {shape} g_angles rows past {lo}", got[4][:, lo:], want[4][:, lo:], e32[4])


def test_angle_rows_past_the_tokens_are_exactly_zero():
    shape = (2, 17, 33, 3, 30)
    case, got, want, e32 = check_case(shape, "extra rows")
    assert got[4].shape[1] == 36 and bool((got[4][:, 33:] == 0).all()) and bool((got[4][:, :33] != 0).any())


@pytest.mark.parametrize("variant", ["saturated", "zero angles", "angles 30", "zero q", "zero v"])
def test_numerics(variant):
    case, got, want, e32 = check_case(NUMERIC, variant)
    q, k, v, angles, wgt = case
    if variant == "zero v":
        assert bool((got[0][1] == 0).all()) and bool((got[1][1] == 0).all()) and bool((got[2][1] == 0).all())
    if variant == "zero q":
        mean = v.view(2, 50, 2, 30).mean(1)       # uniform rows: every query returns the mean value
        assert float((got[0].detach().cpu().view(2, 40, 2, 30) - mean[:, None]).abs().max()) <= 1e-6
    if variant == "zero angles":                  # no rotation: the biased op with a zero table, on the same input
        d = dev()
        a = [t.to(d).requires_grad_(True) for t in (q, k, v)]
        out = att.window_attention(*a, torch.zeros(1, 2, device=d), torch.zeros(40, 50, dtype=torch.int64, device=d))
        biased = (out.detach(), *torch.autograd.grad((out * wgt.to(d)).sum(), a))
        ok = True
        for name, g, b, w, e in zip(NAMES, got, biased, want, e32):
            ok &= held(f"rope zero angles {name} against the biased op", g, b.detach().cpu().double(), e)
            assert float(w.abs().max()) > 0
        assert ok


def test_plumbing():
    shape = (2, 17, 33, 3, 30)
    (q, k, v, angles, wgt), want, e32 = yardsticks(shape)
    d = dev()
    # q / k / v as views of one fused tensor, grad_out non-contiguous
    nq, nk, C = 17, 33, 90
    fused = torch.zeros(2, nk, 3 * C, device=d)
    fused[:, :nq, :C], fused[:, :, C:2 * C], fused[:, :, 2 * C:] = q.to(d), k.to(d), v.to(d)
    fused.requires_grad_(True)
    tq, tk, tv = fused[:, :nq, :C], fused[:, :, C:2 * C], fused[:, :, 2 * C:]
    assert not tq.is_contiguous() and not tk.is_contiguous()
    ang = angles.to(d).requires_grad_(True)
    out = att.window_attention_rope(tq, tk, tv, ang)
    gout = wgt.to(d).transpose(0, 1).contiguous().transpose(0, 1)
    assert not gout.is_contiguous()
    gf, ga = torch.autograd.grad(out, [fused, ang], gout)
    ok = held("rope views out", out, want[0], e32[0])
    ok &= held("rope views g_q", gf[:, :nq, :C], want[1], e32[1]) & held("rope views g_k", gf[:, :, C:2 * C], want[2], e32[2])
    ok &= held("rope views g_v", gf[:, :, 2 * C:], want[3], e32[3]) & held("rope views g_angles", ga, want[4], e32[4])
    assert ok and float(gf[:, nq:, :C].abs().max()) == 0.0
    # no_grad forward == training forward, bitwise; all five results bitwise equal across two runs
    runs = [evaluate(att.window_attention_rope, q, k, v, angles, wgt, device=d) for _ in range(2)]
    with torch.no_grad():
        plain = att.window_attention_rope(q.to(d), k.to(d), v.to(d), angles.to(d))
    assert torch.equal(plain, runs[0][0]) and torch.equal(plain, out)
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b)
    assert torch.equal(ga, runs[0][4])
    # a non-default current stream
    s = torch.cuda.Stream(device=d)
    s.wait_stream(torch.cuda.current_stream(d))
    with torch.cuda.stream(s):
        on_s = evaluate(att.window_attention_rope, q, k, v, angles, wgt, device=d)
    s.synchronize()
    for a, b in zip(on_s, runs[0]):
        assert torch.equal(a, b)
    # only the angles require a gradient
    only = evaluate(att.window_attention_rope, q, k, v, angles, wgt, device=d, need=(False, False, False, True))
    assert only[1] is None and only[2] is None and only[3] is None and torch.equal(only[4], runs[0][4]) and torch.equal(only[0], runs[0][0])
    # only q, k, v do: their bits are those of the run that also asked for the angles'
    qkv = evaluate(att.window_attention_rope, q, k, v, angles, wgt, device=d, need=(True, True, True, False))
    assert qkv[4] is None
    for a, b in zip(qkv[:4], runs[0][:4]):
        assert torch.equal(a, b)
    # under bf16 autocast with bf16 inputs: an fp32 result, bitwise the op's on .float() of those inputs
    qb, kb, vb = (t.to(d).bfloat16() for t in (q, k, v))
    with torch.autocast("cuda", dtype=torch.bfloat16):
        cast = att.window_attention_rope(qb, kb, vb, angles.to(d))
    assert cast.dtype == torch.float32
    assert torch.equal(cast, att.window_attention_rope(qb.float(), kb.float(), vb.float(), angles.to(d)))
    # many windows: the two-stage angle sum gives the same bits twice as well
    case = yardsticks((70, 9, 9, 6, 32))[0]
    a, b = (evaluate(att.window_attention_rope, *case, device=d) for _ in range(2))
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    # a bad shape on the device is a ValueError before any launch
    with pytest.raises(ValueError):
        att.window_attention_rope(q.to(d), k.to(d), v.to(d), angles.to(d)[:, :20])
    with pytest.raises(ValueError):
        att.window_attention_rope(q.to(d), k.to(d), v.to(d), angles)


@pytest.mark.parametrize("name", list(GOLDEN_CASES))
def test_goldens_through_use_hip_attention(name):
    m, data, want, e32 = golden_yardsticks(name)
    sw = copy.deepcopy(m)
    assert att.use_hip_attention(sw) == 1
    got = run_case(sw, GOLDEN_CASES[name], device=dev())
    assert "g_rope_freqs" in want
    assert all([held(f"rope {name} gpu {k}", got[k], want[k], e32[k]) for k in want])


def test_decoder_modes_agree():
    """tools/c5_models.Fea2GSDecoder(position="rope", channels=192, attention="hip") against attention="torch" with the same
    weights, feat [2, 64, 24, 12]: output and the gradients in seed, feat and one layer's frequencies; the yardstick is the
    float64 run of the torch mode, e32 the torch mode in fp32 against it (as tests/test_window_attention_gpu.py does it).  One
    cross block of 2 layers and one self block of 2 layers: every kind of layer once."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import c5_models
    torch.manual_seed(0)
    kw = dict(position="rope", channel=192, cross_layers=2, self_blocks=1, self_layers=2)
    base = c5_models.Fea2GSDecoder(**kw)
    feat, scale = torch.randn(2, 64, 24, 12), torch.tensor([2.0, 3.5])
    wgt = torch.randn(2, 16 * 24 * 12, 9)

    def run(net, device="cpu", dtype=torch.float32):
        net = net.to(device=device, dtype=dtype)
        f = feat.to(device=device, dtype=dtype).requires_grad_(True)
        out = net(f, scale.to(device=device, dtype=dtype))
        freqs = net.cross[0].layers[1].attn.rope_freqs
        gs = torch.autograd.grad((out * wgt.to(device=device, dtype=dtype)).sum(), [net.seed, f, freqs])
        return (out.detach(), *gs)

    want = run(copy.deepcopy(base), dtype=torch.float64)
    f32 = run(copy.deepcopy(base))
    hip = c5_models.Fea2GSDecoder(**kw, attention="hip")
    hip.load_state_dict(base.state_dict())
    got = run(hip, device=dev())
    assert all([held(f"rope decoder {n}", g, w, float((f.double() - w).abs().max())) for n, g, w, f in zip(("out", "g_seed", "g_feat", "g_freqs"), got, want, f32)])
