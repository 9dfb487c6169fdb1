"""The bf16 mode of the masked family on the GPU (window_attention(..., compute="bf16", mask=) and window_attention_qkv(...,
compute="bf16"): gsasr_window_attn_masked_bf16 -- the forward on the bf16 matrix instruction with the fp32 mask added to the fp32
score sum after `scale` and the bias, the backward the fp32 kernels instantiated on bf16 activations).

Parity: forward and the four gradients against the float64 evaluation of the fp32 contract on the bf16-rounded inputs, under the
bar of tests/test_window_attention_bf16_gpu.py (4 x e + 1e-6 x max-abs), where e is, per quantity, the error of torch's own bf16
evaluation of the same case on the CPU: F.scaled_dot_product_attention on bf16 q, k, v with bias + mask as the bf16 `attn_mask`,
and autograd through it.  Every check prints its ratio.  Shapes (W, nq, nk, H, d, nW) and masks are those of
tests/test_window_attention_masked_gpu.py.

Recorded on an MI355X (largest ratio to the bar per quantity): out 0.27, g_q 0.42, g_k 0.44, g_v 0.25, g_table 0.66; through the
switched modules 0.20-0.25."""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F

import test_window_attention_masked as cpu_masked
import test_window_attention_masked_gpu as gpu_masked
from gsasr_amd import attention as att
from test_window_attention import held

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
SHAPES = gpu_masked.SHIPPED + gpu_masked.TAILS[:3] + gpu_masked.LIMITS[:1] + gpu_masked.SLOTS + gpu_masked.DISPATCH
NAMES = gpu_masked.NAMES


def dev():
    return torch.device("cuda:0")


def heads_first(x, H):
    W, n, C = x.shape
    return x.view(W, n, H, C // H).permute(0, 2, 1, 3)


def sdpa_masked(q, k, v, table, index, mask):
    """torch's own bf16 evaluation: SDPA on bf16 q, k, v with bias + mask as a bf16 attn_mask [W, H, nq, nk]"""
    W, nq, C = q.shape
    H = table.shape[1]
    bias = table[index.long()].permute(2, 0, 1)
    full = (bias[None] + mask[torch.arange(W) % mask.shape[0]][:, None]).to(BF)
    out = F.scaled_dot_product_attention(heads_first(q, H), heads_first(k, H), heads_first(v, H), attn_mask=full, scale=(C // H) ** -0.5)
    return out.transpose(1, 2).reshape(W, nq, C)


def evaluate(fn, acts, table, index, mask, wgt, device="cpu", act_dtype=torch.float32, table_dtype=torch.float32):
    leaves = [t.detach().to(device=device, dtype=act_dtype, copy=True).requires_grad_(True) for t in acts]
    leaves.append(table.detach().to(device=device, dtype=table_dtype, copy=True).requires_grad_(True))
    out = fn(*leaves, index.to(device), mask.to(device=device, dtype=table_dtype))
    return (out.detach(), *torch.autograd.grad(out, leaves, wgt.to(device=device, dtype=out.dtype)))


@functools.lru_cache(maxsize=None)
def yardsticks(shape, variant="random"):
    """((q, k, v) and wgt rounded to bf16, table, index, mask), the float64 results, e per quantity -- once on the CPU, shared"""
    q, k, v, table, index, mask, wgt = gpu_masked.make_case(shape, variant)
    acts = tuple(t.to(BF).float() for t in (q, k, v))
    wgt = wgt.to(BF).float()
    f64 = lambda q, k, v, t, i, m: att.window_attention_torch(q, k, v, t, i, None, m)        # noqa: E731
    want = evaluate(f64, acts, table, index, mask, wgt, act_dtype=torch.float64, table_dtype=torch.float64)
    own = evaluate(sdpa_masked, acts, table, index, mask, wgt, act_dtype=BF)
    return (acts, table, index, mask, wgt), want, [float((a.double() - b).abs().max()) for a, b in zip(own, want)]


def op(q, k, v, table, index, mask):
    return att.window_attention(q, k, v, table, index, compute="bf16", mask=mask)


def check_case(shape, variant="random"):
    case, want, e = yardsticks(shape, variant)
    got = evaluate(op, *case, device=dev(), act_dtype=BF)
    assert [g.dtype for g in got] == [BF, BF, BF, BF, torch.float32]
    # ("one key": dS cancels to exp(-100) in exact arithmetic; the backward's products are fp32 on the widened operands, so the
    # bounds of gpu_masked.one_key_bounds hold here as they stand)
    bounds = gpu_masked.one_key_bounds(*case[0], case[3], case[4], shape) if variant == "one key" else {}
    ok = True
    for name, g, w, err in zip(NAMES, got, want, e):
        ok &= gpu_masked.held_or_bounded(f"bf16 masked {shape} {variant} {name}", g, w, err, bounds.get(name))
    assert bool((got[4][-3:] == 0).all()), "table rows no (i, j) uses must get exactly 0"
    if shape[1] == shape[2]:        # the packed form: the same bits as the split form on contiguous copies
        acts, table, index, mask, wgt = case
        D = dev()
        qkv = torch.cat(acts, dim=-1).to(D, BF).requires_grad_(True)
        tab = table.to(D).requires_grad_(True)
        out = att.window_attention_qkv(qkv, tab, index.to(D), compute="bf16", mask=mask.to(D))
        g_qkv, g_table = torch.autograd.grad(out, [qkv, tab], wgt.to(D, BF))
        assert out.dtype == BF and g_qkv.dtype == BF and g_qkv.shape[-1] == 3 * acts[0].shape[-1]
        assert torch.equal(out, got[0]) and torch.equal(g_qkv, torch.cat(got[1:4], dim=-1))
        ok &= gpu_masked.held_or_bounded(f"bf16 masked {shape} {variant} packed g_table", g_table, want[4], e[4], bounds.get("g_table"))
    assert ok
    return case, got


@pytest.mark.parametrize("shape", SHAPES, ids=gpu_masked.ident)
def test_forward_and_gradients_with_an_asymmetric_mask(shape):
    check_case(shape)


@pytest.mark.parametrize("shape", gpu_masked.SWIN_PATTERN, ids=gpu_masked.ident)
def test_forward_and_gradients_with_a_swin_mask(shape):
    check_case(shape, "swin")


@pytest.mark.parametrize("variant", ["saturated", "table 50", "one key"])
def test_numerics(variant):
    case, got = check_case(gpu_masked.NUMERIC, variant)
    if variant == "one key":        # every row returns its one key's (bf16) value row, exactly
        W, nq, nk, H, d, nW = gpu_masked.NUMERIC
        key = case[3].argmax(-1)
        want = torch.stack([case[0][2][w][key[w % nW]] for w in range(W)])
        assert float((got[0].float().cpu() - want).abs().max()) <= 1e-6


def test_bitwise_plumbing():
    shape = (6, 17, 33, 3, 30, 3)
    case, want, e = yardsticks(shape)
    (q, k, v), table, index, mask, wgt = case
    D = dev()
    runs = [evaluate(op, *case, device=D, act_dtype=BF) for _ in range(2)]
    for a, b in zip(runs[0][:4], runs[1][:4]):
        assert torch.equal(a, b)
    # a zero mask gives the bits of the call without one (the table gradient under the bar)
    zero = evaluate(op, (q, k, v), table, index, torch.zeros_like(mask), wgt, device=D, act_dtype=BF)
    plain = evaluate(lambda q, k, v, t, i, m: att.window_attention(q, k, v, t, i, compute="bf16"), (q, k, v), table, index, mask, wgt, device=D, act_dtype=BF)
    for name, a, b in zip(NAMES[:4], zero, plain):
        assert torch.equal(a, b), name
    none = torch.zeros_like(mask)
    f64 = lambda q, k, v, t, i, m: att.window_attention_torch(q, k, v, t, i, None, m)        # noqa: E731
    want0 = evaluate(f64, (q, k, v), table, index, none, wgt, act_dtype=torch.float64, table_dtype=torch.float64)[4]
    e0 = float((evaluate(sdpa_masked, (q, k, v), table, index, none, wgt, act_dtype=BF)[4].double() - want0).abs().max())
    assert held("bf16 zero mask g_table", zero[4], want0, e0) and held("bf16 no mask g_table", plain[4], want0, e0)
    # fp32 inputs give the bits of the call on their .bfloat16(); under bf16 autocast the result is bf16 with the same bits
    with torch.no_grad():
        a32 = op(q.to(D), k.to(D), v.to(D), table.to(D), index.to(D), mask.to(D))
        assert a32.dtype == BF and torch.equal(a32, runs[0][0])
        with torch.autocast("cuda", dtype=BF):
            assert torch.equal(op(q.to(D, BF), k.to(D, BF), v.to(D, BF), table.to(D), index.to(D), mask.to(D)), runs[0][0])


def run_amp(m, case, mask, device):
    """cpu_masked.run_case with the module's forward under bf16 autocast on `device` (fp32 module, fp32 inputs)"""
    m = m.to(device)
    x, wgt = (torch.from_numpy(a).to(device) for a in cpu_masked.swin_inputs(case))
    x.requires_grad_(True)
    with torch.autocast(torch.device(device).type, dtype=BF):
        out = m(x, None if mask is None else mask.to(device))
    grads = torch.autograd.grad((out.float() * wgt).sum(), [x, m.qkv.weight, m.qkv.bias, m.relative_position_bias_table])
    return out.dtype, dict(out=out.detach(), **dict(zip(["g_x"] + ["g_" + p for p in cpu_masked.PARAMS], grads)))


@pytest.mark.parametrize("name", list(cpu_masked.SWIN_CASES))
def test_goldens_through_use_hip_attention(name):
    """the switched module under bf16 autocast against the float64 module; e = the unswitched module under CPU bf16 autocast"""
    m, data, mask = cpu_masked.load_golden(name)
    case = cpu_masked.SWIN_CASES[name]
    want = cpu_masked.run_case(copy.deepcopy(m), case, mask, dtype=torch.float64)
    _, amp = run_amp(copy.deepcopy(m), case, mask, "cpu")
    e = {k: float((amp[k].double() - want[k]).abs().max()) for k in want}
    sw = copy.deepcopy(m)
    assert att.use_hip_attention(sw, compute="bf16") == 1
    dtype, got = run_amp(sw, case, mask, dev())
    assert dtype == BF
    assert all([held(f"bf16 {name} gpu {k}", got[k], want[k], e[k]) for k in want])
    # an fp32 model outside autocast keeps working, with fp32 results
    sw32 = copy.deepcopy(m).to(dev())
    att.use_hip_attention(sw32, compute="bf16")
    x = torch.from_numpy(cpu_masked.swin_inputs(case)[0]).to(dev())
    with torch.no_grad():
        assert sw32(x, None if mask is None else mask.to(dev())).dtype == torch.float32
