"""The bf16 mode of the two window attentions on the GPU (window_attention / window_attention_rope with compute="bf16": the forward
on the bf16 matrix instruction, the backward the fp32 kernels instantiated on bf16 activations).

Parity: forward and the four gradients against the float64 evaluation of the fp32 contract on the bf16-rounded inputs, under
`bar()` of tests/test_window_attention.py (4 x e + 1e-6 x max-abs), where e is, per quantity, the error of torch's own bf16
evaluation of the same case on the CPU: the rotation in fp32, `.to(bfloat16)`, F.scaled_dot_product_attention on bf16 tensors and
autograd through it; in the biased variant the same SDPA with the bias as a bf16 mask (what autocast hands it).  In the biased
variant `out` is additionally held to bar(e_round), e_round = max |bf16(want) - want|: its inputs are exact in bf16, so the
forward's only visible error should be the rounding of the result -- the check that sees a 1 %-level mistake.  Every check prints
its ratio.  The shapes are those of tests/test_window_attention_gpu.py and tests/test_window_attention_rope_gpu.py.

Exact selection: keys of +-1, q = 64 k[perm]: every query's target score exceeds the others by more than 20 (asserted in float64),
p is one-hot, and out must be v[perm] bit for bit -- any mismatch between P's key order and V's, or a wrong tail, shows.

Recorded on an MI355X (largest ratio to the bar per quantity over all shapes and variants; DESIGN.md 3.2i explains the two highest):
rotary out 0.25, g_q 0.26, g_k 0.30, g_v 0.25, g_angles 0.30; biased out 0.33 (0.35 against its own rounding), g_q 0.87 (the
store's rounding at (1, 256, 255, 2, 1)), g_k 0.60, g_v 0.25, g_table 0.87 ("saturated": delta from the stored bf16 out); through the
modules 0.07-0.62; selection margins 93-136."""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F

import test_window_attention as cpu_biased
import test_window_attention_gpu as gpu_biased
import test_window_attention_rope as cpu_rope
import test_window_attention_rope_gpu as gpu_rope
from gsasr_amd import attention as att
from test_window_attention import held

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
BIASED_SHAPES = gpu_biased.SHIPPED + gpu_biased.TAILS + gpu_biased.MANY
ROPE_SHAPES = gpu_rope.SHIPPED + gpu_rope.TAILS + gpu_rope.MANY
NUMERIC = (2, 40, 50, 2, 30)
SELECT = [(256, 32), (255, 30), (33, 30), (17, 32)]


def dev():
    return torch.device("cuda:0")


def ident(s):
    return "x".join(map(str, s))


def rounded(*ts):
    return tuple(t.to(BF).float() for t in ts)


def heads_first(x, H):
    W, n, C = x.shape
    return x.view(W, n, H, C // H).permute(0, 2, 1, 3)


def sdpa_biased(q, k, v, table, index):
    """torch's own bf16 evaluation: SDPA on bf16 q, k, v with the bias as a bf16 mask"""
    W, nq, C = q.shape
    H = table.shape[1]
    mask = table[index.long()].permute(2, 0, 1).to(BF)
    out = F.scaled_dot_product_attention(heads_first(q, H), heads_first(k, H), heads_first(v, H), attn_mask=mask[None], scale=(C // H) ** -0.5)
    return out.transpose(1, 2).reshape(W, nq, C)


def sdpa_rope(q, k, v, angles):
    """torch's own bf16 evaluation: the rotation in fp32, .to(bfloat16), SDPA on bf16 tensors"""
    W, nq, C = q.shape
    nk, H = k.shape[1], angles.shape[0]
    d = C // H
    a = angles.permute(1, 0, 2)
    cos, sin = torch.cos(a), torch.sin(a)
    qr = att._rotate(q.float().view(W, nq, H, d // 2, 2), cos[:nq], sin[:nq]).to(BF).permute(0, 2, 1, 3)
    kr = att._rotate(k.float().view(W, nk, H, d // 2, 2), cos[:nk], sin[:nk]).to(BF).permute(0, 2, 1, 3)
    out = F.scaled_dot_product_attention(qr, kr, heads_first(v, H), scale=d ** -0.5)
    return out.transpose(1, 2).reshape(W, nq, C)


def evaluate(fn, acts, param, tail, wgt, device="cpu", act_dtype=torch.float32, param_dtype=torch.float32, need=(True, True, True, True)):
    """(out, g_q, g_k, g_v, g_param) of fn(q, k, v, param, *tail) with the loss sum(out * wgt); None where `need` is False"""
    leaves = [t.detach().to(device=device, dtype=act_dtype, copy=True).requires_grad_(n) for t, n in zip(acts, need)]
    leaves.append(param.detach().to(device=device, dtype=param_dtype, copy=True).requires_grad_(need[3]))
    out = fn(*leaves, *[t.to(device) for t in tail])
    grads = iter(torch.autograd.grad(out, [t for t, n in zip(leaves, need) if n], wgt.to(device=device, dtype=out.dtype)))
    return (out.detach(), *[next(grads) if n else None for n in need])


@functools.lru_cache(maxsize=None)
def yardsticks(kind, shape, variant="plain"):
    """(acts, param, tail, wgt) on bf16-rounded q, k, v, wgt; the float64 results; e per quantity -- once on the CPU, shared"""
    if kind == "biased":
        q, k, v, param, index, wgt = gpu_biased.make_case(shape, variant)
        tail, f64, own = (index,), att.window_attention_torch, sdpa_biased
    else:
        q, k, v, param, wgt = gpu_rope.make_case(shape, variant)
        tail, f64, own = (), att.window_attention_rope_torch, sdpa_rope
    acts, (wgt,) = rounded(q, k, v), rounded(wgt)
    want = evaluate(f64, acts, param, tail, wgt, act_dtype=torch.float64, param_dtype=torch.float64)
    torch_bf16 = evaluate(own, acts, param, tail, wgt, act_dtype=BF)
    e = [float((a.double() - b).abs().max()) for a, b in zip(torch_bf16, want)]
    return (acts, param, tail, wgt), want, e


def op_of(kind):
    fn = att.window_attention if kind == "biased" else att.window_attention_rope
    return lambda *a: fn(*a, compute="bf16")


def names_of(kind):
    return ("out", "g_q", "g_k", "g_v", "g_table" if kind == "biased" else "g_angles")


def check_case(kind, shape, variant="plain"):
    case, want, e = yardsticks(kind, shape, variant)
    got = evaluate(op_of(kind), *case, device=dev(), act_dtype=BF)
    assert [g.dtype for g in got] == [BF, BF, BF, BF, torch.float32]
    ok = True
    for name, g, w, err in zip(names_of(kind), got, want, e):
        ok &= held(f"bf16 {kind} {shape} {variant} {name}", g, w, err)
    if kind == "biased":
        e_round = float((want[0].to(BF).double() - want[0]).abs().max())
        ok &= held(f"bf16 biased {shape} {variant} out against its own rounding", got[0], want[0], e_round)
        assert bool((got[4][-3:] == 0).all()), "table rows no (i, j) uses must get exactly 0"
    assert ok
    return case, got, want, e


@pytest.mark.parametrize("shape", BIASED_SHAPES, ids=ident)
def test_biased_forward_and_gradients(shape):
    check_case("biased", shape)


@pytest.mark.parametrize("shape", ROPE_SHAPES, ids=ident)
def test_rope_forward_and_gradients(shape):
    check_case("rope", shape)


@pytest.mark.parametrize("variant", ["saturated", "table 50", "zero q"])
def test_biased_numerics(variant):
    check_case("biased", NUMERIC, variant)


@pytest.mark.parametrize("variant", ["saturated", "angles 30", "zero q"])
def test_rope_numerics(variant):
    check_case("rope", NUMERIC, variant)


def selection_case(nk, d, W=2, H=2):
    """keys: per window and head nk distinct rows of +-1; q = 64 k[perm]; the margin of every target score in float64"""
    g = torch.Generator().manual_seed(1000 * nk + d)
    while True:
        k = torch.randint(0, 2, (W, nk, H, d), generator=g).float() * 2 - 1
        if all(torch.unique(k[w, :, h], dim=0).shape[0] == nk for w in range(W) for h in range(H)):
            break
    perm = torch.randperm(nk, generator=g)
    q = 64 * k[:, perm]
    v = torch.randn(W, nk, H * d, generator=g).to(BF)
    s = torch.einsum("wihc,wjhc->whij", q.double(), k.double()) * d ** -0.5
    target = s[:, :, torch.arange(nk), perm]
    s[:, :, torch.arange(nk), perm] = -float("inf")
    margin = float((target - s.max(-1).values).min())
    return q.reshape(W, nk, H * d).to(BF), k.reshape(W, nk, H * d).to(BF), v, perm, margin


@pytest.mark.parametrize("nk,d", SELECT, ids=lambda x: str(x))
def test_exact_selection(nk, d):
    q, k, v, perm, margin = selection_case(nk, d)
    print(f"selection nk {nk} d {d}: margin {margin:.1f}")
    assert margin > 20
    D = dev()
    want = v[:, perm].to(D)
    with torch.no_grad():
        rope = att.window_attention_rope(q.to(D), k.to(D), v.to(D), torch.zeros(2, nk, d // 2, device=D), compute="bf16")
        assert torch.equal(rope, want)
        flat = att.window_attention(q.to(D), k.to(D), v.to(D), torch.zeros(3, 2, device=D), torch.zeros(nk, nk, dtype=torch.int64, device=D), compute="bf16")
        assert torch.equal(flat, want)
        # the biased twin: the index and the bias addressing select, the scores are flat
        table = torch.tensor([[0.0, 0.0], [100.0, 100.0]], device=D)
        index = (torch.arange(nk)[None, :] == perm[:, None]).long().to(D)
        twin = att.window_attention(torch.zeros_like(q).to(D), k.to(D), v.to(D), table, index, compute="bf16")
        assert torch.equal(twin, want)


@pytest.mark.parametrize("kind", ["biased", "rope"])
def test_plumbing(kind):
    shape = (2, 17, 33, 3, 30)
    ((q, k, v), param, tail, wgt), want, e = yardsticks(kind, shape)
    names, op, D = names_of(kind), op_of(kind), dev()
    tail_d = [t.to(D) for t in tail]
    nq, nk, C = 17, 33, 90
    # q / k / v as views of one fused bf16 tensor, grad_out non-contiguous
    fused = torch.zeros(2, nk, 3 * C, device=D, dtype=BF)
    fused[:, :nq, :C], fused[:, :, C:2 * C], fused[:, :, 2 * C:] = q.to(D), k.to(D), v.to(D)
    fused.requires_grad_(True)
    tq, tk, tv = fused[:, :nq, :C], fused[:, :, C:2 * C], fused[:, :, 2 * C:]
    assert not tq.is_contiguous() and not tk.is_contiguous()
    par = param.to(D).requires_grad_(True)
    out = op(tq, tk, tv, par, *tail_d)
    gout = wgt.to(D, BF).transpose(0, 1).contiguous().transpose(0, 1)
    assert not gout.is_contiguous()
    gf, gp = torch.autograd.grad(out, [fused, par], gout)
    assert out.dtype == BF and gf.dtype == BF and gp.dtype == torch.float32
    ok = held(f"bf16 {kind} views out", out, want[0], e[0])
    ok &= held(f"bf16 {kind} views g_q", gf[:, :nq, :C], want[1], e[1]) & held(f"bf16 {kind} views g_k", gf[:, :, C:2 * C], want[2], e[2])
    ok &= held(f"bf16 {kind} views g_v", gf[:, :, 2 * C:], want[3], e[3]) & held(f"bf16 {kind} views {names[4]}", gp, want[4], e[4])
    assert ok and float(gf[:, nq:, :C].abs().max()) == 0.0
    # no_grad forward == training forward, bitwise; two runs bitwise equal (g_table is exempt, as in fp32)
    case = ((q, k, v), param, tail, wgt)
    runs = [evaluate(op, *case, device=D, act_dtype=BF) for _ in range(2)]
    same = 4 if kind == "biased" else 5
    with torch.no_grad():
        plain = op(q.to(D, BF), k.to(D, BF), v.to(D, BF), param.to(D), *tail_d)
    assert torch.equal(plain, runs[0][0]) and torch.equal(plain, out)
    for a, b in zip(runs[0][:same], runs[1][:same]):
        assert torch.equal(a, b)
    # a non-default current stream
    s = torch.cuda.Stream(device=D)
    s.wait_stream(torch.cuda.current_stream(D))
    with torch.cuda.stream(s):
        on_s = evaluate(op, *case, device=D, act_dtype=BF)
    s.synchronize()
    for a, b in zip(on_s[:same], runs[0][:same]):
        assert torch.equal(a, b)
    assert held(f"bf16 {kind} stream {names[4]}", on_s[4], want[4], e[4])
    # only the table / the angles require a gradient
    only = evaluate(op, *case, device=D, act_dtype=BF, need=(False, False, False, True))
    assert only[1] is None and only[2] is None and only[3] is None and torch.equal(only[0], runs[0][0])
    assert torch.equal(only[4], runs[0][4]) if kind == "rope" else held("bf16 biased only g_table", only[4], want[4], e[4])
    # fp32 inputs give the bits of the call on their .bfloat16(); gradients arrive in each input's own dtype
    q32 = torch.randn(2, nq, C, generator=torch.Generator().manual_seed(8)).to(D)
    assert q32.dtype == torch.float32 and not torch.equal(q32.to(BF).float(), q32)
    with torch.no_grad():
        assert torch.equal(op(q32, k.to(D), v.to(D, BF), param.to(D), *tail_d), op(q32.to(BF), k.to(D, BF), v.to(D, BF), param.to(D), *tail_d))
    mixed = evaluate(op, *case, device=D, act_dtype=torch.float32)
    assert [g.dtype for g in mixed] == [BF] + [torch.float32] * 4
    for a, b in zip(mixed[:same], runs[0][:same]):
        assert torch.equal(a.to(BF), b.to(BF))
    # under bf16 autocast: compute="bf16" returns bf16 (with the same bits), the default call still returns fp32
    fp32_op = att.window_attention if kind == "biased" else att.window_attention_rope
    with torch.autocast("cuda", dtype=BF), torch.no_grad():
        cast = op(q.to(D, BF), k.to(D, BF), v.to(D, BF), param.to(D), *tail_d)
        default = fp32_op(q.to(D, BF), k.to(D, BF), v.to(D, BF), param.to(D), *tail_d)
    assert cast.dtype == BF and torch.equal(cast, plain) and default.dtype == torch.float32
    # a bad shape on the device is a ValueError before any launch
    with pytest.raises(ValueError):
        op(q.to(D, BF)[:, :, :60], k.to(D, BF), v.to(D, BF), param.to(D), *tail_d)
    with pytest.raises(ValueError):
        op(q.to(D, BF), k.to(D, BF), v.to(D, BF), param, *tail_d)          # the table / angles on another device
    with pytest.raises(ValueError):
        fp32_op(q.to(D), k.to(D), v.to(D), param.to(D), *tail_d, compute="fp16")


def test_rope_plumbing_of_the_angle_gradient():
    """angle rows past max(nq, nk) are exactly 0; the two-stage angle sum over many windows gives the same bits twice"""
    case, got, want, e = check_case("rope", (2, 17, 33, 3, 30), "extra rows")
    assert got[4].shape[1] == 36 and bool((got[4][:, 33:] == 0).all()) and bool((got[4][:, :33] != 0).any())
    many = yardsticks("rope", (70, 9, 9, 6, 32))[0]
    a, b = (evaluate(op_of("rope"), *many, device=dev(), act_dtype=BF) for _ in range(2))
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def run_amp(mod, m, case, device):
    """mod.run_case with the module's forward under bf16 autocast on `device` (fp32 module, fp32 inputs)"""
    m = m.to(device)
    gs, feat, wgt = (torch.from_numpy(a).to(device) for a in mod.attention_inputs(case))
    gs.requires_grad_(True)
    feat.requires_grad_(True)
    cross = case["kind"] == "cross"
    with torch.autocast(torch.device(device).type, dtype=BF):
        out = m(gs, feat) if cross else m(gs)
    last = m.rope_freqs if hasattr(m, "rope_freqs") else m.relative_position_bias_table
    ps = [m.qhead.weight, m.qhead.bias, m.khead.weight, m.khead.bias, m.vhead.weight, m.vhead.bias, last]
    grads = torch.autograd.grad((out.float() * wgt).sum(), ([gs, feat] if cross else [gs]) + ps)
    names = (["g_gs", "g_feat"] if cross else ["g_gs"]) + ["g_" + p for p in mod.PARAMS]
    return out.dtype, dict(out=out.detach(), **dict(zip(names, grads)))


@functools.lru_cache(maxsize=None)
def module_yardsticks(kind, name):
    mod = cpu_rope if kind == "rope" else cpu_biased
    m, data = mod.load_golden(name)
    case = mod.GOLDEN_CASES[name]
    want = mod.run_case(copy.deepcopy(m), case, dtype=torch.float64)
    _, amp = run_amp(mod, copy.deepcopy(m), case, "cpu")
    return mod, m, case, want, {k: float((amp[k].double() - want[k]).abs().max()) for k in want}


@pytest.mark.parametrize("kind,name", [(kind, name) for kind in ("rope", "biased") for name in cpu_rope.GOLDEN_CASES])
def test_goldens_through_use_hip_attention(kind, name):
    """the switched module under bf16 autocast against the float64 module; e = the unswitched module under CPU bf16 autocast"""
    mod, m, case, want, e = module_yardsticks(kind, name)
    sw = copy.deepcopy(m)
    assert att.use_hip_attention(sw, compute="bf16") == 1
    dtype, got = run_amp(mod, sw, case, dev())
    assert dtype == BF
    assert all([held(f"bf16 {kind} {name} gpu {k}", got[k], want[k], e[k]) for k in want])
    # an fp32 model outside autocast keeps working, with fp32 results
    sw32 = copy.deepcopy(m).to(dev())
    att.use_hip_attention(sw32, compute="bf16")
    gs = torch.from_numpy(mod.attention_inputs(case)[0]).to(dev())
    with torch.no_grad():
        assert (sw32(gs, gs) if case["kind"] == "cross" else sw32(gs)).dtype == torch.float32
