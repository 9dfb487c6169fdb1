"""The decoder's window attention (gsasr_amd.window_attention / use_hip_attention / attention.constant_key_attention;
gsasr_window_attn_forward / _backward): what can be checked without a GPU -- the torch expression that is the op's contract and
its CPU path against the reference's modules (tests/golden/attention_*.npz, written by tests/golden/make_golden_attention.py),
the argument errors, the constant-key helper against nn.MultiheadAttention, the ABI surface.  tests/test_window_attention_gpu.py
has the kernels.

The bar of every fp32 result (`bar`, the form of tests/test_ssim_loss.py): its error against the float64 evaluation of the torch
expression on the same input may be 4 x the error of the fp32 torch expression against that float64 value (e32) plus 1e-6 of
the quantity's max-abs.  The factor covers another summation order over at most 256 terms; it cannot hide a wrong term (zeroing
one key's value moves the output by 0.14-0.36 on these inputs, the bar is about 3e-6).  Every check prints its ratio to the bar."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

from gsasr_amd import _cabi, build
from gsasr_amd import attention as att

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
WINDOWS = 2
GOLDEN_CASES = {      # the reference's GSSelfAttn / WindowCrossAttn: d = 30 on 12 x 12 tokens, d = 32 on 16 x 16
    "self_12": dict(kind="self", dim=60, heads=2, side=12, seed=11),
    "self_16": dict(kind="self", dim=64, heads=2, side=16, seed=12),
    "cross_12": dict(kind="cross", dim=60, heads=2, side=12, seed=13),
    "cross_16": dict(kind="cross", dim=64, heads=2, side=16, seed=14),
}
PARAMS = ("qhead_weight", "qhead_bias", "khead_weight", "khead_bias", "vhead_weight", "vhead_bias", "table")


def attention_inputs(case):
    """(gs, feat, loss weights) of a golden case, fp32 [2, side^2, dim] each, from its NumPy seed"""
    rng = np.random.default_rng(1000 + case["seed"])
    shape = (WINDOWS, case["side"] ** 2, case["dim"])
    return tuple(rng.standard_normal(shape).astype(np.float32) for _ in range(3))


def bar(e32, scale):
    return 4.0 * e32 + 1e-6 * scale


def held(what, got, want, e32):
    """print the ratio of |got - want| to the bar and return whether it is held (`want` float64, `e32` a tensor's error)"""
    err = float((got.detach().cpu().double() - want).abs().max())
    b = bar(e32, float(want.abs().max()))
    print(f"{what}: err {err:.3e}, e32 {e32:.3e}, ratio to the bar {err / b if b > 0 else 0.0:.3f}")
    return err <= b


class StandIn(nn.Module):
    """a module with the attribute names of the reference's attention modules (own code): forward = the three Linears, the
    torch expression and proj; `use_hip_attention` replaces it"""

    def __init__(self, dim, heads, table_rows, index):
        super().__init__()
        self.num_heads, self.scale = heads, (dim // heads) ** -0.5
        self.qhead, self.khead, self.vhead, self.proj = (nn.Linear(dim, dim) for _ in range(4))
        self.relative_position_bias_table = nn.Parameter(torch.zeros(table_rows, heads))
        self.register_buffer("relative_position_index", index)

    def forward(self, gs, feat=None):
        src = gs if feat is None else feat
        return self.proj(att.window_attention_torch(self.qhead(gs), self.khead(src), self.vhead(src), self.relative_position_bias_table,
                                                    self.relative_position_index, self.scale))


def load_golden(name):
    """(stand-in module with the golden's weights, the file's arrays)"""
    data = np.load(os.path.join(GOLDEN, f"attention_{name}.npz"))
    case = GOLDEN_CASES[name]
    m = StandIn(case["dim"], case["heads"], data["table"].shape[0], torch.from_numpy(data["index"].astype(np.int64)))
    with torch.no_grad():
        for lin in ("qhead", "khead", "vhead", "proj"):
            getattr(m, lin).weight.copy_(torch.from_numpy(data[lin + "_weight"]))
            getattr(m, lin).bias.copy_(torch.from_numpy(data[lin + "_bias"]))
        m.relative_position_bias_table.copy_(torch.from_numpy(data["table"]))
    return m, data


def run_case(m, case, device="cpu", dtype=torch.float32):
    """{out, g_gs, [g_feat,] g_<parameter>...} of module `m` (moved to device / dtype) on the case's inputs"""
    m = m.to(device=device, dtype=dtype)
    gs, feat, wgt = (torch.from_numpy(a).to(device=device, dtype=dtype) for a in attention_inputs(case))
    gs.requires_grad_(True)
    feat.requires_grad_(True)
    cross = case["kind"] == "cross"
    out = m(gs, feat) if cross else m(gs)
    ps = [m.qhead.weight, m.qhead.bias, m.khead.weight, m.khead.bias, m.vhead.weight, m.vhead.bias, m.relative_position_bias_table]
    grads = torch.autograd.grad((out * wgt).sum(), ([gs, feat] if cross else [gs]) + ps)
    names = (["g_gs", "g_feat"] if cross else ["g_gs"]) + ["g_" + p for p in PARAMS]
    return dict(out=out.detach(), **dict(zip(names, grads)))


def golden_yardsticks(name):
    """(module, arrays, float64 results, e32 per quantity) -- the float64 and fp32 evaluations of the torch expression"""
    m, data = load_golden(name)
    case = GOLDEN_CASES[name]
    want = run_case(copy.deepcopy(m), case, dtype=torch.float64)
    f32 = run_case(copy.deepcopy(m), case)
    e32 = {k: float((f32[k].double() - want[k]).abs().max()) for k in want}
    return m, data, want, e32


@pytest.mark.parametrize("name", list(GOLDEN_CASES))
def test_goldens_on_cpu(name):
    m, data, want, e32 = golden_yardsticks(name)
    case = GOLDEN_CASES[name]
    if case["kind"] == "cross":     # (the cross module's index leaves the table's last rows unused: they are part of the fixture)
        assert int(data["index"].max()) == {12: 506, 16: 930}[case["side"]] and data["table"].shape[0] == {12: 529, 16: 961}[case["side"]]
    ok = True
    # the reference's own fp32 numbers are an fp32 evaluation of the same expression: held to the same bar
    for k in want:
        ok &= held(f"{name} reference {k}", torch.from_numpy(data[k]), want[k], e32[k])
    # the switched module on CPU tensors
    sw = copy.deepcopy(m)
    assert att.use_hip_attention(sw) == 1
    got = run_case(sw, case)
    for k in want:
        ok &= held(f"{name} switched {k}", got[k], want[k], e32[k])
    assert ok
    assert [k for k, _ in sw.state_dict().items()] == [k for k, _ in m.state_dict().items()]


def _args(W=2, nq=5, nk=7, H=2, d=3, T=11, C=None):
    C = H * d if C is None else C
    g = torch.Generator().manual_seed(3)
    return [torch.randn(W, nq, C, generator=g), torch.randn(W, nk, C, generator=g), torch.randn(W, nk, C, generator=g),
            torch.randn(T, H, generator=g), torch.randint(0, T, (nq, nk), generator=g)]


def test_cpu_path_is_the_expression():
    a = _args()
    assert torch.equal(att.window_attention(*a), att.window_attention_torch(*a))
    import gsasr_amd
    assert gsasr_amd.window_attention is att.window_attention and gsasr_amd.use_hip_attention is att.use_hip_attention


@pytest.mark.parametrize("what", ["nq 257", "nk 257", "d 33", "channels", "index range", "index negative", "index float", "table width", "index shape"])
def test_argument_errors(what):
    a = _args()
    if what == "nq 257":
        a = _args(nq=257)
    elif what == "nk 257":
        a = _args(nk=257)
    elif what == "d 33":
        a = _args(d=33)
    elif what == "channels":
        a = _args(C=7)
    elif what == "index range":
        a[4][2, 3] = 11
    elif what == "index negative":
        a[4][0, 0] = -1
    elif what == "index float":
        a[4] = a[4].float()
    elif what == "table width":
        a[3] = torch.randn(11, 4)
    elif what == "index shape":
        a[4] = a[4].t().contiguous()
    with pytest.raises(ValueError):
        att.window_attention(*a)


def test_limits_are_admitted_on_cpu():
    a = _args(W=1, nq=256, nk=256, H=1, d=32, T=5)
    assert att.window_attention(*a).shape == (1, 256, 32)


def test_index_is_checked_once_per_tensor():
    a = _args()
    att.window_attention(*a)
    entry = att._INDEX_CACHE[id(a[4])]
    att.window_attention(*a)
    assert att._INDEX_CACHE[id(a[4])] is entry          # the cached int32 copy served the second call
    a[4][0, 0] = 99                                      # an in-place change is a new version: checked again
    with pytest.raises(ValueError):
        att.window_attention(*a)


def test_gradcheck_of_the_expression():
    g = torch.Generator().manual_seed(5)
    W, n, H, d, T = 2, 5, 2, 3, 9
    q, k, v = (torch.randn(W, n, H * d, dtype=torch.float64, generator=g).requires_grad_(True) for _ in range(3))
    table = torch.randn(T, H, dtype=torch.float64, generator=g).requires_grad_(True)
    index = torch.randint(0, T, (n, n), generator=g)
    assert torch.autograd.gradcheck(lambda *t: att.window_attention_torch(*t, index), (q, k, v, table))
    assert torch.autograd.gradcheck(lambda *t: att.window_attention(*t, index, 0.7), (q, k, v, table))


def test_constant_key_attention_is_the_mha_on_repeated_keys():
    torch.manual_seed(7)
    B, n, c, heads = 3, 10, 24, 4
    mha = nn.MultiheadAttention(c, heads, batch_first=True)
    with torch.no_grad():
        mha.in_proj_bias.normal_()
        mha.out_proj.bias.normal_()
    x, row, wgt = torch.randn(B, n, c), torch.randn(B, 1, c), torch.randn(B, n, c)
    ps = [mha.in_proj_weight, mha.in_proj_bias, mha.out_proj.weight, mha.out_proj.bias]

    def both(dtype):
        m = copy.deepcopy(mha).to(dtype)
        p = [m.in_proj_weight, m.in_proj_bias, m.out_proj.weight, m.out_proj.bias]
        r = row.to(dtype).requires_grad_(True)
        xx = x.to(dtype).requires_grad_(True)
        keys = r.expand(B, n, c)
        full = m(xx, keys, keys, need_weights=False)[0]
        g_full = torch.autograd.grad((full * wgt.to(dtype)).sum(), p + [r, xx])
        short = att.constant_key_attention(m, r)
        assert short.shape == (B, 1, c)
        g_short = torch.autograd.grad((short.expand(B, n, c) * wgt.to(dtype)).sum(), p + [r])
        return [full.detach()] + list(g_full), [short.expand(B, n, c).detach()] + list(g_short)

    want, _ = both(torch.float64)
    f32, got = both(torch.float32)
    assert float(want[-1].abs().max()) <= 1e-12         # the query gets no gradient: the softmax over identical keys is flat
    ok = True
    for name, w, f, g in zip(("out", "in_proj_weight", "in_proj_bias", "out_proj.weight", "out_proj.bias", "row"), want, f32, got):
        ok &= held(f"constant key {name}", g, w, float((f.double() - w).abs().max()))
    assert ok
    assert len(ps) == 4
    # the query rows of in_proj (q, k) get no gradient from the helper and an (almost) zero one from the module
    assert float(got[1][: 2 * c].abs().max()) == 0.0 and float(want[1][: 2 * c].abs().max()) <= 1e-12
    assert att.constant_key_attention(mha, row[:, 0]).shape == (B, 1, c)
    for bad in (nn.MultiheadAttention(c, heads), nn.MultiheadAttention(c, heads, batch_first=True, dropout=0.1),
                nn.MultiheadAttention(c, heads, batch_first=True, add_bias_kv=True)):
        with pytest.raises(ValueError):
            att.constant_key_attention(bad, row)


def test_c5_decoder_keeps_its_default_and_shares_weights_between_modes():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import c5_models
    torch.manual_seed(0)
    kw = dict(inchannel=8, channel=12, heads=2, window=4, cross_layers=2, self_blocks=1, self_layers=2)
    a = c5_models.Fea2GSDecoder(**kw)
    b = c5_models.Fea2GSDecoder(**kw, attention="hip", scale_attention="constant")
    assert list(a.state_dict()) == list(b.state_dict())
    b.load_state_dict(a.state_dict())
    feat, scale = torch.randn(2, 8, 8, 4), torch.tensor([2.0, 3.0])
    ya, yb = a(feat, scale), b(feat, scale)        # (on CPU tensors "hip" is the torch expression)
    assert float((ya - yb).detach().abs().max()) <= 1e-4 * float(ya.detach().abs().max())
    with pytest.raises(ValueError):
        c5_models.Fea2GSDecoder(**kw, attention="other")


def test_abi_surface_of_the_attention_part():
    hdr = open(os.path.join(ROOT, "include", "gsasr_splat.h")).read()
    assert re.search(r"#define\s+GSASR_SPLAT_ABI_VERSION\s+7\b", hdr)
    bare = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(gsasr_[a-z_0-9]+)\s*\(", bare))
    L = ctypes.CDLL(_cabi.LIB_PATH)
    for name in ("gsasr_window_attn_scratch_bytes", "gsasr_window_attn_forward", "gsasr_window_attn_backward"):
        assert name in declared and name in _cabi.EXPORTS and hasattr(L, name), name
    assert declared == set(_cabi.EXPORTS), declared ^ set(_cabi.EXPORTS)
    assert _cabi.lib().gsasr_abi_version() == 7
    assert "splat_attn" in build.PARTS
    assert '#include "splat_attn.hip"' in open(os.path.join(ROOT, "gsasr_amd", "csrc", "gsasr_splat.hip")).read()
    for field in ("windows", "heads", "nq", "nk", "head_dim", "table_rows", "scale", "flags", "q", "k", "v", "table", "index", "out",
                  "stats", "grad_out", "g_q", "g_k", "g_v", "g_table", "scratch"):
        assert field in [f for f, _ in _cabi.WindowAttn._fields_], field


def test_descriptor_checks_come_before_any_launch():
    """gsasr_window_attn_scratch_bytes is 0 and the entry points return GSASR_ERR_ARG on a bad descriptor (no GPU is touched)"""
    lib = _cabi.lib()
    good = _cabi.make_window_attn(2, 6, 144, 144, 30, 529, 30 ** -0.5)
    assert lib.gsasr_window_attn_scratch_bytes(ctypes.byref(good)) > 0
    good.g_table = 256          # (any non-null address: only looked at, never dereferenced here)
    assert lib.gsasr_window_attn_scratch_bytes(ctypes.byref(good)) >= 2 * 6 * 529 * 4
    for field, value in (("nq", 257), ("nk", 0), ("head_dim", 33), ("head_dim", 0), ("windows", 0), ("heads", 0), ("table_rows", 0), ("flags", 1)):
        d = _cabi.make_window_attn(2, 6, 144, 144, 30, 529, 30 ** -0.5)
        setattr(d, field, value)
        assert lib.gsasr_window_attn_scratch_bytes(ctypes.byref(d)) == 0, field
        assert lib.gsasr_window_attn_forward(ctypes.byref(d), None) != 0, field
        assert lib.gsasr_window_attn_backward(ctypes.byref(d), None) != 0, field
    d = _cabi.make_window_attn(2, 6, 144, 144, 30, 529, 30 ** -0.5)      # valid sizes, null pointers
    assert lib.gsasr_window_attn_forward(ctypes.byref(d), None) != 0
    assert lib.gsasr_window_attn_backward(ctypes.byref(d), None) != 0
