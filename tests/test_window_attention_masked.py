"""The masked family of the window attention (gsasr_amd.window_attention(..., mask=), window_attention_qkv, use_hip_attention on
a Swin encoder's modules; gsasr_window_attn_masked / _masked_bf16): what can be checked without a GPU -- the torch forms against
the reference's SwinIR WindowAttention inside a shifted and a plain SwinTransformerBlock (tests/golden/attention_swin_8_*.npz,
written by tests/golden/make_golden_attention_swin.py), the module switch, the argument errors, what the six C entry points say
to a bad descriptor (return code and the exact bytes of gsasr_last_error(); every such call fails before any launch), the ABI
surface.  tests/test_window_attention_masked_gpu.py and tests/test_window_attention_masked_bf16_gpu.py have the kernels.

The bar is `held()` of tests/test_window_attention.py: 4 x e32 + 1e-6 x max-abs against the float64 evaluation of the torch form,
e32 the fp32 torch form's own error on the same input.  Every check prints its ratio."""
import copy
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

from gsasr_amd import _cabi
from gsasr_amd import attention as att
from test_window_attention import held

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
# the reference's SwinTransformerBlock(dim, input_resolution=(16, 16), num_heads, window_size, shift_size): 2 samples x 4 windows
SWIN_CASES = {
    "swin_8_shift": dict(dim=60, heads=2, window=8, shift=4, seed=21),
    "swin_8_plain": dict(dim=60, heads=2, window=8, shift=0, seed=22),
}
SAMPLES, WINDOWS_PER_SAMPLE = 2, 4
PARAMS = ("qkv_weight", "qkv_bias", "table")


def swin_inputs(case):
    """(x, loss weights) of a golden case, fp32 [8, window^2, dim] each, from its NumPy seed"""
    rng = np.random.default_rng(1000 + case["seed"])
    shape = (SAMPLES * WINDOWS_PER_SAMPLE, case["window"] ** 2, case["dim"])
    return tuple(rng.standard_normal(shape).astype(np.float32) for _ in range(2))


class SwinStandIn(nn.Module):
    """a module with the attribute names of SwinIR's WindowAttention (own code): forward(x, mask=None) = the packed Linear, the
    torch form, proj, proj_drop; `use_hip_attention` replaces it"""

    def __init__(self, dim, heads, table_rows, index, attn_drop=0.0):
        super().__init__()
        self.num_heads, self.scale = heads, (dim // heads) ** -0.5
        self.qkv, self.proj = nn.Linear(dim, 3 * dim), nn.Linear(dim, dim)
        self.attn_drop, self.proj_drop = nn.Dropout(attn_drop), nn.Dropout(0.0)
        self.relative_position_bias_table = nn.Parameter(torch.zeros(table_rows, heads))
        self.register_buffer("relative_position_index", index)

    def forward(self, x, mask=None):
        y = att.window_attention_qkv_torch(self.qkv(x), self.relative_position_bias_table, self.relative_position_index, self.scale, mask)
        return self.proj_drop(self.proj(y))


def load_golden(name):
    """(stand-in module with the golden's weights, the file's arrays, the block's mask or None)"""
    data = np.load(os.path.join(GOLDEN, f"attention_{name}.npz"))
    case = SWIN_CASES[name]
    m = SwinStandIn(case["dim"], case["heads"], data["table"].shape[0], torch.from_numpy(data["index"].astype(np.int64)))
    with torch.no_grad():
        for lin in ("qkv", "proj"):
            getattr(m, lin).weight.copy_(torch.from_numpy(data[lin + "_weight"]))
            getattr(m, lin).bias.copy_(torch.from_numpy(data[lin + "_bias"]))
        m.relative_position_bias_table.copy_(torch.from_numpy(data["table"]))
    return m, data, torch.from_numpy(data["mask"]) if "mask" in data else None


def run_case(m, case, mask, device="cpu", dtype=torch.float32):
    """{out, g_x, g_qkv_weight, g_qkv_bias, g_table} of module `m` (moved to device / dtype) on the case's inputs"""
    m = m.to(device=device, dtype=dtype)
    x, wgt = (torch.from_numpy(a).to(device=device, dtype=dtype) for a in swin_inputs(case))
    x.requires_grad_(True)
    out = m(x, None if mask is None else mask.to(device=device, dtype=dtype))
    grads = torch.autograd.grad((out * wgt).sum(), [x, m.qkv.weight, m.qkv.bias, m.relative_position_bias_table])
    return dict(out=out.detach(), **dict(zip(["g_x"] + ["g_" + p for p in PARAMS], grads)))


def golden_yardsticks(name):
    """(module, arrays, mask, float64 results, e32 per quantity) -- the float64 and fp32 evaluations of the torch form"""
    m, data, mask = load_golden(name)
    case = SWIN_CASES[name]
    want = run_case(copy.deepcopy(m), case, mask, dtype=torch.float64)
    f32 = run_case(copy.deepcopy(m), case, mask)
    return m, data, mask, want, {k: float((f32[k].double() - want[k]).abs().max()) for k in want}


@pytest.mark.parametrize("name", list(SWIN_CASES))
def test_goldens_on_cpu(name):
    m, data, mask, want, e32 = golden_yardsticks(name)
    case = SWIN_CASES[name]
    assert (mask is not None) == (case["shift"] > 0)
    if mask is not None:        # the block's own mask: 0 / -100, every row keeps a 0, symmetric in (i, j)
        assert tuple(mask.shape) == (4, 64, 64) and sorted(mask.unique().tolist()) == [-100.0, 0.0]
        assert bool((mask.max(-1).values == 0).all()) and torch.equal(mask, mask.transpose(1, 2))
    assert data["table"].shape == (225, 2) and int(data["index"].max()) == 224
    ok = True
    # the reference's own fp32 numbers are an fp32 evaluation of the same expression: held to the same bar
    for k in want:
        ok &= held(f"{name} reference {k}", torch.from_numpy(data[k]), want[k], e32[k])
    # the switched module on CPU tensors
    sw = copy.deepcopy(m)
    assert att.use_hip_attention(sw) == 1
    got = run_case(sw, case, mask)
    for k in want:
        ok &= held(f"{name} switched {k}", got[k], want[k], e32[k])
    assert ok
    assert list(sw.state_dict()) == list(m.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(sw.state_dict().values(), m.state_dict().values()))


def test_the_switch_counts_every_kind_and_leaves_attention_dropout_alone():
    from test_window_attention import StandIn
    index = torch.zeros(4, 4, dtype=torch.int64)
    net = nn.ModuleList([SwinStandIn(8, 2, 5, index), SwinStandIn(8, 2, 5, index, attn_drop=0.1), StandIn(8, 2, 5, index)])
    before = [m.forward.__func__ for m in net]
    assert att.use_hip_attention(net) == 2
    after = [m.forward.__func__ for m in net]
    assert after[0] is att._swin_module_forward and after[1] is before[1] and after[2] is att._module_forward
    assert att.use_hip_attention(net, compute="bf16") == 2 and net[0].forward.__func__ is att._swin_module_forward_bf16
    # a new mask tensor on every call: nothing is keyed on its identity
    x = torch.randn(4, 4, 8)
    for _ in range(2):
        mask = torch.where(torch.rand(2, 4, 4) < 0.3, -100.0, 0.0)
        mask[:, torch.arange(4), torch.arange(4)] = 0
        att.use_hip_attention(net)
        want = net[0].proj(att.window_attention_qkv_torch(net[0].qkv(x), net[0].relative_position_bias_table, index, net[0].scale, mask))
        assert torch.equal(net[0](x, mask), want)
        assert torch.equal(net[0](x, mask=mask.clone()), want)


def _args(W=4, n=5, H=2, d=3, T=11, nW=2):
    g = torch.Generator().manual_seed(3)
    return dict(qkv=torch.randn(W, n, 3 * H * d, generator=g), table=torch.randn(T, H, generator=g),
                index=torch.randint(0, T, (n, n), generator=g), mask=3 * torch.randn(nW, n, n, generator=g))


def test_the_packed_form_is_the_split_form():
    a = _args()
    C = 6
    q, k, v = a["qkv"][..., :C], a["qkv"][..., C:2 * C], a["qkv"][..., 2 * C:]
    for mask in (None, a["mask"]):
        want = att.window_attention_torch(q, k, v, a["table"], a["index"], None, mask)
        assert torch.equal(att.window_attention_qkv_torch(a["qkv"], a["table"], a["index"], None, mask), want)
        assert torch.equal(att.window_attention_qkv(a["qkv"], a["table"], a["index"], mask=mask), want)
        assert torch.equal(att.window_attention(q, k, v, a["table"], a["index"], mask=mask), want)
        bf = att.window_attention_bf16_torch(q, k, v, a["table"], a["index"], None, mask)
        assert bf.dtype == torch.bfloat16 and torch.equal(att.window_attention_qkv(a["qkv"], a["table"], a["index"], compute="bf16", mask=mask), bf)
    # the mask follows the window modulo nW, in torch's order (bias first), and is not the transposed one
    H, d, n, W = 2, 3, 5, 4
    heads = lambda t: t.reshape(W, n, H, d).permute(0, 2, 1, 3)      # noqa: E731
    attn = (heads(q) * d ** -0.5) @ heads(k).transpose(-2, -1) + a["table"][a["index"]].permute(2, 0, 1)
    attn = attn.view(W // 2, 2, H, n, n) + a["mask"].unsqueeze(1).unsqueeze(0)
    ref = (torch.softmax(attn.view(-1, H, n, n), -1) @ heads(v)).transpose(1, 2).reshape(W, n, H * d)
    assert torch.equal(att.window_attention_qkv_torch(a["qkv"], a["table"], a["index"], None, a["mask"]), ref)
    import gsasr_amd
    assert gsasr_amd.window_attention_qkv is att.window_attention_qkv and gsasr_amd.window_attention_qkv_torch is att.window_attention_qkv_torch


def test_gradcheck_of_the_masked_form():
    a = _args()
    qkv, table = a["qkv"].double().requires_grad_(True), a["table"].double().requires_grad_(True)
    mask = a["mask"].double()
    assert torch.autograd.gradcheck(lambda x, t: att.window_attention_qkv(x, t, a["index"], 0.7, mask=mask), (qkv, table))


ARGUMENT_ERRORS = ["mask rank", "mask shape", "mask device", "mask integer", "windows not a multiple", "mask requires grad", "qkv width", "qkv rank",
                   "index shape", "n 257"]


@pytest.mark.parametrize("what", ARGUMENT_ERRORS)
def test_argument_errors(what):
    a = _args()
    C = 6
    if what == "mask rank":
        a["mask"] = a["mask"][0]
    elif what == "mask shape":
        a["mask"] = a["mask"][:, :, :4]
    elif what == "mask device":
        a["mask"] = a["mask"].to("meta")
    elif what == "mask integer":
        a["mask"] = a["mask"].long()
    elif what == "windows not a multiple":
        a["mask"] = torch.zeros(3, 5, 5)
    elif what == "mask requires grad":
        a["mask"].requires_grad_(True)
    elif what == "qkv width":
        a["qkv"] = a["qkv"][..., :16]        # not a multiple of 3 * H
    elif what == "qkv rank":
        a["qkv"] = a["qkv"][0]
    elif what == "index shape":
        a["index"] = a["index"][:4]
    elif what == "n 257":
        a = _args(n=257, W=2, nW=1)
    with pytest.raises(ValueError):
        att.window_attention_qkv(a["qkv"], a["table"], a["index"], mask=a["mask"])
    if what.startswith("mask") or what == "windows not a multiple":
        with pytest.raises(ValueError):
            att.window_attention(a["qkv"][..., :C], a["qkv"][..., C:2 * C], a["qkv"][..., 2 * C:], a["table"], a["index"], mask=a["mask"])


# ---- the C entry points on a bad descriptor ------------------------------------------------------------------------
ERR_ARG = -1
W, H, NQ, NK, D, ROWS, NW = 4, 3, 20, 36, 8, 97, 2
BASE = 0x10000
STEMS = {"masked": ("gsasr_window_attn_masked", False), "masked_bf16": ("gsasr_window_attn_masked_bf16", True)}
POINTERS = ("q", "k", "v", "table", "index", "out", "stats", "grad_out", "g_q", "g_k", "g_v", "g_table", "scratch", "mask")
PITCHES = ("pitch_q", "pitch_k", "pitch_v", "pitch_gq", "pitch_gk", "pitch_gv")
REQUIRED = {"forward": ("q", "k", "v", "table", "index", "out"), "backward": ("q", "k", "v", "table", "index", "out", "stats", "grad_out")}
M_MISSING = {"forward": b"null q, k, v, table, index or out pointer", "backward": b"null q, k, v, table, index, out, stats or grad_out pointer"}
M_ALIGN = {"forward": (("q", "k", "v", "out"), b"q, k, v and out must be 2-byte aligned"),
           "backward": (("q", "k", "v", "out", "grad_out", "g_q", "g_k", "g_v"), b"q, k, v, out, grad_out, g_q, g_k and g_v must be 2-byte aligned")}
M_NEG, M_MULT = b"mask_windows must not be negative", b"windows must be a multiple of mask_windows"
M_PAIR, M_PITCH = b"mask and mask_windows must be set together (NULL and 0: no mask)", b"a non-zero pitch must be at least heads * head_dim"
SIZE_DEFECTS = [        # the biased family's, then the family's own: every entry point reports them
    ("windows 0", dict(windows=0), b"windows and heads must be at least 1"), ("heads 0", dict(heads=0), b"windows and heads must be at least 1"),
    ("nq 257", dict(nq=257), b"need 1 <= nq, nk <= 256"), ("nk 0", dict(nk=0), b"need 1 <= nq, nk <= 256"),
    ("head_dim 33", dict(head_dim=33), b"need 1 <= head_dim <= 32"), ("head_dim 0", dict(head_dim=0), b"need 1 <= head_dim <= 32"),
    ("table_rows 0", dict(table_rows=0), b"table_rows must be at least 1"), ("flags", dict(flags=1), b"unknown flags (none are defined)"),
    ("NaN scale", dict(scale=math.nan), b"scale is NaN"),
    ("windows * heads", dict(windows=65536, heads=32768, **{p: 0 for p in ("pitch_q", "pitch_k", "pitch_v", "pitch_gq", "pitch_gk", "pitch_gv")}),
     b"windows * heads or table_rows * heads exceeds 2^31 - 1"),
    ("mask_windows -1", dict(mask_windows=-1), M_NEG), ("windows 4, mask_windows 3", dict(mask_windows=3), M_MULT),
    ("windows 2, mask_windows 4", dict(windows=2, mask_windows=4), M_MULT),
] + [(f"{p} short", {p: H * D - 1}, M_PITCH) for p in PITCHES] + [(f"{p} negative", {p: -1}, M_PITCH) for p in PITCHES[:1]]


def make(bf16, pointers=True, **fields):
    d = _cabi.make_window_attn_masked(W, H, NQ, NK, D, ROWS, D ** -0.5, bf16=bf16, mask_windows=NW, pitches=(3 * H * D,) * 3, grad_pitches=(3 * H * D,) * 3)
    if pointers:
        for i, p in enumerate(POINTERS):
            setattr(d, p, BASE + 256 * i)
    for f, value in fields.items():
        setattr(d, f, value)
    return d


def call(stem, what, d):
    lib = _cabi.lib()
    ref = None if d is None else ctypes.byref(d)
    rc = getattr(lib, f"{stem}_{what}")(ref) if what == "scratch_bytes" else getattr(lib, f"{stem}_{what}")(ref, None)
    return rc, lib.gsasr_last_error()


def refused(stem, what, d, msg, case):
    rc, said = call(stem, what, d)
    assert rc == (0 if what == "scratch_bytes" else ERR_ARG), (case, what, rc)
    assert said == msg, (case, what, said)


@pytest.mark.parametrize("family", list(STEMS))
def test_descriptor_defects_are_refused_by_all_three_entry_points(family):
    stem, bf16 = STEMS[family]
    for what in ("scratch_bytes", "forward", "backward"):
        refused(stem, what, None, b"null window-attention descriptor", "null descriptor")
        for case, change, msg in SIZE_DEFECTS:
            refused(stem, what, make(bf16, **change), msg, case)
        assert call(stem, "scratch_bytes", make(bf16))[0] >= 256 + W * H * ROWS * 4


@pytest.mark.parametrize("family", list(STEMS))
def test_descriptor_pointers_are_refused_in_turn(family):
    stem, bf16 = STEMS[family]
    for what in ("forward", "backward"):
        for p in REQUIRED[what]:
            refused(stem, what, make(bf16, **{p: None}), M_MISSING[what], "no " + p)
        refused(stem, what, make(bf16, mask=None), M_PAIR, "mask_windows without mask")
        refused(stem, what, make(bf16, mask_windows=0), M_PAIR, "mask without mask_windows")
        refused(stem, what, make(bf16, mask=None, q=None), M_MISSING[what], "a missing pointer comes first")
        if bf16:
            names, msg = M_ALIGN[what]
            for p in names:
                d = make(bf16)
                setattr(d, p, getattr(d, p) + 1)
                refused(stem, what, d, msg, "misaligned " + p)
    # the scratch of the table gradient, as in the biased family
    refused(stem, "backward", make(bf16, scratch=None), b"null scratch pointer (the table gradient needs gsasr_window_attn_scratch_bytes)", "no scratch")
    # no mask at all and zero pitches (contiguous) are a valid descriptor: scratch_bytes looks at no pointer but g_table
    assert call(stem, "scratch_bytes", make(bf16, pointers=False, mask_windows=0, **{p: 0 for p in PITCHES}))[0] == 256


def test_abi_surface_of_the_masked_family():
    hdr = open(os.path.join(ROOT, "include", "gsasr_splat.h")).read()
    assert re.search(r"#define\s+GSASR_SPLAT_ABI_VERSION\s+7\b", hdr)
    bare = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(gsasr_[a-z_0-9]+)\s*\(", bare))
    L = ctypes.CDLL(_cabi.LIB_PATH)
    for stem, _ in STEMS.values():
        for what in ("scratch_bytes", "forward", "backward"):
            name = f"{stem}_{what}"
            assert name in declared and name in _cabi.EXPORTS and hasattr(L, name), name
    assert declared == set(_cabi.EXPORTS), declared ^ set(_cabi.EXPORTS)
    assert _cabi.lib().gsasr_abi_version() == 7
    # the structs: the biased descriptor's fields, then the mask and the pitches, in the header's order and in both element types
    fields = [f for f, _ in _cabi.WindowAttnMasked._fields_]
    assert fields == [f for f, _ in _cabi.WindowAttn._fields_] + ["mask", "mask_windows", *PITCHES]
    assert [f for f, _ in _cabi.WindowAttnMaskedBf16._fields_] == fields
    for name in ("gsasr_window_attn_masked", "gsasr_window_attn_masked_bf16"):
        body = re.search(r"typedef struct " + name + r" \{(.*?)\} " + name + ";", bare, flags=re.S).group(1)
        order = re.findall(r"\b([a-z_]+)\s*[,;]", body)
        assert order == fields, (name, order)


def test_swin_shaped_stack_modes_share_weights_and_agree_on_cpu():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import c5_models
    torch.manual_seed(0)
    kw = dict(dim=12, heads=2, window=4, layers=4)
    a, b = c5_models.SwinShapedStack(**kw), c5_models.SwinShapedStack(**kw, attention="hip")
    assert list(a.state_dict()) == list(b.state_dict())
    b.load_state_dict(a.state_dict())
    assert [layer.shift for layer in a.layers] == [0, 2, 0, 2]
    mask = a.layers[1].region_mask(8, 8, "cpu")
    assert tuple(mask.shape) == (4, 16, 16) and sorted(mask.unique().tolist()) == [-100.0, 0.0] and bool((mask.max(-1).values == 0).all())
    assert float(mask[0].abs().max()) == 0.0 and float(mask[3].abs().max()) == 100.0       # only windows the shift cuts are masked
    x = torch.randn(2, 8, 8, 12)
    ya, yb = a(x), b(x)         # (on CPU tensors "hip" is the torch form)
    assert float((ya - yb).detach().abs().max()) <= 1e-5 * float(ya.detach().abs().max())
    with pytest.raises(ValueError):
        c5_models.SwinShapedStack(**kw, attention="other")
