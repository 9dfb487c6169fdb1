"""The bf16 mode of the two window attentions (window_attention / window_attention_rope with compute="bf16",
use_hip_attention(model, compute="bf16"); gsasr_window_attn_bf16_* and gsasr_window_attn_rope_bf16_*): what can be checked without
a GPU -- the ABI surface, the descriptor checks (those of the fp32 descriptors, plus the alignment of the bf16 pointers), the
`compute` argument, the CPU path against the contract functions, the switched stand-in modules.
tests/test_window_attention_bf16_gpu.py has the kernels."""
import copy
import ctypes
import os
import re

import pytest
import torch
import torch.nn as nn

from gsasr_amd import _cabi
from gsasr_amd import attention as att
from test_window_attention import StandIn as BiasedStandIn
from test_window_attention import _args as biased_args
from test_window_attention_rope import _args as rope_args
from test_window_attention_rope import _rope_standin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = tuple(f"gsasr_window_attn{kind}_bf16_{what}" for kind in ("", "_rope") for what in ("scratch_bytes", "forward", "backward"))
ACTIVATIONS = ("q", "k", "v", "out", "grad_out", "g_q", "g_k", "g_v")


def test_abi_surface_of_the_bf16_part():
    hdr = open(os.path.join(ROOT, "include", "gsasr_splat.h")).read()
    assert re.search(r"#define\s+GSASR_SPLAT_ABI_VERSION\s+7\b", hdr)
    bare = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(gsasr_[a-z_0-9]+)\s*\(", bare))
    L = ctypes.CDLL(_cabi.LIB_PATH)
    for name in NEW:
        assert name in declared and name in _cabi.EXPORTS and hasattr(L, name), name
    assert declared == set(_cabi.EXPORTS), declared ^ set(_cabi.EXPORTS)
    assert _cabi.lib().gsasr_abi_version() == 7
    assert re.search(r"typedef\s+unsigned\s+short\s+gsasr_bf16\s*;", bare)
    for fp32, bf16, cls32, cls16 in (("gsasr_window_attn", "gsasr_window_attn_bf16", _cabi.WindowAttn, _cabi.WindowAttnBf16),
                                     ("gsasr_window_attn_rope", "gsasr_window_attn_rope_bf16", _cabi.WindowAttnRope, _cabi.WindowAttnRopeBf16)):
        fields = []
        for name in (fp32, bf16):
            struct = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), bare, re.S).group(1)
            fields.append(tuple(re.findall(r"[*\s,]([a-z_]+)\s*[,;]", struct)))
        assert fields[0] == fields[1] == tuple(f for f, _ in cls32._fields_) == tuple(f for f, _ in cls16._fields_)
        assert ctypes.sizeof(cls16) == ctypes.sizeof(cls32) == 8 * 4 + 13 * ctypes.sizeof(ctypes.c_void_p)
        struct = re.search(r"typedef struct %s \{(.*?)\} %s;" % (bf16, bf16), bare, re.S).group(1)
        typed = set(re.findall(r"[*\s,]([a-z_]+)\s*[,;]", " ".join(re.findall(r"gsasr_bf16\s[^;]*;", struct))))
        assert typed == set(ACTIVATIONS), typed         # the eight activation pointers, and only they, are gsasr_bf16
    assert "scale" in hdr and re.search(r"scale.{0,40}multiplies the fp32 score SUM", hdr, re.S)      # the rule is in the header


def _biased(**kw):
    d = _cabi.make_window_attn(2, 6, 144, 144, 30, 529, 30 ** -0.5, bf16=True)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _rope(**kw):
    d = _cabi.make_window_attn_rope(2, 6, 144, 144, 32, 144, 32 ** -0.5, bf16=True)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


BIASED_FWD, BIASED_BWD = ("q", "k", "v", "table", "index", "out"), ("q", "k", "v", "table", "index", "out", "stats", "grad_out")
ROPE_FWD, ROPE_BWD = ("q", "k", "v", "angles", "out", "cossin"), ("q", "k", "v", "out", "stats", "grad_out", "cossin")
GRADS = dict(g_q=256, g_k=256, g_v=256)


def test_biased_descriptor_checks_come_before_any_launch():
    """no GPU is touched: the pointers are addresses that are only looked at"""
    lib = _cabi.lib()
    fwd, bwd, nbytes = lib.gsasr_window_attn_bf16_forward, lib.gsasr_window_attn_bf16_backward, lib.gsasr_window_attn_bf16_scratch_bytes
    ERR_ARG = lib.gsasr_window_attn_forward(None, None)
    assert ERR_ARG != 0 and fwd(None, None) == ERR_ARG and bwd(None, None) == ERR_ARG and nbytes(None) == 0
    assert nbytes(ctypes.byref(_biased())) > 0
    assert nbytes(ctypes.byref(_biased(g_table=256))) >= 2 * 6 * 529 * 4
    same = _cabi.make_window_attn(2, 6, 144, 144, 30, 529, 30 ** -0.5)
    same.g_table = 256
    assert nbytes(ctypes.byref(_biased(g_table=256))) == lib.gsasr_window_attn_scratch_bytes(ctypes.byref(same))
    # the fp32 test's table of bad fields, flags = 1 included, with every pointer set
    for field, value in (("nq", 257), ("nk", 0), ("head_dim", 33), ("head_dim", 0), ("windows", 0), ("heads", 0), ("table_rows", 0), ("flags", 1),
                         ("scale", float("nan"))):
        d = _biased(**{p: 256 for p in BIASED_BWD}, **GRADS, **{field: value})
        assert nbytes(ctypes.byref(d)) == 0, field
        assert fwd(ctypes.byref(d), None) == ERR_ARG, field
        assert bwd(ctypes.byref(d), None) == ERR_ARG, field
    for missing in BIASED_FWD:
        assert fwd(ctypes.byref(_biased(**{p: 256 for p in BIASED_FWD if p != missing})), None) == ERR_ARG, missing
    for missing in BIASED_BWD:
        assert bwd(ctypes.byref(_biased(**{p: 256 for p in BIASED_BWD if p != missing}, **GRADS)), None) == ERR_ARG, missing
    assert bwd(ctypes.byref(_biased(**{p: 256 for p in BIASED_BWD}, **GRADS, g_table=256)), None) == ERR_ARG      # the table gradient needs the scratch
    # an odd activation address, each in turn
    for odd in ("q", "k", "v", "out"):
        assert fwd(ctypes.byref(_biased(**{**{p: 256 for p in BIASED_FWD}, odd: 257})), None) == ERR_ARG, odd
        assert b"aligned" in lib.gsasr_last_error()
    for odd in ACTIVATIONS:
        assert bwd(ctypes.byref(_biased(**{**{p: 256 for p in BIASED_BWD}, **GRADS, odd: 257})), None) == ERR_ARG, odd
        assert b"aligned" in lib.gsasr_last_error()


def test_rope_descriptor_checks_come_before_any_launch():
    lib = _cabi.lib()
    fwd, bwd, nbytes = lib.gsasr_window_attn_rope_bf16_forward, lib.gsasr_window_attn_rope_bf16_backward, lib.gsasr_window_attn_rope_bf16_scratch_bytes
    ERR_ARG = lib.gsasr_window_attn_rope_forward(None, None)
    assert ERR_ARG != 0 and fwd(None, None) == ERR_ARG and bwd(None, None) == ERR_ARG and nbytes(None) == 0
    assert nbytes(ctypes.byref(_rope())) > 0
    assert nbytes(ctypes.byref(_rope(windows=8, g_angles=256))) == nbytes(ctypes.byref(_rope(windows=8)))
    assert nbytes(ctypes.byref(_rope(windows=256, g_angles=256))) >= 2 * 6 * 144 * 16 * 4
    for field, value in (("nq", 257), ("nq", 0), ("nk", 257), ("nk", 0), ("head_dim", 34), ("head_dim", 0), ("head_dim", 31), ("head_dim", 1),
                         ("windows", 0), ("heads", 0), ("angle_rows", 143), ("flags", 1), ("scale", float("nan"))):
        d = _rope(**{p: 256 for p in set(ROPE_FWD + ROPE_BWD)}, **GRADS, **{field: value})
        assert nbytes(ctypes.byref(d)) == 0, field
        assert fwd(ctypes.byref(d), None) == ERR_ARG, field
        assert bwd(ctypes.byref(d), None) == ERR_ARG, field
    for missing in ROPE_FWD:
        assert fwd(ctypes.byref(_rope(**{p: 256 for p in ROPE_FWD if p != missing})), None) == ERR_ARG, missing
    for missing in ROPE_BWD:
        assert bwd(ctypes.byref(_rope(**{p: 256 for p in ROPE_BWD if p != missing}, **GRADS)), None) == ERR_ARG, missing
    for drop in ("g_q", "g_k"):         # the angle gradient is formed from g_q and g_k
        assert bwd(ctypes.byref(_rope(**{**{p: 256 for p in ROPE_BWD}, **GRADS, "g_angles": 256, "scratch": 256, drop: None})), None) == ERR_ARG, drop
    assert bwd(ctypes.byref(_rope(windows=256, **{p: 256 for p in ROPE_BWD}, **GRADS, g_angles=256)), None) == ERR_ARG      # ... and needs the scratch
    # pair loads: an odd address and a 2-mod-4 address of an activation, each in turn; cossin 8-byte aligned
    for address in (257, 258):
        for odd in ("q", "k", "v", "out"):
            assert fwd(ctypes.byref(_rope(**{**{p: 256 for p in ROPE_FWD}, odd: address})), None) == ERR_ARG, (odd, address)
            assert b"aligned" in lib.gsasr_last_error()
        for odd in ACTIVATIONS:
            assert bwd(ctypes.byref(_rope(**{**{p: 256 for p in ROPE_BWD}, **GRADS, odd: address})), None) == ERR_ARG, (odd, address)
            assert b"aligned" in lib.gsasr_last_error()
    assert fwd(ctypes.byref(_rope(**{**{p: 256 for p in ROPE_FWD}, "cossin": 260})), None) == ERR_ARG


def test_compute_argument():
    a, r = biased_args(), rope_args()
    for bad in ("nonsense", "BF16", None, 16):
        with pytest.raises(ValueError):
            att.window_attention(*a, compute=bad)
        with pytest.raises(ValueError):
            att.window_attention_rope(*r, compute=bad)
        with pytest.raises(ValueError):
            att.use_hip_attention(nn.Linear(2, 2), compute=bad)
    assert torch.equal(att.window_attention(*a, compute="fp32"), att.window_attention(*a))
    assert torch.equal(att.window_attention_rope(*r, compute="fp32"), att.window_attention_rope(*r))
    assert torch.equal(att.window_attention(*a, 0.3, compute="fp32"), att.window_attention(*a, 0.3))
    import gsasr_amd
    assert gsasr_amd.window_attention_bf16_torch is att.window_attention_bf16_torch
    assert gsasr_amd.window_attention_rope_bf16_torch is att.window_attention_rope_bf16_torch


def test_cpu_path_is_the_bf16_contract():
    for args, op, contract, expr in ((biased_args(), att.window_attention, att.window_attention_bf16_torch, att.window_attention_torch),
                                     (rope_args(), att.window_attention_rope, att.window_attention_rope_bf16_torch, att.window_attention_rope_torch)):
        got = op(*args, compute="bf16")
        assert got.dtype == torch.bfloat16 and torch.equal(got, contract(*args))
        # the contract is the fp32 expression on the bf16-rounded q, k, v, rounded to bf16 -- whatever the inputs' dtype
        q, k, v = (t.bfloat16() for t in args[:3])
        assert torch.equal(got, expr(q.float(), k.float(), v.float(), *args[3:]).bfloat16())
        assert torch.equal(got, op(q, k, v, *args[3:], compute="bf16"))
        assert torch.equal(got, op(q, k, v, args[3].double(), *args[4:], compute="bf16"))      # the table / angles are taken as fp32
        # gradients arrive in each input's own dtype
        leaves = [q.clone().requires_grad_(True), args[1].clone().requires_grad_(True), args[2].double().requires_grad_(True),
                  args[3].clone().requires_grad_(True)]
        grads = torch.autograd.grad(op(*leaves, *args[4:], compute="bf16").float().sum(), leaves)
        assert [g.dtype for g in grads] == [torch.bfloat16, torch.float32, torch.float64, torch.float32]
    for bad in ("nq 257", "d 33"):      # the shape errors come first in this mode too
        with pytest.raises(ValueError):
            att.window_attention(*(biased_args(nq=257) if bad == "nq 257" else biased_args(d=33)), compute="bf16")
    with pytest.raises(ValueError):
        att.window_attention_rope(*rope_args(d=6, C=10), compute="bf16")


def test_use_hip_attention_in_bf16_mode():
    g = torch.Generator().manual_seed(4)
    index = torch.randint(0, 5, (9, 9), generator=g)
    biased = BiasedStandIn(8, 2, 5, index)
    with torch.no_grad():
        biased.relative_position_bias_table.normal_(generator=g)
    both = nn.ModuleList([_rope_standin(), biased, _rope_standin(mixed=False)])
    before = copy.deepcopy(both.state_dict())
    unswitched = copy.deepcopy(both)
    assert att.use_hip_attention(both, compute="bf16") == 3
    assert list(both.state_dict()) == list(before) and all(torch.equal(both.state_dict()[k], before[k]) for k in before)
    assert both[0].forward.__func__ is att._rope_module_forward_bf16 and both[1].forward.__func__ is att._module_forward_bf16
    x = torch.randn(2, 9, 8, generator=g)
    for m, ref in zip(both, unswitched):
        for dtype in (torch.float32, torch.float64):
            mm, rr, xx = copy.deepcopy(m).to(dtype), copy.deepcopy(ref).to(dtype), x.to(dtype)
            att.use_hip_attention(mm, compute="bf16")         # (a deep copy keeps the switched forward of the ORIGINAL module bound)
            y, y2 = mm(xx), mm(xx, xx)
            assert y.dtype == dtype and torch.equal(y, y2)
            want = rr(xx)           # bf16 attention inside an fp32 module: close to the module, not equal to it
            assert 0 < float((y - want).detach().abs().max()) <= 0.05 * float(want.detach().abs().max())
    # switching back to fp32 restores the fp32 forward
    assert att.use_hip_attention(both) == 3
    assert torch.equal(both[1](x), unswitched[1](x))
