"""The RoPE decoder's window attention (gsasr_amd.window_attention_rope / use_hip_attention;
gsasr_window_attn_rope_forward / _backward): what can be checked without a GPU -- the torch expression that is the op's contract
and its CPU path against the reference's modules (tests/golden/attention_rope_*.npz, written by
tests/golden/make_golden_attention_rope.py), the argument errors, the ABI surface.  tests/test_window_attention_rope_gpu.py has
the kernels.  The bar (`bar` / `held`) is that of tests/test_window_attention.py: 4 x e32 + 1e-6 x max-abs, e32 the fp32 torch
expression's error against its float64 evaluation on the same input.  Every check prints its ratio to the bar."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

from gsasr_amd import _cabi
from gsasr_amd import attention as att
from test_window_attention import StandIn as BiasedStandIn
from test_window_attention import held

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
WINDOWS = 2
GOLDEN_CASES = {      # the reference's GSSelfAttn / WindowCrossAttn of the RoPE decoder: d = 32 on 12 x 12 and on 16 x 16 tokens
    "self_12": dict(kind="self", dim=64, heads=2, side=12, seed=21),
    "self_16": dict(kind="self", dim=64, heads=2, side=16, seed=22),
    "cross_12": dict(kind="cross", dim=64, heads=2, side=12, seed=23),
    "cross_16": dict(kind="cross", dim=64, heads=2, side=16, seed=24),
}
PARAMS = ("qhead_weight", "qhead_bias", "khead_weight", "khead_bias", "vhead_weight", "vhead_bias", "rope_freqs")


def attention_inputs(case):
    """(gs, feat, loss weights) of a golden case, fp32 [2, side^2, dim] each, from its NumPy seed"""
    rng = np.random.default_rng(2000 + case["seed"])
    shape = (WINDOWS, case["side"] ** 2, case["dim"])
    return tuple(rng.standard_normal(shape).astype(np.float32) for _ in range(3))


class RopeStandIn(nn.Module):
    """a module with the attribute names of the RoPE decoder's attention modules (own code): forward = the three Linears, the
    angles, the torch expression and proj; `use_hip_attention` replaces it"""

    def __init__(self, dim, heads, freqs, t_x, t_y, mixed=True):
        super().__init__()
        self.num_heads = heads
        self.qhead, self.khead, self.vhead, self.proj = (nn.Linear(dim, dim) for _ in range(4))
        if mixed:
            self.rope_freqs = nn.Parameter(freqs.clone())
        else:
            self.register_buffer("rope_freqs", freqs.clone())
        self.register_buffer("rope_t_x", t_x.clone())
        self.register_buffer("rope_t_y", t_y.clone())

    def forward(self, gs, feat=None):
        src = gs if feat is None else feat
        angles = att.rope_angles(self.rope_freqs, self.rope_t_x, self.rope_t_y)
        return self.proj(att.window_attention_rope_torch(self.qhead(gs), self.khead(src), self.vhead(src), angles))


def load_golden(name):
    """(stand-in module with the golden's weights, the file's arrays)"""
    data = np.load(os.path.join(GOLDEN, f"attention_rope_{name}.npz"))
    case = GOLDEN_CASES[name]
    m = RopeStandIn(case["dim"], case["heads"], *(torch.from_numpy(data[k]) for k in ("rope_freqs", "rope_t_x", "rope_t_y")))
    with torch.no_grad():
        for lin in ("qhead", "khead", "vhead", "proj"):
            getattr(m, lin).weight.copy_(torch.from_numpy(data[lin + "_weight"]))
            getattr(m, lin).bias.copy_(torch.from_numpy(data[lin + "_bias"]))
    return m, data


def run_case(m, case, device="cpu", dtype=torch.float32):
    """{out, g_gs, [g_feat,] g_<parameter>...} of module `m` (moved to device / dtype) on the case's inputs"""
    m = m.to(device=device, dtype=dtype)
    gs, feat, wgt = (torch.from_numpy(a).to(device=device, dtype=dtype) for a in attention_inputs(case))
    gs.requires_grad_(True)
    feat.requires_grad_(True)
    cross = case["kind"] == "cross"
    out = m(gs, feat) if cross else m(gs)
    ps = [m.qhead.weight, m.qhead.bias, m.khead.weight, m.khead.bias, m.vhead.weight, m.vhead.bias, m.rope_freqs]
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
    assert "g_rope_freqs" in want and data["rope_freqs"].shape == (2, case["heads"], case["dim"] // case["heads"] // 2)
    assert data["rope_t_x"].shape == (case["side"] ** 2,)
    ok = True
    # the reference's own fp32 numbers are an fp32 evaluation of the same expression: held to the same bar
    for k in want:
        ok &= held(f"rope {name} reference {k}", torch.from_numpy(data[k]), want[k], e32[k])
    # the switched module on CPU tensors
    sw = copy.deepcopy(m)
    assert att.use_hip_attention(sw) == 1
    got = run_case(sw, case)
    for k in want:
        ok &= held(f"rope {name} switched {k}", got[k], want[k], e32[k])
    assert ok
    assert [k for k, _ in sw.state_dict().items()] == [k for k, _ in m.state_dict().items()]


def _rope_standin(mixed=True, dim=8, heads=2, side=3):
    g = torch.Generator().manual_seed(9)
    t = torch.arange(side * side, dtype=torch.float32)
    return RopeStandIn(dim, heads, torch.randn(2, heads, dim // heads // 2, generator=g), t % side, torch.div(t, side, rounding_mode="floor"), mixed)


def test_use_hip_attention_counts_both_kinds():
    assert att.use_hip_attention(_rope_standin()) == 1
    assert att.use_hip_attention(_rope_standin(mixed=False)) == 1          # rope_freqs as a buffer (rope_mixed False)
    biased = BiasedStandIn(8, 2, 5, torch.zeros(9, 9, dtype=torch.int64))
    assert att.use_hip_attention(biased) == 1
    both = nn.ModuleList([_rope_standin(), BiasedStandIn(8, 2, 5, torch.zeros(9, 9, dtype=torch.int64))])
    keys = list(both.state_dict())
    assert att.use_hip_attention(both) == 2
    assert list(both.state_dict()) == keys
    assert both[0].forward.__func__ is att._rope_module_forward and both[1].forward.__func__ is att._module_forward
    # a module with the rotary names AND a bias table is a biased one
    odd = _rope_standin()
    odd.relative_position_bias_table = nn.Parameter(torch.zeros(5, 2))
    assert att.use_hip_attention(odd) == 0
    # the switched modules compute what they computed before
    x = torch.randn(2, 9, 8, generator=torch.Generator().manual_seed(1))
    for mixed in (True, False):
        m = _rope_standin(mixed)
        want = m(x)
        att.use_hip_attention(m)
        assert torch.equal(m(x), want) and torch.equal(m(x, x), want)
    assert att.use_hip_attention(nn.Linear(2, 2)) == 0


def _args(W=2, nq=5, nk=7, H=2, d=4, N=None, C=None):
    C = H * d if C is None else C
    N = max(nq, nk) if N is None else N
    g = torch.Generator().manual_seed(3)
    return [torch.randn(W, nq, C, generator=g), torch.randn(W, nk, C, generator=g), torch.randn(W, nk, C, generator=g),
            6 * torch.randn(H, N, d // 2, generator=g)]


def test_cpu_path_is_the_expression():
    for a in (_args(), _args(N=9), _args(nq=7, nk=5)):
        assert torch.equal(att.window_attention_rope(*a), att.window_attention_rope_torch(*a))
        assert torch.equal(att.window_attention_rope(*a, 0.3), att.window_attention_rope_torch(*a, 0.3))
    import gsasr_amd
    assert gsasr_amd.window_attention_rope is att.window_attention_rope
    # zero angles: the biased expression with a zero table
    a = _args()
    a[3] = torch.zeros_like(a[3])
    want = att.window_attention_torch(*a[:3], torch.zeros(1, 2), torch.zeros(5, 7, dtype=torch.int64))
    assert float((att.window_attention_rope(*a) - want).abs().max()) <= 1e-6


@pytest.mark.parametrize("what", ["nq 257", "nk 257", "d 34", "d odd", "channels", "angle rows", "angle width", "angles int", "angles 2-d",
                                  "q int", "v shape", "windows"])
def test_argument_errors(what):
    a = _args()
    if what == "nq 257":
        a = _args(nq=257)
    elif what == "nk 257":
        a = _args(nk=257)
    elif what == "d 34":
        a = _args(d=34)
    elif what == "d odd":           # 2 heads x 3 columns against angles of width 1: not heads x 2 x width
        a = _args(C=6)
    elif what == "channels":
        a = _args(C=7)
    elif what == "angle rows":
        a[3] = a[3][:, :6]
    elif what == "angle width":
        a[3] = a[3][:, :, :1]
    elif what == "angles int":
        a[3] = a[3].long()
    elif what == "angles 2-d":
        a[3] = a[3][0]
    elif what == "q int":
        a[0] = a[0].long()
    elif what == "v shape":
        a[2] = a[2][:, :6]
    elif what == "windows":
        a[1], a[2] = a[1][:1], a[2][:1]
    with pytest.raises(ValueError):
        att.window_attention_rope(*a)


def test_limits_are_admitted_on_cpu():
    assert att.window_attention_rope(*_args(W=1, nq=256, nk=256, H=1, d=32)).shape == (1, 256, 32)
    assert att.window_attention_rope(*_args(W=1, nq=1, nk=1, H=1, d=2)).shape == (1, 1, 2)


def test_gradcheck_of_the_expression_and_the_angle_identity():
    g = torch.Generator().manual_seed(5)
    W, nq, nk, H, d = 2, 4, 5, 2, 4
    q = torch.randn(W, nq, H * d, dtype=torch.float64, generator=g).requires_grad_(True)
    k, v = (torch.randn(W, nk, H * d, dtype=torch.float64, generator=g).requires_grad_(True) for _ in range(2))
    angles = (3 * torch.randn(H, nk + 2, d // 2, dtype=torch.float64, generator=g)).requires_grad_(True)
    assert torch.autograd.gradcheck(att.window_attention_rope_torch, (q, k, v, angles))
    assert torch.autograd.gradcheck(lambda *t: att.window_attention_rope(*t, 0.7), (q, k, v, angles))
    # d L / d angle = sum_w Im(conj(x) dx) over q (rows < nq) and k (rows < nk), dx the gradient of the un-rotated input
    wgt = torch.randn(W, nq, H * d, dtype=torch.float64, generator=g)
    gq, gk, _, ga = torch.autograd.grad((att.window_attention_rope_torch(q, k, v, angles) * wgt).sum(), (q, k, v, angles))

    def im(x, dx):
        x, dx = x.detach().view(W, -1, H, d // 2, 2), dx.view(W, -1, H, d // 2, 2)
        return (x[..., 0] * dx[..., 1] - x[..., 1] * dx[..., 0]).sum(0).permute(1, 0, 2)      # [H, n, d/2]

    want = torch.zeros_like(ga)
    want[:, :nq] += im(q, gq)
    want[:, :nk] += im(k, gk)
    assert float((ga - want).abs().max()) <= 1e-12 * float(ga.abs().max()) + 1e-14
    assert float(ga[:, nk:].abs().max()) == 0.0


def test_c5_decoder_rope_position():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import c5_models
    torch.manual_seed(0)
    kw = dict(inchannel=8, channel=16, heads=2, window=4, cross_layers=2, self_blocks=1, self_layers=2)
    base = c5_models.Fea2GSDecoder(**kw)
    assert list(base.state_dict()) == list(c5_models.Fea2GSDecoder(**kw, position="bias").state_dict())
    a = c5_models.Fea2GSDecoder(**kw, position="rope")
    b = c5_models.Fea2GSDecoder(**kw, position="rope", attention="hip", scale_attention="constant")
    assert list(a.state_dict()) == list(b.state_dict()) and list(a.state_dict()) != list(base.state_dict())
    b.load_state_dict(a.state_dict())
    rot = [m for m in a.modules() if all(hasattr(m, n) for n in att._ROPE_ATTRS)]
    assert len(rot) == 4 and not any(hasattr(m, "relative_position_bias_table") for m in rot)
    assert tuple(rot[0].rope_freqs.shape) == (2, 2, 4) and tuple(rot[0].rope_t_x.shape) == (16,)
    assert att.use_hip_attention(copy.deepcopy(a)) == 4
    feat, scale = torch.randn(2, 8, 8, 4), torch.tensor([2.0, 3.0])
    ya, yb = a(feat, scale), b(feat, scale)        # (on CPU tensors "hip" is the torch expression)
    assert float((ya - yb).detach().abs().max()) <= 1e-4 * float(ya.detach().abs().max())
    assert c5_models.Fea2GSDecoder(inchannel=8, channel=192, cross_layers=1, self_blocks=0, position="rope").cross[0].layers[0].attn.rope_freqs.shape == (2, 6, 16)
    with pytest.raises(ValueError):
        c5_models.Fea2GSDecoder(**kw, position="other")


FIELDS = ("windows", "heads", "nq", "nk", "head_dim", "angle_rows", "scale", "flags", "q", "k", "v", "angles", "out", "stats", "grad_out",
          "g_q", "g_k", "g_v", "g_angles", "cossin", "scratch")


def test_abi_surface_of_the_rotary_part():
    hdr = open(os.path.join(ROOT, "include", "gsasr_splat.h")).read()
    assert re.search(r"#define\s+GSASR_SPLAT_ABI_VERSION\s+7\b", hdr)
    bare = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(gsasr_[a-z_0-9]+)\s*\(", bare))
    L = ctypes.CDLL(_cabi.LIB_PATH)
    for name in ("gsasr_window_attn_rope_scratch_bytes", "gsasr_window_attn_rope_forward", "gsasr_window_attn_rope_backward"):
        assert name in declared and name in _cabi.EXPORTS and hasattr(L, name), name
    assert declared == set(_cabi.EXPORTS), declared ^ set(_cabi.EXPORTS)
    assert _cabi.lib().gsasr_abi_version() == 7
    struct = re.search(r"typedef struct gsasr_window_attn_rope \{(.*?)\} gsasr_window_attn_rope;", bare, re.S).group(1)
    assert tuple(re.findall(r"[*\s,]([a-z_]+)\s*[,;]", struct)) == FIELDS
    assert tuple(f for f, _ in _cabi.WindowAttnRope._fields_) == FIELDS
    # the biased descriptor is what it was: 8 words and 13 pointers
    assert ctypes.sizeof(_cabi.WindowAttn) == 8 * 4 + 13 * ctypes.sizeof(ctypes.c_void_p)
    assert ctypes.sizeof(_cabi.WindowAttnRope) == 8 * 4 + 13 * ctypes.sizeof(ctypes.c_void_p)
    assert [f for f, _ in _cabi.WindowAttn._fields_][5] == "table_rows" and len(_cabi.WindowAttn._fields_) == 21


def _desc(**kw):
    d = _cabi.make_window_attn_rope(2, 6, 144, 144, 32, 144, 32 ** -0.5)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


POINTERS_FWD = ("q", "k", "v", "angles", "out", "cossin")
POINTERS_BWD = ("q", "k", "v", "out", "stats", "grad_out", "cossin")


def test_descriptor_checks_come_before_any_launch():
    """gsasr_window_attn_rope_scratch_bytes is 0 and the entry points return GSASR_ERR_ARG on a bad descriptor; every case
    returns before anything is enqueued (no GPU is touched; the pointers are addresses that are only looked at)"""
    lib = _cabi.lib()
    fwd, bwd, nbytes = lib.gsasr_window_attn_rope_forward, lib.gsasr_window_attn_rope_backward, lib.gsasr_window_attn_rope_scratch_bytes
    ERR_ARG = fwd(None, None)
    assert ERR_ARG != 0 and bwd(None, None) == ERR_ARG and nbytes(None) == 0
    good = _desc()
    assert nbytes(ctypes.byref(good)) > 0
    few = _desc(windows=8, g_angles=256)          # one slice of windows: the sum needs no partials
    assert nbytes(ctypes.byref(few)) == nbytes(ctypes.byref(_desc(windows=8)))
    many = _desc(windows=256, g_angles=256)
    assert nbytes(ctypes.byref(many)) >= 2 * 6 * 144 * 16 * 4
    for field, value in (("nq", 257), ("nq", 0), ("nk", 257), ("nk", 0), ("head_dim", 34), ("head_dim", 0), ("head_dim", 31), ("head_dim", 1),
                         ("windows", 0), ("heads", 0), ("angle_rows", 143), ("flags", 1), ("scale", float("nan"))):
        d = _desc(**{field: value})
        for p in set(POINTERS_FWD + POINTERS_BWD):
            setattr(d, p, 256)
        assert nbytes(ctypes.byref(d)) == 0, field
        assert fwd(ctypes.byref(d), None) == ERR_ARG, field
        assert bwd(ctypes.byref(d), None) == ERR_ARG, field
    d = _desc(nq=100, nk=144, angle_rows=143)     # angle_rows is held against the larger of nq and nk
    assert nbytes(ctypes.byref(d)) == 0
    assert nbytes(ctypes.byref(_desc(nq=100, nk=120, angle_rows=120))) > 0
    # a missing pointer, each in turn
    for missing in POINTERS_FWD:
        d = _desc(**{p: 256 for p in POINTERS_FWD if p != missing})
        assert fwd(ctypes.byref(d), None) == ERR_ARG, missing
    for missing in POINTERS_BWD:
        d = _desc(**{p: 256 for p in POINTERS_BWD if p != missing}, g_q=256, g_k=256, g_v=256)
        assert bwd(ctypes.byref(d), None) == ERR_ARG, missing
    # the angle gradient is formed from g_q and g_k
    for drop in ("g_q", "g_k"):
        d = _desc(**{p: 256 for p in POINTERS_BWD}, g_q=256, g_k=256, g_v=256, g_angles=256, scratch=256)
        setattr(d, drop, None)
        assert bwd(ctypes.byref(d), None) == ERR_ARG, drop
    # ... and, past one slice of windows, needs the scratch
    d = _desc(windows=256, **{p: 256 for p in POINTERS_BWD}, g_q=256, g_k=256, g_v=256, g_angles=256)
    assert bwd(ctypes.byref(d), None) == ERR_ARG
    # pair loads: q, k, g_q, g_k and cossin 8-byte aligned
    d = _desc(**{p: 256 for p in POINTERS_FWD})
    d.q = 260
    assert fwd(ctypes.byref(d), None) == ERR_ARG
    assert b"aligned" in lib.gsasr_last_error()
