"""The window attention kernels at the edges of their LDS layouts (csrc/splat_attn.hip: AttLdsQ, AttLdsKV, AttLdsFwdBf -- one struct
per kernel gives the kernel its pointers and the host its byte count, so a wrong size there moves a sub-buffer onto its neighbour
and corrupts it quietly).  The two shapes put the largest and the smallest padded K / V (or Q / dO) block next to the largest
table column the kernels stage -- 4096 rows, with the binned table gradient of as many rows behind it: 16 queries on 256 keys and
256 queries on 16 keys, one window, one head of 32.  The index reaches the table's first and last row.  The rotary pair runs the
same two shapes without a table.

Forward with the statistic (a training step) and without (no_grad), and the full backward, in fp32 and bf16, held to the float64
torch expression under the bars of tests/test_window_attention_gpu.py (fp32: 4 e32 + 1e-6 max-abs, e32 = the fp32 torch
expression's own error) and tests/test_window_attention_bf16_gpu.py (bf16: the same with e = the error of torch's bf16 SDPA on the
bf16-rounded inputs, and for the biased `out` also its own rounding).  Table rows that no (i, j) uses must get exactly 0."""
import functools

import pytest
import torch

import test_window_attention_bf16_gpu as bf
import test_window_attention_rope_gpu as gpu_rope
from gsasr_amd import attention as att
from test_window_attention import held

pytestmark = pytest.mark.gpu
SHAPES = [(1, 16, 256, 1, 32), (1, 256, 16, 1, 32)]
ROWS = 4096
NAMES = {"biased": ("out", "g_q", "g_k", "g_v", "g_table"), "rope": ("out", "g_q", "g_k", "g_v", "g_angles")}
FORMS = {"biased": (att.window_attention, att.window_attention_torch, bf.sdpa_biased),
         "rope": (att.window_attention_rope, att.window_attention_rope_torch, bf.sdpa_rope)}


def make_case(kind, shape):
    """(q, k, v), the table or the angles, (index,) or (), the loss weights"""
    if kind == "rope":
        q, k, v, angles, wgt = gpu_rope.make_case(shape)
        return (q, k, v), angles, (), wgt
    W, nq, nk, H, d = shape
    g = torch.Generator().manual_seed(23 * sum(shape))
    q, k, v, wgt = (torch.randn(W, n, H * d, generator=g) for n in (nq, nk, nk, nq))
    table = 0.5 * torch.randn(ROWS, H, generator=g)
    index = 15 * (torch.arange(nq)[:, None] - torch.arange(nk)[None, :] + nk - 1)          # 0 .. 15 * 270 = 4050
    index[0, 0], index[-1, -1] = ROWS - 1, 0
    return (q, k, v), table, (index,), wgt


@functools.lru_cache(maxsize=None)
def yardsticks(kind, shape, bf16):
    """(the case as the op gets it, the float64 results, the error per quantity of torch's own evaluation in the op's precision)
    -- once on the CPU, shared and left unchanged"""
    acts, param, tail, wgt = make_case(kind, shape)
    _, f64, sdpa = FORMS[kind]
    if bf16:
        acts, (wgt,) = bf.rounded(*acts), bf.rounded(wgt)
    want = bf.evaluate(f64, acts, param, tail, wgt, act_dtype=torch.float64, param_dtype=torch.float64)
    own = bf.evaluate(sdpa, acts, param, tail, wgt, act_dtype=bf.BF) if bf16 else bf.evaluate(f64, acts, param, tail, wgt)
    return (acts, param, tail, wgt), want, [float((a.double() - b).abs().max()) for a, b in zip(own, want)]


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=bf.ident)
@pytest.mark.parametrize("kind", ["biased", "rope"])
def test_forward_with_and_without_statistic_and_backward(kind, shape, bf16):
    (acts, param, tail, wgt), want, e = yardsticks(kind, shape, bf16)
    fn = FORMS[kind][0]
    op = (lambda *a: fn(*a, compute="bf16")) if bf16 else fn
    what = f"lds edges {kind} {shape} {'bf16' if bf16 else 'fp32'}"
    D, dtype = bf.dev(), bf.BF if bf16 else torch.float32
    got = bf.evaluate(op, acts, param, tail, wgt, device=D, act_dtype=dtype)
    assert [g.dtype for g in got] == [dtype] * 4 + [torch.float32]
    with torch.no_grad():       # (no statistic is kept: the forward's other instantiation)
        plain = op(*[t.to(device=D, dtype=dtype) for t in acts], param.to(D), *[t.to(D) for t in tail])
    ok = held(f"{what} out without the statistic", plain, want[0], e[0])
    for name, g, w, err in zip(NAMES[kind], got, want, e):
        ok &= held(f"{what} {name}", g, w, err)
    if kind == "biased":
        if bf16:
            e_round = float((want[0].to(bf.BF).double() - want[0]).abs().max())
            ok &= held(f"{what} out against its own rounding", got[0], want[0], e_round)
            ok &= held(f"{what} out without the statistic against its own rounding", plain, want[0], e_round)
        used = torch.zeros(ROWS, dtype=torch.bool)
        used[tail[0].flatten()] = True
        assert bool((got[4].cpu()[~used] == 0).all()), "table rows no (i, j) uses must get exactly 0"
    assert ok
