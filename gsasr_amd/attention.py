"""The window attention of GSASR's Fea2GS decoder (`WindowCrossAttn` and `GSSelfAttn`, utils/fea2gs.py:162-194, 321-350: 38
layers in every shipped configuration), fused:

    window_attention(q, k, v, bias_table, bias_index, scale=None)      # == window_attention_torch, one HIP call
    window_attention_rope(q, k, v, angles, scale=None)                 # == window_attention_rope_torch: the RoPE decoder's
    window_attention(..., compute="bf16") / window_attention_rope(..., compute="bf16")      # bf16 in, bf16 out (below)
    window_attention(..., mask=m) / window_attention_qkv(qkv, bias_table, bias_index, mask=m)   # a Swin layer's: an additive mask
                                                                        # per window, q, k, v read in place from one packed tensor
    use_hip_attention(model, compute="fp32")                            # switch a model's attention modules to them
    constant_key_attention(mha, row)                                    # the layers' attention to the scale embedding, closed form

`window_attention_rope` is the attention of `Fea2GS_ROPE_AMP` (utils/fea2gsropeamp.py, the AMP and UltraPerformance models): q and
k rotated by a 2-D rotary embedding with learned angles (`rope_angles`), then bias-free softmax(scale q k^T) v.

CUDA tensors: gsasr_window_attn_forward / _backward and gsasr_window_attn_rope_forward / _backward (hand-written HIP,
csrc/splat_attn.hip) as one autograd node on the current stream, or an error -- no torch fallback.  CPU tensors: the torch
expressions `window_attention_torch` / `window_attention_rope_torch` below, which are also the contracts.  include/gsasr_splat.h has the formulas.

`compute="fp32"` (the default): under autocast the inputs are cast to fp32 at the node's boundary and the result is fp32.
`compute="bf16"`: what the decoder's Linears produce under `torch.autocast(dtype=bfloat16)` goes in as it is -- q, k, v are bf16 in
memory (cast if they are not), the table / angles fp32, the result bf16: gsasr_window_attn_bf16_* / gsasr_window_attn_rope_bf16_*,
whose forward runs on the bf16 matrix instruction with fp32 scores and an fp32 softmax (include/gsasr_splat.h has the contract;
`window_attention_bf16_torch` / `window_attention_rope_bf16_torch` are its torch form and the CPU path).
"""
import types
import weakref

import torch

from ._amp import fp32_boundary_bwd, fp32_boundary_fwd

COMPUTE_MODES = ("fp32", "bf16")

MAX_TOKENS = 256        # queries or keys per window
MAX_HEAD_DIM = 32


def window_attention_torch(q, k, v, bias_table, bias_index, scale=None, mask=None):
    """`q` `[W,nq,H*d]`, `k`, `v` `[W,nk,H*d]` (channel h*d + j = head h, component j), `bias_table` `[T,H]`, `bias_index`
    integer `[nq,nk]` -> `[W,nq,H*d]`: softmax(scale q k^T + bias_table[bias_index]) v per window and head, in the inputs' dtype.
    `mask` `[nW,nq,nk]` with W % nW == 0: window w adds mask[w % nW] to its scores after the bias (the shifted-window mask of a
    Swin layer, utils/swinir.py:244-247); it is a constant"""
    W, nq, C = q.shape
    nk, H = k.shape[1], bias_table.shape[1]
    d = C // H
    scale = d ** -0.5 if scale is None else scale
    qh = q.view(W, nq, H, d).permute(0, 2, 1, 3) * scale
    kh = k.view(W, nk, H, d).permute(0, 2, 1, 3)
    vh = v.view(W, nk, H, d).permute(0, 2, 1, 3)
    attn = qh @ kh.transpose(-2, -1) + bias_table[bias_index.long()].permute(2, 0, 1)
    if mask is not None:
        nW = mask.shape[0]
        attn = (attn.view(W // nW, nW, H, nq, nk) + mask.detach().to(attn.dtype)[None, :, None]).view(W, H, nq, nk)
    return (torch.softmax(attn, dim=-1) @ vh).transpose(1, 2).reshape(W, nq, C)


def _split_qkv(qkv):
    C = qkv.shape[-1] // 3
    return qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]


def window_attention_qkv_torch(qkv, bias_table, bias_index, scale=None, mask=None):
    """`window_attention_torch` on the column blocks of `qkv` `[W,n,3*H*d]`: columns [0, C), [C, 2C), [2C, 3C) are q, k, v, each
    head-major (the layout of `qkv.reshape(W, n, 3, H, d)`) -> `[W,n,C]`"""
    return window_attention_torch(*_split_qkv(qkv), bias_table, bias_index, scale, mask)


def _bf16_rounded(*ts):
    return tuple(t.to(torch.bfloat16).float() for t in ts)


def window_attention_bf16_torch(q, k, v, bias_table, bias_index, scale=None, mask=None):
    """the contract of `window_attention(..., compute="bf16")`: `window_attention_torch` in fp32 on q, k, v rounded to bf16 (and
    the table and the mask as fp32), the result rounded to bf16"""
    mask = None if mask is None else mask.float()
    return window_attention_torch(*_bf16_rounded(q, k, v), bias_table.float(), bias_index, scale, mask).to(torch.bfloat16)


def _check_compute(compute):
    if compute not in COMPUTE_MODES:
        raise ValueError(f"compute must be one of {COMPUTE_MODES} (got {compute!r})")


_INDEX_CACHE = {}       # id(index tensor) -> (weak reference, its version, table rows, device, the int32 copy)


def _checked_index(bias_index, rows: int, device):
    """the contiguous int32 copy of `bias_index` on `device`, its range checked against `rows` -- once per index tensor (the
    check reads the extrema on the host; a training step hits the cache and has no host synchronisation)"""
    key = id(bias_index)
    hit = _INDEX_CACHE.get(key)
    if hit is not None and hit[0]() is bias_index and hit[1:4] == (bias_index._version, rows, device):
        return hit[4]
    lo, hi = (int(x) for x in torch.aminmax(bias_index)) if bias_index.numel() else (0, 0)
    if lo < 0 or hi >= rows:
        raise ValueError(f"bias_index has values in [{lo}, {hi}], bias_table {rows} rows")
    copy = bias_index.detach().to(device=device, dtype=torch.int32).contiguous()
    if len(_INDEX_CACHE) > 4096:        # (dead entries of models long gone)
        for stale in [i for i, e in _INDEX_CACHE.items() if e[0]() is None]:
            del _INDEX_CACHE[stale]
    _INDEX_CACHE[key] = (weakref.ref(bias_index), bias_index._version, rows, device, copy)
    return copy


def _node(name, doc, forward, backward, dtype):
    """the autograd node of a family (`forward(ctx, ...)`, `backward(ctx, grad_out)` below) on activations of `dtype`, which
    `grad_out` is cast to.  fp32: the fp32 boundary around both directions (under autocast the inputs are cast to fp32).  bf16:
    none -- the caller casts, and disables autocast around `apply`"""
    def bwd(ctx, grad_out):
        return backward(ctx, grad_out.to(dtype).contiguous())
    if dtype == torch.float32:
        forward, bwd = fp32_boundary_fwd(forward), fp32_boundary_bwd(bwd)
    return type(name, (torch.autograd.Function,), {"__doc__": doc, "forward": staticmethod(forward),
                                                    "backward": staticmethod(torch.autograd.function.once_differentiable(bwd))})


def _biased_forward(ctx, q, k, v, table, index, scale, keep):
    from . import _cabi
    q, k, v, table = q.contiguous(), k.contiguous(), v.contiguous(), table.contiguous()
    out, stats = _cabi.window_attn_forward(q, k, v, table, index, scale, want_stats=keep)
    if keep:
        ctx.save_for_backward(q, k, v, table, index, out, stats)
        ctx.scale = scale
    return out


def _biased_backward(ctx, grad_out):
    from . import _cabi
    q, k, v, table, index, out, stats = ctx.saved_tensors
    g = _cabi.window_attn_backward(q, k, v, table, index, ctx.scale, out, stats, grad_out, need=tuple(ctx.needs_input_grad[:4]))
    return (*g, None, None, None)


_WindowAttention = _node("_WindowAttention", "(q, k, v, table, int32 index, scale, keep) -> out; `keep`: save the row statistic for a backward",
                         _biased_forward, _biased_backward, torch.float32)
_WindowAttentionBf16 = _node("_WindowAttentionBf16", "_WindowAttention on bf16 q, k, v and an fp32 table -> bf16 out",
                             _biased_forward, _biased_backward, torch.bfloat16)


def _masked_forward(ctx, q, k, v, table, index, mask, scale, keep):
    from . import _cabi
    q, k, v, table = q.contiguous(), k.contiguous(), v.contiguous(), table.contiguous()
    out, stats = _cabi.window_attn_masked_forward(q, k, v, table, index, mask, scale, want_stats=keep)
    if keep:
        ctx.save_for_backward(q, k, v, table, index, out, stats, mask)
        ctx.scale = scale
    return out


def _masked_backward(ctx, grad_out):
    from . import _cabi
    q, k, v, table, index, out, stats, mask = ctx.saved_tensors
    g = _cabi.window_attn_masked_backward(q, k, v, table, index, mask, ctx.scale, out, stats, grad_out, need=tuple(ctx.needs_input_grad[:4]))
    return (*g, None, None, None, None)


def _qkv_forward(ctx, qkv, table, index, mask, scale, keep):
    """q, k, v are read in place: the column blocks of the packed tensor at its row pitch"""
    from . import _cabi
    qkv, table = qkv.contiguous(), table.contiguous()
    out, stats = _cabi.window_attn_masked_forward(*_split_qkv(qkv), table, index, mask, scale, want_stats=keep)
    if keep:
        ctx.save_for_backward(qkv, table, index, out, stats, mask)
        ctx.scale = scale
    return out


def _qkv_backward(ctx, grad_out):
    """ONE `[W,n,3C]` gradient, written in place by the backward kernels through the gradient pitches"""
    from . import _cabi
    qkv, table, index, out, stats, mask = ctx.saved_tensors
    need = (ctx.needs_input_grad[0],) * 3 + (ctx.needs_input_grad[1],)
    if need[0]:
        g_qkv, g_table = _cabi.window_attn_masked_backward(*_split_qkv(qkv), table, index, mask, ctx.scale, out, stats, grad_out, need=need, packed=True)
    else:
        g_qkv, g_table = None, _cabi.window_attn_masked_backward(*_split_qkv(qkv), table, index, mask, ctx.scale, out, stats, grad_out, need=need)[3]
    return g_qkv, g_table, None, None, None, None


_MASKED_DOC = "(q, k, v, table, int32 index, fp32 mask or None, scale, keep) -> out: the masked family (gsasr_window_attn_masked)"
_WindowAttentionMasked = _node("_WindowAttentionMasked", _MASKED_DOC, _masked_forward, _masked_backward, torch.float32)
_WindowAttentionMaskedBf16 = _node("_WindowAttentionMaskedBf16", _MASKED_DOC + " on bf16 q, k, v -> bf16 out", _masked_forward, _masked_backward, torch.bfloat16)
_QKV_DOC = "(qkv [W,n,3C], table, int32 index, fp32 mask or None, scale, keep) -> out [W,n,C]: the masked family on a packed tensor"
_WindowAttentionQKV = _node("_WindowAttentionQKV", _QKV_DOC, _qkv_forward, _qkv_backward, torch.float32)
_WindowAttentionQKVBf16 = _node("_WindowAttentionQKVBf16", _QKV_DOC + " in bf16 -> bf16 out", _qkv_forward, _qkv_backward, torch.bfloat16)


def _check_qkv(q, k, v, side, side_name, compute):
    """what both ops ask of `compute`, of q, k, v and of the dtype of their table / angles `side` -> (W, nq, nk, C)"""
    _check_compute(compute)
    for t, name in ((q, "q"), (k, "k"), (v, "v"), (side, side_name)):
        if not (torch.is_tensor(t) and t.dtype.is_floating_point):
            raise ValueError(f"{name} must be a floating-point tensor")
    if q.dim() != 3 or k.dim() != 3 or v.shape != k.shape or k.shape[0] != q.shape[0] or k.shape[2] != q.shape[2]:
        raise ValueError(f"q {tuple(q.shape)}, k {tuple(k.shape)}, v {tuple(v.shape)}: expected [W,nq,C], [W,nk,C], [W,nk,C]")
    return int(q.shape[0]), int(q.shape[1]), int(k.shape[1]), int(q.shape[2])


def _check_limits(W, nq, nk, d):
    if W < 1 or not 1 <= nq <= MAX_TOKENS or not 1 <= nk <= MAX_TOKENS:
        raise ValueError(f"need W >= 1 and 1 <= nq, nk <= {MAX_TOKENS} (got W {W}, nq {nq}, nk {nk})")
    if d > MAX_HEAD_DIM:
        raise ValueError(f"head dimension {d} exceeds {MAX_HEAD_DIM}")


def _run(nodes, torch_forms, compute, d, scale, q, k, v, side, side_name, *index):
    """the end of both ops, (`nodes`, `torch_forms`) = their (fp32, bf16) pair.  CPU tensors: the torch form.  bf16: q, k, v cast
    to bf16 and `side` to fp32 if they are not, the node with autocast off.  fp32: all four cast to fp32, the node"""
    scale = float(d ** -0.5 if scale is None else scale)
    if not (q.device == k.device == v.device == side.device):
        raise ValueError(f"q, k, v and {side_name} must be on one device")
    bf16 = compute == "bf16"
    if index:
        index = (_checked_index(index[0], side.shape[0], q.device),)
    if not q.is_cuda:
        return torch_forms[bf16](q, k, v, side, *index, scale)
    keep = torch.is_grad_enabled() and any(t.requires_grad for t in (q, k, v, side))
    if bf16:
        q, k, v = (t if t.dtype == torch.bfloat16 else t.to(torch.bfloat16) for t in (q, k, v))
        side = side if side.dtype == torch.float32 else side.float()
        with torch.autocast("cuda", enabled=False):
            return nodes[1].apply(q, k, v, side, *index, scale, keep)
    q, k, v, side = (t if t.dtype == torch.float32 else t.float() for t in (q, k, v, side))
    return nodes[0].apply(q, k, v, side, *index, scale, keep)


def _check_table(bias_table, bias_index, C, nq, nk):
    """what the biased ops ask of the table and the index -> H"""
    if not torch.is_tensor(bias_index) or bias_index.dtype.is_floating_point or bias_index.dtype in (torch.bool, torch.complex64, torch.complex128):
        raise ValueError("bias_index must be an integer tensor")
    if bias_table.dim() != 2 or bias_table.shape[0] < 1 or bias_table.shape[1] < 1:
        raise ValueError(f"bias_table has shape {tuple(bias_table.shape)}, expected [T,H]")
    H = int(bias_table.shape[1])
    if C % H or C == 0:
        raise ValueError(f"{C} channels are not {H} heads (the bias_table's columns) times a head dimension")
    if tuple(bias_index.shape) != (nq, nk):
        raise ValueError(f"bias_index has shape {tuple(bias_index.shape)}, expected [{nq}, {nk}]")
    return H


def _checked_mask(mask, W, nq, nk, device):
    """`mask` `[nW,nq,nk]` floating point on `device`, W % nW == 0, no gradient -> its contiguous fp32 form (itself when it is
    that already: a new tensor on every call costs nothing, nothing is cached and nothing is read on the host)"""
    if not (torch.is_tensor(mask) and mask.dtype.is_floating_point):
        raise ValueError("mask must be a floating-point tensor")
    if mask.dim() != 3 or tuple(mask.shape[1:]) != (nq, nk) or mask.shape[0] < 1:
        raise ValueError(f"mask has shape {tuple(mask.shape)}, expected [nW, {nq}, {nk}]")
    if W % mask.shape[0]:
        raise ValueError(f"{W} windows are not a multiple of the mask's {mask.shape[0]}")
    if mask.device != device:
        raise ValueError(f"mask is on {mask.device}, the inputs on {device}")
    if mask.requires_grad:
        raise ValueError("mask must not require a gradient (it gets none)")
    return mask if mask.dtype == torch.float32 and mask.is_contiguous() else mask.float().contiguous()


def _run_masked(nodes, compute, d, scale, acts, table, index, mask):
    """`_run` for the masked family: `acts` = (q, k, v) or (qkv,), `nodes` the (fp32, bf16) pair that takes them.  CPU tensors: the
    torch forms"""
    scale = float(d ** -0.5 if scale is None else scale)
    if not all(t.device == table.device for t in acts):
        raise ValueError("q, k, v (or qkv) and bias_table must be on one device")
    bf16 = compute == "bf16"
    index = _checked_index(index, table.shape[0], table.device)
    if not table.is_cuda:
        qkv = acts if len(acts) == 3 else _split_qkv(acts[0])
        return (window_attention_bf16_torch if bf16 else window_attention_torch)(*qkv, table, index, scale, mask)
    keep = torch.is_grad_enabled() and any(t.requires_grad for t in (*acts, table))
    table = table if table.dtype == torch.float32 else table.float()
    if bf16:
        acts = tuple(t if t.dtype == torch.bfloat16 else t.to(torch.bfloat16) for t in acts)
        with torch.autocast("cuda", enabled=False):
            return nodes[1].apply(*acts, table, index, mask, scale, keep)
    acts = tuple(t if t.dtype == torch.float32 else t.float() for t in acts)
    return nodes[0].apply(*acts, table, index, mask, scale, keep)


def window_attention_qkv(qkv, bias_table, bias_index, scale=None, compute="fp32", mask=None):
    """`window_attention` on a packed `qkv` `[W,n,3*H*d]` -- what ONE Linear writes: columns [0, C), [C, 2C), [2C, 3C) are q, k, v,
    each head-major (`window_attention_qkv_torch`) -> `[W,n,C]`.  q, k and v are read in place at the packed row pitch and the
    gradient is ONE `[W,n,3C]` tensor that the backward kernels write in place: no split copy, no `cat`.  `mask`, `scale`,
    `compute`, the limits and the errors as in `window_attention`; the masked entry points serve it with or without a mask."""
    _check_compute(compute)
    for t, name in ((qkv, "qkv"), (bias_table, "bias_table")):
        if not (torch.is_tensor(t) and t.dtype.is_floating_point):
            raise ValueError(f"{name} must be a floating-point tensor")
    if qkv.dim() != 3:
        raise ValueError(f"qkv has shape {tuple(qkv.shape)}, expected [W,n,3*H*d]")
    if bias_table.dim() != 2 or bias_table.shape[0] < 1 or bias_table.shape[1] < 1:        # (H is read before _check_table)
        raise ValueError(f"bias_table has shape {tuple(bias_table.shape)}, expected [T,H]")
    W, n, C3 = (int(s) for s in qkv.shape)
    H = int(bias_table.shape[1])
    if C3 == 0 or C3 % (3 * H):
        raise ValueError(f"qkv's {C3} columns are not 3 x {H} heads (the bias_table's columns) times a head dimension")
    C = C3 // 3
    _check_table(bias_table, bias_index, C, n, n)
    _check_limits(W, n, n, C // H)
    if mask is not None:
        mask = _checked_mask(mask, W, n, n, qkv.device)
    return _run_masked((_WindowAttentionQKV, _WindowAttentionQKVBf16), compute, C // H, scale, (qkv,), bias_table, bias_index, mask)


def window_attention(q, k, v, bias_table, bias_index, scale=None, compute="fp32", mask=None):
    """softmax(scale q k^T + bias_table[bias_index]) v per window and head (`window_attention_torch` has the shapes), as ONE
    differentiable call: gradients to `q`, `k`, `v` and `bias_table`.  Limits: 1 <= nq, nk <= 256, 1 <= d <= 32; anything else,
    a non-integer or out-of-range index, or mismatched shapes: ValueError before any launch.  `scale`: default d ** -0.5.
    `compute`: "fp32" (fp32 result; other dtypes are cast to fp32) or "bf16" (q, k, v cast to bf16 if they are not, the table to
    fp32, a bf16 result: `window_attention_bf16_torch`); gradients arrive in each input's own dtype.
    `mask`: a floating-point `[nW,nq,nk]` on the inputs' device with W % nW == 0 -- window w adds mask[w % nW] to its scores after
    the bias (gsasr_window_attn_masked; `window_attention_torch` has the expression).  It is used as contiguous fp32 (cast if it
    is not), gets no gradient (one that requires it: ValueError) and must be finite.  None: the call and the bits without it."""
    W, nq, nk, C = _check_qkv(q, k, v, bias_table, "bias_table", compute)
    H = _check_table(bias_table, bias_index, C, nq, nk)
    _check_limits(W, nq, nk, C // H)
    if mask is not None:
        mask = _checked_mask(mask, W, nq, nk, q.device)
        return _run_masked((_WindowAttentionMasked, _WindowAttentionMaskedBf16), compute, C // H, scale, (q, k, v), bias_table, bias_index, mask)
    return _run((_WindowAttention, _WindowAttentionBf16), (window_attention_torch, window_attention_bf16_torch), compute, C // H, scale,
                q, k, v, bias_table, "bias_table", bias_index)


def _rotate(x, cos, sin):
    """`x` `[W,n,H,d/2,2]` (re, im) times cos + i sin, `cos` / `sin` `[n,H,d/2]` -> `[W,n,H,d]`"""
    re, im = x[..., 0], x[..., 1]
    return torch.stack((re * cos - im * sin, re * sin + im * cos), dim=-1).flatten(-2)


def window_attention_rope_torch(q, k, v, angles, scale=None):
    """`q` `[W,nq,H*d]`, `k`, `v` `[W,nk,H*d]` (channel h*d + j = head h, component j), `angles` real `[H,N,d/2]` with
    N >= max(nq, nk) -> `[W,nq,H*d]`: head h's column pair (2j, 2j+1) of the token at row n of q and of k is the complex number
    re + i im, multiplied by cos + i sin of angles[h, n, j] (query i uses row i, key j row j); then softmax(scale q_rot k_rot^T) v
    per window and head, in the inputs' dtype"""
    W, nq, C = q.shape
    nk, H = k.shape[1], angles.shape[0]
    d = C // H
    scale = d ** -0.5 if scale is None else scale
    a = angles.permute(1, 0, 2)                                                # [N, H, d/2]
    cos, sin = torch.cos(a).to(q.dtype), torch.sin(a).to(q.dtype)
    qh = _rotate(q.view(W, nq, H, d // 2, 2), cos[:nq], sin[:nq]).permute(0, 2, 1, 3) * scale
    kh = _rotate(k.view(W, nk, H, d // 2, 2), cos[:nk], sin[:nk]).permute(0, 2, 1, 3)
    vh = v.view(W, nk, H, d).permute(0, 2, 1, 3)
    attn = qh @ kh.transpose(-2, -1)
    return (torch.softmax(attn, dim=-1) @ vh).transpose(1, 2).reshape(W, nq, C)


def window_attention_rope_bf16_torch(q, k, v, angles, scale=None):
    """the contract of `window_attention_rope(..., compute="bf16")`: `window_attention_rope_torch` in fp32 on q, k, v rounded to
    bf16 (and the angles as fp32), the result rounded to bf16.  The kernels additionally round the ROTATED q and k to bf16, as the
    reference's apply_rotary_emb_single does; include/gsasr_splat.h has that contract."""
    return window_attention_rope_torch(*_bf16_rounded(q, k, v), angles.float(), scale).to(torch.bfloat16)


def _rope_forward(ctx, q, k, v, angles, scale, keep):
    from . import _cabi
    q, k, v, angles = q.contiguous(), k.contiguous(), v.contiguous(), angles.contiguous()
    out, stats, cossin = _cabi.window_attn_rope_forward(q, k, v, angles, scale, want_stats=keep)
    if keep:
        ctx.save_for_backward(q, k, v, angles, out, stats, cossin)
        ctx.scale = scale
    return out


def _rope_backward(ctx, grad_out):
    from . import _cabi
    q, k, v, angles, out, stats, cossin = ctx.saved_tensors
    g = _cabi.window_attn_rope_backward(q, k, v, angles, ctx.scale, out, stats, cossin, grad_out, need=tuple(ctx.needs_input_grad[:4]))
    return (*g, None, None)


_WindowAttentionRope = _node("_WindowAttentionRope", "(q, k, v, angles, scale, keep) -> out; `keep`: save the row statistic and the (cos, sin) "
                             "table for a backward", _rope_forward, _rope_backward, torch.float32)
_WindowAttentionRopeBf16 = _node("_WindowAttentionRopeBf16", "_WindowAttentionRope on bf16 q, k, v and fp32 angles -> bf16 out",
                                 _rope_forward, _rope_backward, torch.bfloat16)


def window_attention_rope(q, k, v, angles, scale=None, compute="fp32"):
    """softmax(scale rot(q) rot(k)^T) v per window and head, q and k rotated by `angles` (`window_attention_rope_torch` has the
    shapes and the rotation), as ONE differentiable call: gradients to `q`, `k`, `v` and `angles`.  Limits: 1 <= nq, nk <= 256,
    d even with 2 <= d <= 32, angles [H, N >= max(nq, nk), d/2] floating point on the inputs' device; anything else: ValueError
    before any launch.  `scale`: default d ** -0.5.  `compute`: "fp32" or "bf16", as in `window_attention` (bf16: the angles are
    cast to fp32, the rotation is evaluated in fp32 and the rotated q, k rounded to bf16)."""
    W, nq, nk, C = _check_qkv(q, k, v, angles, "angles", compute)
    if angles.dim() != 3 or angles.shape[0] < 1 or angles.shape[2] < 1:
        raise ValueError(f"angles has shape {tuple(angles.shape)}, expected [H,N,d/2]")
    H, N, half = (int(s) for s in angles.shape)
    if C != H * 2 * half:
        raise ValueError(f"{C} channels are not {H} heads (angles' first extent) times a head dimension of {2 * half} (twice its last)")
    _check_limits(W, nq, nk, 2 * half)
    if N < max(nq, nk):
        raise ValueError(f"angles has {N} rows, fewer than max(nq, nk) = {max(nq, nk)}")
    return _run((_WindowAttentionRope, _WindowAttentionRopeBf16), (window_attention_rope_torch, window_attention_rope_bf16_torch), compute,
                2 * half, scale, q, k, v, angles, "angles")


_ATTRS = ("qhead", "khead", "vhead", "proj", "relative_position_bias_table", "relative_position_index", "num_heads")
_ROPE_ATTRS = ("qhead", "khead", "vhead", "proj", "num_heads", "rope_freqs", "rope_t_x", "rope_t_y")
_SWIN_ATTRS = ("qkv", "proj", "relative_position_bias_table", "relative_position_index", "num_heads")     # (and no qhead)


def rope_angles(freqs, t_x, t_y):
    """the angles `[H,N,d/2]` of the RoPE modules: t_x freqs[0] + t_y freqs[1] (`compute_cis` of utils/fea2gsropeamp.py without
    the `polar`), in fp32 with autocast disabled; differentiable in `freqs` `[2,H,d/2]`"""
    with torch.autocast(device_type=freqs.device.type, enabled=False):
        return t_x[None, :, None] * freqs[0][:, None, :] + t_y[None, :, None] * freqs[1][:, None, :]


def _rope_module_forward(self, gs, feat=None, compute="fp32"):
    """the RoPE module's own Linears around window_attention_rope: `forward(gs)` or `forward(gs, feat)`"""
    src = gs if feat is None else feat
    angles = rope_angles(self.rope_freqs, self.rope_t_x, self.rope_t_y)
    x = window_attention_rope(self.qhead(gs), self.khead(src), self.vhead(src), angles, compute=compute)
    return self.proj(x if compute == "fp32" else x.to(gs.dtype))      # (bf16: a no-op under autocast; an fp32 model outside it keeps working)


def _module_forward(self, gs, feat=None, compute="fp32"):
    """the module's own Linears around window_attention: `forward(gs)` (self attention) or `forward(gs, feat)` (keys and values
    from `feat`)"""
    src = gs if feat is None else feat
    c = gs.shape[-1]
    scale = getattr(self, "scale", None)
    x = window_attention(self.qhead(gs), self.khead(src), self.vhead(src), self.relative_position_bias_table,
                         self.relative_position_index, (c // self.num_heads) ** -0.5 if scale is None else scale, compute=compute)
    return self.proj(x if compute == "fp32" else x.to(gs.dtype))


def _swin_module_forward(self, x, mask=None, compute="fp32"):
    """SwinIR's WindowAttention (utils/swinir.py:226-257): the module's packed Linear, window_attention_qkv, proj, proj_drop"""
    scale = getattr(self, "scale", None)
    y = window_attention_qkv(self.qkv(x), self.relative_position_bias_table, self.relative_position_index,
                             (x.shape[-1] // self.num_heads) ** -0.5 if scale is None else scale, compute=compute, mask=mask)
    y = self.proj(y if compute == "fp32" else y.to(x.dtype))
    return self.proj_drop(y) if hasattr(self, "proj_drop") else y


def _swin_module_forward_bf16(self, x, mask=None):
    return _swin_module_forward(self, x, mask, "bf16")


def _rope_module_forward_bf16(self, gs, feat=None):
    return _rope_module_forward(self, gs, feat, "bf16")


def _module_forward_bf16(self, gs, feat=None):
    return _module_forward(self, gs, feat, "bf16")


def use_hip_attention(model, compute="fp32") -> int:
    """give every module of `model` that carries the decoder's attention attributes (qhead, khead, vhead, proj,
    relative_position_bias_table, relative_position_index, num_heads: WindowCrossAttn and GSSelfAttn) a `forward` that runs
    its three Linears, `window_attention` and `proj` with the module's own parameters; likewise every module of the RoPE
    decoder (qhead, khead, vhead, proj, num_heads, rope_freqs, rope_t_x, rope_t_y and no relative_position_bias_table:
    WindowCrossAttn and GSSelfAttn of utils/fea2gsropeamp.py, rope_mixed or not) one that runs `rope_angles` and
    `window_attention_rope`; and every module of a Swin encoder (qkv, proj, relative_position_bias_table,
    relative_position_index, num_heads and no qhead: SwinIR's WindowAttention, `forward(x, mask=None)`) one that runs its packed
    Linear, `window_attention_qkv` with the call's mask, `proj` and `proj_drop` -- unless its `attn_drop.p` is not 0 (attention
    dropout is not fused: such a module is left alone and not counted) -> the number of modules switched, all kinds.
    Parameters, buffers and state dicts are untouched.
    `compute="bf16"`: the switched modules call the ops in that mode (for a model run under bf16 autocast) and cast the result to
    their input's dtype before `proj`."""
    _check_compute(compute)
    biased, rope, swin = (_module_forward, _rope_module_forward, _swin_module_forward) if compute == "fp32" else \
        (_module_forward_bf16, _rope_module_forward_bf16, _swin_module_forward_bf16)
    n = 0
    for m in model.modules():
        if all(hasattr(m, a) for a in _ATTRS):
            m.forward = types.MethodType(biased, m)
            n += 1
        elif all(hasattr(m, a) for a in _ROPE_ATTRS) and not hasattr(m, "relative_position_bias_table"):
            m.forward = types.MethodType(rope, m)
            n += 1
        elif all(hasattr(m, a) for a in _SWIN_ATTRS) and not hasattr(m, "qhead") and getattr(getattr(m, "attn_drop", None), "p", 0) == 0:
            m.forward = types.MethodType(swin, m)
            n += 1
    return n


def constant_key_attention(mha, row):
    """`mha(x, keys, keys)[0][:, :1]` for ANY query `x` when every key / value row of a batch element is the same `row`
    (`[B,c]` or `[B,1,c]`) -> `[B,1,c]`: identical keys give every query uniform weights, so each head returns its value
    projection of `row` and the output is out_proj(v_proj(row)), independent of the query (which gets a zero gradient).
    Differentiable in `row` and in `mha`'s value and output projections.  Valid ONLY because the keys are identical.
    Needs batch_first, no dropout, no bias_k / bias_v / zero-attention rows (and is called without masks)."""
    if not isinstance(mha, torch.nn.MultiheadAttention):
        raise ValueError("mha must be an nn.MultiheadAttention")
    if not mha.batch_first or mha.dropout != 0 or mha.bias_k is not None or mha.bias_v is not None or mha.add_zero_attn:
        raise ValueError("constant_key_attention needs batch_first=True, dropout == 0 and no bias_k / bias_v / add_zero_attn")
    if row.dim() == 2:
        row = row[:, None, :]
    c = mha.embed_dim
    if row.dim() != 3 or row.shape[1] != 1 or row.shape[2] != (c if mha._qkv_same_embed_dim else mha.vdim):
        raise ValueError(f"row has shape {tuple(row.shape)}, expected [B,1,{c}]")
    if mha._qkv_same_embed_dim:
        wv = mha.in_proj_weight[2 * c:]
    else:
        wv = mha.v_proj_weight
    bv = None if mha.in_proj_bias is None else mha.in_proj_bias[2 * c:]
    return mha.out_proj(torch.nn.functional.linear(row, wv, bv))
