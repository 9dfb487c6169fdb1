"""Times gsasr_amd.window_attention against the two forms a user can write in torch, and the Fea2GS-shaped decoder of
tools/c5_models.py in its three modes (profiles/window_attention.txt); likewise gsasr_amd.window_attention_rope
against the RoPE decoder's own expression (the rotation of apply_rotary_emb, then F.scaled_dot_product_attention) and against
the explicit torch expression, in fp32 and under bf16 autocast, and the decoder with position="rope"
(profiles/window_attention_rope.txt).

    python tools/window_attention_bench.py [--reps 9] [--iters 20] [--skip-decoder] [--skip-op] [--only-hip] [--skip-bias] [--skip-rope]
    python tools/window_attention_bench.py --bf16 [--only-hip] [--skip-decoder]      # the bf16 mode alone (profiles/window_attention_bf16.txt)

`--bf16`: both ops on bf16 q, k, v under bf16 autocast -- compute="bf16", the default call (fp32 kernels behind the cast to fp32)
and torch's reference expression, interleaved; then the decoder step under autocast with attention "torch", "hip" and "hip_bf16".

Protocol: one process; every variant warmed up first; then `reps` rounds in which the variants take turns (interleaved, so a
drift of the clock hits all of them), each turn `iters` back-to-back calls between two events on the current stream; the
median of the rounds with their min and max, in milliseconds per call.  One JSON line per measurement.
`--only-hip` runs the op alone (for a counter-collecting profiler run of its kernels).

    python tools/window_attention_bench.py --masked [--only-hip] [--skip-decoder]      # profiles/window_attention_masked.txt

`--masked`: gsasr_amd.window_attention_qkv on a packed qkv with a shifted-window mask (SwinIR's WindowAttention) against the
reference's explicit expression and against F.scaled_dot_product_attention with bias + mask as `attn_mask`, in fp32 and on bf16
inputs under bf16 autocast (compute="bf16"), forward and forward + backward; then the SwinIR-shaped stack of tools/c5_models.py
(36 layers) with torch and hip attention, one forward + backward line each."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
from gsasr_amd.attention import (window_attention, window_attention_qkv, window_attention_rope, window_attention_rope_torch,      # noqa: E402
                                 window_attention_torch)

MASKED_SHAPES = [(576, 64, 6, 30, 36), (64, 256, 6, 32, 4)]     # (W, n, H, d, nW): config 5's batch in SwinIR (16 samples of 48 x 48 LR in 8 x 8 windows); 16 x 16 windows
OP_SHAPES = [(256, 144, 6, 30), (64, 256, 6, 32)]      # (W, n, H, d): config 5's batch (16 samples x 16 windows); the 16 x 16 configs
ROPE_SHAPES = [(256, 144, 6, 32), (64, 256, 6, 32)]    # the RoPE decoder's: 192 channels; EDSR / RDN / SwinIR 144 tokens, HATL 256


def sdpa_form(q, k, v, table, index, scale=None):
    """F.scaled_dot_product_attention with the bias as attn_mask, as tools/c5_models.py writes it"""
    W, nq, C = q.shape
    H = table.shape[1]
    d = C // H
    qh, kh, vh = (t.view(W, -1, H, d).transpose(1, 2) for t in (q, k, v))
    bias = table[index].permute(2, 0, 1).unsqueeze(0)
    return F.scaled_dot_product_attention(qh, kh, vh, attn_mask=bias).transpose(1, 2).reshape(W, nq, C)


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def interleaved(variants, reps, iters, warmup=3):
    for fn in variants.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(reps):
        for name, fn in variants.items():
            times[name].append(timed(fn, iters))
    return {name: dict(median_ms=statistics.median(t), min_ms=min(t), max_ms=max(t)) for name, t in times.items()}


def op_level(args, dev):
    for (W, n, H, d) in OP_SHAPES:
        g = torch.Generator().manual_seed(0)
        q, k, v, wgt = (torch.randn(W, n, H * d, generator=g).to(dev) for _ in range(4))
        side = int(round(n ** 0.5))
        T = (2 * side - 1) ** 2
        table = (0.5 * torch.randn(T, H, generator=g)).to(dev)
        yy, xx = torch.meshgrid(torch.arange(side), torch.arange(side), indexing="ij")
        cy, cx = yy.flatten(), xx.flatten()
        index = ((cy[:, None] - cy[None, :] + side - 1) * (2 * side - 1) + cx[:, None] - cx[None, :] + side - 1).to(dev)
        forms = {"hip": window_attention} if args.only_hip else {"hip": window_attention, "torch_explicit": window_attention_torch, "torch_sdpa": sdpa_form}
        leaves = [t.clone().requires_grad_(True) for t in (q, k, v, table)]

        def fwd(fn):
            with torch.no_grad():
                return fn(q, k, v, table, index)

        def fwd_bwd(fn):
            out = fn(*leaves, index)
            torch.autograd.grad(out, leaves, wgt)

        for what, run in (("forward", fwd), ("forward+backward", fwd_bwd)):
            res = interleaved({name: (lambda f=fn: run(f)) for name, fn in forms.items()}, args.reps, args.iters)
            for name, r in res.items():
                print(json.dumps(dict(level="op", shape=dict(W=W, n=n, H=H, d=d), what=what, form=name, **{k: round(x, 4) for k, x in r.items()})), flush=True)


def rope_reference_form(q, k, v, angles, scale=None):
    """the RoPE modules' own expression (utils/fea2gsropeamp.py): head split, complex pairs times cis through fp32 temporaries,
    `type_as`, bias-free F.scaled_dot_product_attention, head merge"""
    W, nq, C = q.shape
    H = angles.shape[0]
    d = C // H
    qh, kh, vh = (t.view(W, -1, H, d).permute(0, 2, 1, 3) for t in (q, k, v))
    cis = torch.polar(torch.ones_like(angles), angles)
    qh, kh = (torch.view_as_real(torch.view_as_complex(x.float().reshape(*x.shape[:-1], -1, 2)) * cis[:, :x.shape[2]]).flatten(3).type_as(x)
              for x in (qh, kh))
    return F.scaled_dot_product_attention(qh, kh, vh).transpose(1, 2).reshape(W, nq, C)


def rope_op_level(args, dev):
    for (W, n, H, d) in ROPE_SHAPES:
        g = torch.Generator().manual_seed(0)
        q, k, v, wgt = (torch.randn(W, n, H * d, generator=g).to(dev) for _ in range(4))
        side = int(round(n ** 0.5))
        t = torch.arange(n, dtype=torch.float32)
        freqs = torch.rand(2, H, d // 2, generator=g)                  # (magnitudes up to 1: angles up to 2 (side - 1) rad)
        angles = ((t % side)[None, :, None] * freqs[0][:, None, :] + torch.div(t, side, rounding_mode="floor")[None, :, None] * freqs[1][:, None, :]).to(dev)
        forms = {"hip": window_attention_rope}
        if not args.only_hip:
            forms.update(torch_explicit=window_attention_rope_torch, torch_reference=rope_reference_form)
            # the biased op on the same q, k, v (a table of the window's relative offsets; its 4th leaf is the table): what the rotation costs
            table = (0.5 * torch.randn((2 * side - 1) ** 2, H, generator=g)).to(dev)
            cy, cx = torch.div(t, side, rounding_mode="floor").long(), (t % side).long()
            index = ((cy[:, None] - cy[None, :] + side - 1) * (2 * side - 1) + cx[:, None] - cx[None, :] + side - 1).to(dev)
            forms["hip_biased_op"] = lambda a, b, c, ang: window_attention(a, b, c, table if ang is angles else ang, index)
        for amp in (False, True):
            cast = (lambda x: x.bfloat16()) if amp else (lambda x: x)
            qa, ka, va, wa = (cast(x) for x in (q, k, v, wgt))
            leaves = [x.clone().requires_grad_(True) for x in (qa, ka, va)] + [angles.clone().requires_grad_(True)]
            if not args.only_hip:
                bias_leaves = leaves[:3] + [table.clone().requires_grad_(True)]

            def fwd(fn):
                with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
                    return fn(qa, ka, va, angles)

            def fwd_bwd(fn):
                ls = bias_leaves if fn is forms.get("hip_biased_op") else leaves
                with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
                    out = fn(*ls)
                torch.autograd.grad(out, ls, wa.to(out.dtype))

            for what, run in (("forward", fwd), ("forward+backward", fwd_bwd)):
                res = interleaved({name: (lambda f=fn: run(f)) for name, fn in forms.items()}, args.reps, args.iters)
                for name, r in res.items():
                    print(json.dumps(dict(level="op", position="rope", precision="bf16 autocast" if amp else "fp32", shape=dict(W=W, n=n, H=H, d=d), what=what,
                                          form=name, **{k: round(x, 4) for k, x in r.items()})), flush=True)


def bf16_op_level(args, dev):
    """both ops on bf16 inputs under bf16 autocast: compute="bf16" / the default call / torch's reference expression"""
    for kind, (W, n, H, d) in [("rope", s) for s in ROPE_SHAPES] + [("bias", s) for s in OP_SHAPES] + [("bias", (256, 144, 6, 32))]:
        g = torch.Generator().manual_seed(0)
        q, k, v, wgt = (torch.randn(W, n, H * d, generator=g).to(dev).bfloat16() for _ in range(4))
        side = int(round(n ** 0.5))
        t = torch.arange(n, dtype=torch.float32)
        cy, cx = torch.div(t, side, rounding_mode="floor").long(), (t % side).long()
        if kind == "rope":
            freqs = torch.rand(2, H, d // 2, generator=g)
            param = ((t % side)[None, :, None] * freqs[0][:, None, :] + torch.div(t, side, rounding_mode="floor")[None, :, None] * freqs[1][:, None, :]).to(dev)
            tail, op, ref = (), window_attention_rope, rope_reference_form
        else:
            param = (0.5 * torch.randn((2 * side - 1) ** 2, H, generator=g)).to(dev)
            tail = (((cy[:, None] - cy[None, :] + side - 1) * (2 * side - 1) + cx[:, None] - cx[None, :] + side - 1).to(dev),)
            op, ref = window_attention, lambda a, b, c, tb, ix: sdpa_form(a, b, c, tb.to(a.dtype), ix)      # (the bias as a bf16 mask, as autocast hands it)
        forms = {"hip_bf16": lambda *a: op(*a, compute="bf16"), "hip_default": op}
        if not args.only_hip:
            forms["torch_reference"] = ref
        leaves = [x.clone().requires_grad_(True) for x in (q, k, v, param)]

        def fwd(fn):
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                return fn(q, k, v, param, *tail)

        def fwd_bwd(fn):
            with torch.autocast("cuda", dtype=torch.bfloat16):
                out = fn(*leaves, *tail)
            torch.autograd.grad(out, leaves, wgt.to(out.dtype))

        for what, run in (("forward", fwd), ("forward+backward", fwd_bwd)):
            res = interleaved({name: (lambda f=fn: run(f)) for name, fn in forms.items()}, args.reps, args.iters)
            for name, r in res.items():
                print(json.dumps(dict(level="op", position=kind, precision="bf16 inputs, bf16 autocast", shape=dict(W=W, n=n, H=H, d=d), what=what,
                                      form=name, **{k: round(x, 4) for k, x in r.items()})), flush=True)


def swin_explicit_form(qkv, table, index, mask, scale=None):
    """the expression of SwinIR's WindowAttention.forward (utils/swinir.py:233-254) between its two Linears"""
    W, n, C3 = qkv.shape
    H = table.shape[1]
    d = C3 // (3 * H)
    q, k, v = qkv.reshape(W, n, 3, H, d).permute(2, 0, 3, 1, 4).unbind(0)
    attn = (q * d ** -0.5) @ k.transpose(-2, -1)
    attn = attn + table[index.view(-1)].view(n, n, -1).permute(2, 0, 1).contiguous().unsqueeze(0)
    nW = mask.shape[0]
    attn = (attn.view(W // nW, nW, H, n, n) + mask.unsqueeze(1).unsqueeze(0)).view(-1, H, n, n)
    return (torch.softmax(attn, dim=-1) @ v).transpose(1, 2).reshape(W, n, C3 // 3)


def swin_sdpa_form(qkv, table, index, mask, scale=None):
    """F.scaled_dot_product_attention with bias + mask as attn_mask ([nW, H, n, n], broadcast over the samples)"""
    W, n, C3 = qkv.shape
    H = table.shape[1]
    d = C3 // (3 * H)
    nW = mask.shape[0]
    q, k, v = qkv.reshape(W // nW, nW, n, 3, H, d).permute(3, 0, 1, 4, 2, 5).unbind(0)
    both = (table[index].permute(2, 0, 1).unsqueeze(0) + mask.unsqueeze(1)).to(q.dtype)
    return F.scaled_dot_product_attention(q, k, v, attn_mask=both).permute(0, 1, 3, 2, 4).reshape(W, n, C3 // 3)


def shifted_window_mask(side, nW, dev):
    """[nW, side^2, side^2] of 0 / -100: the regions of a half-window shift, as SwinIR's calculate_mask labels them, on an image of
    sqrt(nW) x sqrt(nW) windows"""
    per = int(round(nW ** 0.5))
    size, shift = per * side, side // 2
    label = torch.zeros(size, size)
    cuts = (slice(0, -side), slice(-side, -shift), slice(-shift, None))
    for a, ys in enumerate(cuts):
        for b, xs in enumerate(cuts):
            label[ys, xs] = 3 * a + b
    win = label.view(per, side, per, side).permute(0, 2, 1, 3).reshape(nW, side * side)
    diff = win[:, None, :] - win[:, :, None]
    return torch.where(diff != 0, -100.0, 0.0).to(dev)


def masked_op_level(args, dev):
    for (W, n, H, d, nW) in MASKED_SHAPES:
        g = torch.Generator().manual_seed(0)
        C, side = H * d, int(round(n ** 0.5))
        qkv32, wgt32 = torch.randn(W, n, 3 * C, generator=g).to(dev), torch.randn(W, n, C, generator=g).to(dev)
        table = (0.5 * torch.randn((2 * side - 1) ** 2, H, generator=g)).to(dev)
        yy, xx = torch.meshgrid(torch.arange(side), torch.arange(side), indexing="ij")
        cy, cx = yy.flatten(), xx.flatten()
        index = ((cy[:, None] - cy[None, :] + side - 1) * (2 * side - 1) + cx[:, None] - cx[None, :] + side - 1).to(dev)
        mask = shifted_window_mask(side, nW, dev)
        for amp in (False, True):
            qkv, wgt = (qkv32.bfloat16(), wgt32.bfloat16()) if amp else (qkv32, wgt32)
            hip = (lambda a, t, i, m: window_attention_qkv(a, t, i, compute="bf16", mask=m)) if amp else (lambda a, t, i, m: window_attention_qkv(a, t, i, mask=m))
            forms = {"hip": hip} if args.only_hip else {"hip": hip, "torch_explicit": swin_explicit_form, "torch_sdpa": swin_sdpa_form}
            leaves = [qkv.clone().requires_grad_(True), table.clone().requires_grad_(True)]

            def fwd(fn):
                with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
                    return fn(qkv, table, index, mask)

            def fwd_bwd(fn):
                with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
                    out = fn(*leaves, index, mask)
                torch.autograd.grad(out, leaves, wgt.to(out.dtype))

            for what, run in (("forward", fwd), ("forward+backward", fwd_bwd)):
                res = interleaved({name: (lambda f=fn: run(f)) for name, fn in forms.items()}, args.reps, args.iters)
                for name, r in res.items():
                    print(json.dumps(dict(level="op", position="bias+mask, packed qkv", precision="bf16 inputs, bf16 autocast" if amp else "fp32",
                                          shape=dict(W=W, n=n, H=H, d=d, nW=nW), what=what, form=name, **{k: round(x, 4) for k, x in r.items()})), flush=True)


def swin_stack_level(args, dev):
    """the SwinIR-shaped stack (36 layers, dim 180, window 8, alternating shift) on config 5's batch, fp32 and bf16 autocast"""
    import c5_models
    torch.manual_seed(0)
    nets = {}
    for name in ("torch", "hip", "hip_bf16"):
        nets[name] = c5_models.SwinShapedStack(attention=name).to(dev)
        nets[name].load_state_dict(nets["torch"].state_dict())
    x = torch.randn(16, 48, 48, 180, device=dev)
    for amp in (False, True):
        def step(net):
            for p in net.parameters():
                p.grad = None
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
                loss = net(x).float().square().mean()
            loss.backward()

        run = {name: (lambda m=net: step(m)) for name, net in nets.items() if amp or name != "hip_bf16"}
        for name, r in interleaved(run, max(3, args.reps // 2), 2, warmup=2).items():
            print(json.dumps(dict(level="swin stack", layers=36, precision="bf16 autocast" if amp else "fp32", x=[16, 48, 48, 180], what="forward+backward",
                                  mode=f"attention={name}", **{k: round(v, 3) for k, v in r.items()})), flush=True)


def bf16_decoder_level(args, dev, position):
    """the decoder step under bf16 autocast: attention "torch", "hip" (fp32 kernels behind the cast) and "hip_bf16" """
    import c5_models
    torch.manual_seed(0)
    extra = dict(position="rope", channel=192) if position == "rope" else {}
    nets = {}
    for name in ("torch", "hip", "hip_bf16"):
        nets[name] = c5_models.Fea2GSDecoder(attention=name, scale_attention="constant", **extra).to(dev)
        nets[name].load_state_dict(nets["torch"].state_dict())
    feat = torch.randn(16, 64, 48, 48, device=dev)
    scale = torch.full((16,), 4.0, device=dev)

    def step(net):
        for p in net.parameters():
            p.grad = None
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = net(feat, scale).float().square().mean()
        loss.backward()

    res = interleaved({name: (lambda m=net: step(m)) for name, net in nets.items()}, max(3, args.reps // 2), 2, warmup=2)
    for name, r in res.items():
        print(json.dumps(dict(level="decoder", position=position, precision="bf16 autocast", feat=[16, 64, 48, 48], what="forward+backward",
                              mode=f"attention={name},scale_attention=constant", **{k: round(x, 3) for k, x in r.items()})), flush=True)


def decoder_level(args, dev, position="bias"):
    import c5_models
    torch.manual_seed(0)
    modes = {"default": dict(), "attention=hip": dict(attention="hip"), "attention=hip,scale_attention=constant": dict(attention="hip", scale_attention="constant")}
    if position == "rope":     # 192 channels, full depth; the constant-key form with the torch attention as well
        modes = {"default": dict(), "scale_attention=constant": dict(scale_attention="constant"), **{k: v for k, v in modes.items() if k != "default"}}
        modes = {name: dict(kw, position="rope", channel=192) for name, kw in modes.items()}
    nets = {}
    for name, kw in modes.items():
        nets[name] = c5_models.Fea2GSDecoder(**kw).to(dev)
        nets[name].load_state_dict(nets["default"].state_dict())
    feat = torch.randn(16, 64, 48, 48, device=dev)
    scale = torch.full((16,), 4.0, device=dev)

    def step(net):
        for p in net.parameters():
            p.grad = None
        net(feat, scale).square().mean().backward()

    res = interleaved({name: (lambda m=net: step(m)) for name, net in nets.items()}, max(3, args.reps // 2), 2, warmup=2)
    for name, r in res.items():
        print(json.dumps(dict(level="decoder", position=position, feat=[16, 64, 48, 48], what="forward+backward", mode=name, **{k: round(x, 3) for k, x in r.items()})), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--skip-decoder", action="store_true")
    ap.add_argument("--skip-op", action="store_true", help="the decoder level alone")
    ap.add_argument("--only-hip", action="store_true")
    ap.add_argument("--skip-bias", action="store_true", help="leave out the biased op and its decoder")
    ap.add_argument("--skip-rope", action="store_true", help="leave out the rotary op and its decoder")
    ap.add_argument("--bf16", action="store_true", help="the bf16 mode alone: both ops and the decoder step under bf16 autocast")
    ap.add_argument("--masked", action="store_true", help="the masked op on a packed qkv and the SwinIR-shaped stack alone")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    if args.masked:
        if not args.skip_op:
            masked_op_level(args, dev)
        if not args.skip_decoder and not args.only_hip:
            swin_stack_level(args, dev)
        return
    if args.bf16:
        if not args.skip_op:
            bf16_op_level(args, dev)
        if not args.skip_decoder and not args.only_hip:
            for position in ("rope", "bias"):
                bf16_decoder_level(args, dev, position)
        return
    if not args.skip_bias and not args.skip_op:
        op_level(args, dev)
    if not args.skip_rope and not args.skip_op:
        rope_op_level(args, dev)
    if not args.skip_decoder and not args.only_hip:
        if not args.skip_bias:
            decoder_level(args, dev)
        if not args.skip_rope:
            decoder_level(args, dev, "rope")


if __name__ == "__main__":
    main()
