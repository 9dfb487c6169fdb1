"""Times gsasr_amd.window_attention against the two forms a user can write in torch, and the Fea2GS-shaped decoder of
tools/c5_models.py in its three modes (profiles/window_attention.txt).

    python tools/window_attention_bench.py [--reps 9] [--iters 20] [--skip-decoder] [--only-hip]

Protocol: one process; every variant warmed up first; then `reps` rounds in which the variants take turns (interleaved, so a
drift of the clock hits all of them), each turn `iters` back-to-back calls between two events on the current stream; the
median of the rounds with their min and max, in milliseconds per call.  One JSON line per measurement.
`--only-hip` runs the op alone (for a counter-collecting profiler run of its kernels)."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
from gsasr_amd.attention import window_attention, window_attention_torch      # noqa: E402

OP_SHAPES = [(256, 144, 6, 30), (64, 256, 6, 32)]      # (W, n, H, d): config 5's batch (16 samples x 16 windows); the 16 x 16 configs


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


def decoder_level(args, dev):
    import c5_models
    torch.manual_seed(0)
    modes = {"default": dict(), "attention=hip": dict(attention="hip"), "attention=hip,scale_attention=constant": dict(attention="hip", scale_attention="constant")}
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
        print(json.dumps(dict(level="decoder", feat=[16, 64, 48, 48], what="forward+backward", mode=name, **{k: round(x, 3) for k, x in r.items()})), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--skip-decoder", action="store_true")
    ap.add_argument("--only-hip", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    op_level(args, dev)
    if not args.skip_decoder and not args.only_hip:
        decoder_level(args, dev)


if __name__ == "__main__":
    main()
