#!/usr/bin/env python
"""What the SSIM loss costs: device time, on the same GPU, of

  (a) the SSIM term alone, value + d loss / d image from a stored image and its target:
        hip      gsasr_ssim_loss (k_ssim_stats, k_ssim_grad, k_ssim_reduce) through gsasr_amd.ssim_loss + backward
        torch    the fp32 torch expression of gsasr_amd/ssim.py (pytorch_msssim's: depthwise convolutions and elementwise kernels)
                 + autograd -- what a user of SSIMLoss runs today
      at config 5's shape (batch 16 x 3 x 192^2) and at 3 x 720^2;
  (b) the whole training call at config 5 (16 x 192^2, 36 864 Gaussians each), raw decoder parameters and the target in, the loss and
      d loss / d gs_parameters out:
        hip      generate_2D_gaussian_splatting_batch_loss(loss='l1', ssim_weight=1) + backward: one autograd node
        torch    generate_2D_gaussian_splatting_batch + F.l1_loss + the torch SSIM + backward

hipEvent timing around batches of calls, the two variants alternated round by round in one process, at least `--seconds` of work per
variant; the figure is the median of the rounds, the spread their range.  Before timing the two variants must agree (the loss to
2e-5; the image gradient to 1e-4 of its max-abs, the parameter gradient to the project's 2e-4).  The condition per shape: hip's
median is below torch's minimum.

    python tools/ssim_bench.py [--seconds 0.5] [--rounds 9] [--only NAME] [--out profiles/ssim_loss_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gsasr_amd import _cabi, ssim_loss, synthetic  # noqa: E402
from gsasr_amd import gaussian_splatting as gsp  # noqa: E402
from gsasr_amd import ssim as ssim_mod  # noqa: E402

DMAX = 0.1


def batch_ms(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def torch_ssim(x, y, weight):
    """SSIMLoss on a batch of equal sizes: the mean over the batch of the per-sample means is the mean over everything"""
    return weight * (1.0 - ssim_mod.ssim_map(x, y).mean())


def term_shape(batch, side, dev):
    g = torch.Generator().manual_seed(side)
    x = torch.rand(batch, 3, side, side, generator=g).to(dev).requires_grad_(True)
    y = (x.detach() + 0.1 * torch.randn(batch, 3, side, side, generator=g).to(dev)).clamp(0, 1)

    def hip():
        value = ssim_loss(x, y, 1.0)
        return value, torch.autograd.grad(value, x)[0]

    def torch_():
        value = torch_ssim(x, y, 1.0)
        return value, torch.autograd.grad(value, x)[0]

    return {"hip": hip, "torch": torch_}, 1e-4


def step_shape(dev, lr=48, gpp=16, scale=4.0, B=16):
    side = int(lr * scale)
    p = torch.stack([synthetic.gs_parameters(lr, lr, seed=b, gpp=gpp) for b in range(B)]).to(dev).requires_grad_(True)
    sizes, scales = [(side, side)] * B, [scale] * B
    sms = torch.tensor([[scale, scale]] * B, device=dev)
    t = torch.rand(B, 3, side, side, generator=torch.Generator().manual_seed(3)).to(dev)

    def hip():
        value = gsp.generate_2D_gaussian_splatting_batch_loss(sizes, p, scales, sms, t, loss="l1", dmax=DMAX, ssim_weight=1.0)
        return value, torch.autograd.grad(value, p)[0]

    def torch_():
        out = gsp.generate_2D_gaussian_splatting_batch(sizes, p, scales, sms, dmax=DMAX)
        value = F.l1_loss(out, t) + torch_ssim(out, t, 1.0)
        return value, torch.autograd.grad(value, p)[0]

    return {"hip": hip, "torch": torch_}, 2e-4


def agree(a, b, rtol, name):
    (va, ga), (vb, gb) = a, b
    va, vb = float(va.detach()), float(vb.detach())
    assert abs(va - vb) <= 2e-5 * abs(vb), (name, va, vb)
    rel = float((ga - gb).abs().max() / gb.abs().max())
    assert rel <= rtol, (name, rel)
    return {"loss_hip": va, "loss_torch": vb, "gradient_rel_err": rel}


def shapes(dev):
    return {
        "(a) SSIM term, c5: 16 x 3 x 192^2": lambda: term_shape(16, 192, dev),
        "(a) SSIM term, 3 x 720^2": lambda: term_shape(1, 720, dev),
        "(b) training call, c5: 16 x 192^2, 36 864 each, l1 + ssim": lambda: step_shape(dev),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5, help="device work per variant and shape, at least")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--only", default=None, help="run the shapes whose name contains this (e.g. for a kernel trace of one shape)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/ssim_bench.py measures on the GPU; there is none")
    dev = torch.device("cuda:0")
    report = {"device": torch.cuda.get_device_name(dev), "rounds": args.rounds, "seconds_per_variant": args.seconds, "dmax": DMAX,
              "shapes": {}}
    for name, make in shapes(dev).items():
        if args.only and args.only not in name:
            continue
        fns, rtol = make()
        variants = tuple(fns)
        row = {"agreement": agree(fns["hip"](), fns["torch"](), rtol, name)}
        counts = {}
        for v in variants:
            for _ in range(3):
                fns[v]()
            batch_ms(fns[v], 5)                      # (cold: allocator, pool and code objects settle)
            ms = batch_ms(fns[v], 20)                # warm: what the call counts are sized from, with a margin
            counts[v] = max(5, int(1.1 * args.seconds * 1000.0 / ms / args.rounds) + 1)
        while True:
            times = {v: [] for v in variants}
            for _ in range(args.rounds):             # alternated: hip torch hip torch ...
                for v in variants:
                    times[v].append(batch_ms(fns[v], counts[v]))
            short = [v for v in variants if sum(times[v]) * counts[v] / 1000.0 < args.seconds]
            if not short:
                break
            for v in short:                          # a variant that fell short of `--seconds` of work: all rounds again, longer
                counts[v] = int(counts[v] * 1.25 * args.seconds / (sum(times[v]) * counts[v] / 1000.0)) + 1
        for v in variants:
            t = times[v]
            row[v] = {"call_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t), "calls_per_round": counts[v],
                      "total_s": sum(t) * counts[v] / 1000.0}
        row["torch_over_hip"] = row["torch"]["call_ms"] / row["hip"]["call_ms"]
        row["hip_median_below_torch_minimum"] = row["hip"]["call_ms"] < row["torch"]["min_ms"]
        report["shapes"][name] = row
        print(f"{name} | call ms | " + " | ".join(
            f"{v} {row[v]['call_ms']:.4f} [{row[v]['min_ms']:.4f}, {row[v]['max_ms']:.4f}]" for v in variants) +
            f" | torch / hip {row['torch_over_hip']:.2f}", flush=True)
        del fns
        gsp.deferred_asserts.flush()
        _cabi.clear_workspace_pool()
        torch.cuda.empty_cache()
    text = json.dumps(report, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)
    lost = [n for n, r in report["shapes"].items() if not r["hip_median_below_torch_minimum"]]
    if lost:
        sys.exit("the HIP path is not ahead on: " + "; ".join(lost))


if __name__ == "__main__":
    main()
