#!/usr/bin/env python
"""What the 8-bit output costs or saves: device time of the forward in three forms, on one plan each,

    (a) float   the planar fp32 image as today                          gsasr_splat_forward, CHW, overwrite
    (b) torch   (a) + the reference's epilogue as torch ops on the GPU  clamp(0, 1) -> [[2, 1, 0]] -> HWC -> (x * 255).round() -> uint8
    (c) u8      the bytes stored by the forward kernels themselves      gsasr_splat_forward_u8, b g r order

at the 720^2 x4 paper shape with 16 Gaussians per LR pixel and at config 3 (6144^2 x12).  hipEvent timing around batches of
calls, the variants alternated round by round in one process, at least `--seconds` of work per variant in all; the figure is
the median of the rounds, the spread their range.

    python tools/u8_epilogue.py [--seconds 0.6] [--rounds 9] [--out profiles/u8_epilogue.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gsasr_amd import _cabi, synthetic  # noqa: E402

SHAPES = {
    # name: (h_lr, w_lr, scale, Gaussians per LR pixel, dmax)
    "720^2 x4, 16 per LR px": (180, 180, 4.0, 16, 0.1),
    "config 3: 6144^2 x12": (512, 512, 12.0, 1, 0.1),
}


def variants(plan, H, W, dev):
    img = torch.empty(3, H, W, device=dev)
    out = torch.empty(H, W, 3, dtype=torch.uint8, device=dev)

    def a():
        _cabi.forward(plan, img, overwrite=True, chw=True)

    def b():
        _cabi.forward(plan, img, overwrite=True, chw=True)
        return (img.clamp(0, 1)[[2, 1, 0]].permute(1, 2, 0) * 255.0).round().to(torch.uint8)

    def c():
        _cabi.forward_u8(plan, bgr=True, out=out)

    return {"float": a, "torch": b, "u8": c}, img, out


def batch_ms(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.6, help="device work per variant and shape, at least")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/u8_epilogue.py measures on the GPU; there is none")
    dev = torch.device("cuda:0")
    report = {"device": torch.cuda.get_device_name(dev), "rounds": args.rounds, "seconds_per_variant": args.seconds, "shapes": {}}
    for name, (h_lr, w_lr, scale, gpp, dmax) in SHAPES.items():
        sig, xy, col, H, W = synthetic.kernel_inputs(h_lr, w_lr, scale, seed=0, gpp=gpp)
        plan = _cabi.plan(sig.to(dev), xy.to(dev), col.to(dev), H, W, dmax, flags=_cabi.FLAG_FORWARD_ONLY)
        fns, img, out = variants(plan, H, W, dev)
        # the three forms give the same picture (one level where a sum lies on a rounding boundary)
        ref = fns["torch"]()
        fns["u8"]()
        diff = (ref.int() - out.int()).abs()
        assert int(diff.max()) <= 1, int(diff.max())
        counts = {}
        for k, fn in fns.items():       # warm-up, and the calls per round that make `seconds` in all
            for _ in range(3):
                fn()
            ms = batch_ms(fn, 5)
            counts[k] = max(5, int(args.seconds * 1000.0 / ms / args.rounds) + 1)
        times = {k: [] for k in fns}
        for _ in range(args.rounds):    # alternated: a b c a b c ...
            for k, fn in fns.items():
                times[k].append(batch_ms(fn, counts[k]))
        row = {"H": H, "W": W, "gaussians": int(sig.shape[0]), "differing_values": int((diff != 0).sum()),
               "bytes_float_image": 12 * H * W, "bytes_u8_image": 3 * H * W}
        for k, t in times.items():
            row[k] = {"ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t), "calls_per_round": counts[k],
                      "total_s": sum(t) * counts[k] / 1000.0}
        row["u8_not_slower_than_float"] = row["u8"]["ms"] <= row["float"]["ms"] + (row["float"]["max_ms"] - row["float"]["min_ms"])
        report["shapes"][name] = row
        print(f"{name}: " + ", ".join(f"{k} {row[k]['ms']:.4f} ms [{row[k]['min_ms']:.4f}, {row[k]['max_ms']:.4f}]" for k in fns)
              + f"; u8 <= float + float's spread: {row['u8_not_slower_than_float']}", flush=True)
        del plan, img, out, ref
    text = json.dumps(report, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
