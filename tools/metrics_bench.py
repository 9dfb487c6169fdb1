#!/usr/bin/env python
"""What the validation metrics cost on the device: at 720 x 720 (the paper benchmark's extent) and 2040 x 1356,

  ssim_value   gsasr_ssim_loss, value only (k_ssim_stats<false>, k_ssim_reduce) on a float [3,h,w] image and target: the nearest
               kernel the library had -- the same window work on 12 bytes per pixel of input where the metrics read 6
  metrics_rgb  gsasr_image_metrics, PSNR + SSIM of the three channels (k_metric_stats<false>, k_metric_reduce)
  metrics_y    gsasr_image_metrics with GSASR_METRIC_Y | GSASR_METRIC_BGR and crop_border 4 (k_metric_stats<true>, k_metric_reduce):
               the setting of the paper's tables, one channel

Every variant is the bare C call on descriptors built once (no allocation, no tensor work per call).  hipEvent timing around
batches of calls, the variants alternated round by round in one process after a warm-up; the figure is the median of the rounds
(at least 20), the spread their range.  Nothing is asserted on the times; the expectations (RGB not slower than the value-only
SSIM loss, Y clearly faster) are reported as booleans.

    python tools/metrics_bench.py [--rounds 21] [--calls 50] [--out profiles/metrics_bench.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gsasr_amd import _cabi  # noqa: E402


def batch_ms(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def variants(h, w, dev):
    L = _cabi.lib()
    g = torch.Generator().manual_seed(h)
    ref = torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8)
    img = (ref.int() + torch.randint(-4, 5, (h, w, 3), generator=g)).clamp(0, 255).to(torch.uint8)
    ref, img = ref.to(dev), img.to(dev)
    x, y = (img.permute(2, 0, 1).float() / 255.0).contiguous(), (ref.permute(2, 0, 1).float() / 255.0).contiguous()
    stream = _cabi._stream(dev)
    keep = [ref, img, x, y]

    ds = _cabi.make_ssim(1, h, w, None, h, 0, 1.0, 0)
    ds.img, ds.target, ds.grad_img = x.data_ptr(), y.data_ptr(), None
    scratch = torch.empty(int(L.gsasr_ssim_scratch_bytes(ctypes.byref(ds))) // 4, dtype=torch.float32, device=dev)
    loss = torch.empty(2, dtype=torch.float32, device=dev)
    ds.loss, ds.scratch = loss.data_ptr(), scratch.data_ptr()
    keep += [scratch, loss, ds]
    fns = {"ssim_value": lambda: _cabi.check(L.gsasr_ssim_loss(ctypes.byref(ds), stream), "gsasr_ssim_loss")}
    outs = {"ssim_value": loss}

    def metric(name, flags, cb):
        d = _cabi.make_metrics(1, h, w, None, cb, _cabi.METRIC_PSNR | _cabi.METRIC_SSIM | flags)
        sc = torch.empty(int(L.gsasr_metrics_scratch_bytes(ctypes.byref(d))) // 8, dtype=torch.float64, device=dev)
        out = torch.empty(1, 2, dtype=torch.float64, device=dev)
        d.img, d.ref, d.out, d.scratch = img.data_ptr(), ref.data_ptr(), out.data_ptr(), sc.data_ptr()
        keep.extend([d, sc, out])
        fns[name] = lambda: _cabi.check(L.gsasr_image_metrics(ctypes.byref(d), stream), "gsasr_image_metrics")
        outs[name] = out

    metric("metrics_rgb", 0, 0)
    metric("metrics_y", _cabi.METRIC_Y | _cabi.METRIC_BGR, 4)
    return fns, outs, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=21)
    ap.add_argument("--calls", type=int, default=50, help="calls per timed batch")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/metrics_bench.py measures on the GPU; there is none")
    dev = torch.device("cuda:0")
    report = {"device": torch.cuda.get_device_name(dev), "rounds": args.rounds, "calls_per_round": args.calls, "shapes": {}}
    for h, w in ((720, 720), (1356, 2040)):
        fns, outs, keep = variants(h, w, dev)
        for fn in fns.values():                       # warm-up: code objects, clocks
            batch_ms(fn, 20)
        times = {v: [] for v in fns}
        for _ in range(args.rounds):                  # alternated: ssim_value metrics_rgb metrics_y ssim_value ...
            for v, fn in fns.items():
                times[v].append(batch_ms(fn, args.calls))
        row = {v: {"call_us": 1e3 * statistics.median(t), "min_us": 1e3 * min(t), "max_us": 1e3 * max(t)} for v, t in times.items()}
        row["values"] = {v: [float(a) for a in o.flatten().cpu()] for v, o in outs.items()}
        row["rgb_not_slower_than_ssim_value"] = row["metrics_rgb"]["call_us"] <= row["ssim_value"]["call_us"]
        row["y_over_rgb"] = row["metrics_y"]["call_us"] / row["metrics_rgb"]["call_us"]
        report["shapes"][f"{w} x {h}"] = row
        print(f"{w} x {h} | call us | " + " | ".join(f"{v} {row[v]['call_us']:.1f} [{row[v]['min_us']:.1f}, {row[v]['max_us']:.1f}]" for v in fns),
              flush=True)
        del fns, outs, keep
    text = json.dumps(report, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
