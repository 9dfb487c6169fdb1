#!/usr/bin/env python
"""What one window per sample of a batch costs: device time of a whole step -- prologue + plan + forward +
backward, raw decoder parameters in, their gradient out -- for three ways to the same `[B, 3, h, w]` patches,

    batch    one canvas whose slots are the windows, each on its own full grid     gsasr_step_forward_view, dims.batch = B
    loop     B single-view steps, one after the other                              gsasr_step_forward_view, B times
    whole    the whole batch rendered on a canvas of full grids, then sliced       gsasr_step_forward (the gradient zero-padded)

on config 5's batch -- 16 samples of 48^2 LR pixels at 16 Gaussians per LR pixel (36 864 each) -- at x8 (full grids 384^2,
windows 192^2) and at x4 (192^2, 96^2), the windows at random origins.  The backward kernel of each variant is the one the
host functions' rule picks for it (gaussian_splatting._backward_kernel: the Gaussians a window can expect), reported next to
the numbers.  hipEvent timing around batches of steps, the variants alternated round by round in one process, at least
`--seconds` of work per variant; the figure is the median of the rounds, the spread their range.

    python tools/batch_view_bench.py [--seconds 0.5] [--rounds 9] [--out profiles/batch_view_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gsasr_amd import _cabi, synthetic  # noqa: E402
from gsasr_amd import gaussian_splatting as gsp  # noqa: E402

B, LR, GPP, DMAX = 16, 48, 16, 0.1
SHAPES = {"x8: 192^2 windows of 384^2 grids": (8.0, 192), "x4: 96^2 windows of 192^2 grids": (4.0, 96)}
VARIANTS = ("batch", "loop", "whole")
KERNELS = {_cabi.FLAG_BWD_GAUSSIAN: "gaussian", _cabi.FLAG_BWD_TILE: "tile", _cabi.FLAG_BWD_HOME: "home"}


def batch_ms(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def variants_of(p, steps, full, win, origins, wgt, dev):
    """{variant: (step callable -> (patches [B,3,win,win], gradient [B,N,9]), backward kernel's name)}"""
    n_per = p.shape[1]
    live = max(1, n_per * win * win // (full * full))
    k_batch = gsp._backward_kernel(B * win * win, B * live)
    k_one = gsp._backward_kernel(win * win, live)
    k_whole = gsp._backward_kernel(B * full * full, B * n_per, gsp._batch_shape(n_per, [(full, full)] * B, DMAX))
    views = [(full, full, y0, x0) for y0, x0 in origins]
    pad = torch.zeros(B, 3, full, full, device=dev)
    for b, (y0, x0) in enumerate(origins):
        pad[b, :, y0:y0 + win, x0:x0 + win] = wgt[b]
    ones = [p[b].contiguous() for b in range(B)]
    one_steps = [steps[b: b + 1].clone() for b in range(B)]

    def batch():
        img, plan = _cabi.batch_forward(p, steps, [(win, win)] * B, DMAX, gsp._plan_flags(True, k_batch), views=views)
        return img[:, :, :win], _cabi.batch_backward(plan, p, steps, wgt, chw=True)

    def loop():
        imgs, grads = [], []
        for b in range(B):
            img, plan = _cabi.step_forward(ones[b], one_steps[b], win, win, DMAX, gsp._plan_flags(True, k_one), view=views[b])
            imgs.append(img)
            grads.append(_cabi.step_backward(plan, ones[b], one_steps[b], wgt[b], chw=True))
        return imgs, grads

    def whole():
        img, plan = _cabi.batch_forward(p, steps, [(full, full)] * B, DMAX, gsp._plan_flags(True, k_whole))
        return img, _cabi.batch_backward(plan, p, steps, pad, chw=True)

    def patches(v, out):
        if v == "loop":
            return torch.stack(out[0]), torch.stack(out[1])
        if v == "whole":
            return torch.stack([out[0][b, :, y0:y0 + win, x0:x0 + win] for b, (y0, x0) in enumerate(origins)]), out[1]
        return out

    return {"batch": (batch, KERNELS[k_batch]), "loop": (loop, KERNELS[k_one]), "whole": (whole, KERNELS[k_whole])}, patches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5, help="device work per variant and shape, at least")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/batch_view_bench.py measures on the GPU; there is none")
    dev = torch.device("cuda:0")
    report = {"device": torch.cuda.get_device_name(dev), "rounds": args.rounds, "seconds_per_variant": args.seconds,
              "batch": B, "gaussians_per_sample": LR * LR * GPP, "dmax": DMAX, "shapes": {}}
    p = torch.stack([synthetic.gs_parameters(LR, LR, seed=b, gpp=GPP) for b in range(B)]).to(dev)
    for name, (scale, win) in SHAPES.items():
        full = int(LR * scale)
        g = torch.Generator().manual_seed(int(scale))
        origins = [tuple(int(v) for v in torch.randint(0, full - win + 1, (2,), generator=g)) for _ in range(B)]
        steps = torch.full((B,), 1.2 / scale, device=dev)
        wgt = torch.rand(B, 3, win, win, generator=g).to(dev)
        fns, patches = variants_of(p, steps, full, win, origins, wgt, dev)
        # the three variants give the same patches and gradients (the same sums in another order)
        ref_img, ref_grad = patches("batch", fns["batch"][0]())
        row = {"full": full, "window": win, "origins": origins, "same_pixels": {}, "same_gradient": {}}
        for v in VARIANTS[1:]:
            img, grad = patches(v, fns[v][0]())
            row["same_pixels"][v] = float((img - ref_img).abs().max())
            row["same_gradient"][v] = float((grad - ref_grad).abs().max() / ref_grad.abs().max())
            assert row["same_pixels"][v] <= 2e-5 * max(1.0, float(ref_img.abs().max())), (name, v, row["same_pixels"][v])
            assert row["same_gradient"][v] <= 2e-4, (name, v, row["same_gradient"][v])
        del img, grad, ref_img, ref_grad
        counts = {}
        for v in VARIANTS:
            for _ in range(3):
                fns[v][0]()
            ms = batch_ms(fns[v][0], 5)
            counts[v] = max(5, int(args.seconds * 1000.0 / ms / args.rounds) + 1)
        times = {v: [] for v in VARIANTS}
        for _ in range(args.rounds):        # alternated: batch loop whole batch loop whole ...
            for v in VARIANTS:
                times[v].append(batch_ms(fns[v][0], counts[v]))
        for v in VARIANTS:
            t = times[v]
            row[v] = {"step_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t), "steps_per_round": counts[v],
                      "total_s": sum(t) * counts[v] / 1000.0, "backward_kernel": fns[v][1]}
        row["batch_not_slower_than_loop"] = row["batch"]["step_ms"] <= row["loop"]["max_ms"]
        row["batch_faster_than_whole"] = row["batch"]["step_ms"] < row["whole"]["step_ms"]
        report["shapes"][name] = row
        print(f"{name} | step ms | " + " | ".join(
            f"{v} ({row[v]['backward_kernel']}) {row[v]['step_ms']:.4f} [{row[v]['min_ms']:.4f}, {row[v]['max_ms']:.4f}]" for v in VARIANTS), flush=True)
        print(f"{name} | batch's median <= loop's maximum: {row['batch_not_slower_than_loop']}; batch faster than whole: "
              f"{row['batch_faster_than_whole']}", flush=True)
        del fns
        _cabi.clear_workspace_pool()
        torch.cuda.empty_cache()
    text = json.dumps(report, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)
    if not all(r["batch_not_slower_than_loop"] for r in report["shapes"].values()):
        sys.exit("the batched windows are slower than the loop of single views")


if __name__ == "__main__":
    main()
