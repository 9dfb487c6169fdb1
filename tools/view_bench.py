#!/usr/bin/env python
"""What a window of the HR grid costs: device time of plan / forward / backward for three ways to the same pixels,

    view    the window planned and rendered as such                       gsasr_splat_plan_view + ..._view
    band    the row band [y0, y0 + h) at full width, columns sliced       dims.row0 / row1 (what the library could do before)
    whole   the whole grid, sliced
    view-home   (backward shapes only) the view with GSASR_FLAG_BWD_HOME set by hand: the home-tile backward launches over the
            window's cells, where the Gaussian-stationary one -- the rule's choice below 1024 tiles -- spends a wave on every
            Gaussian of the grid, dead ones included

on (a) config 3's grid (6144^2, 262 144 Gaussians), forward only, a 1024^2 window at the centre and in a corner; (b) the c2x16
grid (1024^2, 1 M Gaussians), plan + forward + backward, a 512^2 window; (c) a x30 grid (120^2 LR pixels at 16 Gaussians each
on 3600^2), a 1024^2 window, forward-only 8-bit.  The plan classifies all the Gaussians in every variant: that fixed cost is
reported on its own.  hipEvent timing around batches of calls, the variants alternated round by round in one process, at
least `--seconds` of work per variant and stage; the figure is the median of the rounds, the spread their range.

    python tools/view_bench.py [--seconds 0.5] [--rounds 9] [--out profiles/view_bench.json]
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
    # name: (h_lr, w_lr, scale, Gaussians per LR pixel, dmax, window size, (y0, x0) or None = the far corner, backward, 8-bit)
    "a: config 3, 1024^2 centre": (512, 512, 12.0, 1, 0.1, 1024, (2560, 2560), False, False),
    "a: config 3, 1024^2 corner": (512, 512, 12.0, 1, 0.1, 1024, None, False, False),
    "b: c2x16, 512^2 centre": (256, 256, 4.0, 16, 0.1, 512, (256, 256), True, False),
    "c: x30 of 120^2, 1024^2 centre, u8": (120, 120, 30.0, 16, 0.1, 1024, (1288, 1288), False, True),
}
VARIANTS = ("view", "band", "whole")


def batch_ms(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def stages(variant, tensors, H, W, dmax, win, y0, x0, backward, u8, dev):
    """{stage: callable} of one variant, and a callable that returns its window's pixels (for the equality check)"""
    a, b, c = tensors
    flags = 0 if backward else _cabi.FLAG_FORWARD_ONLY
    if variant == "view-home":
        flags |= _cabi.FLAG_BWD_HOME
    if variant.startswith("view"):
        kw = dict(h=win, w=win, view=(H, W, y0, x0))
        rows, cols = win, win
    elif variant == "band":
        kw = dict(h=H, w=W, rows=(y0, y0 + win))
        rows, cols = win, W
    else:
        kw = dict(h=H, w=W)
        rows, cols = H, W

    def make_plan():
        return _cabi.plan(a, b, c, kw["h"], kw["w"], dmax, rows=kw.get("rows"), flags=flags, view=kw.get("view"))

    plan = make_plan()
    out = {"plan": make_plan}
    if u8:
        # (the crop counts rows and columns of the whole grid from its top-left corner: band and whole stop at the window's end)
        crop = None if variant == "view" else (y0 + win, x0 + win)
        img = _cabi.forward_u8(plan, crop=crop)
        out["forward"] = lambda: _cabi.forward_u8(plan, crop=crop, out=img)
    else:
        img = torch.empty(rows, cols, 3, device=dev)
        out["forward"] = lambda: _cabi.forward(plan, img, overwrite=True)
    if variant.startswith("view"):
        pixels = lambda: img
    elif variant == "band" or u8:
        pixels = lambda: img[-win:, x0:x0 + win]
    else:
        pixels = lambda: img[y0:y0 + win, x0:x0 + win]
    if backward:
        wgt = synthetic.grad_image(win, win, 1).to(dev)
        grad = torch.zeros(rows, cols, 3, device=dev)
        if variant.startswith("view"):
            grad.copy_(wgt)
        elif variant == "band":
            grad[:, x0:x0 + win] = wgt
        else:
            grad[y0:y0 + win, x0:x0 + win] = wgt
        g = [torch.empty_like(t) for t in tensors]
        out["backward"] = lambda: _cabi.backward(plan, a, b, c, grad, *g, overwrite=True)
        return out, pixels, g
    return out, pixels, None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5, help="device work per variant, stage and shape, at least")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/view_bench.py measures on the GPU; there is none")
    dev = torch.device("cuda:0")
    report = {"device": torch.cuda.get_device_name(dev), "rounds": args.rounds, "seconds_per_variant_and_stage": args.seconds, "shapes": {}}
    for name, (h_lr, w_lr, scale, gpp, dmax, win, origin, backward, u8) in SHAPES.items():
        sig, xy, col, H, W = synthetic.kernel_inputs(h_lr, w_lr, scale, seed=0, gpp=gpp)
        tensors = tuple(t.to(dev) for t in (sig, xy, col))
        y0, x0 = origin if origin is not None else (H - win, W - win)
        fns, pixels, grads = {}, {}, {}
        variants = VARIANTS + (("view-home",) if backward else ())
        for v in variants:
            fns[v], pixels[v], grads[v] = stages(v, tensors, H, W, dmax, win, y0, x0, backward, u8, dev)
        # the three variants give the same pixels (the same sums in another order; 8-bit: one level on a rounding boundary)
        for v in variants:
            fns[v]["forward"]()
            if backward:
                fns[v]["backward"]()
        ref = pixels["view"]().float()
        row = {"H": H, "W": W, "gaussians": int(sig.shape[0]), "window": [y0, x0, win, win], "same_pixels": {}}
        for v in variants[1:]:
            diff = float((pixels[v]().float() - ref).abs().max())
            row["same_pixels"][v] = diff
            assert diff <= (1.0 if u8 else 2e-5 * max(1.0, float(ref.abs().max()))), (name, v, diff)
            if backward:
                for gv, gr in zip(grads[v], grads["view"]):
                    assert float((gv - gr).abs().max()) <= 2e-4 * float(gr.abs().max()), (name, v)
        stage_names = list(fns["view"])
        counts = {}
        for v in variants:
            for st in stage_names:
                for _ in range(3):
                    fns[v][st]()
                ms = batch_ms(fns[v][st], 5)
                counts[v, st] = max(5, int(args.seconds * 1000.0 / ms / args.rounds) + 1)
        times = {k: [] for k in counts}
        for _ in range(args.rounds):        # alternated: view band whole view band whole ...
            for st in stage_names:
                for v in variants:
                    times[v, st].append(batch_ms(fns[v][st], counts[v, st]))
        for v in variants:
            row[v] = {}
            for st in stage_names:
                t = times[v, st]
                row[v][st] = {"ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t), "calls_per_round": counts[v, st],
                              "total_s": sum(t) * counts[v, st] / 1000.0}
            row[v]["step_ms"] = sum(row[v][st]["ms"] for st in stage_names)
        row["view_step_not_slower_than_band"] = row["view"]["step_ms"] <= row["band"]["step_ms"]
        report["shapes"][name] = row
        for st in stage_names + ["step"]:
            cells = []
            for v in variants:
                if st == "step":
                    cells.append(f"{v} {row[v]['step_ms']:.4f}")
                else:
                    r = row[v][st]
                    cells.append(f"{v} {r['ms']:.4f} [{r['min_ms']:.4f}, {r['max_ms']:.4f}]")
            print(f"{name} | {st} ms | " + " | ".join(cells), flush=True)
        print(f"{name} | view's step <= band's step: {row['view_step_not_slower_than_band']}", flush=True)
        del fns, pixels, grads, tensors, ref
        _cabi.clear_workspace_pool()
        torch.cuda.empty_cache()
    text = json.dumps(report, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
