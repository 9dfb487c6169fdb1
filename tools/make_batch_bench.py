#!/usr/bin/env python
"""What a training batch costs on the device, at the training shape: 16 samples, lr_size 48, scales uniform in
[1, 4] (crops of 48..192 pixels, drawn once from a seeded `random.Random` by the dataset's rule), sixteen 2040 x 1356 uint8 sources
resident on the device, all eight flip / transposition combinations.

  make_batch   gsasr_amd.make_batch: the public call (validation, three allocations, the descriptor, gsasr_batch_make)
  c_call       gsasr_batch_make alone, on a descriptor and buffers built once: what the kernels cost
  composition  the same batch from torch ops -- per sample: slice, .float() / 255, permute, channel flip, a padded copy for the
               resize; the library's own `imresize_batch` once; per sample: flip / transpose of GT and LR, padded copy -- the
               way a user would have built it before.  Needs nothing this call added, so it runs on an older library too: with
               `--tree DIR` the package is imported from DIR (a checkout of the parent commit with its library built), where
               `gsasr_amd.data` does not exist and only this variant is timed.

Every call is timed by a pair of device events around it (so a call's host time counts where the device waits for it), and by
the host clock around the call without a synchronisation.  The variants alternate call by call in one process: 5 warm-up rounds,
then 20 timed ones; the figure is the median, the spread the range.  Nothing is asserted on the times.

    python tools/make_batch_bench.py [--rounds 20] [--warmup 5] [--tree DIR] [--out profiles/make_batch.json]
"""
import argparse
import ctypes
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL8 = [(h, v, r) for r in (0, 1) for v in (0, 1) for h in (0, 1)]


def timed(fn, torch):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    t0 = time.perf_counter()
    fn()
    host = time.perf_counter() - t0
    e1.record()
    e1.synchronize()
    return 1e3 * e0.elapsed_time(e1), 1e6 * host      # both in microseconds


def draw(B, lr, hw, seed):
    """the training shape's crops, without the package (the parent tree has no draw_batch): uniform scale, ceil, two offsets"""
    import math
    rng = random.Random(seed)
    crops = []
    for _ in range(B):
        g = math.ceil(rng.uniform(1, 4) * lr)
        crops.append((rng.randint(0, hw[0] - g), rng.randint(0, hw[1] - g), g, g))
    return crops


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--tree", default=ROOT, help="import gsasr_amd from this checkout")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch
    if not torch.cuda.is_available():
        sys.exit("tools/make_batch_bench.py measures on the GPU; there is none")
    from gsasr_amd import _cabi
    from gsasr_amd.resize import imresize_batch
    try:
        from gsasr_amd import data as D
    except ImportError:
        D = None
    dev = torch.device("cuda:0")
    B, lr, hw = 16, 48, (1356, 2040)
    g = torch.Generator().manual_seed(1)
    images = [torch.randint(0, 256, hw + (3,), generator=g, dtype=torch.uint8).to(dev) for _ in range(B)]
    crops = draw(B, lr, hw, 2024)
    flags = [ALL8[b % 8] for b in range(B)]
    f = [[a[i] for a in flags] for i in range(3)]
    Gh = Gw = max(c[2] for c in crops)
    sizes = [(c[2], c[3]) for c in crops]

    def composition():
        x = torch.zeros(B, 3, Gh, Gw, device=dev)
        for b, (t, (y0, x0, gh, gw)) in enumerate(zip(images, crops)):
            x[b, :, :gh, :gw] = (t[y0:y0 + gh, x0:x0 + gw].float() / 255).permute(2, 0, 1).flip(0)
        y = imresize_batch(x, sizes, out_size=(lr, lr))
        gt, lq = torch.zeros(B, 3, Gh, Gw, device=dev), torch.empty(B, 3, lr, lr, device=dev)
        for b, (h, v, r) in enumerate(flags):
            s, q = x[b, :, :sizes[b][0], :sizes[b][1]], y[b]
            if h:
                s, q = s.flip(-1), q.flip(-1)
            if v:
                s, q = s.flip(-2), q.flip(-2)
            if r:
                s, q = s.transpose(-1, -2), q.transpose(-1, -2)
            gt[b, :, :s.shape[1], :s.shape[2]] = s
            lq[b] = q
        return gt, lq

    fns = {"composition": composition}
    if D is not None:
        fns["make_batch"] = lambda: D.make_batch(images, crops, lr, *f)
        aug = [h | 2 * v | 4 * r for h, v, r in flags]
        d = _cabi.make_batch_desc([t.data_ptr() for t in images], [hw] * B, crops, aug, (Gh, Gw), (lr, lr), _cabi.BATCH_BGR)
        L = _cabi.lib()
        gt, lq = torch.empty(B, 3, Gh, Gw, device=dev), torch.empty(B, 3, lr, lr, device=dev)
        scratch = torch.empty(int(L.gsasr_batch_scratch_bytes(ctypes.byref(d))), dtype=torch.uint8, device=dev)
        d.gt, d.lq, d.scratch = gt.data_ptr(), lq.data_ptr(), scratch.data_ptr()
        stream = _cabi._stream(dev)
        fns["c_call"] = lambda: _cabi.check(L.gsasr_batch_make(ctypes.byref(d), stream), "gsasr_batch_make")
        # the three variants make the same batch (the composition's GPU `/ 255` multiplies by a reciprocal: to 1 ulp)
        want, got = composition(), D.make_batch(images, crops, lr, *f)
        fns["c_call"]()
        torch.cuda.synchronize()
        assert torch.equal(got["gt"], gt) and torch.equal(got["lq"], lq)
        assert float((got["gt"] - want[0]).abs().max()) <= 2.0 ** -23 and float((got["lq"] - want[1]).abs().max()) <= 1e-6
    for _ in range(args.warmup):
        for fn in fns.values():
            timed(fn, torch)
    times = {v: [] for v in fns}
    for _ in range(args.rounds):                  # alternated call by call
        for v, fn in fns.items():
            times[v].append(timed(fn, torch))
    report = {"device": torch.cuda.get_device_name(dev), "library": _cabi.LIB_PATH, "rounds": args.rounds, "warmup": args.warmup,
              "batch": B, "lr_size": lr, "source_hw": list(hw), "crop_sizes": [c[2] for c in crops], "variants": {}}
    for v, t in times.items():
        ev, host = [a for a, _ in t], [b for _, b in t]
        report["variants"][v] = {"event_us": statistics.median(ev), "event_min_us": min(ev), "event_max_us": max(ev),
                                 "host_us": statistics.median(host), "host_min_us": min(host), "host_max_us": max(host)}
        print(f"{v:12s} | device events {statistics.median(ev):8.1f} us [{min(ev):.1f}, {max(ev):.1f}] | host {statistics.median(host):8.1f} us "
              f"[{min(host):.1f}, {max(host):.1f}]", flush=True)
    text = json.dumps(report, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
