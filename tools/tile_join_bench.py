"""Tiled inference, default path against `tile_batch`: wall time per image and peak device memory of
`split_and_joint_image` on the tiled workload VERDICT.md names -- 1440 x 1440 LR x4, split 480, overlap 8, crop 4, dmax 0.1,
16 Gaussians per LR pixel (4 x 4 tiles of 1920^2 SR pixels, a 7584^2 picture) -- with a stand-in encoder and decoder that cost
next to nothing (a 16-Gaussian cousin of tests/tiled_models.py), so that the rasterizer and the join are what is timed.

    python tools/tile_join_bench.py [--repo DIR] [--modes none,2,4,max] [--lr 1440] [--reps 5]

`--repo DIR`: import gsasr_amd from another checkout (the parent commit, for the baseline: only `none` exists there).  One JSON
line per (output type, mode).  Time: host clock around calls that end in a device synchronise, median of `--reps` after two
warm-up calls; memory: torch.cuda.max_memory_allocated over one call that starts with an empty workspace pool and allocator
cache (`held_before_MiB`: the input image and the stand-in's table, held throughout).
Bench harness, not product."""
import argparse
import json
import os
import sys
import time

import torch


def models(gpp=16, seed=0):
    """'encoder': the LR tile itself; 'decoder': `gpp` Gaussians per LR pixel on a 4 x 4 sub-grid of the pixel, raw parameters
    [1, s * s * gpp, 9] = [sx, sy, rho, alpha, r, g, b, mu_x, mu_y] from the pixel's colour plus a fixed table"""
    side = int(round(gpp ** 0.5))
    assert side * side == gpp
    table = {}

    def model_g(tile):
        return tile

    def model_fea2gs(feat, scale_vector):
        _, _, h, w = feat.shape
        dev = feat.device
        if dev not in table:
            g = torch.Generator().manual_seed(seed)
            t = 0.5 * torch.randn(gpp, 9, generator=g)
            t[:, 7] = (torch.arange(gpp) % side + 0.5) / side
            t[:, 8] = (torch.arange(gpp) // side + 0.5) / side
            table[dev] = t.to(dev)
        t = table[dev]
        rgb = feat[0].permute(1, 2, 0).reshape(h * w, 1, 3)
        p = t.unsqueeze(0).expand(h * w, gpp, 9).clone()
        p[:, :, 4:7] += 2 * rgb - 1
        p[:, :, 3] += 1.0
        jj = torch.arange(w, device=dev, dtype=feat.dtype).repeat(h).reshape(h * w, 1)
        ii = torch.arange(h, device=dev, dtype=feat.dtype).repeat_interleave(w).reshape(h * w, 1)
        p[:, :, 7] = (jj + t[:, 7]) / w
        p[:, :, 8] = (ii + t[:, 8]) / h
        return p.reshape(1, h * w * gpp, 9)

    return model_g, model_fea2gs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repo", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--modes", default="none,2,4,max")
    ap.add_argument("--lr", type=int, default=1440)
    ap.add_argument("--split", type=int, default=480)
    ap.add_argument("--overlap", type=int, default=8)
    ap.add_argument("--crop", type=int, default=4)
    ap.add_argument("--scale", type=float, default=4.0)
    ap.add_argument("--dmax", type=float, default=0.1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.repo))
    import gsasr_amd
    from gsasr_amd import _cabi
    from gsasr_amd.gaussian_splatting import max_canvas_batch
    from gsasr_amd.split_and_joint_image import split_and_joint_image
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    dev = torch.device("cuda:0")
    model_g, model_fea2gs = models()
    lq = torch.rand(1, 3, args.lr, args.lr, generator=torch.Generator().manual_seed(1)).to(dev)
    sm = torch.tensor([args.scale, args.scale], device=dev)
    import math
    cap = max_canvas_batch(math.ceil(args.split * args.scale))
    for out_uint8 in (False, True):
        for mode in args.modes.split(","):
            kw = {} if mode == "none" else {"tile_batch": cap if mode == "max" else int(mode)}

            def call():
                with torch.no_grad():
                    return split_and_joint_image(lq, args.scale, args.split, args.overlap, model_g, model_fea2gs, sm, crop_size=args.crop,
                                                 if_dmax=True, dmax_mode="fix", dmax=args.dmax, out_uint8=out_uint8, **kw)

            _cabi.clear_workspace_pool()      # (plan workspaces pooled by the mode before are not this mode's footprint)
            torch.cuda.empty_cache()
            for _ in range(2):
                out = call()
            shape = tuple(out.shape)
            del out
            torch.cuda.synchronize(dev)
            times = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                out = call()
                torch.cuda.synchronize(dev)
                times.append((time.perf_counter() - t0) * 1e3)
                del out
            _cabi.clear_workspace_pool()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats(dev)
            base = torch.cuda.memory_allocated(dev)
            out = call()
            torch.cuda.synchronize(dev)
            peak = torch.cuda.max_memory_allocated(dev)
            del out
            times.sort()
            print(json.dumps({"label": args.label, "package": os.path.dirname(gsasr_amd.__file__), "out": "uint8" if out_uint8 else "float",
                              "tile_batch": kw.get("tile_batch"), "picture": shape, "ms_median": round(times[len(times) // 2], 2),
                              "ms_min": round(times[0], 2), "ms_max": round(times[-1], 2),
                              "peak_MiB": round(peak / 2 ** 20, 1), "held_before_MiB": round(base / 2 ** 20, 1)}), flush=True)


if __name__ == "__main__":
    main()
