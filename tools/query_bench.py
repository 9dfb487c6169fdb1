#!/usr/bin/env python
"""What a query at fractional pixel positions costs: device time of plan / sort + forward / backward for four
ways to the values at the SAME integer-valued points,

    int-plain   int32 points on a plain plan                    gsasr_splat_sample_*          (what the library could do before)
    int-cont    int32 points on a GSASR_FLAG_CONTINUOUS plan    isolates the price of the one-pixel padding of the windows
    float-cont  float points on a continuous plan               gsasr_splat_query_*
    refine-m2   what a caller had to do for half-pixel positions: render the m = 2 grid and gather (reported only)

on (a) 1024^2 x4 at 65 536 Gaussians with 65 536 points and (b) the config-5 batch (16 x 192^2, 16 Gaussians per LR pixel) with
6.25% of its pixels as points.  int-cont and float-cont run the same kernels on the same sorted records everywhere but in the
sort, so on every other stage their medians may differ by no more than int-cont's own spread (`float_within_int_spread`);
int-cont against int-plain is reported beside the ratio the padding predicts, the mean of (w + 2)(h + 2) / (w h) over the
windows (restated on the host from the plan's own cutoff).  float-cont has one more stage, "position backward": the gradient
with respect to the positions (gsasr_splat_query_backward_points with points = NULL: the gather of grad_out + k_query_bwd_pts),
which must cost less than four sort + forward of the same run -- what central differences in r and c cost
(`position_backward_below_four_forwards`).  The sort is timed as the difference of the backward with and
without a re-sort of the points.  hipEvent timing around batches of calls, the variants alternated round by round in one
process, at least `--seconds` of work per variant and stage; the figure is the median of the rounds, the spread their range.

    python tools/query_bench.py [--seconds 0.5] [--rounds 9] [--out profiles/query_bench.json]
"""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gsasr_amd import _cabi, synthetic  # noqa: E402

SHAPES = {
    # name: (batch, h_lr, w_lr, scale, Gaussians per LR pixel, dmax, points per sample)
    "a: 1024^2 x4, 65 536 Gaussians, 65 536 points": (1, 256, 256, 4.0, 1, 0.1, 65536),
    "b: config-5 batch, 16 x 192^2, 6.25% of the pixels": (16, 48, 48, 4.0, 16, 0.5, 2304),
}
VARIANTS = ("int-plain", "int-cont", "float-cont")
GATED = ("plan", "backward", "forward")


def batch_ms(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def make_plan(tensors, B, n_per, H, W, dmax, flags, dev, list_cap=-1):
    """a callable that plans (again) on one workspace, and the Plan"""
    a, b, c = tensors
    if B == 1:
        d = _cabi.make_dims(n_per, H, W, dmax, flags=flags, list_cap=list_cap)
    else:
        d = _cabi.make_batch_dims(n_per, [(H, W)] * B, W, H, dmax, flags=flags)
        d.list_cap = list_cap
    nbytes = _cabi.lib().gsasr_splat_workspace_bytes(ctypes.byref(d))
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def plan():
        _cabi.check(_cabi.lib().gsasr_splat_plan(a.data_ptr(), b.data_ptr(), c.data_ptr(), ctypes.byref(d), ws.data_ptr(), nbytes, stream),
                    "gsasr_splat_plan")
    plan()
    return plan, _cabi.Plan(d, ws, dev)


def padding_ratio(tensors, B, H, W, dmax, tau):
    """mean (w + 2)(h + 2) / (w h) over the live windows: gaussian_box restated on the host with the plan's cutoff"""
    sig, xy = tensors[0].double().cpu(), tensors[1].double().cpu()
    k = math.sqrt(2.0 * tau) * (1.0 + 1e-6)
    tot, n = 0.0, 0
    ws = []
    for axis, size in ((0, W), (1, H)):
        hx = 0.5 * (size - 1)
        ext = torch.clamp(k * sig[:, axis].abs(), max=dmax) * hx
        ctr = (xy[:, axis] + 1.0) * hx
        lo = torch.ceil(ctr - ext - 0.02).clamp(min=0)
        hi = torch.floor(ctr + ext + 0.02).clamp(max=size - 1)
        ws.append(hi - lo + 1)
    live = (ws[0] >= 1) & (ws[1] >= 1)
    w, h = ws[0][live], ws[1][live]
    tot, n = float(((w + 2) * (h + 2) / (w * h)).sum()), int(live.sum())
    return tot / max(n, 1), float(w.mean()), float(h.mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5, help="device work per variant, stage and shape, at least")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/query_bench.py measures on the GPU; there is none")
    dev = torch.device("cuda:0")
    report = {"device": torch.cuda.get_device_name(dev), "rounds": args.rounds, "seconds_per_variant_and_stage": args.seconds, "shapes": {}}
    ok_all = True
    for name, (B, h_lr, w_lr, scale, gpp, dmax, S) in SHAPES.items():
        parts = [synthetic.kernel_inputs(h_lr, w_lr, scale, seed=b, gpp=gpp) for b in range(B)]
        H, W = parts[0][3], parts[0][4]
        tensors = tuple(torch.cat([p[k] for p in parts]).contiguous().to(dev) for k in range(3))
        n_per = parts[0][0].shape[0]
        g = torch.Generator().manual_seed(0)
        ipts = torch.stack([torch.stack([torch.randint(0, H, (S,), generator=g), torch.randint(0, W, (S,), generator=g)], 1) for _ in range(B)])
        ipts = (ipts if B > 1 else ipts[0]).to(dev)
        gout = torch.rand((B, 3, S) if B > 1 else (3, S), device=dev)
        fns, outs, grads, plans = {}, {}, {}, {}
        for v in VARIANTS:
            flags = _cabi.FLAG_CONTINUOUS if v.endswith("cont") else 0
            planfn, plan = make_plan(tensors, B, n_per, H, W, dmax, flags, dev)
            pts = ipts.float() if v.startswith("float") else ipts
            fwd, bwd = (_cabi.query_forward, _cabi.query_backward) if v.startswith("float") else (_cabi.sample_forward, _cabi.sample_backward)
            out, state = fwd(plan, pts)
            gr = [torch.empty_like(t) for t in tensors]
            a, b, c = tensors

            def f_fwd(plan=plan, pts=pts, fwd=fwd):
                return fwd(plan, pts)

            def f_bwd(plan=plan, state=state, bwd=bwd, gr=gr, resort=False):
                bwd(plan, state, a, b, c, gout, *gr, overwrite=True, resort=resort)

            fns[v] = {"plan": planfn, "sort+forward": f_fwd, "backward": f_bwd, "sort+backward": lambda f=f_bwd: f(resort=True)}
            f_bwd()
            if v == "float-cont":
                def posbwd(plan=plan, state=state):
                    return _cabi.query_backward_points(plan, state, gout)
                gpos = posbwd()
                assert bool(torch.isfinite(gpos).all()) and float(gpos.abs().max()) > 0
            outs[v], grads[v], plans[v] = out, gr, plan
        # the same values and gradients, three ways
        row = {"H": H, "W": W, "batch": B, "gaussians": int(tensors[0].shape[0]), "points": int(S * B), "same_values": {}}
        for v in VARIANTS[1:]:
            diff = float((outs[v] - outs["int-plain"]).abs().max())
            row["same_values"][v] = diff
            assert diff <= 1e-4, (name, v, diff)
            for gv, gr in zip(grads[v], grads["int-plain"]):
                assert float((gv - gr).abs().max()) <= 2e-4 * float(gr.abs().max()), (name, v)
        tau, K = _cabi.plan_cutoff(plans["int-cont"])
        tau0, K0 = _cabi.plan_cutoff(plans["int-plain"])
        ratio, wm, hm = padding_ratio(tensors, B, H, W, dmax, tau0)
        row["cutoff"] = {"int-plain": [tau0, K0], "int-cont": [tau, K]}
        row["expected_padding_ratio"] = ratio
        row["mean_window"] = [wm, hm]
        # (iv) the m = 2 grid and a gather: plan + forward of (2H - 1) x (2W - 1) on the same kernel-frame tensors
        H2, W2 = 2 * H - 1, 2 * W - 1
        if B == 1:
            d2 = _cabi.make_dims(n_per, H2, W2, dmax, flags=_cabi.FLAG_OVERWRITE_IMAGE | _cabi.FLAG_FORWARD_ONLY)
        else:
            d2 = _cabi.make_batch_dims(n_per, [(H2, W2)] * B, W2, H2, dmax, flags=_cabi.FLAG_OVERWRITE_IMAGE | _cabi.FLAG_FORWARD_ONLY)
        nb2 = _cabi.lib().gsasr_splat_workspace_bytes(ctypes.byref(d2))
        ws2 = torch.empty(nb2, dtype=torch.uint8, device=dev)
        img2 = torch.empty(d2.h, W2, 3, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        flat = ipts.reshape(-1, 2).long()
        smp = torch.arange(B, device=dev).repeat_interleave(S)

        def refine():
            _cabi.check(_cabi.lib().gsasr_splat_plan(tensors[0].data_ptr(), tensors[1].data_ptr(), tensors[2].data_ptr(), ctypes.byref(d2),
                                                     ws2.data_ptr(), nb2, stream), "gsasr_splat_plan")
            _cabi.check(_cabi.lib().gsasr_splat_forward(ctypes.byref(d2), ws2.data_ptr(), nb2, img2.data_ptr(), stream), "gsasr_splat_forward")
            return img2[smp * (d2.slot if B > 1 else 0) + 2 * flat[:, 0], 2 * flat[:, 1], :]
        got = refine().reshape(B, S, 3).permute(0, 2, 1)
        row["same_values"]["refine-m2"] = float((got - outs["int-plain"].reshape(B, 3, S)).abs().max())
        assert row["same_values"]["refine-m2"] <= 1e-4
        stage_names = list(fns[VARIANTS[0]])
        counts = {}
        for v in VARIANTS:
            for st in stage_names:
                for _ in range(3):
                    fns[v][st]()
                counts[v, st] = max(5, int(args.seconds * 1000.0 / batch_ms(fns[v][st], 5) / args.rounds) + 1)
        for _ in range(3):
            refine()
        counts["refine"] = max(3, int(args.seconds * 1000.0 / batch_ms(refine, 3) / args.rounds) + 1)
        for _ in range(3):
            posbwd()
        counts["posbwd"] = max(5, int(args.seconds * 1000.0 / batch_ms(posbwd, 5) / args.rounds) + 1)
        times = {k: [] for k in counts}
        for _ in range(args.rounds):        # alternated: int-plain int-cont float-cont int-plain ...
            for st in stage_names:
                for v in VARIANTS:
                    times[v, st].append(batch_ms(fns[v][st], counts[v, st]))
            times["refine"].append(batch_ms(refine, counts["refine"]))
            times["posbwd"].append(batch_ms(posbwd, counts["posbwd"]))

        def cell(t, n):
            return {"ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t), "calls_per_round": n, "total_s": sum(t) * n / 1000.0}
        for v in VARIANTS:
            row[v] = {st: cell(times[v, st], counts[v, st]) for st in stage_names}
            # per round: the sort = (sort + backward) - backward, the forward = (sort + forward) - sort
            sort = [x - y for x, y in zip(times[v, "sort+backward"], times[v, "backward"])]
            row[v]["sort"] = cell(sort, counts[v, "sort+backward"])
            row[v]["forward"] = cell([x - y for x, y in zip(times[v, "sort+forward"], sort)], counts[v, "sort+forward"])
        row["refine-m2"] = {"plan+forward+gather": cell(times["refine"], counts["refine"])}
        row["float-cont"]["position backward"] = cell(times["posbwd"], counts["posbwd"])
        row["position_backward_over_sort+forward"] = row["float-cont"]["position backward"]["ms"] / row["float-cont"]["sort+forward"]["ms"]
        row["position_backward_below_four_forwards"] = row["position_backward_over_sort+forward"] < 4.0
        ok_all = ok_all and row["position_backward_below_four_forwards"]
        row["float_within_int_spread"] = {}
        for st in GATED:
            ii, fl = row["int-cont"][st], row["float-cont"][st]
            row["float_within_int_spread"][st] = abs(fl["ms"] - ii["ms"]) <= ii["max_ms"] - ii["min_ms"]
            ok_all = ok_all and row["float_within_int_spread"][st]
        row["padding_measured_ratio"] = {st: row["int-cont"][st]["ms"] / row["int-plain"][st]["ms"] for st in ("plan", "sort+forward", "backward")}
        report["shapes"][name] = row
        for st in stage_names + ["sort", "forward"]:
            print(f"{name} | {st} ms | " + " | ".join(f"{v} {row[v][st]['ms']:.4f} [{row[v][st]['min_ms']:.4f}, {row[v][st]['max_ms']:.4f}]" for v in VARIANTS), flush=True)
        r = row["refine-m2"]["plan+forward+gather"]
        print(f"{name} | refine-m2 plan+forward+gather ms | {r['ms']:.4f} [{r['min_ms']:.4f}, {r['max_ms']:.4f}]", flush=True)
        print(f"{name} | expected padding ratio {ratio:.3f} (mean window {wm:.1f} x {hm:.1f}); measured int-cont / int-plain: {row['padding_measured_ratio']}", flush=True)
        print(f"{name} | float-cont within int-cont's spread: {row['float_within_int_spread']}", flush=True)
        pb = row["float-cont"]["position backward"]
        print(f"{name} | float-cont position backward ms | {pb['ms']:.4f} [{pb['min_ms']:.4f}, {pb['max_ms']:.4f}] = "
              f"{row['position_backward_over_sort+forward']:.2f} x sort+forward (must be < 4)", flush=True)
        del fns, outs, grads, plans, tensors, ws2, img2
        torch.cuda.empty_cache()
    report["conditions_hold"] = ok_all
    text = json.dumps(report, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
