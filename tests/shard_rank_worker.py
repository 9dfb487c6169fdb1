"""One rank of tests/test_shard_ranks_gpu.py: the row-band shard's product path (HipBackend, the autograd Functions, a real
process group) on the GPU, over gloo, with every rank on the one device.  Started by `python -m torch.distributed.run`;
writes what each variant produced to `--out` as `<variant>.<name>.r<rank>.npy` and `<variant>.r<rank>.json`, and exits
non-zero on any exception.  Nothing is compared here: the parent holds the files against the float64 oracle."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import bandref  # noqa: E402
from gsasr_amd import shard, synthetic  # noqa: E402

# (geometry, transport, overlap, busy).  busy: the stream still has milliseconds of other work in front of `select` and of the
# backward when the host issues the swap, and the send buffers start out as dead records -- a transport that reads the buffers
# before the stream has filled them (gloo's send / recv, which BandExchange synchronises for) ships those
LOCAL = [(g, t, o, False) for g in ("adjacent", "thin") for t in ("alltoall", "p2p") for o in (False, True)] + \
        [("thin", t, o, True) for t in ("p2p", "alltoall") for o in (False, True)]
REDUCE = ("all_reduce", "reduce_scatter")


def local_name(geom, transport, overlap, busy=False):
    return f"local-{geom}-{transport}-{'overlap' if overlap else 'plain'}{'-busy' if busy else ''}"


def keep_busy(dev):
    """about ten milliseconds of memory traffic on the current stream (no host synchronisation)"""
    if dev.type != "cuda":
        return
    x = torch.ones(1 << 27, device=dev)
    for _ in range(30):
        x.mul_(1.0001)


class Out:
    def __init__(self, root, rank):
        self.root, self.rank = root, rank

    def save(self, variant, meta, **arrays):
        for name, a in arrays.items():
            if torch.is_tensor(a):
                a = a.detach().cpu().numpy()
            np.save(os.path.join(self.root, f"{variant}.{name}.r{self.rank}.npy"), np.asarray(a))
        with open(os.path.join(self.root, f"{variant}.r{self.rank}.json"), "w") as f:
            json.dump(meta, f)


def _check_text(ex):
    try:
        ex.check()
        return None
    except RuntimeError as e:
        return str(e)


def run_local(out, variant, geom, transport, overlap, rank, world, dev, cap=None, busy=False):
    rec, H, W, dmax, cutoff, gcap, own = bandref.geometry(geom, world)
    a, b = own[rank]
    ex = shard.BandExchange(b - a, gcap if cap is None else cap, H, W, dmax, cutoff=cutoff, device=dev, transport=transport,
                            overlap=overlap)
    p = torch.from_numpy(rec[a:b]).to(dev).requires_grad_(True)
    if busy:
        ex.send.zero_()
        keep_busy(dev)
    slab = shard.splat_band_local(p, ex)
    err = _check_text(ex)
    r0, r1 = ex.rows
    wgt = synthetic.grad_image(H, W, bandref.GRAD_SEED, device=dev)
    loss = (slab * wgt[r0:r1]).sum()
    if busy:
        keep_busy(dev)
    loss.backward()
    out.save(variant, dict(rows=[r0, r1], own=[a, b], counts=ex.counts.tolist(), err=err, tau=ex.cutoff, cap=ex.cap),
             slab=slab, g=p.grad, up_index=ex.up_index, down_index=ex.down_index)


def run_band(out, variant, packed, mode, rank, world, dev):
    """broadcast from rank 0 (the others start from zeros), splat_band / splat_band_packed, gather_image"""
    rec, H, W, dmax, _, _, _ = bandref.geometry("adjacent", world)
    n = rec.shape[0]
    src = torch.from_numpy(rec).to(dev) if rank == 0 else torch.zeros(n, 8, device=dev)
    r0, r1 = shard.row_band(H, rank, world)
    wgt = synthetic.grad_image(H, W, bandref.GRAD_SEED, device=dev)
    if packed:
        leaves = [shard.broadcast_packed(src, src=0).clone().requires_grad_(True)]
        slab = shard.splat_band_packed(leaves[0], H, W, dmax=dmax, grad_reduce=mode)
    else:
        leaves = [t.clone().requires_grad_(True) for t in shard.broadcast_gaussians(*shard.unpack(src), src=0)]
        slab = shard.splat_band(*leaves, H, W, dmax=dmax, grad_reduce=mode)
    full = shard.gather_image(slab.detach(), H)
    meta = dict(rows=[r0, r1], slice=list(shard.gaussian_slice(n, rank, world)), unsupported=None)
    try:
        (slab * wgt[r0:r1]).sum().backward()
    except Exception as e:      # (the parent decides whether this is the process group lacking the collective, and fails otherwise)
        if mode != "reduce_scatter":
            raise
        meta["unsupported"] = f"{type(e).__name__}: {e}"
        out.save(variant, meta, slab=slab, full=full)
        return
    g = leaves[0].grad if packed else torch.cat([t.grad for t in leaves], dim=1)
    out.save(variant, meta, slab=slab, full=full, g=g)


def run_reuse(out, rank, world, dev):
    """two forwards on one BandExchange, then the older one's backward: every rank takes the same steps, so the collectives of
    the newer backward pair up and the older one raises before it issues any"""
    rec, H, W, dmax, cutoff, cap, own = bandref.geometry("adjacent", world)
    a, b = own[rank]
    ex = shard.BandExchange(b - a, cap, H, W, dmax, cutoff=cutoff, device=dev)
    p1 = torch.from_numpy(rec[a:b]).to(dev).requires_grad_(True)
    p2 = p1.detach().clone().requires_grad_(True)
    first = shard.splat_band_local(p1, ex)
    second = shard.splat_band_local(p2, ex)
    second.sum().backward()
    raised = None
    try:
        first.sum().backward()
    except RuntimeError as e:
        raised = str(e)
    out.save("reuse", dict(raised=raised, finite=bool(torch.isfinite(second).all() and torch.isfinite(p2.grad).all())))


def run_all(out, rank, world, dev):
    for geom, transport, overlap, busy in LOCAL:
        run_local(out, local_name(geom, transport, overlap, busy), geom, transport, overlap, rank, world, dev, busy=busy)
    for overlap in (False, True):
        run_local(out, f"overflow-{'overlap' if overlap else 'plain'}", "adjacent", "alltoall", overlap, rank, world, dev, cap=2)
    run_reuse(out, rank, world, dev)
    for mode in REDUCE:       # (reduce_scatter last: a group that lacks it has then nothing left to run)
        run_band(out, f"band-{mode}", False, mode, rank, world, dev)
        run_band(out, f"packed-{mode}", True, mode, rank, world, dev)
    dist.barrier()
    out.save("done", dict(ok=True))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        run_all(Out(args.out, rank), rank, world, dev)
        torch.cuda.synchronize()
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
