"""The row-band shard's product path on real ranks, held to the float64 oracle.

W = 2 and W = 3 ranks share the one GPU over gloo (tests/shard_rank_worker.py, started once per world size through
`python -m torch.distributed.run`): HipBackend, the autograd Functions of gsasr_amd/shard.py and a real process group -- the
kernels k_band_select / k_band_merge in the flow that calls them, the stream ordering around the asynchronous swaps, `_poison_if`
on a device scalar, the cached all_to_all_single views of the edge ranks, the in-place reduce_scatter_tensor on a slice of its own
input and forward_packed_into(accumulate=True).  Every variant the worker ran reports here as its own test, against
oracle.gs_oracle.forward_f64 / backward_f64 of the WHOLE image:

  image      |slab - ref| <= IMG_ATOL * max(1, max|ref|)                      (IMG_ATOL of tests/test_hip_parity.py)
  gradients  gradbars.check_kernel with SYNTHETIC_SHARE on the rank's own Gaussians (every Gaussian after an all_reduce)

The gradient of a Gaussian in a halo list is a sum of two or three band partials, added in fp32 by k_band_merge or by the
collective.  Measured on an MI355X: the element bar holds on those rows as on the others, worst error / bar 0.028 over the band-local
variants (adjacent geometry, two ranks; 0.022 on the middle rank of the thin geometry, rows in both lists included) against
0.015 on rows that never travel, so no allowance for the split is taken.  One launch took 5 to 8 s there, two ranks or three
(interpreter, HIP and process-group start-up; the shapes are tiny); the limit is LAUNCH_TIMEOUT.
"""
import functools
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import bandref
import gradbars
from shard_rank_worker import LOCAL, REDUCE, local_name

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "shard_rank_worker.py")
IMG_ATOL = 1e-4            # tests/test_hip_parity.py
LAUNCH_TIMEOUT = 120       # s: fifteen times the slowest measured launch, for a machine that others use as well
TERMINATE_GRACE = 45       # s a launcher that ran out of time gets to end its ranks
WORLDS = (2, 3)


# ---------------------------------------------------------------------------------------------------
# the truth, once per geometry
# ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _truth(geom):
    import torch
    from gsasr_amd import synthetic
    from oracle import gs_oracle
    rec, H, W, dmax, _, _, _ = bandref.geometry(geom, 1)
    wgt = synthetic.grad_image(H, W, bandref.GRAD_SEED).numpy()
    sig, xy, col = rec[:, 0:3], rec[:, 3:5], rec[:, 5:8]
    ref = gs_oracle.forward_f64(sig, xy, col, H, W, dmax)
    gref = gs_oracle.backward_f64(sig, xy, col, wgt, dmax)
    assert torch.get_default_dtype() == torch.float32
    for a in (ref, *gref):
        a.setflags(write=False)
    return rec, ref, gref


# ---------------------------------------------------------------------------------------------------
# what the geometries must be, checked without a GPU
# ---------------------------------------------------------------------------------------------------
def test_thin_geometry_crowds_both_lists_of_the_middle_rank():
    """by the float64 window: at three ranks the middle one has at least 8 Gaussians in BOTH lists, nobody reaches past a
    neighbour, every list fits its capacity -- and none of the rank's Gaussians is outside the gradient bars' scope"""
    for geom in bandref.GEOMETRIES:
        for world in WORLDS:
            rec, H, W, dmax, cutoff, cap, own = bandref.geometry(geom, world)
            assert rec.shape[0] == 288 and (H, W) == (96, 48)
            for r, (a, b) in enumerate(own):
                tau = bandref.exchange_tau(cutoff, b - a, cap)
                sel = bandref.select(rec[a:b], H, W, dmax, tau, r, world)
                assert sel["far"].size == 0 and sel["up"].size <= cap and sel["down"].size <= cap, (geom, world, r)
                assert (sel["up"].size > 0) == (r > 0) and (sel["down"].size > 0) == (r < world - 1)
                assert (gradbars.kappa_of(rec[a:b, 2]) >= gradbars.KAPPA_MIN).all()
                both = np.intersect1d(sel["up"], sel["down"]).size
                if geom == "thin" and world == 3 and r == 1:
                    assert both >= 8, both
                if geom == "adjacent":
                    assert both == 0
    assert all((b - a) % 64 for a, b in bandref.geometry("thin", 3)[6])


# ---------------------------------------------------------------------------------------------------
# the launches: one per world size
# ---------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _launch(world, out):
    """start `world` ranks and wait for them; returns None, or what went wrong with the tail of the ranks' stderr"""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), WORKER, "--out", out]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    log = os.path.join(out, "launch.stderr")
    late = False
    # stderr goes to a file, not a pipe: the ranks inherit it, and a pipe is only at its end when the last of them is gone
    with open(log, "w") as err:
        p = subprocess.Popen(cmd, stdout=subprocess.DEVNULL, stderr=err, cwd=ROOT, env=env)
        try:
            p.wait(timeout=LAUNCH_TIMEOUT)
        except subprocess.TimeoutExpired:
            # The launcher puts every rank in a session of its own and ends them all when it is ASKED to end; killed outright
            # (what subprocess.run(timeout=) does) it would leave ranks behind that hold the GPU.  So: SIGTERM, time to clean up
            # (it gives its ranks 30 s before it kills them), and only then the hard way.
            late = True
            p.terminate()
            try:
                p.wait(timeout=TERMINATE_GRACE)
            except subprocess.TimeoutExpired:
                p.kill()
                p.wait()
    with open(log) as f:
        tail = f.read()[-3000:]
    if late:
        return f"{world} ranks did not finish within {LAUNCH_TIMEOUT} s:\n{tail}"
    if p.returncode != 0:
        return f"{world} ranks exited with {p.returncode}:\n{tail}"
    return None


@pytest.fixture(scope="module")
def ranks(tmp_path_factory):
    """`ranks(world)` -> the directory the worker's ranks wrote; each world size is launched once, a failure is kept and
    fails every test that asks for that world size (no second try)"""
    done = {}

    def get(world):
        if world not in done:
            out = str(tmp_path_factory.mktemp(f"ranks{world}"))
            done[world] = (out, _launch(world, out))
        out, failure = done[world]
        assert failure is None, failure
        return out
    return get


def _meta(out, variant, rank):
    with open(os.path.join(out, f"{variant}.r{rank}.json")) as f:
        return json.load(f)


def _arr(out, variant, name, rank):
    return np.load(os.path.join(out, f"{variant}.{name}.r{rank}.npy"))


def _check_image(slab, ref, what):
    assert np.isfinite(slab).all(), what
    scale = max(1.0, float(np.abs(ref).max()))
    err = float(np.abs(slab - ref).max())
    print(f"{what}: image max|err| {err:.3e} (bar {IMG_ATOL * scale:.3e})")
    assert err <= IMG_ATOL * scale, f"{what}: image max|err| {err:.3e}"


def _check_grads(g8, want, sig, what, travelled=None):
    """`g8` [n, 8] against the float64 truth `want` (three arrays of the same rows) under the suite's own bars; prints the worst
    error / element bar first, apart for the rows that sat in a halo list (`travelled`) and for those that never left"""
    got = (g8[:, 0:3], g8[:, 3:5], g8[:, 5:8])
    if travelled is not None and np.isfinite(g8).all():
        worst = {True: 0.0, False: 0.0}
        for g, w, name in zip(got, want, ("sigmas", "coords", "colors")):
            _, _, scope, err, tol = gradbars.ratios(g, w, sig[:, 2], gradbars.KERNEL_GROUPS[name])
            for kind in (True, False):
                rows = scope & (travelled == kind)
                if rows.any():
                    worst[kind] = max(worst[kind], float((err[rows] / tol[rows]).max()))
        print(f"{what}: worst error / element bar {worst[True]:.3f} on rows of a halo list, {worst[False]:.3f} on the others")
    return gradbars.check_kernel(got, want, sig, gradbars.SYNTHETIC_SHARE, what)


# ---------------------------------------------------------------------------------------------------
# splat_band_local
# ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("geom,transport,overlap,busy", LOCAL, ids=[local_name(*v)[6:] for v in LOCAL])
def test_band_local_on_ranks_matches_the_oracle(geom, transport, overlap, busy, world, ranks):
    """busy: the swap is issued while the stream is still milliseconds away from `select` (and from the backward), over send
    buffers that start as dead records.  gloo's send / recv read a device tensor from the host the moment they are issued; without
    the stream synchronisation BandExchange does for them the neighbours got those dead records: the p2p variants failed on an
    MI355X, three ranks, with an image error of 0.51 -- once in three runs when nothing else kept the stream busy"""
    out = ranks(world)
    variant = local_name(geom, transport, overlap, busy)
    rec, ref, gref = _truth(geom)
    _, H, W, dmax, cutoff, cap, own = bandref.geometry(geom, world)
    for r in range(world):
        m = _meta(out, variant, r)
        what = f"{variant} rank {r}/{world}"
        assert m["err"] is None, m["err"]
        assert tuple(m["rows"]) == bandref.row_band(H, r, world) and tuple(m["own"]) == own[r]
        n_up, n_down, n_far, spare = m["counts"]
        assert n_far == 0 and spare == 0 and 0 <= n_up <= cap and 0 <= n_down <= cap, m["counts"]
        assert (n_up > 0) == (r > 0) and (n_down > 0) == (r < world - 1)
        up, down = _arr(out, variant, "up_index", r)[:n_up], _arr(out, variant, "down_index", r)[:n_down]
        both = np.intersect1d(up, down)
        if geom == "thin" and world == 3 and r == 1:
            assert both.size >= 8, both.size         # the reason k_band_merge adds atomically, with real data
        a, b = own[r]
        # every Gaussian that must travel by its own float64 image did (the lists themselves: tests/test_band_kernels_gpu.py)
        must_up, must_down = bandref.lower_bound(rec[a:b], H, W, dmax, m["tau"], r, world)
        assert set(np.flatnonzero(must_up)) <= set(up.tolist()) and set(np.flatnonzero(must_down)) <= set(down.tolist())
        r0, r1 = m["rows"]
        _check_image(_arr(out, variant, "slab", r), ref[r0:r1], what)
        travelled = np.zeros(b - a, dtype=bool)
        travelled[up] = True
        travelled[down] = True
        _check_grads(_arr(out, variant, "g", r), [g[a:b] for g in gref], rec[a:b, 0:3], what, travelled)


# ---------------------------------------------------------------------------------------------------
# broadcast + splat_band / splat_band_packed + the gradient collective
# ---------------------------------------------------------------------------------------------------
def _lacks_collective(text):
    """is `text` the process group saying that it has no reduce_scatter for device tensors"""
    t = text.lower()
    return ("reduce_scatter" in t or "reducescatter" in t) and any(k in t for k in ("support", "implement", "unsupported", "no backend"))


@pytest.mark.gpu
@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("mode", REDUCE)
@pytest.mark.parametrize("form", ["band", "packed"])
def test_broadcast_band_on_ranks_matches_the_oracle(form, mode, world, ranks):
    out = ranks(world)
    variant = f"{form}-{mode}"
    rec, ref, gref = _truth("adjacent")
    H = ref.shape[0]
    n = rec.shape[0]
    metas = [_meta(out, variant, r) for r in range(world)]
    for r, m in enumerate(metas):
        what = f"{variant} rank {r}/{world}"
        r0, r1 = m["rows"]
        assert (r0, r1) == bandref.row_band(H, r, world)
        _check_image(_arr(out, variant, "slab", r), ref[r0:r1], what)
        _check_image(_arr(out, variant, "full", r), ref, what + " gather_image")       # every rank gathers the whole image
    lacking = [m["unsupported"] for m in metas if m["unsupported"]]
    if lacking:
        assert mode == "reduce_scatter" and len(lacking) == world and all(_lacks_collective(t) for t in lacking), lacking
        pytest.skip(f"the process group has no reduce_scatter_tensor for device tensors: {lacking[0][:300]}")
    for r, m in enumerate(metas):
        what = f"{variant} rank {r}/{world}"
        g = _arr(out, variant, "g", r)
        assert g.shape == (n, 8)
        if mode == "all_reduce":
            _check_grads(g, gref, rec[:, 0:3], what)
        else:
            a, b = m["slice"]
            per = (n + world - 1) // world
            assert (a, b) == (min(n, r * per), min(n, (r + 1) * per))
            assert not g[:a].any() and not g[b:].any(), what                           # exactly zero outside the rank's slice
            _check_grads(g[a:b], [w[a:b] for w in gref], rec[a:b, 0:3], what)


# ---------------------------------------------------------------------------------------------------
# overflow and reuse
# ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("form", ["plain", "overlap"])
def test_overflow_poisons_exactly_the_ranks_that_dropped(form, world, ranks):
    """cap = 2 on the adjacent geometry: a rank whose check() says "enlarge cap" carries a NaN in its slab AND its gradient (from
    the device-side counts, nobody has to call check()); a rank whose counts fit carries none; every rank got through"""
    out = ranks(world)
    variant = f"overflow-{form}"
    flagged = 0
    for r in range(world):
        m = _meta(out, variant, r)
        slab, g = _arr(out, variant, "slab", r), _arr(out, variant, "g", r)
        n_up, n_down, n_far, _ = m["counts"]
        assert m["cap"] == 2 and n_far == 0
        if max(n_up, n_down) > 2:
            assert m["err"] is not None and "enlarge cap" in m["err"], m["err"]
            assert np.isnan(slab).any() and np.isnan(g).any(), (variant, r)
            flagged += 1
        else:
            assert m["err"] is None, m["err"]
            assert not np.isnan(slab).any() and not np.isnan(g).any(), (variant, r)
    assert flagged > 0


@pytest.mark.gpu
@pytest.mark.parametrize("world", WORLDS)
def test_reused_exchange_raises_on_ranks(world, ranks):
    out = ranks(world)
    for r in range(world):
        m = _meta(out, "reuse", r)
        assert m["raised"] is not None and "one BandExchange per forward" in m["raised"], m["raised"]
        assert m["finite"]
        assert _meta(out, "done", r)["ok"]
