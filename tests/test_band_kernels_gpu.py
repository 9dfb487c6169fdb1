"""The two kernels of the row-band exchange alone, in one process: k_band_select against an independent float64 window
(tests/bandref.py), its capacity guard inside sentinel-framed buffers, k_band_merge against a float64 index_add, and the emulated
exchange of tests/test_hip_parity.py::test_band_exchange_emulated_on_one_gpu held to the ORACLE instead of the library's own
full-image render -- which tells a failure of tests/test_shard_ranks_gpu.py apart: the kernels, or the plumbing around them.

The preconditions of the cases (what the float64 window says about them, that nudging moves and never drops, that the set
which must travel by the Gaussians' own images lies within the window's set) are checked without a GPU.
"""
import functools

import numpy as np
import pytest
import torch

import bandref
import gradbars

IMG_ATOL = 1e-4            # tests/test_hip_parity.py
SENTINEL, ISENTINEL = 777.0, -7


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the MI355X box)"
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------------
# k_band_select against the float64 window
# ---------------------------------------------------------------------------------------------------
CASES = {
    # 64 x 24 LR x4 = 256 x 96: three ranks have bands of 85 / 85 / 86 rows, aligned with nothing; eight have 32
    "bounded-w3": dict(lr=(64, 24), scale=4.0, seed=92, dmax=0.08, cutoff=0.0, world=3),
    "bounded-w8": dict(lr=(64, 24), scale=4.0, seed=92, dmax=0.08, cutoff=0.0, world=8),
    # the unbounded op: tau = 16 keeps a synthetic Gaussian (sigma <= 2.7 px) within 15.3 rows; the adaptive default is ln(N / 1e-5)
    "unbounded-tau16": dict(lr=(64, 24), scale=4.0, seed=94, dmax=None, cutoff=16.0, world=8),
    "unbounded-adaptive": dict(lr=(64, 24), scale=4.0, seed=94, dmax=None, cutoff=0.0, world=3),
    # 55 rows over four ranks: 13 / 14 / 14 / 14, rank 1 has 13 above and 14 below; the 21.6-row box reaches past a neighbour
    "uneven": dict(lr=(11, 6), scale=5.0, seed=95, dmax=0.8, cutoff=104.0, world=4),
}
SELECT = [(name, r) for name, c in CASES.items() for r in range(c["world"])]


@functools.lru_cache(maxsize=None)
def _case(name):
    """(records [N, 8] float32, H, W, [(a, b) own slice per rank]): rank r owns the Gaussians of its LR rows"""
    from gsasr_amd import synthetic
    c = CASES[name]
    h_lr, w_lr = c["lr"]
    sig, xy, col, H, W = synthetic.kernel_inputs(h_lr, w_lr, c["scale"], seed=c["seed"])
    rec = torch.cat([sig, xy, col], dim=1).contiguous().numpy()
    rec.setflags(write=False)
    return rec, H, W, [tuple(v * w_lr for v in bandref.row_band(h_lr, r, c["world"])) for r in range(c["world"])]


def _dead_mix(own, H, W):
    """every fourth record of `own` replaced by a dead one, in turn: NaN / +inf / -inf in a sigma or a centre, a zero sigma
    (centred between two rows and two columns, where even the widened window holds no pixel), a centre far off the grid"""
    own = np.array(own, dtype=np.float32)
    dead = np.arange(1, own.shape[0], 4)
    for k, i in enumerate(dead):
        kind, col = k % 6, (0, 1, 3, 4)[(k // 6) % 4]
        if kind < 3:
            own[i, col] = (np.nan, np.inf, -np.inf)[kind]
        elif kind == 3:
            own[i, (k // 6) % 2] = 0.0
            own[i, 3] = (np.floor((own[i, 3] + 1.0) * 0.5 * (W - 1)) + 0.5) / (0.5 * (W - 1)) - 1.0
            own[i, 4] = (np.floor((own[i, 4] + 1.0) * 0.5 * (H - 1)) + 0.5) / (0.5 * (H - 1)) - 1.0
        else:
            own[i, 3 + (k // 6) % 2] = (5.0, -5.0)[kind - 4]
    return own, dead


def _own_set(name, rank):
    """(own records, H, W, dmax, cutoff, world, dead indices or None) of a select case; "dead" and "ragged" are cut from the
    middle rank of bounded-w3"""
    if name in CASES:
        rec, H, W, own = _case(name)
        a, b = own[rank]
        c = CASES[name]
        return np.array(rec[a:b]), H, W, c["dmax"], c["cutoff"], c["world"], None
    rec, H, W, own = _case("bounded-w3")
    c = CASES["bounded-w3"]
    a, b = own[1]
    mine = np.array(rec[a:b])
    dead = None
    if name == "dead":
        mine, dead = _dead_mix(mine, H, W)
    elif name == "ragged-1":      # one record, and one that travels
        tau = bandref.exchange_tau(c["cutoff"], 1, 1)
        mine = mine[bandref.select(mine, H, W, c["dmax"], tau, 1, 3)["up"][:1]]
    else:
        mine = mine[np.r_[0:129, mine.shape[0] - 128: mine.shape[0]]]      # 257: the band's top and bottom Gaussians
    return mine, H, W, c["dmax"], c["cutoff"], 3, dead


EXTRA = [("dead", 1), ("ragged-1", 1), ("ragged-257", 1)]


def _reference(own, H, W, dmax, tau, rank, world, dead):
    """nudge, then the reference selection and the set that must travel by the Gaussians' own images; asserts what has to hold
    before anything is sent to a GPU"""
    n = own.shape[0]
    own, moved = bandref.nudge(own, H, dmax, tau, rank, world)
    assert own.shape[0] == n and moved.sum() <= max(2, n // 3)                     # moved, none dropped, and not the whole case
    ref = bandref.select(own, H, W, dmax, tau, rank, world)
    must_up, must_down = bandref.lower_bound(own, H, W, dmax, tau, rank, world)
    assert set(np.flatnonzero(must_up)) <= set(ref["up"].tolist()) and set(np.flatnonzero(must_down)) <= set(ref["down"].tolist())
    if dead is not None:
        assert not ref["live"][dead].any() and ref["live"].sum() == n - dead.size
        assert not np.isin(dead, np.concatenate([ref["up"], ref["down"], ref["far"]])).any()
    return own, ref, (must_up, must_down)


@pytest.mark.parametrize("name,rank", SELECT + EXTRA, ids=[f"{n}-r{r}" for n, r in SELECT + EXTRA])
def test_select_cases_on_the_cpu(name, rank):
    """the preconditions, with the documented tau in place of the one the library resolves (the GPU test asserts they agree)"""
    own, H, W, dmax, cutoff, world, dead = _own_set(name, rank)
    n = own.shape[0]
    tau = bandref.exchange_tau(cutoff, n, max(n, 1))
    own, ref, must = _reference(own, H, W, dmax, tau, rank, world, dead)
    above, below = bandref.neighbours(H, rank, world)
    if name == "ragged-1":
        assert n == 1 and ref["up"].size == 1
    else:
        assert (ref["up"].size > 0) == (above > 0) and (ref["down"].size > 0) == (below > 0), (name, rank)
        assert must[0].sum() > 0 or above == 0
        assert must[1].sum() > 0 or below == 0
        assert 0 < ref["live"].sum() - np.union1d(ref["up"], ref["down"]).size or name == "uneven"   # ... and some stay at home
    if name == "uneven" and rank == 1:
        assert (above, below) == (13, 14) and H % world != 0
        assert 0 < ref["far"].size < ref["live"].sum()
    if name in ("bounded-w3", "bounded-w8", "unbounded-tau16"):
        assert ref["far"].size == 0


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("name,rank", SELECT + EXTRA, ids=[f"{n}-r{r}" for n, r in SELECT + EXTRA])
def test_select_equals_the_float64_window(name, rank, dev):
    from gsasr_amd import shard
    own, H, W, dmax, cutoff, world, dead = _own_set(name, rank)
    n = own.shape[0]
    cap = max(n, 1)
    ex = shard.BandExchange(n, cap, H, W, dmax, cutoff=cutoff, device=dev, rank=rank, world=world)
    tau = ex.cutoff                                                   # resolved: what `select` and the local plan use
    assert abs(tau - bandref.exchange_tau(cutoff, n, cap)) <= 1e-5 * tau
    assert (ex.rows, (ex.rows_above, ex.rows_below)) == (bandref.row_band(H, rank, world), bandref.neighbours(H, rank, world))
    own, ref, (must_up, must_down) = _reference(own, H, W, dmax, tau, rank, world, dead)
    ex.own.copy_(torch.from_numpy(own))
    ex.counts.fill_(ISENTINEL)                                        # (the call itself clears them)
    ex.select()
    counts = ex.counts.tolist()
    assert counts == [ref["up"].size, ref["down"].size, ref["far"].size, 0], (counts, [ref[k].size for k in ("up", "down", "far")])
    for send, index, cnt, want, must in ((ex.send_up, ex.up_index, counts[0], ref["up"], must_up),
                                         (ex.send_down, ex.down_index, counts[1], ref["down"], must_down)):
        idx = index[:cnt].cpu().numpy()
        assert np.unique(idx).size == idx.size                                   # no duplicates
        assert np.array_equal(np.sort(idx), want)                                # the reference set
        assert torch.equal(_bits(send[:cnt]), _bits(ex.own[index[:cnt].long()]))  # bit-equal copies of own[index]
        assert torch.isnan(send[cnt:]).all()                                     # dead padding behind them
        assert set(np.flatnonzero(must)) <= set(idx.tolist())                    # (no window formula behind this one)
    if dead is not None:
        sel = np.concatenate([ex.up_index[:counts[0]].cpu().numpy(), ex.down_index[:counts[1]].cpu().numpy()])
        assert not np.isin(dead, sel).any() and counts[2] == 0 and counts[3] == 0


# ---------------------------------------------------------------------------------------------------
# capacity: counts of exactly cap, cap + 1, cap + 64, inside buffers framed by sentinels
# ---------------------------------------------------------------------------------------------------
CAP, PAD = 70, 5
EDGE_H, EDGE_W, EDGE_DMAX = 96, 48, 4.3 / 47.5        # the middle rank of three: rows [32, 64); a box of 4.3 rows, no support cutoff


def _edge_records(n_up, n_down, n_home, seed):
    """hand-made own set in shuffled order: `n_up` Gaussians 1.5 rows below the band's first row (their box reaches 2.8 rows
    above it), `n_down` 2.5 rows above its end, `n_home` in the middle; +-0.3 rows of jitter keeps every edge clear"""
    rng = np.random.default_rng(seed)
    n = n_up + n_down + n_home
    cyp = np.concatenate([np.full(n_up, 33.5), np.full(n_down, 61.5), np.full(n_home, 48.0)]) + rng.uniform(-0.3, 0.3, n)
    rec = np.empty((n, 8), dtype=np.float32)
    rec[:, 0:2] = rng.uniform(0.02, 0.06, (n, 2))
    rec[:, 2] = rng.uniform(-0.5, 0.5, n)
    rec[:, 3] = rng.uniform(-0.9, 0.9, n)
    rec[:, 4] = cyp / (0.5 * (EDGE_H - 1)) - 1.0
    rec[:, 5:8] = rng.uniform(0.0, 1.0, (n, 3))
    return rec[rng.permutation(n)]


def test_capacity_records_on_the_cpu():
    own = _edge_records(CAP + 1, CAP - 3, 300, 7)
    assert not bandref.near_edge(own, EDGE_H, EDGE_DMAX, -1.0, 1, 3).any()
    ref = bandref.select(own, EDGE_H, EDGE_W, EDGE_DMAX, -1.0, 1, 3)
    assert (ref["up"].size, ref["down"].size, ref["far"].size) == (CAP + 1, CAP - 3, 0)
    assert np.intersect1d(ref["up"], ref["down"]).size == 0


@pytest.mark.gpu
@pytest.mark.parametrize("side", ["up", "down"])
@pytest.mark.parametrize("extra", [0, 1, 64])
def test_select_capacity_guard(extra, side, dev):
    """one list holds cap + `extra` Gaussians, the other cap - 3.  `up` and `down` are the two halves of ONE tensor (as in
    BandExchange: send[:c], send[c:]) with sentinel rows before and after, the two index arrays and the counts likewise: a
    store past `cap` would land in the neighbour list or in a sentinel"""
    from gsasr_amd import _cabi
    n_over, n_other = CAP + extra, CAP - 3
    n_up, n_down = (n_over, n_other) if side == "up" else (n_other, n_over)
    own_np = _edge_records(n_up, n_down, 300, 11 + extra)
    ref = bandref.select(own_np, EDGE_H, EDGE_W, EDGE_DMAX, -1.0, 1, 3)
    assert (ref["up"].size, ref["down"].size) == (n_up, n_down)
    own = torch.from_numpy(own_np).to(dev)
    buf = torch.full((PAD + 2 * CAP + PAD, 8), SENTINEL, device=dev)
    ibuf = torch.full((PAD + 2 * CAP + PAD,), ISENTINEL, device=dev, dtype=torch.int32)
    cbuf = torch.full((12,), ISENTINEL, device=dev, dtype=torch.int32)
    up, down = buf[PAD: PAD + CAP], buf[PAD + CAP: PAD + 2 * CAP]
    up_index, down_index = ibuf[PAD: PAD + CAP], ibuf[PAD + CAP: PAD + 2 * CAP]
    counts = cbuf[4:8]
    _cabi.band_select(own, EDGE_H, EDGE_W, EDGE_DMAX, (32, 64), 32, 32, up, down, up_index, down_index, counts, cutoff=-1.0)
    torch.cuda.synchronize()
    # the frames
    assert (buf[:PAD] == SENTINEL).all() and (buf[-PAD:] == SENTINEL).all()
    assert (ibuf[:PAD] == ISENTINEL).all() and (ibuf[-PAD:] == ISENTINEL).all()
    assert (cbuf[:4] == ISENTINEL).all() and (cbuf[8:] == ISENTINEL).all()
    assert counts.tolist() == [n_up, n_down, 0, 0]                                 # the true totals, overflow or not
    for send, index, cnt, want in ((up, up_index, n_up, ref["up"]), (down, down_index, n_down, ref["down"])):
        kept = min(cnt, CAP)
        idx = index[:kept].cpu().numpy()
        assert np.unique(idx).size == kept and np.isin(idx, want).all()            # distinct Gaussians of THIS list
        assert torch.equal(_bits(send[:kept]), _bits(own[index[:kept].long()]))    # ... as they are in `own`
        if cnt <= CAP:                                                             # the list that fits is whole and intact
            assert np.array_equal(np.sort(idx), want)
            assert torch.isnan(send[cnt:]).all()


# ---------------------------------------------------------------------------------------------------
# k_band_merge against a float64 index_add (integer-valued floats: the order of the atomic adds cannot matter)
# ---------------------------------------------------------------------------------------------------
MERGE = {
    "both-lists": dict(s=300, cap=40, counts=(35, 33), shared=20),
    "at-cap": dict(s=300, cap=40, counts=(40, 40), shared=40),
    "above-cap": dict(s=300, cap=40, counts=(49, 140), shared=25),            # only the first `cap` rows of a list are added
    "zero-up": dict(s=300, cap=40, counts=(0, 17), shared=20),
    "zero-down": dict(s=300, cap=40, counts=(23, 0), shared=20),
    "outside": dict(s=300, cap=40, counts=(40, 31), shared=12, outside=True),  # an index outside [0, s) is ignored
    "one-gaussian": dict(s=1, cap=3, counts=(1, 1), shared=1),
    "no-gaussian": dict(s=0, cap=4, counts=(0, 0), shared=0),
    "no-capacity": dict(s=50, cap=0, counts=(0, 0), shared=0),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(MERGE))
def test_merge_equals_a_float64_index_add(name, dev):
    from gsasr_amd import _cabi
    c = MERGE[name]
    s, cap, shared = c["s"], c["cap"], c["shared"]
    rng = np.random.default_rng(sorted(MERGE).index(name))
    g_own = rng.integers(-8, 9, (s, 8)).astype(np.float32)
    # within a list an index appears once; `shared` of them appear in both
    up_index = rng.permutation(s)[:cap].astype(np.int32) if s >= cap else np.zeros(cap, dtype=np.int32)
    rest = np.setdiff1d(np.arange(s), up_index)
    down_index = np.concatenate([up_index[:shared], rng.permutation(rest)[:cap - shared]]).astype(np.int32)[:cap] \
        if s >= 2 * cap else up_index.copy()
    if c.get("outside"):
        up_index[[1, 7, 20]] = (-1, s, 2 ** 30)
        down_index[[0, 5]] = (-(2 ** 31), s + 3)
    g_up = rng.integers(-8, 9, (cap, 8)).astype(np.float32)
    g_down = rng.integers(-8, 9, (cap, 8)).astype(np.float32)
    want = g_own.astype(np.float64)
    named = np.zeros(s, dtype=bool)
    for g, index, cnt in ((g_up, up_index, c["counts"][0]), (g_down, down_index, c["counts"][1])):
        k = min(cnt, cap)
        ok = (index[:k] >= 0) & (index[:k] < s)
        np.add.at(want, index[:k][ok], g[:k][ok].astype(np.float64))
        named[index[:k][ok]] = True
        g[k:] = np.nan                                  # rows past the count are never read into a sum
    if (~named).any():
        g_own[np.flatnonzero(~named)[::3], 2] = np.nan    # rows that no index names stay as they are, bit for bit
        g_own[np.flatnonzero(~named)[1::3], 5] = -0.0
    t = lambda a: torch.from_numpy(a).to(dev)
    got = t(g_own.copy())
    before = _bits(got).clone()
    _cabi.band_merge(got, t(g_up), t(g_down), t(up_index), t(down_index),
                     torch.tensor([*c["counts"], 0, 0], device=dev, dtype=torch.int32))
    torch.cuda.synchronize()
    if name == "both-lists":
        k0, k1 = c["counts"]
        assert np.intersect1d(up_index[:k0], down_index[:k1]).size >= 8
    assert torch.equal(_bits(got)[t(~named)], before[t(~named)])
    assert np.array_equal(got.cpu().numpy()[named].astype(np.float64), want[named])


# ---------------------------------------------------------------------------------------------------
# the emulated exchange against the oracle
# ---------------------------------------------------------------------------------------------------
def _grads_ok(g8, want, sig, what):
    g8 = g8.detach().cpu().numpy()
    return gradbars.check_kernel((g8[:, 0:3], g8[:, 3:5], g8[:, 5:8]), want, sig, gradbars.SYNTHETIC_SHARE, what)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["thin", "unbounded-tau16"])
def test_emulated_exchange_matches_the_oracle(case, dev):
    """the flow of test_band_exchange_emulated_on_one_gpu -- select, copies for the swap, one plan over [own | halos], backward,
    return, merge, then the two-render form -- on three ranks of the thin geometry (33 Gaussians of the middle rank in both lists)
    and on the unbounded op with tau = 16; image and per-rank gradients against forward_f64 / backward_f64 of the whole image"""
    from gsasr_amd import shard, synthetic
    from oracle import gs_oracle
    world = 3
    rec_np, H, W, dmax, cutoff, cap, own = bandref.geometry("thin", world)
    if case == "unbounded-tau16":
        dmax, cutoff = None, 16.0
    wgt_np = synthetic.grad_image(H, W, bandref.GRAD_SEED).numpy()
    sig, xy, col = rec_np[:, 0:3], rec_np[:, 3:5], rec_np[:, 5:8]
    ref = gs_oracle.forward_f64(sig, xy, col, H, W, dmax)
    gref = gs_oracle.backward_f64(sig, xy, col, wgt_np, dmax)
    bar = IMG_ATOL * max(1.0, float(np.abs(ref).max()))
    rec, wgt = torch.from_numpy(rec_np).to(dev), torch.from_numpy(wgt_np).to(dev)
    be = shard.HipBackend

    def image_ok(slab, ex, what):
        err = float(np.abs(slab.cpu().numpy() - ref[ex.rows[0]: ex.rows[1]]).max())
        assert err <= bar, f"{what} rank {ex.rank}: image max|err| {err:.3e}"

    def swap_back_and_check(exs, what):
        for r, ex in enumerate(exs):
            c = ex.cap
            if r > 0:
                ex.ret_up.copy_(exs[r - 1].g_records[exs[r - 1].n + c:])          # what rank r-1 computed for my send_up
            if r < world - 1:
                ex.ret_down.copy_(exs[r + 1].g_records[exs[r + 1].n: exs[r + 1].n + c])
        for r, ex in enumerate(exs):
            a, b = own[r]
            _grads_ok(ex.merge(), [g[a:b] for g in gref], sig[a:b], f"{what} rank {r}")

    exs = []
    for r, (a, b) in enumerate(own):
        ex = shard.BandExchange(b - a, cap, H, W, dmax, cutoff=cutoff, device=dev, rank=r, world=world)
        ex.own.copy_(rec[a:b])
        ex.select()
        exs.append(ex)
    for r, ex in enumerate(exs):
        n_up, n_down = ex.check()
        if r > 0:
            ex.from_above.copy_(exs[r - 1].send_down)
        if r < world - 1:
            ex.from_below.copy_(exs[r + 1].send_up)
        if case == "thin" and r == 1:
            both = np.intersect1d(ex.up_index[:n_up].cpu().numpy(), ex.down_index[:n_down].cpu().numpy())
            assert both.size >= 8
    # one plan over [own | halos]
    for ex in exs:
        flags = dict(flags=ex.plan_flags) if ex.plan_flags else {}
        slab, st = be.forward_packed(ex.records, H, W, dmax, ex.rows, ex.cutoff, **flags)
        image_ok(slab, ex, "one plan")
        be.backward_packed(st, ex.records, wgt[ex.rows[0]: ex.rows[1]].contiguous(), ex.g_records)
    swap_back_and_check(exs, f"{case} one plan")
    # the two-render form: own Gaussians stored, the halo records added on top; backward halo part first
    for ex in exs:
        n = ex.n
        ex.g_records.fill_(float("nan"))
        slab = torch.full((ex.rows[1] - ex.rows[0], W, 3), float("nan"), device=dev)
        first = be.forward_packed_into(ex.records[:n], slab, H, W, dmax, ex.rows, ex.cutoff, ex.plan_flags, False)
        halo = be.forward_packed_into(ex.records[n:], slab, H, W, dmax, ex.rows, ex.cutoff, 0, True)
        image_ok(slab, ex, "two renders")
        gs = wgt[ex.rows[0]: ex.rows[1]].contiguous()
        be.backward_packed(halo, ex.records[n:], gs, ex.g_records[n:])
        be.backward_packed(first, ex.records[:n], gs, ex.g_records[:n])
    swap_back_and_check(exs, f"{case} two renders")
