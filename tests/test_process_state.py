"""Process-wide state that outlives a call: the plan notes (what a plan decided about its workspace's layout, kept per
workspace address), the kernel-choice registry changed between a plan and its use, the workspace pools, and host threads.

Every other parity test plans, renders and differentiates from a clean process state on one thread.  Here the registry is
registered / switched / cleared between the plan and the calls that use it, the plan's note is pushed out of its
direct-mapped entry by a colliding workspace, and several host threads share the pools.  Every result is held to the CPU
oracle at the suite's bars; a deterministic backward (tile-stationary, home-tile) also to the bits of its repeated run.
"""
import ctypes
import os
import random
import re
import sys
import threading
import time

import numpy as np
import pytest
import torch

from test_bwd_tile import per_gaussian_ok

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_PLAN = -1, -3
IMG_ATOL = 2e-4
NOTES = 1024


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the MI355X box)"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _clean_registry():
    from gsasr_amd import _cabi
    _cabi.clear_kernel_choices()
    yield
    _cabi.clear_kernel_choices()


# ---- the note table's slot, restated --------------------------------------------------------------

def note_slot(addr: int) -> int:
    """the direct-mapped entry of a workspace's plan note: note_slot() of gsasr_amd/csrc/splat_api.hip, restated
    ((addr >> 8) * 2654435761 in 64-bit arithmetic, bits 22..31)"""
    return ((((addr >> 8) * 2654435761) & 0xFFFFFFFFFFFFFFFF) >> 22) & (NOTES - 1)


def colliding_offsets(base: int, nbytes: int, steps: int = 8192):
    """offsets (0, k * 256 >= nbytes) from the 256-byte aligned address `base` of two non-overlapping workspaces of `nbytes`
    whose notes share one direct-mapped entry"""
    first = (nbytes + 255) // 256 * 256
    want = note_slot(base)
    for k in range(steps):
        off = first + 256 * k
        if note_slot(base + off) == want:
            return 0, off
    raise AssertionError("no colliding workspace address found")


def colliding_workspaces(nbytes: int, dev):
    """two non-overlapping, 256-byte aligned uint8 workspaces of `nbytes` carved from one buffer, same note entry"""
    first = (nbytes + 255) // 256 * 256
    buf = torch.empty(2 * first + 8192 * 256 + 256, dtype=torch.uint8, device=dev)
    pad = (-buf.data_ptr()) % 256
    a, b = colliding_offsets(buf.data_ptr() + pad, nbytes)
    wa, wb = buf[pad + a:pad + a + nbytes], buf[pad + b:pad + b + nbytes]
    assert note_slot(wa.data_ptr()) == note_slot(wb.data_ptr()) and wa.data_ptr() + nbytes <= wb.data_ptr()
    return buf, wa, wb


def test_note_slot_helper_matches_the_library_source():
    """the helper pins the C formula: a change to the hash fails HERE, not the eviction tests silently (they would then
    plan two workspaces that no longer collide)"""
    src = open(os.path.join(ROOT, "gsasr_amd", "csrc", "splat_api.hip")).read()
    m = re.search(r"static unsigned note_slot\(const void \*ws\) \{ (.*?) \}", src)
    assert m, "note_slot() not found in splat_api.hip"
    assert m.group(1) == "return (unsigned)(((uintptr_t)ws >> 8) * 2654435761u >> 22) & (NOTES - 1);"
    assert re.search(r"constexpr int NOTES = 1024;", src)
    # known answers (64-bit product, bits 22..31)
    assert note_slot(0) == 0
    assert note_slot(0x7F0000000000) == ((((0x7F0000000000 >> 8) * 2654435761) % (1 << 64)) >> 22) % 1024
    assert note_slot(0x100) == (2654435761 >> 22) & 1023 == 632
    assert note_slot(0x7FFF_FFFF_FF00) == ((((0x7FFF_FFFF_FF00 >> 8) * 2654435761) & (2 ** 64 - 1)) >> 22) & 1023


def test_colliding_offsets_always_found():
    """for any 256-byte aligned base and workspace size the search finds a non-overlapping colliding neighbour"""
    rng = random.Random(7)
    for _ in range(300):
        base = rng.randrange(1 << 36, 1 << 47) & ~255
        n = rng.choice([256, 4096, 123456, 3 << 20])
        a, b = colliding_offsets(base, n)
        assert a == 0 and b >= n and b % 256 == 0 and note_slot(base) == note_slot(base + b)


# ---- host-decided errors (no launch happens: these run without a GPU) ------------------------------

def _buf(nbytes):
    """memory standing in for a workspace the library never plans into, and for the call's inputs and outputs: device
    memory where there is a GPU (should the refusal ever come after a launch, the kernel still reads valid memory), host
    memory otherwise; returns (owner, 256-byte aligned address)"""
    if torch.cuda.is_available():
        a = torch.zeros(nbytes + 256, dtype=torch.uint8, device="cuda")
        p = a.data_ptr()
    else:
        a = np.zeros(nbytes + 256, dtype=np.uint8)
        p = a.ctypes.data
    return a, p + (-p) % 256


def test_calls_on_a_workspace_without_a_plan_are_refused():
    """a forward / backward / step backward on a workspace the library holds no plan note for (never planned, or planned
    for another shape) is GSASR_ERR_PLAN -- never a layout re-derived from the caller's dims and the registry of the moment"""
    from gsasr_amd import _cabi
    L = _cabi.lib()
    d = _cabi.make_dims(1073, 87, 111, 0.3)
    n = L.gsasr_step_workspace_bytes(ctypes.byref(d))
    keep, ws = _buf(n)
    keep2, p = _buf(4 * (1073 * 9 + 111 * 87 * 3 + 4096))
    assert L.gsasr_splat_forward(ctypes.byref(d), ws, n, p, None) == ERR_PLAN
    assert "re-plan" in L.gsasr_last_error().decode()
    assert L.gsasr_splat_backward(p, p, p, p, p, p, p, ctypes.byref(d), ws, n, None) == ERR_PLAN
    assert L.gsasr_step_backward(p, p, p, p, ctypes.byref(d), ws, n, None) == ERR_PLAN
    assert L.gsasr_step_sample_backward(p, p, p, p, ctypes.byref(d), ws, n, None, 0, p, 4096, None) == ERR_PLAN
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    del keep, keep2


def test_home_with_planar_gradient_is_refused_not_rerouted():
    """GSASR_FLAG_BWD_HOME | GSASR_FLAG_CHW_GRAD on gsasr_splat_backward: GSASR_ERR_ARG (the home-tile kernel reads interleaved
    gradients), not a quiet switch to the order-dependent atomic kernel.  Decided before any launch."""
    from gsasr_amd import _cabi
    L = _cabi.lib()
    d = _cabi.make_dims(1073, 87, 111, 0.3, flags=_cabi.FLAG_BWD_HOME | _cabi.FLAG_CHW_GRAD)
    n = L.gsasr_splat_workspace_bytes(ctypes.byref(d))
    keep, ws = _buf(n)
    keep2, p = _buf(4 * 111 * 87 * 3)
    assert L.gsasr_splat_backward(p, p, p, p, p, p, p, ctypes.byref(d), ws, n, None) == ERR_ARG
    assert "CHW_GRAD" in L.gsasr_last_error().decode()
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    del keep, keep2


def test_cpp_node_pool_key_covers_the_same_layout_flags():
    """the C++ autograd node's workspace pool and the Python one agree on what counts as a layout (GSASR_FLAG_BWD_HOME
    included)"""
    from gsasr_amd import _cabi, _cpp_node
    ext = _cpp_node.load()
    assert ext is not None, "the C++ autograd node is built by build()"
    assert ext.layout_flags() == _cabi._LAYOUT_FLAGS
    assert _cabi._LAYOUT_FLAGS & _cabi.FLAG_BWD_HOME


class _FakeParams:
    """stands in for a CUDA gs_parameters tensor where tune_step never reaches the GPU (its measurement is stubbed)"""
    is_cuda = True

    def __init__(self, n):
        self.shape = (n, 9)
        self.device = torch.device("cpu")

    def detach(self):
        return self

    def contiguous(self):
        return self


def test_tune_default_candidate_is_the_kernel_the_rule_runs(monkeypatch):
    """tune_step on a dense shape where the rule picks the home-tile backward: when "default" wins it is registered as
    "follow the rule" (flags 0), so the default candidate must BE the rule's kernel -- the kernel later calls run is the
    one that was measured"""
    from gsasr_amd import _cabi, gaussian_splatting as gsp, tune
    H, W, n = 512, 1024, 16 * 128 * 256       # 16 Gaussians per LR pixel at x4, 1024 tiles of 32 x 16 px
    assert gsp._backward_kernel(H * W, n) == _cabi.FLAG_BWD_HOME
    seen = {}

    def fake_measure(cands, step, iters, rounds):
        seen["default"] = cands[0]
        res = tune.TuneResult(cands[0][0], cands[0][1], cands[0][2])
        res.ms = {name: (1.0 if name == "default" else 2.0) for name, _, _ in cands}
        return res

    monkeypatch.setattr(tune, "_measure", fake_measure)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    res = tune.tune_step(_FakeParams(n), None, H, W, 0.1)
    assert res.name == "default" and res.registered
    runs = gsp._backward_kernel(H * W, n, gsp._step_shape(n, H, W, 0.1))
    assert runs == seen["default"][1] == _cabi.FLAG_BWD_HOME


class _SlowDict(dict):
    """the pool's key -> list map, with a pause inside every pop: two threads that give or take for ONE key without the
    pool's lock then both run their read-modify-write inside the other's"""

    def pop(self, *a):
        v = dict.pop(self, *a)
        time.sleep(0.002)
        return v


def test_workspace_pool_gives_under_one_lock():
    """four threads give eight workspaces each to the same key at once (CPU tensors): all 32 are kept, the byte count
    balances -- without the lock a give that pops the key's list while another holds it loses the other's workspaces"""
    from gsasr_amd import _cabi
    pool = _cabi._WorkspacePool()
    pool.KEEP = 64
    pool.free = _SlowDict()
    start = threading.Barrier(4)
    errors = []

    def giver(t):
        try:
            start.wait()
            for i in range(8):
                pool.give("k", torch.empty(100 + t, dtype=torch.uint8), 0)
        except BaseException as e:       # noqa: BLE001 (reported on the main thread)
            errors.append(e)

    th = [threading.Thread(target=giver, args=(t,)) for t in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors[0]
    held = [ws for lst in pool.free.values() for ws, _ in lst]
    assert len(held) == 32 and pool.bytes == sum(ws.numel() for ws in held) == 8 * (100 + 101 + 102 + 103)
    # ... and taken back by four threads at once: each workspace exactly once
    got, got_lock = [], threading.Lock()
    start2 = threading.Barrier(4)

    def taker():
        try:
            start2.wait()
            for _ in range(8):
                ws, _, clean = pool.take("k", 1, "cpu")
                assert clean, "a pooled workspace was missed"
                with got_lock:
                    got.append(ws)
        except BaseException as e:       # noqa: BLE001
            errors.append(e)

    th = [threading.Thread(target=taker) for _ in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors[0]
    assert len({id(w) for w in got}) == 32 and pool.bytes == 0 and not pool.free


def test_workspace_pool_is_thread_safe():
    """take / give hammered from several threads (CPU tensors): no workspace is handed out twice, the byte count balances"""
    from gsasr_amd import _cabi
    pool = _cabi._WorkspacePool()
    pool.KEEP = 64
    keys = [("k", i) for i in range(3)]
    out = {}
    out_lock = threading.Lock()
    errors = []
    start = threading.Barrier(6)

    def worker(seed):
        rng = random.Random(seed)
        mine = []
        try:
            start.wait()
            for it in range(3000):
                if mine and rng.random() < 0.5:
                    key, ws, par = mine.pop(rng.randrange(len(mine)))
                    with out_lock:
                        del out[id(ws)]
                    pool.give(key, ws, par)
                else:
                    key = rng.choice(keys)
                    ws, par, _ = pool.take(key, 64 + keys.index(key), "cpu")
                    with out_lock:
                        assert id(ws) not in out, "a pooled workspace was handed out twice"
                        out[id(ws)] = ws
                    mine.append((key, ws, par))
            for key, ws, par in mine:
                with out_lock:
                    del out[id(ws)]
                pool.give(key, ws, par)
        except BaseException as e:       # noqa: BLE001 (reported on the main thread)
            errors.append(e)

    th = [threading.Thread(target=worker, args=(s,)) for s in range(6)]
    old = sys.getswitchinterval()
    sys.setswitchinterval(1e-6)      # (switch threads inside the pool's read-modify-write sequences, not only between them)
    try:
        for t in th:
            t.start()
        for t in th:
            t.join()
    finally:
        sys.setswitchinterval(old)
    assert not errors, errors[0]
    assert not out
    held = sum(ws.numel() for lst in pool.free.values() for ws, _ in lst)
    assert pool.bytes == held
    ids = [id(ws) for lst in pool.free.values() for ws, _ in lst]
    assert len(ids) == len(set(ids))


# ---- GPU: evicted notes with the registry changed between plan and use ---------------------------

def _flags():
    from gsasr_amd import _cabi
    return _cabi.FLAG_BWD_GAUSSIAN, _cabi.FLAG_BWD_TILE, _cabi.FLAG_BWD_HOME


def _plan_choices():
    G, T, Hm = _flags()
    return {"none": None, "gaussian": (G, 0), "tile": (T, 0), "home": (Hm, 0), "tile-cap": (T, 256)}


def _use_choices(plan_name):
    """what the registry holds at use time: cleared, switched to another backward, another list capacity"""
    G, T, Hm = _flags()
    pc = _plan_choices()[plan_name]
    switched = {"none": (T, 0), "gaussian": (T, 0), "tile": (G, 0), "home": (T, 0), "tile-cap": (Hm, 0)}[plan_name]
    flags = pc[0] if pc else 0
    cap = (flags, -1) if pc and pc[1] > 0 else (flags, 128)
    return {"cleared": None, "switched": switched, "list_cap": cap}


def _register(shape, choice):
    from gsasr_amd import _cabi
    _cabi.clear_kernel_choices()
    if choice is not None:
        _cabi.set_kernel_choice(shape, *choice)


def _max_bytes(fn, d, shape, choices):
    """workspace bytes large enough for a plan under any of the registry states"""
    n = 0
    for c in choices:
        _register(shape, c)
        n = max(n, fn(ctypes.byref(d)))
    _register(shape, None)
    return n


def _copy(d, extra=0):
    from gsasr_amd import _cabi
    e = _cabi.Dims.from_buffer_copy(d)
    e.flags |= extra
    return e


class _Inputs:
    """raw parameters, their kernel frame (the step prologue's own output: one oracle serves the splat and the step entry
    points) and the oracle's image and gradients, per sample"""

    def __init__(self, sizes, n_lr, scale, gpp, dmax, seed, dev):
        from gsasr_amd import _cabi, synthetic
        from oracle import gs_oracle
        self.sizes, self.dmax, self.B = sizes, dmax, len(sizes)
        self.gp = torch.stack([synthetic.gs_parameters(*n_lr, seed=seed + b, gpp=gpp) for b in range(self.B)]).to(dev)
        self.steps = torch.tensor([1.2 / scale] * self.B, device=dev)
        self.frames, self.img_ref, self.grad_img, self.gref, self.gp_ref = [], [], [], [], []
        for b, (h, w) in enumerate(sizes):
            sig, xy, col = _cabi.prologue_forward(self.gp[b].contiguous(), self.steps[b:b + 1], h, w)
            fr = [t.cpu().numpy() for t in (sig, xy, col)]
            wgt = synthetic.grad_image(h, w, seed + 100 + b).numpy()
            self.frames.append(fr)
            self.grad_img.append(wgt)
            self.img_ref.append(gs_oracle.forward_f64(*fr, h, w, dmax))
            g = gs_oracle.backward_f64(*fr, wgt, dmax)
            self.gref.append(g)
            gt = [torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev) for x in g]
            self.gp_ref.append(_cabi.prologue_backward(self.gp[b].contiguous(), self.steps[b:b + 1], h, w, *gt).cpu().numpy())
        torch.cuda.synchronize()


_INPUTS = {}


def _inputs(name, dev):
    if name not in _INPUTS:
        if name == "ragged":        # 37 x 29 LR at x3: 111 x 87, nothing a multiple of a tile or a cell
            _INPUTS[name] = _Inputs([(111, 87)], (37, 29), 3.0, 1, 0.3, 11, dev)
        elif name == "batch":       # a canvas of three ragged samples (one size per canvas: what training crops are)
            _INPUTS[name] = _Inputs([(111, 87)] * 3, (37, 29), 3.0, 1, 0.3, 21, dev)
        else:                       # 16 per LR pixel at x4, 512 x 1024: the home-tile backward and tile lists by default
            _INPUTS[name] = _Inputs([(512, 1024)], (128, 256), 4.0, 16, 0.1, 31, dev)
    return _INPUTS[name]


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def _run_splat(inp, plan_c, use_c, evict, dev):
    """gsasr_splat_plan (registry `plan_c`) -> registry `use_c` -> [a plan in a colliding workspace] -> forward + backward
    with flags 0 (the library picks)"""
    from gsasr_amd import _cabi
    L, st = _cabi.lib(), _cabi._stream(dev)
    (h, w), fr = inp.sizes[0], inp.frames[0]
    sig, xy, col = (_t(x, dev) for x in fr)
    n = sig.shape[0]
    d = _cabi.make_dims(n, h, w, inp.dmax)
    shape = _cabi.make_dims(n, h, w, inp.dmax)
    nb = _max_bytes(L.gsasr_splat_workspace_bytes, d, shape, [plan_c, use_c])
    buf, wa, wb = colliding_workspaces(nb, dev)
    ptrs = (sig.data_ptr(), xy.data_ptr(), col.data_ptr())
    _register(shape, plan_c)
    _cabi.check(L.gsasr_splat_plan(*ptrs, ctypes.byref(d), wa.data_ptr(), nb, st), "plan")
    _register(shape, use_c)
    if evict:
        _cabi.check(L.gsasr_splat_plan(*ptrs, ctypes.byref(d), wb.data_ptr(), nb, st), "colliding plan")
    img = torch.full((h, w, 3), float("nan"), device=dev)
    rc_f = L.gsasr_splat_forward(ctypes.byref(_copy(d, _cabi.FLAG_OVERWRITE_IMAGE)), wa.data_ptr(), nb, img.data_ptr(), st)
    g = [torch.full_like(t, float("nan")) for t in (sig, xy, col)]
    gw = _t(inp.grad_img[0], dev)
    rc_b = L.gsasr_splat_backward(*ptrs, gw.data_ptr(), *(t.data_ptr() for t in g), ctypes.byref(_copy(d, _cabi.FLAG_OVERWRITE_GRADS)),
                                  wa.data_ptr(), nb, st)
    torch.cuda.synchronize()
    return (rc_f, rc_b), [img.cpu().numpy()] + [t.cpu().numpy() for t in g]


def _step_dims(inp):
    from gsasr_amd import _cabi
    f = _cabi.FLAG_OVERWRITE_IMAGE | _cabi.FLAG_CHW_IMAGE
    if inp.B == 1:
        h, w = inp.sizes[0]
        return _cabi.make_dims(inp.gp.shape[1], h, w, inp.dmax, flags=f), _cabi.make_dims(inp.gp.shape[1], h, w, inp.dmax)
    h, w = inp.sizes[0]
    return (_cabi.make_batch_dims(inp.gp.shape[1], inp.sizes, w, h, inp.dmax, flags=f),
            _cabi.make_batch_dims(inp.gp.shape[1], inp.sizes, w, h, inp.dmax))


def _run_step(inp, plan_c, use_c, evict, dev):
    """gsasr_step_forward (registry `plan_c`) -> registry `use_c` -> [a step forward in a colliding workspace] ->
    gsasr_step_backward on an interleaved gradient"""
    from gsasr_amd import _cabi
    L, st = _cabi.lib(), _cabi._stream(dev)
    d, shape = _step_dims(inp)
    nb = _max_bytes(L.gsasr_step_workspace_bytes, d, shape, [plan_c, use_c])
    buf, wa, wb = colliding_workspaces(nb, dev)
    gp = inp.gp[0].contiguous() if inp.B == 1 else inp.gp.contiguous()
    steps = inp.steps.contiguous()
    slot = d.slot if inp.B > 1 else d.h
    img = torch.full((inp.B, 3, slot, d.w), float("nan"), device=dev)
    _register(shape, plan_c)
    _cabi.check(L.gsasr_step_forward(gp.data_ptr(), steps.data_ptr(), ctypes.byref(d), wa.data_ptr(), nb, img.data_ptr(), st), "step")
    _register(shape, use_c)
    if evict:
        scratch = torch.empty_like(img)
        _cabi.check(L.gsasr_step_forward(gp.data_ptr(), steps.data_ptr(), ctypes.byref(d), wb.data_ptr(), nb, scratch.data_ptr(), st),
                    "colliding step")
    grad = torch.zeros(inp.B * slot, d.w, 3, device=dev)
    for b, (h, w) in enumerate(inp.sizes):
        grad[b * slot:b * slot + h, :w] = _t(inp.grad_img[b], dev)
    gpar = torch.full_like(gp, float("nan"))
    rc = L.gsasr_step_backward(gp.data_ptr(), steps.data_ptr(), grad.data_ptr(), gpar.data_ptr(), ctypes.byref(d), wa.data_ptr(), nb, st)
    torch.cuda.synchronize()
    return (0, rc), [img.cpu().numpy(), gpar.cpu().numpy().reshape(inp.B, -1, 9)]


def _points(h, w, n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randint(0, h, (n,), generator=g), torch.randint(0, w, (n,), generator=g)], 1).to(torch.int32)


def _run_sampled(inp, plan_c, use_c, evict, dev):
    """gsasr_step_sample_forward (registry `plan_c`) -> registry `use_c` -> [colliding] -> gsasr_step_sample_backward"""
    from gsasr_amd import _cabi
    L, st = _cabi.lib(), _cabi._stream(dev)
    d, shape = _step_dims(inp)
    d = _copy(d)
    d.flags = 0
    nb = _max_bytes(L.gsasr_step_workspace_bytes, d, shape, [plan_c, use_c])
    buf, wa, wb = colliding_workspaces(nb, dev)
    (h, w) = inp.sizes[0]
    pts = _points(h, w, 777, 5).to(dev)
    npt = pts.shape[0]
    sws = _cabi._sample_ws(d, npt, dev)
    sws2 = _cabi._sample_ws(d, npt, dev)
    gp, step = inp.gp[0].contiguous(), inp.steps[:1].contiguous()
    out = torch.full((3, npt), float("nan"), device=dev)
    _register(shape, plan_c)
    _cabi.check(L.gsasr_step_sample_forward(gp.data_ptr(), step.data_ptr(), ctypes.byref(d), wa.data_ptr(), nb, pts.data_ptr(), npt,
                                            out.data_ptr(), sws.data_ptr(), sws.numel(), st), "sampled step")
    _register(shape, use_c)
    if evict:
        o2 = torch.empty_like(out)
        _cabi.check(L.gsasr_step_sample_forward(gp.data_ptr(), step.data_ptr(), ctypes.byref(d), wb.data_ptr(), nb, pts.data_ptr(), npt,
                                                o2.data_ptr(), sws2.data_ptr(), sws2.numel(), st), "colliding sampled step")
    gout = _t(np.random.default_rng(3).uniform(0, 1, (3, npt)), dev)
    gpar = torch.full_like(gp, float("nan"))
    rc = L.gsasr_step_sample_backward(gp.data_ptr(), step.data_ptr(), gout.data_ptr(), gpar.data_ptr(), ctypes.byref(d), wa.data_ptr(),
                                      nb, None, npt, sws.data_ptr(), sws.numel(), st)
    torch.cuda.synchronize()
    return (0, rc), [out.cpu().numpy(), gpar.cpu().numpy(), pts.cpu().numpy(), gout.cpu().numpy()]


def _check_splat(inp, res):
    img, gs, gc, gk = res
    assert np.abs(img - inp.img_ref[0]).max() <= IMG_ATOL, float(np.abs(img - inp.img_ref[0]).max())
    rho = inp.frames[0][0][:, 2]
    for got, want, name in zip((gs, gc, gk), inp.gref[0], ("sigmas", "coords", "colors")):
        per_gaussian_ok(got, want, name, rho=rho)


def _check_step(inp, res):
    img, gpar = res
    for b, (h, w) in enumerate(inp.sizes):
        got = img[b, :, :h, :w].transpose(1, 2, 0)
        assert np.abs(got - inp.img_ref[b]).max() <= IMG_ATOL, (b, float(np.abs(got - inp.img_ref[b]).max()))
        assert (img[b, :, h:, :] == 0).all() and (img[b, :, :, w:] == 0).all()      # the slot's padding
        per_gaussian_ok(gpar[b], inp.gp_ref[b], "g_parameters[%d]" % b)


def _check_sampled(inp, res, dev):
    from gsasr_amd import _cabi
    from oracle import gs_oracle
    out, gpar, pts, gout = res
    ref = inp.img_ref[0][pts[:, 0], pts[:, 1]].T
    assert np.abs(out - ref).max() <= IMG_ATOL
    (h, w) = inp.sizes[0]
    gimg = np.zeros((h, w, 3))
    np.add.at(gimg, (pts[:, 0], pts[:, 1]), gout.T.astype(np.float64))
    g = gs_oracle.backward_f64(*inp.frames[0], gimg, inp.dmax)
    gp_ref = _cabi.prologue_backward(inp.gp[0].contiguous(), inp.steps[:1], h, w, *(_t(x, dev) for x in g)).cpu().numpy()
    per_gaussian_ok(gpar, gp_ref, "g_parameters")


_ENTRIES = {"splat": _run_splat, "step": _run_step, "batch": _run_step, "sampled": _run_sampled}


def _matrix(entry, inp, plan_names, use_names, dev, tile_bitwise=True):
    G, T, Hm = _flags()
    n = 0
    for pn in plan_names:
        uses = _use_choices(pn)
        for un in use_names:
            # (the tile-stationary kernel runs on a plan with slots unless the choice at use time names another kernel)
            tile_runs = pn in ("tile", "tile-cap") and (uses[un] is None or not uses[un][0] & (G | Hm))
            runs = {}
            for evict in (False, True):
                rcs, res = _ENTRIES[entry](inp, _plan_choices()[pn], uses[un], evict, dev)
                # (a clean, re-plan error would be allowed; with lossless notes there is none, evicted or not)
                assert rcs == (0, 0), (entry, pn, un, evict, rcs)
                runs[evict] = res
            # the evicted note changes nothing: the same layout and kernels.  Gradients bit for bit (a Gaussian's gradient
            # is a sum over its own pixels, whatever order the plan placed the others in); the image to the order in which a
            # plan's atomics place the Gaussians of one cell; the sampled backward's points come through a counting sort
            for k, (a, b) in enumerate(zip(runs[False], runs[True])):
                if k == 0 or entry == "sampled" or (tile_runs and not tile_bitwise):
                    assert np.isfinite(b).all() and np.abs(a - b).max() <= 1e-6 * max(1.0, np.abs(a).max()), (entry, pn, un, k)
                else:
                    assert np.array_equal(a, b), (entry, pn, un, k)
            if entry == "splat":
                _check_splat(inp, runs[True])
            elif entry == "sampled":
                _check_sampled(inp, runs[True], dev)
            else:
                _check_step(inp, runs[True])
            n += 1
    return n


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["splat", "step", "batch", "sampled"])
def test_evicted_notes_and_a_changed_registry_ragged(entry, dev):
    """plan under each registry state, change it (cleared / switched / another list capacity), push the plan's note out of
    its entry by planning a colliding workspace or not: the oracle's image and gradients, never an error; with and without
    the eviction the gradients are bit-identical and the image agrees to fp32 rounding"""
    inp = _inputs("batch" if entry == "batch" else "ragged", dev)
    n = _matrix(entry, inp, list(_plan_choices()), ["cleared", "switched", "list_cap"], dev)
    assert n == 15


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["splat", "step"])
def test_evicted_notes_and_a_changed_registry_dense(entry, dev):
    """the dense crop (home-tile backward and tile lists by default): plans with and without slots and lists"""
    inp = _inputs("dense", dev)
    # (here the tile-stationary gradients of two plans differ in the last bits: held to 1e-6 of their max and the oracle)
    n = _matrix(entry, inp, ["none", "tile", "tile-cap"], ["cleared", "switched"], dev, tile_bitwise=False)
    assert n == 6


# ---- GPU: deterministic flag combinations ---------------------------------------------------------

@pytest.mark.gpu
def test_deterministic_flag_combinations_repeat_bit_for_bit(dev):
    """every combination the header calls deterministic -- the forward, the tile-stationary backward (interleaved and planar
    gradient), the home-tile backward, and the step backward that interleaves a planar gradient for the home-tile kernel --
    gives the same bits three runs in a row, at 16 Gaussians per LR pixel (thousands per tile); the image and gradients also
    meet the oracle"""
    from gsasr_amd import _cabi, synthetic
    from oracle import gs_oracle
    G, T, Hm = _flags()
    sig, xy, col, H, W = synthetic.kernel_inputs(48, 48, 4.0, seed=30, gpp=16)
    wgt = synthetic.grad_image(H, W, 31)
    a, b, c = (t.contiguous().to(dev) for t in (sig, xy, col))
    gw = wgt.to(dev)
    gw_chw = gw.permute(2, 0, 1).contiguous()
    L, st = _cabi.lib(), _cabi._stream(dev)
    ref_img = gs_oracle.forward_f64(sig.numpy(), xy.numpy(), col.numpy(), H, W, 0.2)
    gref = gs_oracle.backward_f64(sig.numpy(), xy.numpy(), col.numpy(), wgt.numpy(), 0.2)
    for plan_flag, chw in ((T, False), (T, True), (Hm, False)):
        outs = []
        for _ in range(3):
            p = _cabi.plan(a, b, c, H, W, 0.2, flags=plan_flag)
            img = _cabi.forward(p, torch.empty(H, W, 3, device=dev), overwrite=True)
            g = [torch.full_like(t, float("nan")) for t in (a, b, c)]
            d = _copy(p.dims, _cabi.FLAG_OVERWRITE_GRADS | (_cabi.FLAG_CHW_GRAD if chw else 0))
            _cabi.check(L.gsasr_splat_backward(a.data_ptr(), b.data_ptr(), c.data_ptr(), (gw_chw if chw else gw).data_ptr(),
                                               *(t.data_ptr() for t in g), ctypes.byref(d), p.workspace.data_ptr(), p.workspace.numel(), st),
                        "backward")
            torch.cuda.synchronize()
            outs.append([img.cpu().numpy()] + [t.cpu().numpy() for t in g])
            del p
        for o in outs[1:]:
            # gradients bit for bit; the image to fp32 rounding (two plans may place a cell's Gaussians in another order)
            for x, y in zip(outs[0][1:], o[1:]):
                assert np.array_equal(x, y), (plan_flag, chw)
            assert np.abs(outs[0][0] - o[0]).max() <= 1e-6 * max(1.0, np.abs(outs[0][0]).max())
        assert np.abs(outs[0][0] - ref_img).max() <= IMG_ATOL
        for got, want, name in zip(outs[0][1:], gref, ("sigmas", "coords", "colors")):
            per_gaussian_ok(got, want, name, rho=sig[:, 2].numpy())
    # the step backward with a planar gradient and the home-tile kernel (interleaved into the step's scratch first)
    gp = synthetic.gs_parameters(48, 48, seed=30, gpp=16).to(dev)
    step = torch.tensor([1.2 / 4.0], device=dev)
    outs = []
    for _ in range(3):
        img, plan = _cabi.step_forward(gp, step, H, W, 0.2, _cabi.FLAG_CHW_GRAD | Hm)
        gpar = _cabi.step_backward(plan, gp, step, gw_chw, chw=True)
        torch.cuda.synchronize()
        outs.append((img.cpu().numpy(), gpar.cpu().numpy()))
    for o in outs[1:]:
        assert np.array_equal(outs[0][1], o[1]) and np.abs(outs[0][0] - o[0]).max() <= 1e-6 * max(1.0, np.abs(outs[0][0]).max())
    fr = [t.cpu().numpy() for t in _cabi.prologue_forward(gp, step, H, W)]
    gr = gs_oracle.backward_f64(*fr, wgt.numpy(), 0.2)
    gp_ref = _cabi.prologue_backward(gp, step, H, W, *(_t(x, dev) for x in gr)).cpu().numpy()
    per_gaussian_ok(outs[0][1], gp_ref, "g_parameters")


@pytest.mark.gpu
def test_cpp_node_pools_home_plans_apart(dev):
    """the C++ node's version of test_host_path.py::test_pooled_workspaces_are_not_shared_between_layouts: a workspace a
    home-tile plan gives back is pooled under a key that carries GSASR_FLAG_BWD_HOME, the two kernels alternating on one
    shape keep one pooled workspace each, and the fused step through the node gives the same gradient every time"""
    from gsasr_amd import _cabi, _cpp_node, gaussian_splatting as gsp, synthetic
    ext = _cpp_node.load()
    assert ext is not None
    G, T, Hm = _flags()
    H, W = 96, 80
    p = synthetic.gs_parameters(24, 20, seed=9).to(dev)
    wgt = synthetic.grad_image(H, W, 3).permute(2, 0, 1).contiguous().to(dev)
    ref = {}
    old = gsp.BACKWARD_KERNEL
    ext.clear_pool()
    try:
        for it in range(4):
            for kernel, flag in (("home", Hm), ("gaussian", G)):
                gsp.BACKWARD_KERNEL = kernel
                pa = p.clone().requires_grad_(True)
                out = gsp.generate_2D_gaussian_splatting_step((H, W), pa, 4.0, (4.0, 4.0), dmax=0.3)
                out.backward(wgt)
                del out
                torch.cuda.synchronize()
                kinds = sorted(k[4] & (G | T | Hm) for k in ext.pool_keys() if (k[1], k[2], k[3]) == (480, H, W))
                assert kinds == ([G, Hm] if it or kernel == "gaussian" else [Hm]), (it, kernel, kinds)
                if kernel not in ref:
                    ref[kernel] = pa.grad.clone()
                assert float((pa.grad - ref[kernel]).abs().max()) <= 1e-6 * float(ref[kernel].abs().max())
        assert float((ref["home"] - ref["gaussian"]).abs().max()) <= 2e-4 * float(ref["gaussian"].abs().max())
    finally:
        gsp.BACKWARD_KERNEL = old
        ext.clear_pool()


@pytest.mark.gpu
def test_registered_interleaved_kernel_with_planar_gradient_is_refused(dev):
    """a planar gradient (GSASR_FLAG_CHW_GRAD, no kernel flag) on a plan without slots, for a shape whose registered choice is
    the home-tile or the Gaussian-stationary kernel: GSASR_ERR_ARG, not the atomic kernel in the registered one's place.
    With the tile-stationary choice registered the same call runs (deterministically) and meets the oracle."""
    from gsasr_amd import _cabi, synthetic
    from oracle import gs_oracle
    G, T, Hm = _flags()
    sig, xy, col, H, W = synthetic.kernel_inputs(37, 29, 3.0, seed=12)
    wgt = synthetic.grad_image(H, W, 13)
    a, b, c = (t.contiguous().to(dev) for t in (sig, xy, col))
    gw = wgt.permute(2, 0, 1).contiguous().to(dev)
    L, st = _cabi.lib(), _cabi._stream(dev)
    shape = _cabi.make_dims(a.shape[0], H, W, 0.3)
    for choice, want in ((Hm, ERR_ARG), (G, ERR_ARG), (T, 0)):
        _register(shape, (choice, 0))
        p = _cabi.plan(a, b, c, H, W, 0.3)
        g = [torch.full_like(t, float("nan")) for t in (a, b, c)]
        d = _copy(p.dims, _cabi.FLAG_OVERWRITE_GRADS | _cabi.FLAG_CHW_GRAD)
        rc = L.gsasr_splat_backward(a.data_ptr(), b.data_ptr(), c.data_ptr(), gw.data_ptr(), *(t.data_ptr() for t in g),
                                    ctypes.byref(d), p.workspace.data_ptr(), p.workspace.numel(), st)
        assert rc == want, (choice, rc, L.gsasr_last_error().decode())
        torch.cuda.synchronize()
        if rc == 0:
            gref = gs_oracle.backward_f64(sig.numpy(), xy.numpy(), col.numpy(), wgt.numpy(), 0.3)
            for got, r, name in zip(g, gref, ("sigmas", "coords", "colors")):
                per_gaussian_ok(got.cpu().numpy(), r, name, rho=sig[:, 2].numpy())
        del p


# ---- GPU: several host threads ----------------------------------------------------------------------

def _same(ref, got, what):
    """images to fp32 rounding (two plans of the same inputs may place a cell's Gaussians in another order: the forward
    is not bit-reproducible from plan to plan, even on one thread), gradients bit for bit"""
    for (kind, r), g in zip(ref, got):
        if kind == "img":
            assert np.abs(r - g).max() <= 1e-6 * max(1.0, np.abs(r).max()), what
        else:
            assert np.array_equal(r, g), what


def _worker_ops(name, dev):
    """one thread's calls: its own shapes and registered kernel choices; returns a function of the iteration that
    enqueues them on the current stream and returns [(kind, tensor)]"""
    from gsasr_amd import _cabi, gaussian_splatting as gsp, gscuda, synthetic
    G, T, Hm = _flags()
    if name == "tile":          # fused step + the plan API
        lr, scale, choice = (24, 20), 4.0, T
    elif name == "home":        # fused step + the batched step
        lr, scale, choice = (37, 29), 3.0, Hm
    else:                       # fused step + the reference-shaped launchers
        lr, scale, choice = (18, 22), 4.0, G
    H, W = int(lr[0] * scale), int(lr[1] * scale)
    ps = [synthetic.gs_parameters(*lr, seed=100 * len(name) + k).to(dev) for k in range(3)]
    n = ps[0].shape[0]
    _cabi.set_kernel_choice(_cabi.make_dims(n, H, W, 0.3), choice, 0)
    assert gsp._backward_kernel(H * W, n, gsp._step_shape(n, H, W, 0.3)) == choice
    wgt = synthetic.grad_image(H, W, 7).permute(2, 0, 1).contiguous().to(dev)
    sig, xy, col, _, _ = synthetic.kernel_inputs(*lr, scale, seed=3)
    sig, xy, col = (t.contiguous().to(dev) for t in (sig, xy, col))
    wgt_hwc = wgt.permute(1, 2, 0).contiguous()
    if name == "home":
        sizes = [(64, 48), (64, 48)]
        bp = torch.stack([synthetic.gs_parameters(16, 12, seed=50 + b) for b in range(2)]).to(dev)
        _cabi.set_kernel_choice(_cabi.make_batch_dims(16 * 12, sizes, 48, 64, 0.3), G, 0)
        bw = torch.rand(2, 3, 64, 48, generator=torch.Generator().manual_seed(5)).to(dev)

    def run(it):
        out = []
        pa = ps[it % 3].clone().requires_grad_(True)
        img = gsp.generate_2D_gaussian_splatting_step((H, W), pa, scale, (scale, scale), dmax=0.3)
        img.backward(wgt)
        out += [("img", img.detach()), ("grad", pa.grad)]
        if name == "tile":
            p = _cabi.plan(sig, xy, col, H, W, 0.3)
            im = _cabi.forward(p, torch.empty(H, W, 3, device=dev), overwrite=True)
            g = [torch.empty_like(t) for t in (sig, xy, col)]
            _cabi.backward(p, sig, xy, col, wgt_hwc, *g, overwrite=True)
            out += [("img", im)] + [("grad", t) for t in g]
        elif name == "home":
            pb = bp.clone().requires_grad_(True)
            ib = gsp.generate_2D_gaussian_splatting_batch(sizes, pb, [4.0, 4.0], [(4.0, 4.0)] * 2, dmax=0.3)
            ib.backward(bw)
            out += [("img", ib.detach()), ("grad", pb.grad)]
        else:
            im = torch.zeros(H, W, 3, device=dev)
            gscuda.gs_render(sig, xy, col, im, n, H, W, 3, 0.3)
            g = [torch.zeros_like(t) for t in (sig, xy, col)]
            gscuda.gs_render_backward(sig, xy, col, wgt_hwc, *g, n, H, W, 3, 0.3)
            out += [("img", im)] + [("grad", t) for t in g]
        return out

    return run


@pytest.mark.gpu
def test_three_host_threads_and_a_registry_churner_match_one_thread(dev):
    """three threads, each on its own stream with its own shapes and registered kernel choices (tile-stationary, home-tile,
    Gaussian-stationary), 20 iterations of the fused step + backward and of the plan API / the batched step / the
    reference-shaped launchers; a fourth thread registers and clears choices for shapes nobody else uses.  Every output
    equals the same call made on one thread beforehand (gradients bit for bit)."""
    from gsasr_amd import _cabi
    names = ["tile", "home", "gaussian"]
    runs = {nm: _worker_ops(nm, dev) for nm in names}
    ref = {}
    for nm in names:            # single-threaded, on the default stream
        ref[nm] = [[(k, t.cpu().numpy()) for k, t in runs[nm](it)] for it in range(3)]
    torch.cuda.synchronize()
    stop, errors = threading.Event(), []

    def churn():
        others = [_cabi.make_dims(1000 + 7 * k, 64 + k, 64, 0.3) for k in range(8)]
        G, T, Hm = _flags()
        k = 0
        try:
            while not stop.is_set():
                shape = others[k % 8]
                _cabi.set_kernel_choice(shape, (G, T, Hm)[k % 3], 64 * (k % 4))
                _cabi.set_kernel_choice(shape, 0, 0)
                k += 1
        except BaseException as e:       # noqa: BLE001 (reported on the main thread)
            errors.append(e)

    def worker(nm):
        try:
            s = torch.cuda.Stream(dev)
            got = []
            with torch.cuda.stream(s):
                for it in range(20):
                    got.append((it, runs[nm](it)))
            s.synchronize()
            for it, out in got:
                _same(ref[nm][it % 3], [t.cpu().numpy() for _, t in out], (nm, it))
        except BaseException as e:       # noqa: BLE001
            errors.append(e)

    th = [threading.Thread(target=churn)] + [threading.Thread(target=worker, args=(nm,)) for nm in names]
    for t in th:
        t.start()
    for t in th[1:]:
        t.join()
    stop.set()
    th[0].join()
    torch.cuda.synchronize()
    assert not errors, errors[0]


@pytest.mark.gpu
@pytest.mark.parametrize("node", ["python", "cpp"])
def test_plan_next_sample_while_the_engine_runs_the_last_backward(node, dev, monkeypatch):
    """the training loop's overlap: sample k's backward runs (and frees its Plan, handing the workspace back to the pool)
    on another thread while this thread plans sample k+1 -- through the Python autograd node and the C++ one; every image
    and gradient equals the sequential run"""
    from gsasr_amd import _cpp_node, gaussian_splatting as gsp, synthetic
    if node == "python":
        monkeypatch.setattr(_cpp_node, "load", lambda: None)
    else:
        assert _cpp_node.load() is not None
    H, W = 96, 80
    ps = [synthetic.gs_parameters(24, 20, seed=200 + k).to(dev) for k in range(12)]
    wgt = synthetic.grad_image(H, W, 9).permute(2, 0, 1).contiguous().to(dev)

    def forward(p):
        pa = p.clone().requires_grad_(True)
        return pa, gsp.generate_2D_gaussian_splatting_step((H, W), pa, 4.0, (4.0, 4.0), dmax=0.3)

    ref = []
    for p in ps:
        pa, out = forward(p)
        out.backward(wgt)
        ref.append([("img", out.detach().cpu().numpy()), ("grad", pa.grad.cpu().numpy())])
    errors, got = [], []

    def backward(holder):
        try:
            o = holder.pop()
            o.backward(wgt)
            del o                # the last reference to the graph, its node and its Plan: freed on this thread
        except BaseException as e:       # noqa: BLE001
            errors.append(e)

    th = None
    for k, p in enumerate(ps):
        pa, out = forward(p)     # (planned while the previous sample's backward runs)
        if th is not None:
            th.join()
        got.append((pa, out.detach()))
        holder = [out]
        del out
        th = threading.Thread(target=backward, args=(holder,))
        th.start()
    th.join()
    torch.cuda.synchronize()
    assert not errors, errors[0]
    for k, (pa, img) in enumerate(got):
        _same(ref[k], [img.cpu().numpy(), pa.grad.cpu().numpy()], k)
