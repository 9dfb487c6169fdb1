"""The routing of the host API, pinned: for a matrix of public calls, which launch-level functions gsasr_amd.gaussian_splatting
calls, in which order and with which arguments, compared with a table recorded once (tests/golden/host_routing.json.gz).

Recorded (the recorders call through): the `_cabi` launches, `_cpp_node.fused_step_apply`, `gsp._backward_kernel`, and
`deferred_asserts.watch` / `.add`.  Every argument is bound to the callee's parameter name (so a keyword that becomes positional
is not a difference) and normalised: a tensor as [dtype, shape, stride, device type, whose storage it is (the caller's
`gs_parameters`, `scale_modify` or target, with the offset into it) or None]; ints, floats, bools, strings and None verbatim;
a tuple tagged as one; the `shape` of `_backward_kernel` as the fields (s, h, w, batch, slot, dmax) of the Dims it returns.
The last entry of a case is what the public call returned (tensor layouts and requires_grad, no values).

The table is data: it was written by `python tests/test_host_routing_gpu.py --write` on the commit before the host layer's
argument resolution was shared, and a change of this layer that needs it rewritten has changed behaviour.  It is stored
gzipped (300 kB of JSON, one case per line: `zcat tests/golden/host_routing.json.gz`), and the git blob hash of the text is
checked against the recorded one (`BLOB`).

Shapes: N = 96 Gaussians on grids of 24 x 20 and 20 x 28, B = 3, S = 7 points -- the smallest at which the arms differ."""
import contextlib
import gzip
import hashlib
import inspect
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from gsasr_amd import _cabi, _cpp_node, gaussian_splatting as gsp, synthetic  # noqa: E402

pytestmark = pytest.mark.gpu
TABLE = os.path.join(ROOT, "tests", "golden", "host_routing.json.gz")
BLOB = "4b257b21da95032ccfc13462719c5d29e0076c64"      # `git hash-object` of the plain table as it was recorded


def _blob(text: bytes) -> str:
    return hashlib.sha1(b"blob %d\0" % len(text) + text).hexdigest()


CABI_NAMES = ("step_forward", "step_forward_u8", "step_forward_loss", "batch_forward", "batch_forward_loss", "step_sample_forward",
              "batch_sample_forward", "step_query_forward", "batch_query_forward", "plan", "forward")
G1, G2 = (24, 20), (20, 28)
SIZES = [G1, G2, G1]
B, S = 3, 7
WIN = (2, 4, 16, 12)
WINS = [(2, 4, 16, 12), (0, 8, 12, 16), (8, 0, 16, 14)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the MI355X box)"
    return torch.device("cuda:0")


# ---- the recorders ------------------------------------------------------------------------------------------------------

def _owner(t, own):
    if t.numel() == 0:
        return None
    for name, o in own:
        if o.numel() and t.device == o.device and t.untyped_storage().data_ptr() == o.untyped_storage().data_ptr():
            return f"{name}+{t.storage_offset() - o.storage_offset()}"
    return None


def _norm(v, own):
    if torch.is_tensor(v):
        return [str(v.dtype), list(v.shape), list(v.stride()), v.device.type, _owner(v, own)]
    if isinstance(v, torch.device):
        return ["device", v.type]
    if isinstance(v, tuple):
        return ["tuple"] + [_norm(e, own) for e in v]
    if isinstance(v, list):
        return [_norm(e, own) for e in v]
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    return [type(v).__name__]          # (a Plan, a ctypes struct: its presence, not its contents)


def _dims(shape):
    if shape is None:
        return None
    d = shape()
    return {"s": d.s, "h": d.h, "w": d.w, "batch": d.batch, "slot": d.slot, "dmax": float(d.dmax)}


@contextlib.contextmanager
def _recording(log, own, node=True):
    """recorders on the launch-level functions for the length of the block; `node=False`: the C++ node absent"""
    saved = []

    def patch(obj, name, value):
        saved.append((obj, name, obj.__dict__.get(name, saved)))      # (`saved` itself: "was not in the object's own dict")
        setattr(obj, name, value)

    def recorder(label, orig):
        sig = inspect.signature(orig)

        def call(*a, **kw):
            bound = sig.bind(*a, **kw)
            bound.apply_defaults()
            if label == "_backward_kernel":
                args = {"n_pixels": bound.arguments["n_pixels"], "n_gaussians": bound.arguments["n_gaussians"],
                        "shape": _dims(bound.arguments["shape"])}
            else:
                args = {k: _norm(v, own) for k, v in bound.arguments.items()}
            log.append([label, args])
            return orig(*a, **kw)
        return call

    try:
        for name in CABI_NAMES:
            patch(_cabi, name, recorder("_cabi." + name, getattr(_cabi, name)))
        patch(_cpp_node, "fused_step_apply", recorder("_cpp_node.fused_step_apply", _cpp_node.fused_step_apply))
        patch(gsp, "_backward_kernel", recorder("_backward_kernel", gsp._backward_kernel))
        patch(gsp.deferred_asserts, "watch", recorder("deferred_asserts.watch", gsp.deferred_asserts.watch))
        patch(gsp.deferred_asserts, "add", recorder("deferred_asserts.add", gsp.deferred_asserts.add))
        if not node:
            patch(_cpp_node, "load", lambda: None)
        yield
    finally:
        for obj, name, old in reversed(saved):
            if old is saved:
                delattr(obj, name)
            else:
                setattr(obj, name, old)


# ---- the matrix ---------------------------------------------------------------------------------------------------------

def _sm_single(form, dev):
    if form == "t2":
        return torch.tensor([2.0, 2.0], device=dev)
    if form == "numbers":
        return (2.0, 2.0)
    if form == "f64":
        return torch.tensor([2.0, 2.0], device=dev, dtype=torch.float64)
    if form == "strided":
        return torch.full((4,), 2.0, device=dev)[::2]
    if form == "cpu":
        return torch.tensor([2.0, 2.0])
    raise KeyError(form)


def _sm_batch(form, dev, n):
    if form == "B2":
        return torch.full((n, 2), 2.0, device=dev)
    if form == "list":
        return [torch.tensor([2.0, 2.0], device=dev) for _ in range(n)]
    if form == "expand":
        return torch.tensor([2.0, 2.0], device=dev).expand(n, 2)
    if form == "numbers":
        return [(2.0, 2.0)] * n
    if form == "f64":
        return torch.full((n, 2), 2.0, device=dev, dtype=torch.float64)
    if form == "wide":
        return torch.full((n, 4), 2.0, device=dev)[:, :2]
    raise KeyError(form)


SINGLE_FORMS = ("t2", "numbers", "f64", "strided", "cpu")
BATCH_FORMS = ("B2", "list", "expand", "numbers", "f64", "wide")


class _Ctx:
    """the inputs of one case: `p` [96,9] or [B,96,9], `sm` in the case's form, and the tensors the recorders recognise"""

    def __init__(self, dev, batched, form, grad, n=B):
        self.dev = dev
        if batched:
            self.p = torch.stack([synthetic.gs_parameters(12, 8, seed=3 + b) for b in range(n)]).to(dev).requires_grad_(grad)
            self.sm = _sm_batch(form, dev, n)
        else:
            self.p = synthetic.gs_parameters(12, 8, seed=3).to(dev).requires_grad_(grad)
            self.sm = _sm_single(form, dev)
        self.own = [("gs_parameters", self.p)]
        if torch.is_tensor(self.sm):
            self.own.append(("scale_modify", self.sm))
        elif torch.is_tensor(self.sm[0]):
            self.own += [(f"scale_modify[{i}]", t) for i, t in enumerate(self.sm)]

    def target(self, *shape):
        g = torch.Generator().manual_seed(11)
        t = torch.rand(*shape, generator=g).to(self.dev)
        self.own.append(("target", t))
        return t

    def targets(self, shapes):
        g = torch.Generator().manual_seed(11)
        ts = [torch.rand(*s, generator=g).to(self.dev) for s in shapes]
        self.own += [(f"target[{i}]", t) for i, t in enumerate(ts)]
        return ts

    def points(self, *lead, floating=False, grad=False):
        g = torch.Generator().manual_seed(5)
        if floating:
            return (torch.rand(*lead, 2, generator=g) * 18.0).to(self.dev).requires_grad_(grad)
        return torch.randint(0, 20, (*lead, 2), generator=g).to(self.dev)


def _no_grad(fn):
    def run(c):
        with torch.no_grad():
            return fn(c)
    return run


step, query, view = gsp.generate_2D_gaussian_splatting_step, gsp.generate_2D_gaussian_splatting_query, gsp.generate_2D_gaussian_splatting_view
u8, loss_ = gsp.generate_2D_gaussian_splatting_step_uint8, gsp.generate_2D_gaussian_splatting_loss
batch, batch_loss = gsp.generate_2D_gaussian_splatting_batch, gsp.generate_2D_gaussian_splatting_batch_loss
SC3 = [2.0] * B
WSHAPES = [(3, w[2], w[3]) for w in WINS]

SINGLE_ROWS = {
    "step": lambda c: step(G1, c.p, 2.0, c.sm),
    "step_points_tensor": lambda c: step(G1, c.p, 2.0, c.sm, sample_coords=c.points(S)),
    "step_points_list": lambda c: step(G1, c.p, 2.0, c.sm, sample_coords=c.points(S).tolist()),
    "step_no_dmax": lambda c: step(G1, c.p, 2.0, c.sm, if_dmax=False),
    "step_dynamic": lambda c: step(G1, c.p, 2.0, c.sm, dmax_mode='dynamic'),
    "step_mode_scale": lambda c: step(G1, c.p, 2.0, c.sm, mode='scale'),
    "query": lambda c: query(G1, c.p, 2.0, c.sm, c.points(S, floating=True)),
    "query_coords_grad": lambda c: query(G1, c.p, 2.0, c.sm, c.points(S, floating=True, grad=True), coords_grad=True),
    "query_empty": lambda c: query(G1, c.p, 2.0, c.sm, c.points(0, floating=True)),
    "u8": lambda c: u8(G1, c.p, 2.0, c.sm),
    "u8_crop": lambda c: u8(G1, c.p, 2.0, c.sm, crop=(20, 16)),
    "u8_bgr": lambda c: u8(G1, c.p, 2.0, c.sm, bgr=True),
    "u8_window": lambda c: u8(G1, c.p, 2.0, c.sm, window=WIN),
    "view": lambda c: view(G1, c.p, 2.0, c.sm, WIN),
    "loss_l1": lambda c: loss_(G1, c.p, 2.0, c.sm, c.target(3, *G1)),
    "loss_mse": lambda c: loss_(G1, c.p, 2.0, c.sm, c.target(3, *G1), loss='mse'),
    "loss_charbonnier": lambda c: loss_(G1, c.p, 2.0, c.sm, c.target(3, *G1), loss='charbonnier', reduction='sum'),
    "loss_window": lambda c: loss_(G1, c.p, 2.0, c.sm, c.target(3, 16, 12), window=WIN),
    "loss_ssim": lambda c: loss_(G1, c.p, 2.0, c.sm, c.target(3, *G1), ssim_weight=0.5),
    "loss_ssim_image_terms": lambda c: loss_(G1, c.p, 2.0, c.sm, c.target(3, *G1), ssim_weight=0.5, return_image=True, return_terms=True),
    "loss_image": lambda c: loss_(G1, c.p, 2.0, c.sm, c.target(3, *G1), return_image=True),
    "loss_terms": lambda c: loss_(G1, c.p, 2.0, c.sm, c.target(3, *G1), return_terms=True),
    "loss_no_grad": _no_grad(lambda c: loss_(G1, c.p, 2.0, c.sm, c.target(3, *G1))),
}
BATCH_ROWS = {
    "batch": lambda c: batch(SIZES, c.p, SC3, c.sm),
    "batch_sizes_tensor": lambda c: batch(torch.tensor(SIZES, device=c.dev), c.p, SC3, c.sm),
    "batch_points": lambda c: batch(SIZES, c.p, SC3, c.sm, sample_coords=c.points(B, S)),
    "batch_query": lambda c: batch(SIZES, c.p, SC3, c.sm, query_coords=c.points(B, S, floating=True)),
    "batch_windows": lambda c: batch(SIZES, c.p, SC3, c.sm, windows=WINS),
    "batch_dynamic_per_sample": lambda c: batch(SIZES, c.p, SC3, c.sm, dmax_mode='dynamic'),
    "batch_mode_scale": lambda c: batch(SIZES, c.p, SC3, c.sm, mode='scale'),
    "batch_loss_tensor": lambda c: batch_loss(SIZES, c.p, SC3, c.sm, c.target(B, 3, 24, 28)),
    "batch_loss_list": lambda c: batch_loss(SIZES, c.p, SC3, c.sm, c.targets([(3, h, w) for h, w in SIZES])),
    "batch_loss_windows": lambda c: batch_loss(SIZES, c.p, SC3, c.sm, c.target(B, 3, 16, 16), windows=WINS),
    "batch_loss_per_sample": lambda c: batch_loss(SIZES, c.p, SC3, c.sm, c.target(B, 3, 24, 28), dmax_mode='dynamic'),
    "batch_loss_ssim_all": lambda c: batch_loss(SIZES, c.p, SC3, c.sm, c.target(B, 3, 24, 28), ssim_weight=0.5, return_per_sample=True,
                                                return_images=True, return_terms=True),
    "batch_loss_images_terms": lambda c: batch_loss(SIZES, c.p, SC3, c.sm, c.target(B, 3, 24, 28), return_images=True, return_terms=True),
}
ONE_ROWS = {       # B = 1: the per-sample path of the batch functions
    "batch_of_one": lambda c: batch(SIZES[:1], c.p, SC3[:1], c.sm),
    "batch_loss_of_one": lambda c: batch_loss(SIZES[:1], c.p, SC3[:1], c.sm, c.target(1, 3, 24, 20)),
}


def _cases():
    """id -> (rows, row, form, requires_grad, BACKWARD_KERNEL, C++ node present, autocast)"""
    out = {}
    for rows, forms, kind in ((SINGLE_ROWS, SINGLE_FORMS, "single"), (BATCH_ROWS, BATCH_FORMS, "batch"), (ONE_ROWS, BATCH_FORMS, "one")):
        for row in rows:
            for form in forms:                                      # every form of scale_modify, everything else at its default
                out[f"{row}-{form}"] = (kind, row, form, True, "auto", True, False)
            f0 = forms[0]
            out[f"{row}-{f0}-nograd"] = (kind, row, f0, False, "auto", True, False)
            for k in ("tile", "home"):
                out[f"{row}-{f0}-{k}"] = (kind, row, f0, True, k, True, False)
            for k in ("auto", "tile", "home"):                      # the Python node: the same flags as the C++ node's rows above
                out[f"{row}-{f0}-{k}-pynode"] = (kind, row, f0, True, k, False, False)
            out[f"{row}-numbers-auto-pynode"] = (kind, row, "numbers", True, "auto", False, False)
    out["step-t2-autocast"] = ("single", "step", "t2", True, "auto", True, True)
    out["step-numbers-autocast-pynode"] = ("single", "step", "numbers", True, "auto", False, True)
    out["batch-B2-autocast"] = ("batch", "batch", "B2", True, "auto", True, True)
    out["batch-numbers-autocast-pynode"] = ("batch", "batch", "numbers", True, "auto", False, True)
    return out


CASES = _cases()
ROWS = {"single": SINGLE_ROWS, "batch": BATCH_ROWS, "one": ONE_ROWS}


def _returned(out):
    if torch.is_tensor(out):
        return [str(out.dtype), list(out.shape), list(out.stride()), out.device.type, bool(out.requires_grad)]
    return ["tuple"] + [_returned(o) for o in out]


def run_case(case, dev):
    kind, row, form, grad, kernel, node, autocast = CASES[case]
    if node:
        assert _cpp_node.load() is not None, "the C++ autograd node is built by build()"
    c = _Ctx(dev, kind != "single", form, grad, 1 if kind == "one" else B)
    log, old = [], gsp.BACKWARD_KERNEL
    gsp.BACKWARD_KERNEL = kernel
    try:
        with _recording(log, c.own, node), torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            out = ROWS[kind][row](c)
    finally:
        gsp.BACKWARD_KERNEL = old
    log.append(["return", _returned(out)])
    return log


@pytest.fixture(scope="module")
def table():
    with gzip.open(TABLE, "rb") as f:
        text = f.read()
    assert _blob(text) == BLOB, "tests/golden/host_routing.json.gz is not the recorded table"
    return json.loads(text)


def test_the_table_holds_exactly_the_matrix(table):
    assert sorted(table) == sorted(CASES)


@pytest.mark.parametrize("case", sorted(CASES))
def test_host_routing(case, table, dev):
    got = run_case(case, dev)
    want = table[case]
    # (compared as JSON text: 1 and 1.0 and true stay apart)
    got_s, want_s = [json.dumps(e, sort_keys=True) for e in got], [json.dumps(e, sort_keys=True) for e in want]
    for k, (g, w) in enumerate(zip(got_s, want_s)):
        assert g == w, f"{case}: call {k} differs\n  got      {g}\n  recorded {w}"
    assert len(got_s) == len(want_s), f"{case}: {[e[0] for e in got]} against the recorded {[e[0] for e in want]}"
    gsp.deferred_asserts.flush()


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: python tests/test_host_routing_gpu.py --write   (on the GPU; rewrites tests/golden/host_routing.json.gz)")
    device = torch.device("cuda:0")
    rows = []
    for name in sorted(CASES):
        rows.append(f" {json.dumps(name)}: {json.dumps(run_case(name, device), sort_keys=True, separators=(',', ':'))}")
        gsp.deferred_asserts.flush()
    text = ("{\n" + ",\n".join(rows) + "\n}\n").encode()
    with open(TABLE, "wb") as raw, gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as f:
        f.write(text)
    print(f"{len(rows)} cases -> {TABLE}; BLOB = {_blob(text)}")
