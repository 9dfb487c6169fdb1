"""What the window attention's entry points say to a bad descriptor, for all four families (gsasr_window_attn, _rope, _bf16,
_rope_bf16) and all three entry points of each: the return code and the exact bytes of gsasr_last_error().  One host path serves
the twelve symbols (csrc/splat_attn.hip: AttnFamily, attn_check, attn_forward, attn_backward); this table is what a change to
it could silently move.  Every call here fails before any launch: no GPU is touched, and the pointers are plain numbers."""
import ctypes
import math

import pytest

from gsasr_amd import _cabi

ERR_ARG = -1
W, H, NQ, NK, D, ROWS = 2, 3, 20, 36, 8, 97        # a valid geometry (rotary: ROWS angle rows >= max(nq, nk))
BASE = 0x10000                                      # pointers: distinct multiples of 256, never dereferenced

FAMILIES = {
    "biased": ("gsasr_window_attn", False, False),
    "biased_bf16": ("gsasr_window_attn_bf16", False, True),
    "rope": ("gsasr_window_attn_rope", True, False),
    "rope_bf16": ("gsasr_window_attn_rope_bf16", True, True),
}
POINTERS = {False: ("q", "k", "v", "table", "index", "out", "stats", "grad_out", "g_q", "g_k", "g_v", "g_table", "scratch"),
            True: ("q", "k", "v", "angles", "out", "stats", "grad_out", "g_q", "g_k", "g_v", "g_angles", "cossin", "scratch")}

M_WH = b"windows and heads must be at least 1"
M_N = b"need 1 <= nq, nk <= 256"
M_FLAGS = b"unknown flags (none are defined)"
M_NAN = b"scale is NaN"
M_NULL = {False: b"null window-attention descriptor", True: b"null rotary window-attention descriptor"}
M_D = {False: b"need 1 <= head_dim <= 32", True: b"need an even head_dim, 2 <= head_dim <= 32"}
M_ROWS = {False: b"table_rows must be at least 1", True: b"angle_rows must be at least max(nq, nk)"}
M_BIG = {False: b"windows * heads or table_rows * heads exceeds 2^31 - 1",
         True: b"windows * heads or heads * angle_rows * head_dim / 2 exceeds 2^31 - 1"}
M_MISSING = {(False, "forward"): b"null q, k, v, table, index or out pointer",
             (False, "backward"): b"null q, k, v, table, index, out, stats or grad_out pointer",
             (True, "forward"): b"null q, k, v, angles, out or cossin pointer",
             (True, "backward"): b"null q, k, v, out, stats, grad_out or cossin pointer"}
REQUIRED = {(False, "forward"): ("q", "k", "v", "table", "index", "out"),
            (False, "backward"): ("q", "k", "v", "table", "index", "out", "stats", "grad_out"),
            (True, "forward"): ("q", "k", "v", "angles", "out", "cossin"),
            (True, "backward"): ("q", "k", "v", "out", "stats", "grad_out", "cossin")}
# (rope, bf16, entry point) -> (the pointers with an alignment rule as {name: an offset that breaks it}, the message); fp32 biased has no rule
ACT8 = ("q", "k", "v", "out", "grad_out", "g_q", "g_k", "g_v")
M_ALIGN = {
    (False, True, "forward"): ({p: 1 for p in ACT8[:4]}, b"q, k, v and out must be 2-byte aligned"),
    (False, True, "backward"): ({p: 1 for p in ACT8}, b"q, k, v, out, grad_out, g_q, g_k and g_v must be 2-byte aligned"),
    (True, False, "forward"): ({"q": 4, "k": 4, "cossin": 4}, b"q, k and cossin must be 8-byte aligned"),
    (True, False, "backward"): ({"q": 4, "k": 4, "cossin": 4, "g_q": 4, "g_k": 4}, b"q, k, cossin, g_q and g_k must be 8-byte aligned"),
    (True, True, "forward"): ({**{p: 2 for p in ACT8[:4]}, "cossin": 4}, b"q, k, v and out must be 4-byte aligned and cossin 8-byte aligned"),
    (True, True, "backward"): ({**{p: 2 for p in ACT8}, "cossin": 4},
                               b"q, k, v, out, grad_out, g_q, g_k and g_v must be 4-byte aligned and cossin 8-byte aligned"),
}
M_SCRATCH = {False: b"null scratch pointer (the table gradient needs gsasr_window_attn_scratch_bytes)",
             True: b"null scratch pointer (the angle gradient needs gsasr_window_attn_rope_scratch_bytes)"}
M_SCRATCH_ALIGN = b"scratch must be 8-byte aligned"
M_ANGLES_NEED = b"g_angles needs g_q and g_k (it is formed from them)"


def make(rope, bf16, pointers=True, **sizes):
    s = dict(windows=W, heads=H, nq=NQ, nk=NK, head_dim=D, rows=ROWS, scale=D ** -0.5)
    s.update(sizes)
    mk = _cabi.make_window_attn_rope if rope else _cabi.make_window_attn
    d = mk(s["windows"], s["heads"], s["nq"], s["nk"], s["head_dim"], s["rows"], s["scale"], bf16=bf16)
    if pointers:
        for i, p in enumerate(POINTERS[rope]):
            setattr(d, p, BASE + 256 * i)
    return d


def size_defects(rope):
    """(name, the descriptor's changed sizes or a function that spoils it, the message): defects every entry point reports"""
    out = [("windows 0", dict(windows=0), M_WH), ("heads 0", dict(heads=0), M_WH),
           ("nq 0", dict(nq=0), M_N), ("nq 257", dict(nq=257, rows=300), M_N), ("nk 0", dict(nk=0), M_N), ("nk 257", dict(nk=257, rows=300), M_N),
           ("head_dim 0", dict(head_dim=0), M_D[rope]), ("head_dim past 32", dict(head_dim=34 if rope else 33), M_D[rope]),
           ("rows", dict(rows=NK - 1 if rope else 0), M_ROWS[rope]),
           ("flags", lambda d: setattr(d, "flags", 1), M_FLAGS), ("NaN scale", dict(scale=math.nan), M_NAN),
           ("windows * heads", dict(windows=65536, heads=32768), M_BIG[rope]),
           ("rows * heads", dict(rows=1 << 20, heads=(1 << 9) if rope else (1 << 11)), M_BIG[rope])]
    if rope:
        out += [("head_dim odd", dict(head_dim=7), M_D[rope]), ("head_dim 1", dict(head_dim=1), M_D[rope])]
    return out


def call(stem, what, d):
    """(return value, the message afterwards) of one entry point; `d` None: the null descriptor"""
    lib = _cabi.lib()
    ref = None if d is None else ctypes.byref(d)
    rc = getattr(lib, f"{stem}_{what}")(ref) if what == "scratch_bytes" else getattr(lib, f"{stem}_{what}")(ref, None)
    return rc, lib.gsasr_last_error()


def refused(stem, what, d, msg, case):
    rc, said = call(stem, what, d)
    assert rc == (0 if what == "scratch_bytes" else ERR_ARG), (case, what, rc)
    assert said == msg, (case, what, said)


@pytest.mark.parametrize("family", list(FAMILIES))
def test_sizes_flags_and_scale_are_refused_by_all_three_entry_points(family):
    stem, rope, bf16 = FAMILIES[family]
    for what in ("scratch_bytes", "forward", "backward"):
        refused(stem, what, None, M_NULL[rope], "null descriptor")
        for case, change, msg in size_defects(rope):
            d = make(rope, bf16, **(change if isinstance(change, dict) else {}))
            if not isinstance(change, dict):
                change(d)
            refused(stem, what, d, msg, case)


@pytest.mark.parametrize("family", list(FAMILIES))
def test_pointers_are_refused_in_turn(family):
    stem, rope, bf16 = FAMILIES[family]
    for what in ("forward", "backward"):
        for p in REQUIRED[rope, what]:
            d = make(rope, bf16)
            setattr(d, p, None)
            refused(stem, what, d, M_MISSING[rope, what], "no " + p)
            assert call(stem, "scratch_bytes", d)[0] > 0, p         # (looks at no pointer but the optional gradient's)
        if (rope, bf16, what) in M_ALIGN:
            offsets, msg = M_ALIGN[rope, bf16, what]
            for p, off in offsets.items():
                d = make(rope, bf16)
                setattr(d, p, getattr(d, p) + off)
                refused(stem, what, d, msg, "misaligned " + p)
        # a missing pointer is reported before a misaligned one
        if (rope, bf16, what) in M_ALIGN:
            d = make(rope, bf16)
            d.q, d.v = d.q + 1, None
            refused(stem, what, d, M_MISSING[rope, what], "missing before misaligned")


@pytest.mark.parametrize("family", list(FAMILIES))
def test_backward_wants_its_scratch(family):
    stem, rope, bf16 = FAMILIES[family]
    if rope:
        for p in ("g_q", "g_k"):
            d = make(rope, bf16)
            setattr(d, p, None)
            refused(stem, "backward", d, M_ANGLES_NEED, "g_angles without " + p)
        d = make(rope, bf16, windows=9)         # (two slices of windows: the partial sums need the scratch)
        d.scratch = None
        refused(stem, "backward", d, M_SCRATCH[rope], "angle gradient without scratch")
    else:
        for rows in (ROWS, 4096, 4097):
            d = make(rope, bf16, rows=rows)
            d.scratch = None
            refused(stem, "backward", d, M_SCRATCH[rope], f"table gradient without scratch, {rows} rows")
        d = make(rope, bf16, rows=4097)
        d.scratch += 4
        refused(stem, "backward", d, M_SCRATCH_ALIGN, "misaligned scratch above 4096 rows")


def _up(n):
    return (n + 255) // 256 * 256


@pytest.mark.parametrize("rope", [False, True])
def test_scratch_bytes_is_the_same_for_both_element_types(rope):
    """and is what include/gsasr_splat.h documents: 256 bytes, plus the partial table columns (one per window slot, at most 256,
    and head; above 4096 rows the table in double), or the angle gradient's partials (slices of at least 8 windows, at most 64)"""
    stems = [s for s, r, _ in FAMILIES.values() if r == rope]
    for windows in (1, 8, 9, 256, 600):
        for rows in (ROWS, 4096, 4097):
            for grad in (False, True):
                got = []
                for stem, bf16 in zip(stems, (False, True)):
                    d = make(rope, bf16, pointers=False, windows=windows, rows=rows)
                    setattr(d, "g_angles" if rope else "g_table", BASE if grad else None)
                    got.append(call(stem, "scratch_bytes", d)[0])
                if rope:
                    chunk = max(8, -(-windows // 64))
                    slices = -(-windows // chunk)
                    want = 256 + (_up(slices * H * rows * (D // 2) * 4) if grad and slices > 1 else 0)
                else:
                    want = 256 + (0 if not grad else _up(rows * H * 8) if rows > 4096 else _up(min(windows, 256) * H * rows * 4))
                assert got == [want, want], (windows, rows, grad, got, want)
