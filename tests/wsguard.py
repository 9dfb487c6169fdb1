"""Caller-supplied workspaces and scratch areas at exactly their declared size, between guards, on garbage.

Every entry point of the C ABI works in memory the caller hands over, sized by a `*_workspace_bytes` / `*_scratch_bytes` function.
`torch.empty(nbytes)` cannot show a disagreement between that size and what the kernels index: the caching allocator rounds up
to 512 bytes and carves from segments of megabytes, so a write past the end lands in padding or in a free block.  `GuardedBytes`
is one allocation `[G | n | G]`: the middle is what the library gets, with `workspace_bytes == n`; the guards must not change.

G = 64 KiB is a condition, not a measurement: wider than every 256-byte alignment pad of the layouts, and wide enough for an array
of a few hundred elements sized with the wrong element width (the shapes these tests use: a few hundred Gaussians of 32 bytes).

The three fills are what the memory holds on entry (guards and middle alike):
  "ff"      every byte 0xFF: NaN floats, counters and cursors of 4 * 10^9 -- tends to fail loudly;
  "zero"    every byte 0;
  "seeded"  bytes of numpy.random.default_rng(seed): finite floats of every magnitude, counters and cursors with plausible low
            bits -- what a pooled workspace holds, the previous step's data, and the kind that fails quietly.
"""
import numpy as np
import torch

G = 64 << 10
ALIGN = 256
FILLS = ("ff", "zero", "seeded")


def fill_bytes(fill, count, seed=0):
    """`count` bytes of fill `fill` as a uint8 numpy array"""
    if fill == "ff":
        return np.full(count, 0xFF, np.uint8)
    if fill == "zero":
        return np.zeros(count, np.uint8)
    if fill == "seeded":
        return np.random.default_rng(seed).integers(0, 256, count, dtype=np.uint8)
    raise ValueError(f"unknown fill {fill!r}")


class Changed:
    """what `GuardedBytes.intact()` returns: true when no guard byte changed; else `first` / `last`, the offsets of the first and
    the last changed byte relative to the start of the middle (negative: in front of it; >= n: behind it), and their `count`"""

    def __init__(self, first=None, last=None, count=0):
        self.first, self.last, self.count = first, last, count

    def __bool__(self):
        return self.count == 0

    def __repr__(self):
        return "intact" if self.count == 0 else f"{self.count} guard bytes changed, offsets {self.first} .. {self.last} of the middle"


class GuardedBytes:
    """`n` bytes on device `dev` with at least G bytes of guard on either side, all of it filled with `fill`.
    `.mid`: the uint8 view of the n bytes (starts on a 256-byte boundary) that is handed to the library."""

    def __init__(self, n, dev, fill, seed=0):
        n = int(n)
        assert n >= 0
        self.n, self.fill = n, fill
        self.buf = torch.empty(G + ALIGN + n + G, dtype=torch.uint8, device=dev)
        self.off = G + (-(self.buf.data_ptr() + G)) % ALIGN
        self.pattern = torch.from_numpy(fill_bytes(fill, self.buf.numel(), seed))     # (host copy of what everything held on entry)
        self.buf.copy_(self.pattern)
        self.mid = self.buf[self.off:self.off + n]
        assert self.mid.data_ptr() % ALIGN == 0 and self.mid.numel() == n
        assert self.off >= G and self.buf.numel() - (self.off + n) >= G

    def span(self, nbytes):
        """the view of `nbytes` bytes from the start of the middle, n <= nbytes <= n + G: what a test that wants the library to
        write into the guard (all of it this object's own memory) hands over instead of `.mid`"""
        assert self.n <= nbytes <= self.n + G
        return self.buf[self.off:self.off + int(nbytes)]

    def _host(self):
        return self.buf.cpu()

    def intact(self):
        """compare both guards with what they were filled with (synchronises)"""
        now = self._host()
        diff = now != self.pattern
        diff[self.off:self.off + self.n] = False
        idx = torch.nonzero(diff).flatten()
        if idx.numel() == 0:
            return Changed()
        return Changed(int(idx[0]) - self.off, int(idx[-1]) - self.off, int(idx.numel()))

    def check(self, what):
        c = self.intact()
        assert c, f"{what}: {c!r} (n = {self.n})"

    def mid_bytes(self):
        """the middle as a numpy array (a copy)"""
        return self.mid.cpu().numpy().copy()

    def written(self):
        """bool [n]: bytes of the middle that differ from the fill they started with"""
        return (self.mid.cpu() != self.pattern[self.off:self.off + self.n]).numpy()

    def highest_written(self, other):
        """`other`: the same call run on a buffer of the same size that started from ANOTHER fill.  The highest offset of the
        middle at which either run differs from its own fill (a byte a kernel wrote equals at most one of two different fills
        by accident), -1 if neither run changed anything.  `n - 1 - highest` is the slack at the end of the region that this
        case leaves unwritten: where an overrun by less than that could still hide."""
        assert other.n == self.n and other.fill != self.fill
        w = self.written() | other.written()
        idx = np.nonzero(w)[0]
        return int(idx[-1]) if idx.size else -1

    def restore(self):
        """put the fill back everywhere"""
        self.buf.copy_(self.pattern)
