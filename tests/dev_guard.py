"""Caller-owned device buffers with guard bytes on both sides, for the tests of the `_dev` entry points.

A `_dev` call writes into memory the caller allocated.  A store one element behind an output changes no value inside it, so a
comparison of the output alone cannot see it; what it hits is the caller's next allocation.  `Guarded` puts every buffer of a
call into an allocation of its own, of exactly the documented size and at a chosen alignment, between two runs of a
position-dependent byte pattern, and afterwards says which pattern bytes changed.

Nothing here needs a GPU: the ctx is anything with malloc_device / free_device / copy_h2d / copy_d2h / sync
(tests/test_dev_guard.py drives it with a bytearray)."""
from __future__ import annotations

import numpy as np

PATTERN_LO, PATTERN_SPAN = 0x81, 0x7D          # bytes 0x81 .. 0xFD: never 0x00, 0xFF, an ASCII base, 'N' or '!'
GAP = 64                                        # pattern bytes between two payloads carved from one allocation


def pattern(nbytes: int, seed: int = 0) -> np.ndarray:
    """Byte i is 0x81 + ((i * 7 + seed) % 0x7D): neighbours differ, the period (125) is no power of two, and no value a kernel
    of this library stores (ASCII text, small integers, 0x00, 0xFF, -1, -2) is in its range."""
    i = np.arange(nbytes, dtype=np.int64)
    return (PATTERN_LO + ((i * 7 + seed) % PATTERN_SPAN)).astype(np.uint8)


def _round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


def default_trail(row_pitch: int = 0) -> int:
    """A whole 64-row tile plus one 1 KiB chunk, at least 4 KiB: the widest overrun a kernel of this library could plausibly make."""
    return _round_up(max(4096, 64 * row_pitch + 1024), 16)


def _as_bytes(x) -> np.ndarray | None:
    if isinstance(x, (int, np.integer)):
        return None
    return np.ascontiguousarray(x).reshape(-1).view(np.uint8)


def _nbytes(x) -> int:
    return int(x) if isinstance(x, (int, np.integer)) else int(np.asarray(x).nbytes)


def _pitch(x) -> int:
    if isinstance(x, (int, np.integer)):
        return 0
    a = np.asarray(x)
    return int(a.shape[-1] * a.itemsize) if a.ndim >= 2 else 0


class _Alloc:
    def __init__(self, base: int, image: np.ndarray, regions):
        self.base = base
        self.image = image                      # what the allocation held when the call under test began
        self.regions = regions                  # [(offset, nbytes)] of the payloads, ascending
        self.is_guard = np.ones(image.size, dtype=bool)
        for off, nb in regions:
            self.is_guard[off:off + nb] = False


class Guarded:
    """Device buffers between guards.  put() / carve() allocate, fetch() reads back, assert_guards() / assert_unchanged() check,
    close() frees (also as a context manager)."""

    def __init__(self, ctx):
        self.ctx = ctx
        self._allocs: list[_Alloc] = []
        self._by_ptr: dict[int, tuple[_Alloc, int]] = {}
        self._seed = 0

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ---- allocation ---------------------------------------------------------------------------------------------
    def carve(self, items, align=16, skew=0, lead: int = 256, trail: int | None = None, gap: int = GAP) -> list[int]:
        """ONE allocation holding every item (an array, copied in, or a byte count, left as pattern) in order: `lead` pattern
        bytes, the first payload at base + lead + skew, at least `gap` pattern bytes between neighbours (more where the next
        payload has to move up to the next multiple of 16 + skew), `trail` pattern bytes behind the last.  align and skew may
        be lists, one entry per item (columns of different types in one allocation).  Returns the payloads' device pointers."""
        aligns = list(align) if isinstance(align, (list, tuple)) else [align] * len(items)
        skews = list(skew) if isinstance(skew, (list, tuple)) else [skew] * len(items)
        assert len(aligns) == len(skews) == len(items) and lead % 256 == 0
        for a_k, s_k in zip(aligns, skews):
            assert a_k >= 1 and 0 <= s_k < 256 and s_k % a_k == 0 and 256 % a_k == 0, (a_k, s_k)
        if trail is None:
            trail = default_trail(max([_pitch(x) for x in items] + [0]))
        regions = []
        at = lead + skews[0]
        for k, x in enumerate(items):
            if k:
                at = _round_up(at + gap - skews[k], max(aligns[k], 16)) + skews[k]
            regions.append((at, _nbytes(x)))
            at += _nbytes(x)
        total = at + trail
        self._seed += 37
        image = pattern(total, self._seed)
        for (off, nb), x in zip(regions, items):
            b = _as_bytes(x)
            if b is not None:
                image[off:off + nb] = b
        base = self.ctx.malloc_device(total)
        assert base % 256 == 0, f"device allocation at {base:#x} is not 256-byte aligned"
        a = _Alloc(base, image, regions)
        self._allocs.append(a)
        self.ctx.copy_h2d(base, image)
        self.ctx.sync()
        ptrs = [base + off for off, _ in regions]
        for k, p in enumerate(ptrs):
            self._by_ptr[p] = (a, k)
        return ptrs

    def put(self, data, align: int = 16, skew: int = 0, lead: int = 256, trail: int | None = None) -> int:
        """One allocation of lead + skew + nbytes + trail bytes, all pattern; the payload (if an array was given) copied to
        base + lead + skew, which is returned.  base is 256-byte aligned, so `skew` alone decides the pointer's alignment;
        `align` is what the entry point asks for and is checked against it."""
        return self.carve([data], align=align, skew=skew, lead=lead, trail=trail)[0]

    def close(self) -> None:
        self.ctx.sync()
        for a in self._allocs:
            self.ctx.free_device(a.base)
        self._allocs, self._by_ptr = [], {}

    # ---- read-back ----------------------------------------------------------------------------------------------
    def _now(self, a: _Alloc) -> np.ndarray:
        got = np.empty(a.image.size, dtype=np.uint8)
        self.ctx.copy_d2h(got, a.base)
        self.ctx.sync()
        return got

    def fetch(self, ptr: int):
        """(lead_guard, payload_bytes, trail_guard) of the payload at ptr: the guards reach to the neighbouring payloads, or to
        the allocation's ends."""
        a, k = self._by_ptr[ptr]
        got = self._now(a)
        off, nb = a.regions[k]
        lo = a.regions[k - 1][0] + a.regions[k - 1][1] if k else 0
        hi = a.regions[k + 1][0] if k + 1 < len(a.regions) else got.size
        return got[lo:off], got[off:off + nb], got[off + nb:hi]

    def payload(self, ptr: int, dtype=np.uint8) -> np.ndarray:
        return self.fetch(ptr)[1].copy().view(dtype)

    def _report(self, ptr: int, what: str, only_guards: bool) -> None:
        a, k = self._by_ptr[ptr]
        got = self._now(a)
        bad = got != a.image
        if only_guards:
            bad &= a.is_guard
        idx = np.flatnonzero(bad)
        if idx.size:
            off, nb = a.regions[k]
            first, last = int(idx[0]) - off, int(idx[-1]) - off
            raise AssertionError(f"{what}: {idx.size} byte(s) changed around a payload of {nb} bytes, first at payload{first:+d} "
                                 f"({a.image[idx[0]]:#04x} -> {got[idx[0]]:#04x}), last at payload{last:+d}")

    def assert_guards(self, ptr: int, what: str = "output") -> None:
        """Every pattern byte of ptr's allocation (lead, gaps, trail) is what it was; offsets in the message count from ptr's
        payload (negative: in front of it; >= its size: behind it)."""
        self._report(ptr, f"guards of {what}", True)

    def assert_unchanged(self, ptr: int, what: str = "input") -> None:
        """The same for an input: its payload must be untouched too."""
        self._report(ptr, what, False)

    def assert_all(self, outputs=(), inputs=()) -> None:
        for p in outputs:
            self.assert_guards(p)
        for p in inputs:
            self.assert_unchanged(p)
