"""tests/dev_guard.py on a ctx made of a bytearray: every guard position it has to see, it sees, at the offset it says."""
import re

import numpy as np
import pytest

from tests.dev_guard import GAP, Guarded, default_trail, pattern


class StubCtx:
    """`Device memory` in a bytearray; addresses start at a 256-byte aligned base, like hipMalloc's."""
    BASE = 0x7000_0000

    def __init__(self):
        self.mem = bytearray()
        self.live = {}

    def malloc_device(self, nbytes):
        at = (len(self.mem) + 255) // 256 * 256
        self.mem.extend(bytes(at - len(self.mem) + nbytes))
        self.live[self.BASE + at] = nbytes
        return self.BASE + at

    def free_device(self, p):
        del self.live[p]

    def copy_h2d(self, dst, src):
        b = np.ascontiguousarray(src).reshape(-1).view(np.uint8).tobytes()
        self.mem[dst - self.BASE:dst - self.BASE + len(b)] = b

    def copy_d2h(self, dst, src):
        dst.reshape(-1).view(np.uint8)[:] = np.frombuffer(bytes(self.mem[src - self.BASE:src - self.BASE + dst.nbytes]), dtype=np.uint8)

    def sync(self):
        pass

    def poke(self, addr, delta=1):
        self.mem[addr - self.BASE] = (self.mem[addr - self.BASE] + delta) & 0xFF


def test_pattern_has_none_of_the_values_a_kernel_stores():
    p = pattern(4096, seed=11)
    assert p.min() >= 0x81 and p.max() <= 0xFD
    for v in (0x00, 0xFF, 0xFE, *b"ACGTUNacgtun!#I+\n"):
        assert v not in p
    assert np.all(p[1:] != p[:-1])                                     # position dependent: a shifted copy is seen too
    assert np.array_equal(p, 0x81 + ((np.arange(4096) * 7 + 11) % 0x7D))
    assert not np.array_equal(pattern(256, 1), pattern(256, 2))


def test_default_trail_is_a_tile_and_a_chunk():
    assert default_trail(0) == 4096 and default_trail(150) == 64 * 150 + 1024 and default_trail(151) % 16 == 0
    assert default_trail(151) >= 64 * 151 + 1024


def test_layout_sizes_alignment_and_payload():
    c = StubCtx()
    with Guarded(c) as g:
        data = np.arange(100, dtype=np.uint16)
        p = g.put(data, align=4, skew=4, lead=256, trail=512)
        assert (p - c.BASE) % 256 == 4 and list(c.live.values()) == [256 + 4 + 200 + 512]
        lead, pay, trail = g.fetch(p)
        assert lead.size == 260 and trail.size == 512 and np.array_equal(pay.view(np.uint16), data)
        assert np.array_equal(g.payload(p, np.uint16), data)
        q = g.put(37)                                                  # a size alone: the payload is pattern as well
        lead, pay, trail = g.fetch(q)
        assert (lead.size, pay.size, trail.size) == (256, 37, 4096) and pay.min() >= 0x81
        g.assert_all(outputs=[p, q], inputs=[p, q])
        with pytest.raises(AssertionError):
            g.put(8, align=16, skew=4)                                 # a pointer short of what the caller said it asks for
    assert c.live == {}


@pytest.mark.parametrize("where", ["lead first", "lead last", "trail first", "trail last"])
def test_a_changed_guard_byte_is_reported_with_its_offset(where):
    c = StubCtx()
    with Guarded(c) as g:
        nb, lead, skew, trail = 1000, 256, 16, 4096
        p = g.put(np.zeros(nb, dtype=np.uint8), skew=skew, lead=lead, trail=trail)
        off = {"lead first": -(lead + skew), "lead last": -1, "trail first": nb, "trail last": nb + trail - 1}[where]
        c.poke(p + off)
        at = re.escape(f"payload{off:+d}")
        with pytest.raises(AssertionError, match=rf"1 byte\(s\) changed .* first at {at} .* last at {at}$"):
            g.assert_guards(p)
        with pytest.raises(AssertionError, match=rf"first at {at} "):
            g.assert_unchanged(p)


def test_first_last_and_count_of_several_changed_bytes():
    c = StubCtx()
    with Guarded(c) as g:
        p = g.put(64, trail=128)
        for off in (-3, 64, 70, 191):
            c.poke(p + off)
        c.poke(p + 5)                                                  # inside an OUTPUT's payload: not the guards' business
        with pytest.raises(AssertionError, match=r"4 byte\(s\) changed .* first at payload-3 .* last at payload\+191$"):
            g.assert_guards(p)
        with pytest.raises(AssertionError, match=r"5 byte\(s\) changed"):
            g.assert_unchanged(p)


def test_a_changed_payload_byte_of_an_input_is_reported():
    c = StubCtx()
    with Guarded(c) as g:
        p = g.put(np.full((7, 150), ord("A"), dtype=np.uint8))
        g.assert_unchanged(p)
        for off in (0, 7 * 150 - 1):
            c.poke(p + off)
            g.assert_guards(p)                                         # (the guards are intact)
            with pytest.raises(AssertionError, match=rf"input: 1 byte\(s\) changed .* first at payload\+{off} \(0x41 -> 0x42\), last at payload\+{off}$"):
                g.assert_unchanged(p)
            c.poke(p + off, -1)
        g.assert_unchanged(p)


def test_a_store_of_the_pattern_of_another_position_is_seen():
    c = StubCtx()
    with Guarded(c) as g:
        p = g.put(16, trail=64)
        c.mem[p + 16 - c.BASE] = c.mem[p + 17 - c.BASE]               # the neighbour's guard value, one byte early
        with pytest.raises(AssertionError, match=r"first at payload\+16 "):
            g.assert_guards(p)


def test_carved_payloads_keep_their_alignment_and_their_gaps_are_guards():
    c = StubCtx()
    with Guarded(c) as g:
        sizes = [4 * 1, 4 * 64, 4 * 257, 4 * 1000, 4 * 3]
        ptrs = g.carve([np.full(s // 4, -7, dtype=np.int32) for s in sizes], align=16, skew=16, trail=256)
        assert len(c.live) == 1
        for a, b, s in zip(ptrs, ptrs[1:], sizes):
            assert b % 16 == 0 and GAP <= b - (a + s) < GAP + 16
        g.assert_guards(ptrs[0])
        lead, pay, trail = g.fetch(ptrs[2])
        assert lead.size == ptrs[2] - (ptrs[1] + sizes[1]) and trail.size == ptrs[3] - (ptrs[2] + sizes[2])
        assert np.all(pay.view(np.int32) == -7)
        c.poke(ptrs[1] + sizes[1])                                     # batch 1 runs one byte into the gap before batch 2
        with pytest.raises(AssertionError, match=rf"first at payload\+{sizes[1]} "):
            g.assert_guards(ptrs[1])
        with pytest.raises(AssertionError, match=rf"first at payload-{ptrs[2] - ptrs[1] - sizes[1]} "):
            g.assert_guards(ptrs[2])                                   # the same byte, counted from its other neighbour
        c.poke(ptrs[1] + sizes[1], -1)
        c.poke(ptrs[4] + sizes[4] + 255)                               # the allocation's last byte
        with pytest.raises(AssertionError, match=rf"last at payload\+{sizes[4] + 255}$"):
            g.assert_guards(ptrs[4])
