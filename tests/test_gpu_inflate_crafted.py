"""bgzf_inflate_kernel against zlib's verdict on DEFLATE members zlib's own encoder never writes (tests/deflate_corpus.py, made bit
by bit with tests/deflate_writer.py; tests/test_deflate_writer.py holds the corpus to its claims on any CPU): length and distance
codes longer than the tables' index bits with maximal extra bits (48-bit tokens in a row), legal header shapes no zlib stream
has, empty blocks, stored blocks at every bit phase, matches placed against the ring's 512-byte units for the very output
address the member lands on, the device deflater's own dialect, and structured invalid streams.  The rule for every member,
with the trailer's CRC checked:
  * status 0  =>  zlib accepts the member and the bytes are identical — no exceptions;
  * zlib accepts  =>  status 0 and identical bytes — except the enumerated members below, which the kernel reports by design;
  * nothing outside the members' own output ranges is written (inflate_on_device's canary), neighbours of an invalid member
    are untouched."""
import struct
import zlib

import numpy as np
import pytest

from tests import bam_spec
from tests import deflate_corpus as dc
from tests import deflate_writer as dw
from tests.cli_util import bgzf_member, write_bam
from tests.test_gpu_inflate import inflate_on_device

pytestmark = pytest.mark.gpu

# zlib accepts these and the kernel reports them (the caller's zlib then inflates them): a literal/length alphabet that is
# incomplete with a single code.  inf_build (seqkit_amd/csrc/sk_inflate.hip) returns 3 at
#     if (!(WHICH == 1 && (total == 0u || (total == 1u && cnt[1] == 1u)))) return 3u;
# — only a DISTANCE alphabet may be empty or a lone 1-bit code — where zlib's inflate_table lets any alphabet but the code-length
# one be a lone 1-bit code (max == 1).  Such a block can hold nothing but its end-of-block code; no BGZF writer makes one.
DEVICE_REPORTS_BY_DESIGN = ("by design: lone 1-bit end-of-block code, empty member",
                            "by design: lone 1-bit end-of-block code, behind a fixed block of data",
                            "by design: lone 1-bit end-of-block code, behind a stored block of data")


def crc_of(c):
    return zlib.crc32(c.out) & 0xFFFFFFFF


def hold_to_zlib(cases, status, outs, where, exceptions=DEVICE_REPORTS_BY_DESIGN):
    """the two-way rule; returns how many members zlib accepts"""
    accepted = 0
    for c, st, got in zip(cases, status, outs):
        ok, want = dc.zlib_verdict(c.payload, len(c.out), crc_of(c))
        assert ok == c.valid, f"{c.name}: the corpus's claim and zlib's verdict differ"
        if st == 0:
            assert ok, f"{c.name} ({where}): status 0 for a member zlib does not accept"
            assert got == want, f"{c.name} ({where}): status 0 and other bytes than zlib's"
        if ok:
            accepted += 1
            if c.name in exceptions:
                assert st != 0, f"{c.name} ({where}): listed as reported by design, but the kernel inflates it: the list is stale"
            else:
                assert st == 0, f"{c.name} ({where}): zlib accepts it, status {int(st):#x}"
                assert got == want == c.out, f"{c.name} ({where}): inflated bytes differ"
    return accepted


def place(cases, off, rng):
    """out_gaps that put every member's first output byte at `off` modulo the ring unit; input gaps 0-8"""
    out_gaps, at = [], 0
    for c in cases:
        g = (off - at) % dc.UNIT
        out_gaps.append(g)
        at += g + len(c.out)
    return [int(g) for g in rng.integers(0, 9, len(cases))], out_gaps


@pytest.mark.parametrize("off", dc.DEVICE_OFFSETS)
def test_valid_corpus_inflates_to_zlibs_bytes_at_every_placement(ctx, off):
    """every zlib-valid member — the named ones, the geometry cases built for this very output address, the random part — at a first
    output address of `off` modulo 512 and every alignment of its input"""
    rng = np.random.default_rng(100 + off)
    cases = dc.corpus_valid(off)
    gaps, out_gaps = place(cases, off, rng)
    print(f"launch: {len(cases)} valid members at output address {off} mod {dc.UNIT}", flush=True)
    status, outs = inflate_on_device(ctx, [c.payload for c in cases], [c.out for c in cases], gaps, out_gaps, crcs=[crc_of(c) for c in cases])
    n = hold_to_zlib(cases, status, outs, f"offset {off}")
    assert n == len(cases)
    # the random part draws no member of the excepted class: none of it is left out
    assert all(st == 0 for c, st in zip(cases, status) if c.name.startswith("random ")) and sum(1 for c in cases if c.name.startswith("random ")) == dc.RANDOM_MEMBERS
    assert sum(1 for st in status if st != 0) == len(DEVICE_REPORTS_BY_DESIGN)


@pytest.mark.parametrize("off", (0, 511, 259))
def test_invalid_corpus_is_reported_and_neighbours_stay_intact(ctx, off):
    """valid and invalid members interleaved in one launch: every invalid one has a status (zlib then decides), every valid one is
    inflated as if alone"""
    rng = np.random.default_rng(200 + off)
    bad = dc.corpus_invalid()
    good = [c for c in dc.corpus_valid(off, random_part=False) if c.name not in DEVICE_REPORTS_BY_DESIGN]
    cases = []
    for i, c in enumerate(bad):
        cases += [good[(7 * i) % len(good)], c]
    cases.append(good[-1])
    gaps, out_gaps = place(cases, off, rng)
    print(f"launch: {len(bad)} invalid members between valid ones at output address {off} mod {dc.UNIT}:", "; ".join(c.name for c in bad), flush=True)
    status, outs = inflate_on_device(ctx, [c.payload for c in cases], [c.out for c in cases], gaps, out_gaps, crcs=[crc_of(c) for c in cases])
    n = hold_to_zlib(cases, status, outs, f"offset {off}")
    assert n == len(bad) + 1
    assert all(st != 0 for c, st in zip(cases, status) if not c.valid)


def bgzf_members(data: bytes):
    """(compressed payload, crc32, isize) of every member, by the framing bam_spec.bgzf_blocks reads (SAMv1 §4.1)"""
    at = 0
    while at < len(data):
        assert data[at:at + 4] == b"\x1f\x8b\x08\x04"
        (xlen,) = struct.unpack_from("<H", data, at + 10)
        extra = data[at + 12:at + 12 + xlen]
        assert extra[:4] == b"BC\x02\x00" and xlen == 6
        total = struct.unpack_from("<H", extra, 4)[0] + 1
        crc, isize = struct.unpack_from("<II", data, at + total - 8)
        yield data[at + 12 + xlen:at + total - 8], crc, isize
        at += total


def test_device_deflater_members_inflate_on_the_device(ctx):
    """sk_bgzf_deflate's members are a dialect of their own (every code length explicit, HCLEN 15) that only zlib has read so far:
    the device inflater reads them too — status 0, the input's bytes, the trailer's CRC"""
    from tests.test_gpu_deflate import corpus as deflate_corpus
    rng = np.random.default_rng(31)
    inputs = [(name, data, 0xff00) for name, data in deflate_corpus()]
    noise = rng.integers(0, 6, 70000, dtype=np.uint8).tobytes()
    inputs += [(f"blocks of {b} bytes", noise[:20 * b] if b < 100 else noise[:40000], b) for b in (77, 1000, 4097)]
    payloads, raws, crcs = [], [], []
    for name, data, block in inputs:
        comp = ctx.bgzf_deflate(data, block)
        assert b"".join(bam_spec.bgzf_blocks(comp)) == data, name
        at = 0
        for payload, crc, isize in bgzf_members(comp):
            payloads.append(payload); raws.append(data[at:at + isize]); crcs.append(crc)
            at += isize
        assert at == len(data), name
    assert len(payloads) >= 90
    for off in (0, 511):
        out_gaps, at = [], 0
        for r in raws:
            out_gaps.append((off - at) % dc.UNIT if len(out_gaps) % 3 == 0 else 0)
            at += out_gaps[-1] + len(r)
        status, outs = inflate_on_device(ctx, payloads, raws, [int(g) for g in rng.integers(0, 9, len(raws))], out_gaps, crcs=crcs)
        assert (status == 0).all(), [(i, hex(int(s))) for i, s in enumerate(status) if s][:10]
        assert all(o == r for o, r in zip(outs, raws))


def crafted_bam(path, rng, spoil=None):
    """a BAM in write_bam's framing whose blocks' payloads are this writer's, in rotating dialects; returns the names of the members
    zlib is expected to be asked for.  spoil: the member whose payload loses its last byte."""
    refs = [("chr1", 100000), ("chr2", 50000)]
    records = [dict(tid=int(rng.integers(0, 2)), pos=i, flag=int(rng.choice([99, 147, 83, 163, 1123, 4, 355, 2147, 65, 129])), mtid=int(rng.integers(0, 2)), mpos=i + 3,
                    tlen=int(rng.integers(-6000, 6000)), name="r%d" % i, seq_len=int(rng.integers(1, 60))) for i in range(900)]
    plain = str(path) + ".plain"
    write_bam(plain, refs, records)
    with open(plain, "rb") as f:
        raw = b"".join(bam_spec.bgzf_blocks(f.read()))
    lone = dw.single_lengths(257, 256)
    members, host = [], []
    at, i = 0, 0
    while at < len(raw):
        data = raw[at:at + int(rng.integers(2000, 6000))]
        at += len(data)
        a, b = len(data) // 3, 2 * len(data) // 3
        kind = i % 7
        if kind == 0:
            blocks = [dw.make_dynamic(dw.greedy_tokens(data), lit="deep", dist="deep")]
        elif kind == 1:
            blocks = [dw.make_dynamic(dw.greedy_tokens(data), rle="none", hlit=286, hdist=30, hclen=19)]
        elif kind == 2:
            blocks = [dw.Fixed(dw.greedy_tokens(data[:a])), dw.make_dynamic(dw.greedy_tokens(data[a:b], data[:a]), lit="flat", dist="flat"), dw.Fixed(dw.greedy_tokens(data[b:], data[:b]))]
        elif kind == 3:
            blocks = [dw.Fixed(dw.greedy_tokens(data[:a])), dw.Stored(data[a:b]), dw.make_dynamic(dw.greedy_tokens(data[b:], data[:b]))]
        elif kind in (4, 6) and len(host) < 2:
            blocks = [dw.Fixed(dw.greedy_tokens(data), final=0), dw.Dynamic([], lone, [0])]      # reported by design
            host.append(i)
        else:
            blocks = [dw.make_dynamic(dw.greedy_tokens(data), cl_lens=dw.flat_lengths(19, range(19)))]
        payload, _ = dw.write_member(blocks)
        assert dw.expected_output(blocks) == data
        if spoil == i:
            payload = payload[:-1]
        members.append(bgzf_member(payload, data))
        i += 1
    with open(path, "wb") as f:
        f.write(b"".join(members) + bgzf_member(b"\x03\x00", b""))
    return host, i


def test_bam_file_of_crafted_members(ctx, tmp_path):
    """the whole-file entry point on a BAM whose blocks are this writer's dialects: handled, the results the specification's reader
    gets, and exactly the two members of the reported-by-design class went to the host's zlib; with one member's payload made
    invalid the file is left to the caller's reader, because zlib refuses that member too"""
    path = str(tmp_path / "crafted.bam")
    host, n_members = crafted_bam(path, np.random.default_rng(41))
    assert len(host) == 2 and n_members >= 8
    _, recs = bam_spec.read_bam(path)                              # (zlib reads every member: asserted inside)
    assert len(recs) == 900
    e_stats, e_hist = bam_spec.statistics(recs), bam_spec.fragment_lengths(recs, 5000)
    handled, counters, hist, total, info = ctx.bam_file_reduce(path, 5000)
    assert handled, info
    assert tuple(int(x) for x in counters) == tuple(e_stats)
    assert [int(x) for x in hist] == e_hist[0] and total == e_hist[1]
    assert info[3] == len(recs) and info[4] == len(host) == 2
    bad = str(tmp_path / "spoiled.bam")
    crafted_bam(bad, np.random.default_rng(41), spoil=3)
    handled, counters, _, _, info = ctx.bam_file_reduce(bad, 5000)
    assert not handled and info[5] == -16 and not counters.any()
