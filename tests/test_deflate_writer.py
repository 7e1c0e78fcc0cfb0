"""The crafted DEFLATE corpus (tests/deflate_corpus.py, written by tests/deflate_writer.py) is what it claims, by zlib's word:
every member of corpus_valid() inflates to exactly the intended bytes, every member of corpus_invalid() is refused (zlib
raises, or does not reach the stream's end, or makes another length), and the structural claims — which decoder paths the
members reach — hold by the writer's own report of what it wrote.  No GPU: this is the half of the argument that the device
and host decoder tests (tests/test_gpu_inflate_crafted.py, tests/cpp/inflate_streams_test.cpp) rest on."""
import zlib

import pytest

from tests import deflate_corpus as dc
from tests import deflate_writer as dw


def by_name(cases, prefix):
    found = [c for c in cases if c.name.startswith(prefix)]
    assert found, f"no case named {prefix!r}"
    return found


def test_writer_primitives():
    # RFC 1951 §3.2.2's example: lengths (3, 3, 3, 3, 3, 2, 4, 4) -> codes 010 011 100 101 110 00 1110 1111
    assert dw.canonical_codes([3, 3, 3, 3, 3, 2, 4, 4]) == [0b010, 0b011, 0b100, 0b101, 0b110, 0b00, 0b1110, 0b1111]
    assert dw.deep_lengths(16, range(16)) == list(range(1, 15)) + [15, 15]
    for lens in (dw.deep_lengths(286, range(270)), dw.deep_lengths(30, range(30)), dw.flat_lengths(286, range(286)), dw.flat_lengths(19, range(19)),
                 dw.limited_lengths([1 << (i % 20) for i in range(286)], 15), dw.limited_lengths([1 << i for i in range(19)], 7),
                 dw.limited_lengths([0, 0, 5, 0], 15)):
        assert dw.kraft(lens) == 32768 and max(lens) <= 15
    assert max(dw.limited_lengths([1 << i for i in range(19)], 7)) == 7 and max(dw.deep_lengths(286, range(270))) == 15
    assert dw.kraft(dw.single_lengths(30, 4)) == 16384
    assert [dw.length_symbol(l) for l in (3, 10, 11, 257, 258)] == [(257, 0, 0), (264, 0, 0), (265, 1, 0), (284, 5, 30), (285, 0, 0)]
    assert [dw.dist_symbol(d) for d in (1, 4, 5, 32768)] == [(0, 0, 0), (3, 0, 0), (4, 1, 0), (29, 13, 8191)]
    sink = dw.BitSink()
    sink.bits(0b101, 3); sink.code(0b110, 3); sink.bits(0x3FF, 10)
    assert sink.bitpos == 16 and sink.getvalue() == bytes([0b11011101, 0xFF])
    data = b"abracadabra abracadabra abracadabra, said the writer's own tokenizer" * 9
    toks = dw.greedy_tokens(data)
    assert any(not isinstance(t, int) for t in toks)
    for blocks in ([dw.Fixed(toks)], [dw.make_dynamic(toks)], [dw.make_dynamic(toks, lit="deep", dist="flat", rle="none")], [dw.Stored(data)]):
        payload, rep = dw.write_member(blocks)
        assert zlib.decompress(payload, wbits=-15) == data == dw.expected_output(blocks) and rep.out_len == len(data)


def test_valid_corpus_is_valid_by_zlib():
    seen = set()
    for off in dc.DEVICE_OFFSETS:
        for c in dc.corpus_valid(off):
            if c.name in seen:
                continue
            seen.add(c.name)
            assert c.valid
            ok, got = dc.zlib_verdict(c.payload, len(c.out), zlib.crc32(c.out) & 0xFFFFFFFF)
            assert ok and got == c.out, c.name
            if c.report is not None:
                assert c.report.out_len == len(c.out), c.name
            assert len(c.out) <= 65536 and len(c.payload) < 2 * 65536, c.name
    assert sum(1 for n in seen if n.startswith("random ")) == dc.RANDOM_MEMBERS
    for name in dc.BY_DESIGN:
        assert name in seen


def test_invalid_corpus_is_invalid_by_zlib():
    cases = dc.corpus_invalid()
    assert len({c.name for c in cases}) == len(cases)
    for c in cases:
        assert not c.valid
        ok, _ = dc.zlib_verdict(c.payload, len(c.out), zlib.crc32(c.out) & 0xFFFFFFFF)
        assert not ok, c.name
    for name in dc.INVALID_NAMES:
        by_name(cases, name)
    assert len(by_name(cases, "distance op + 1")) >= 6
    # the named ones are invalid for the reason their name gives: the header's own figures
    K = 32768
    for name, alphabet, sign in (("over-subscribed literal/length code", 0, 1), ("over-subscribed distance code", 1, 1), ("over-subscribed code-length code", 2, 1),
                                 ("incomplete literal/length code", 0, -1), ("incomplete distance code", 1, -1), ("incomplete code-length code", 2, -1)):
        for c in by_name(cases, name):
            k = c.report.headers[0]["kraft"]
            assert (k[alphabet] - K) * sign > 0, (c.name, k)
            assert all(k[a] == K or (a == 1 and k[a] == 0) for a in range(3) if a != alphabet), (c.name, k)
    for name, field, value in (("HLIT 287", "hlit", 287), ("HLIT 288", "hlit", 288), ("HDIST 31", "hdist", 31), ("HDIST 32", "hdist", 32), ("HCLEN 4", "hclen", 4)):
        assert by_name(cases, name)[0].report.headers[0][field] == value
    for k in (1, 2, 3):
        c = by_name(cases, f"fixed block cut {k} byte")[0]
        whole, _ = dw.write_member([dw.Fixed(list(c.out))])
        assert c.report.kinds == ["fixed"] and len(c.payload) == len(whole) - k and whole.startswith(c.payload)
    # (the last byte of that block holds nothing but the end-of-block code's last two bits: cut, the zeros a decoder reads in their place decode)
    assert (3 + 8 * 40 + 7) % 8 == 2
    assert by_name(cases, "empty input, out_len 0")[0].payload == b"" and by_name(cases, "empty input, out_len 0")[0].out == b""


def test_valid_corpus_reaches_the_paths_it_names():
    cases = dc.corpus_valid(0, random_part=False)
    reports = [c.report for c in cases]
    # codes longer than the tables' index bits (device 10 / 8, host 11 / 8), in every role; second-level distance codes of 13 bits and more
    assert by_name(cases, "deep literal codes")[0].report.max_lit_code >= 12
    assert by_name(cases, "deep length codes")[0].report.max_len_code >= 12
    assert by_name(cases, "deep distance codes")[0].report.max_dist_code >= 13
    assert any(r.max_len_code >= 11 for r in reports) and any(r.max_dist_code >= 9 for r in reports)
    wide = by_name(cases, "48-bit tokens in a row")[0].report
    assert wide.widest_token == 15 + 5 + 15 + 13 == 48 and wide.wide_run >= 3 and wide.max_len_code == 15 and wide.max_dist_code == 15
    assert wide.kinds == ["stored", "dynamic"] and min(d for _, _, d in wide.matches if d > 16384) > 16384
    # dialects
    h = by_name(cases, "HLIT 257, HDIST 1, HCLEN 5")[0].report.headers[0]
    assert (h["hlit"], h["hdist"], h["hclen"]) == (257, 1, 5)
    for c in by_name(cases, "code lengths without run symbols"):
        assert c.report.headers[0]["rle_symbols"] == []
    h = by_name(cases, "code lengths without run symbols, HLIT 286")[0].report.headers[0]
    assert (h["hlit"], h["hdist"], h["hclen"]) == (286, 30, 19)
    h = by_name(cases, "repeat 16 crosses")[0].report.headers[0]
    assert h["run_crosses_boundary"] and 16 in h["rle_symbols"]
    h = by_name(cases, "zero run 18 crosses")[0].report.headers[0]
    assert h["run_crosses_boundary"] and 18 in h["rle_symbols"]
    for c in by_name(cases, "a code-length code other than zlib's"):
        assert sorted(c.report.headers[0]["cl_lens"]) == [4] * 13 + [5] * 6 and c.report.headers[0]["hclen"] == 19
    for c in by_name(cases, "length 258 as symbol 284"):
        assert sum(1 for _, l, _ in c.report.matches if l == 258) >= 2
    assert by_name(cases, "empty blocks of every type")[0].report.kinds == ["fixed", "dynamic", "stored", "fixed", "stored", "dynamic", "fixed"]
    for kind in ("stored", "fixed", "dynamic"):
        c = by_name(cases, f"lone end-of-block, {kind}")[0]
        assert c.report.kinds == [kind] and c.out == b""
    c = by_name(cases, "stored LEN 65535 in the middle")[0]
    assert c.report.kinds == ["fixed", "stored", "fixed"] and len(c.out) == 65536
    c = by_name(cases, "matches reach back across a block boundary")[0]
    assert c.report.kinds[0] == "stored" and any(p - d < c.report.block_out[1] <= p for p, _, d in c.report.matches)
    # positions
    assert (1, 258, 1) in by_name(cases, "distance == op: the member's first byte")[0].report.matches
    assert (700, 100, 700) in by_name(cases, "distance == op at op 700")[0].report.matches
    for c in by_name(cases, "distance 32768 at op 32768"):
        assert (32768, 258, 32768) in c.report.matches and any(d == 32768 and p > 40000 for p, _, d in c.report.matches)
    for c in by_name(cases, "match ends exactly at out_len") + by_name(cases, "match of 258 ends exactly at out_len"):
        p, l, _ = c.report.matches[-1]
        assert p + l == len(c.out)
    # 1-5 blocks of the three types; stored blocks at every bit phase with every LEN 0-9 and a Huffman block behind
    assert sorted(len(c.report.kinds) for c in cases if c.name[0] in "12345" and " blocks: " in c.name) == [1, 2, 3, 4, 5]
    assert {k for c in cases if " blocks: " in c.name for k in c.report.kinds} == {"stored", "fixed", "dynamic"}
    seen = set()
    for c in by_name(cases, "stored LEN "):
        if "bit phase" in c.name:
            assert c.report.kinds[1] == "stored" and c.report.kinds[2] in ("fixed", "dynamic")
            seen.add((c.report.starts[1], c.report.block_out[2] - c.report.block_out[1]))
    assert seen == {(phase, n) for phase in range(8) for n in range(10)}
    for c in by_name(cases, "trailing bytes"):
        dz = zlib.decompressobj(wbits=-15)
        dz.decompress(c.payload)
        assert dz.eof and len(dz.unused_data) >= 5
    # the host decoder leaves its unchecked loop 269 bytes before the end of the output: members that end in every kind of token there
    for c in by_name(cases, "long member"):
        assert len(c.out) > 9000 and len(c.payload) > 1000
    # reported by design: a single code of one bit, the end-of-block's, is the whole literal/length alphabet of the last block
    for name in dc.BY_DESIGN:
        c = by_name(cases, name)[0]
        assert c.report.kinds[-1] == "dynamic" and c.report.headers[-1]["kraft"][0] == 16384 and c.report.headers[-1]["hlit"] == 257
    # the random part draws no member of that class, and covers every helper and recipe
    rnd = [c for c in dc.corpus_valid(0) if c.name.startswith("random ")]
    assert all(k[0] == 32768 for c in rnd for k in (h["kraft"] for h in c.report.headers))
    for word in ("stored", "fixed", "dynamic/deep/", "dynamic/flat/", "dynamic/optimal/", "/deep/none", "/flat/greedy", "noise", "dense", "far", "runs", "text", "65536 bytes"):
        assert any(word in c.name for c in rnd), word
    assert any(c.report.max_len_code >= 11 and c.report.max_dist_code >= 9 for c in rnd)


@pytest.mark.parametrize("off", dc.DEVICE_OFFSETS)
def test_geometry_cases_are_what_they_say_at_every_device_offset(off):
    """the ring and batch geometry of the device decoder, for each first-output address the device test uses"""
    cases = [c for c in dc.corpus_valid(off, random_part=False) if f"(first output address {off} mod" in c.name]
    assert len(cases) == 8
    for c in cases:
        assert c.report.out_offset == off
    assert all(c.report.match_ends_at_unit_end() for c in by_name(cases, "matches end exactly at a unit's end"))
    for c in by_name(cases, "matches end exactly at a unit's end"):
        assert sum(1 for p, l, _ in c.report.matches if (off + p + l) % dw.UNIT == 0) == 3
    for c in by_name(cases, "matches cross a unit's end by one byte"):
        assert c.report.match_crosses_unit_by_one() and sum(1 for p, l, _ in c.report.matches if (off + p + l) % dw.UNIT == 1) == 3
    for c in by_name(cases, "overlapping matches of distance 1-8 split"):
        assert c.report.overlapping_match_split_by_unit() == [1, 2, 3, 4, 5, 6, 7, 8]
    assert {c.report.kinds[0] for c in by_name(cases, "overlapping matches")} == {"fixed", "dynamic"}
    per = by_name(cases, "more than 64 matches inside one unit")[0].report.matches_per_unit()
    assert max(per.values()) >= 150 and sum(1 for v in per.values() if v > 64) >= 2
    ages = by_name(cases, "a batch mixes sources")[0].report.source_ages()
    assert sum(1 for kinds in ages.values() if kinds == {"flushed_short", "flushed_long", "recent", "pending"}) >= 3
