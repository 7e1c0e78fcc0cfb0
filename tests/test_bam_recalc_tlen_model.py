"""CPU: tests/bam_recalc_tlen_model.py against hand-computed pairs, its two statements against each other on the generator's file, and
the stops of the reference's loop: status, message and the records already flushed."""
import pytest

from tests import bam_recalc_tlen_model as m
from tests.bam_recalc_tlen_model import D, H, I, M, N, S

I32 = 1 << 32

# (pos a, reverse a, cigar a, pos b, reverse b, cigar b) -> t: b gets t, a gets -t.  end_pos - 1 of a reverse read by hand.
PAIRS = [
    ((100, False, ((M, 20),), 200, True, ((M, 20),)), -120),            # converging: |219 - 100| + 1, b to the right
    ((200, True, ((M, 20),), 100, False, ((M, 20),)), 120),             # the same pair, the reverse mate first
    ((100, True, ((M, 20),), 300, False, ((M, 20),)), 0),               # diverging: start(b) 300 > start(a) 119, b forward
    ((300, False, ((M, 20),), 100, True, ((M, 20),)), 0),               # diverging: start(b) 119 < start(a) 300, b reverse
    ((100, False, ((M, 20),), 100, True, ((S, 4), (M, 1))), 1),         # one 5' end: |100 - 100| + 1, pos equal
    ((100, False, ((M, 20),), 100, True, ((M, 20),)), 20),              # pos equal, b's 5' end at 119
    ((100, True, ((M, 20),), 100, False, ((M, 20),)), 20),              # start(b) 100 < start(a) 119, b forward: kept
    ((100, False, ((M, 30),), 90, True, ((M, 5),)), 0),                 # b reverse ends at 94 < 100
    ((100, True, ((M, 10), (D, 5), (M, 10)), 150, True, ((M, 8), (N, 300), (M, 12))), -346),    # both reverse: |469 - 124| + 1
    ((100, False, ((M, 20),), 150, False, ((M, 20),)), 0),              # both forward: start(b) > start(a), b forward
    ((150, False, ((M, 20),), 100, False, ((M, 20),)), 51),             # both forward, b to the left: |100 - 150| + 1
    ((100, False, ((M, 20),), 160, True, ((H, 4), (S, 3), (M, 10), (I, 2), (M, 8), (S, 2))), -78),   # only M D N = X move: 160 + 18 - 1
    ((100, False, ((M, 10),), 101, True, m.LONG_N), -(101 + 10 + 9 * ((1 << 28) - 1) - 1 - 100 + 1)),   # above 2^31: cut by `as i32`
]


def two(spec, name=b"r"):
    pa, ra, ca, pb, rb, cb = spec
    return [m.cand(name, 0, pa, pb, ra, True, ca), m.cand(name, 0, pb, pa, rb, False, cb)]


def bam(recs):
    return m.md.rm.header(b"@HD\tVN:1.6\n", m.md.rm.REFS) + b"".join(recs)


@pytest.mark.parametrize("spec,t", PAIRS)
def test_hand_computed_pairs(spec, t):
    a, b = two(spec)
    assert m.pair_tlen(a, b) == t
    for f in (m.literal, m.grouped):
        out, err, code = f(bam([a, b]), 1 << 40)
        got = list(m.records(out))
        assert (code, err) == (0, b"") and [m.tlen_of(r) for r in got] == [((-t + (1 << 31)) % I32) - (1 << 31), ((t + (1 << 31)) % I32) - (1 << 31)]
        assert [r[:32] + r[36:] for r in got] == [r[:32] + r[36:] for r in (a, b)]       # only the TLEN changes


def test_the_cut_to_32_bits_shows():
    t = PAIRS[-1][1]
    assert abs(t) > 1 << 31
    a, b = two(PAIRS[-1][0])
    got = list(m.records(m.literal(bam([a, b]), 5000)[0]))
    assert m.tlen_of(got[1]) == t + I32 and m.tlen_of(got[0]) == -t - I32


@pytest.mark.parametrize("max_len", [1, 5000, 1 << 40])
def test_literal_equals_grouped_on_the_generator(max_len):
    raw = bam(m.served_records(3000, seed=1))
    lit = m.literal(raw, max_len)
    assert lit[2] == 0 and m.grouped(raw, max_len) == lit
    recs = list(m.records(raw))
    cls = [m.classify(r, max_len) for r in recs]
    assert "S" not in cls and cls.count("Z") > 300 and cls.count("C") > 900
    hdr, written, lone = m.grouped_parts(raw, max_len)
    assert 100 < len(lone) and len(written) + len(lone) == len(recs)
    assert lit[1].count(b"\n") == len(lone)
    assert all(m.tlen_of(r) for r in recs)                               # junk in every input TLEN
    tl = [m.tlen_of(r) for r in written]
    assert tl.count(0) > cls.count("Z") and sum(1 for t in tl if t > 0) > 200 and sum(1 for t in tl if t < 0) > 200
    assert any(abs(t) > 1 << 30 for t in tl)                             # the pair cut by `as i32`


def test_the_generator_covers_the_branches():
    recs = m.served_records(3000, seed=1)
    by_name = {}
    for k, r in enumerate(recs):
        if m.classify(r, 1 << 40) == "C":
            by_name.setdefault(m.qname(r), []).append(k)
    counts = {len(v) for v in by_name.values()}
    assert {1, 2, 3, 4} <= counts and max(counts) > 20
    gaps = [v[1] - v[0] for v in by_name.values() if len(v) >= 2]
    assert gaps.count(1) > 300 and sum(1 for g in gaps if 600 < g < 900) > 30
    # the distance at max_len is a candidate, one above it is not
    for max_len in (1, 5000):
        d = {abs(m.fields(r)[1] - m.fields(r)[4]) for r in recs if m.classify(r, 1 << 40) == "C"}
        assert {max_len, max_len + 1} <= d
        assert sum(1 for r in recs if m.classify(r, max_len) != m.classify(r, 1 << 40)) > 100
    # 0x100 / 0x800 records that are Z by their first line
    assert sum(1 for r in recs if m.fields(r)[2] & 0x900 and m.classify(r, 1 << 40) == "Z") > 50
    # reverse candidates whose end_pos is not pos + l_seq
    assert sum(1 for r in recs if m.fields(r)[2] & 0x10 and m.classify(r, 1) == "C" and m.md.end_pos(r) != m.fields(r)[1] + m.md.core(r)[5]) > 100


@pytest.mark.parametrize("what", sorted(m.stop_files()))
def test_stops(what):
    recs, at, status, msg = m.stop_files()[what]
    raw = bam(recs)
    out, err, code = m.literal(raw, 5000)
    assert (code, err) == (status, msg) and m.grouped(raw, 5000) is None
    # what was flushed: the served prefix's output up to its first record that still waits when the loop stops
    full = m.literal(bam(recs[:at]), 5000)
    assert full[2] == 0 and full[0].startswith(out)
    got = list(m.records(out))
    waiting = {}
    for k, r in enumerate(recs[:at]):
        if m.classify(r, 5000) == "C":
            if m.qname(r) in waiting:
                del waiting[m.qname(r)]
            else:
                waiting[m.qname(r)] = k
    assert len(got) == min(list(waiting.values()) + [at])
    if what == "first record":
        assert out == m.out_header(raw)


def test_an_unpaired_bad_cigar_is_served():
    """cigar() is reached only for a record that ends up in a pair"""
    lone = m.md.rec(b"lone", 0, 200, flag=0x1 | 0x80 | 0x10, cigar=((M, 10), (9, 3)), l_seq=10, mtid=0, mpos=100)
    zero = m.md.rec(b"zero", 0, 200, flag=0x10, cigar=((M, 10), (9, 3)), l_seq=10)
    raw = bam([lone, zero])
    assert m.literal(raw, 5000) == m.grouped(raw, 5000) == (m.out_header(raw) + m.with_tlen(zero, 0), m.discard_line(b"lone"), 0)


@pytest.mark.parametrize("text,value", [("5000", 5000), ("+7", 7), ("-3", -3), ("0", 0), ("", 0), ("abc", 0), ("1e3", 0), (" 5", 0), ("5 ", 0),
                                        ("9223372036854775807", (1 << 63) - 1), ("9223372036854775808", 0), ("-9223372036854775808", -(1 << 63)),
                                        ("0x10", 0), ("1_000", 0), ("+", 0), ("--5", 0)])
def test_parse_max_len(text, value):
    assert m.parse_max_len(text) == value
