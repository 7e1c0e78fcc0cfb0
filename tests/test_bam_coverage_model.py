"""CPU: the two statements of `sam coverage histogram` in tests/bam_coverage_model.py — one counter per position (literal) and sorted
events with one sweep (events) — hold equal on generated files in all three modes, and give histograms derived by hand."""
import pytest

from tests import bam_coverage_model as m
from tests.bam_coverage_model import D, EQ, H, I, M, N, S, X, rec

TEXT = b"@HD\tVN:1.6\n"


def raw_of(recs, refs):
    return m.header(TEXT, refs) + b"".join(recs)


def hist_of(pairs):
    h = [0] * m.BINS
    for k, v in pairs.items():
        h[k] = v
    return h


def both(raw, mode=("everywhere",)):
    a, b = m.literal(raw, mode), m.events(raw, mode)
    assert a == b
    hist, dropped, n_pos, n_counted = a
    assert sum(hist) + dropped == n_pos == m.target_size(raw, mode)
    return a


BED = (b"#comment\ntrack name=x\nbrowser position\n\nref1\t10\t200\nref1 150 400\nref1\t400\t450\nref3\t0\t99999\nnope\t1\t2\nref5  400\t500  extra\n"
       b"ref7\t50\t50\nref9\t3000\t9000\n")


@pytest.mark.parametrize("seed,n", [(1, 50), (2, 999), (3, 2300), (4, 6000)])
def test_literal_equals_events(seed, n):
    refs = m.refs_for(seed=seed)
    raw = raw_of(m.sorted_records(n, refs, seed=seed, skip_refs=(4,)), refs)
    for mode in (("everywhere",), ("region", b"ref2"), ("region", b"ref2:100-1,000"), ("region", b"ref6:0"), ("region", b"ref4"), ("region", b"nope"),
                 ("bed", BED)):
        hist, dropped, n_pos, n_counted = both(raw, mode)
        assert n_counted == sum(1 for r in m.records(raw) if m.counted(r, len(refs)))
    assert both(raw)[2] == sum(ln for t, (_, ln) in enumerate(refs) if t != 4)


def test_by_hand():
    refs = [(b"a", 10), (b"b", 12)]
    one = lambda *recs: both(raw_of(list(recs), refs))[0]                   # noqa: E731
    assert one(rec(b"x", 0, 2, cigar=((M, 3),))) == hist_of({0: 7, 1: 3})
    # mates that overlap are each counted
    assert one(rec(b"x", 0, 0, 1 | 0x40, ((M, 5),)), rec(b"x", 0, 3, 1 | 0x80, ((M, 5),))) == hist_of({0: 2, 1: 6, 2: 2})
    # D and N advance without covering; I S H P and codes above 8 do neither; = and X cover
    assert one(rec(b"x", 0, 1, cigar=((M, 2), (D, 3), (M, 2)))) == hist_of({0: 6, 1: 4})
    assert one(rec(b"x", 0, 1, cigar=((S, 4), (EQ, 2), (I, 3), (X, 1), (N, 2), (9, 5), (M, 1), (H, 2)), l_seq=11)) == hist_of({0: 6, 1: 4})
    # clipped at both ends
    assert one(rec(b"x", 0, -1, cigar=((M, 4),)), rec(b"y", 0, 8, cigar=((M, 5),))) == hist_of({0: 5, 1: 5})
    # a record that covers nothing still makes its reference reported; the other reference is not
    assert one(rec(b"x", 1, 5, cigar=((I, 2), (S, 3)))) == hist_of({0: 12})
    # not counted: 0x4 0x100 0x200 0x400, and a record without a reference; 0x800 is counted
    skipped = [rec(b"s%d" % f, 0, 1, f) for f in (4, 0x100, 0x200, 0x400)] + [rec(b"u", -1, 1, 0), rec(b"v", 2, 1, 0)]
    assert one(*skipped) == hist_of({})
    assert one(*skipped, rec(b"sup", 0, 1, 0x800, ((M, 2),))) == hist_of({0: 8, 1: 2})


def test_regions_by_hand():
    refs = [(b"a", 100), (b"a:1-5", 50)]
    raw = raw_of([rec(b"x", 0, 10, cigar=((M, 20),)), rec(b"u", 0, 10, 4, ())], refs)
    assert both(raw, ("region", b"a"))[0] == hist_of({0: 80, 1: 20})
    assert both(raw, ("region", b"a:11-30"))[0] == hist_of({1: 20})
    assert both(raw, ("region", b"a:30"))[0] == hist_of({0: 70, 1: 1})
    assert both(raw, ("region", b"a:0-12"))[0] == hist_of({0: 10, 1: 2})          # beg < 1 reads as 1
    assert both(raw, ("region", b"a:91-1,000"))[0] == hist_of({0: 10})            # cut to the reference; commas ignored
    assert both(raw, ("region", b"a:1-5"))[0] == hist_of({0: 50})                 # a whole name wins over the split; no record needed
    assert both(raw, ("region", b"a:1-5:2-3"))[0] == hist_of({0: 2})
    for bad in (b"b", b"a:", b"a:x", b"a:1-", b"a:-5", b"a:1-2-3", b"a:1.5"):
        assert m.targets(raw, ("region", bad)) == ({}, False) and both(raw, ("region", bad))[0] == hist_of({})
    only_unmapped = raw_of([rec(b"u", 0, 10, 4, ())], refs)
    assert both(only_unmapped, ("region", b"a:1-40"))[0] == hist_of({0: 40}) and both(only_unmapped)[0] == hist_of({})


def test_bed_by_hand():
    refs = [(b"a", 100), (b"b", 100), (b"c", 100)]
    recs = [rec(b"x", 0, 10, cigar=((M, 20),)), rec(b"y", 1, 50, cigar=((M, 10),)), rec(b"z", 2, 5, cigar=((I, 3),), l_seq=3)]
    raw = raw_of(recs, refs)
    # overlapping and adjacent intervals are a union; an interval past the end is cut; b's record overlaps none of b's: b is not reported
    bed = b"a\t0\t15\na 12 20\na\t20\t25\na\t90\t500\nb\t0\t50\nb\t60\t70\nzz\t0\t5\nc\t5\t6\n"
    assert both(raw, ("bed", bed))[0] == hist_of({0: 10 + 10 + 1, 1: 15})
    # a span [pos, pos + 1) for a record without a reference-consuming op
    assert both(raw, ("bed", b"c\t6\t9\n"))[0] == hist_of({})
    assert both(raw, ("bed", b"b\t59\t61\n"))[0] == hist_of({0: 1, 1: 1})
    with pytest.raises(m.BadBed):
        m.parse_bed(b"a\t1\n", m.refs_of(raw))
    with pytest.raises(m.BadBed):
        m.parse_bed(b"a\t1\tx\n", m.refs_of(raw))


def test_deeper_than_the_last_bin_is_dropped():
    refs = [(b"a", 20000)]
    recs = [rec(b"p%d" % i, 0, 100, cigar=((M, i + 1),), l_seq=0) for i in range(10002)]
    hist, dropped, n_pos, _ = both(raw_of(recs, refs))
    assert dropped == 2 and hist[10000] == 1 and hist[9999] == 1 and hist[0] == 20000 - 10002 and n_pos == 20000


# ---- the inputs that take the device path's fixed-size structures past their capacity (tests/test_gpu_bam_coverage.py runs them) ----
@pytest.fixture(scope="module")
def carry():
    refs, recs = m.carry_input()
    raw = raw_of(recs, refs)
    return raw, m.sweep(raw)


def test_carry_input_by_arithmetic(carry):
    """no counter per position for 20 references of 2^31 - 1: the events statement against the sums written out by hand"""
    raw, swept = carry
    exp = m.carry_expected()
    assert m.events(raw, swept=swept) == exp
    hist, dropped, n_pos, n_counted = exp
    assert (n_counted, hist[1], n_pos, hist[0], dropped) == (327680, 21474508800, 42949672940, 21475164140, 0)
    assert sum(hist) == n_pos == m.target_size(raw, ("everywhere",))
    # every gap is 65 535 positions but the one behind each reference's last run
    widths = {}
    for depth, inside, w in swept[0]:
        if w:
            assert inside == 1
            widths[(depth, w)] = widths.get((depth, w), 0) + 1
    assert widths == {(1, 65535): 327680, (0, 65535): 20 * 16383, (0, 98302): 20}


def test_carry_input_wraps_an_lds_counter_on_four_workgroups_only(carry):
    """the precondition of the GPU case: on the grid of a context planned for one CU some workgroup's counters of depth 0 and of depth
    1 both pass 2^32; on the grid of a whole chip none comes near.  17 references are the fewest that still do, 16 do not."""
    raw, swept = carry
    n_events = len(swept[0]) + 1
    assert n_events == 2 * 327680 + 2 * 20
    assert m.hist_grid(n_events, 1) == 4 and m.hist_grid(n_events, 256) == 1024 and m.hist_grid(700, 256) == 3
    four = m.lds_sums(swept, 4)
    assert set(four) == {0, 1} and min(four.values()) > 1.2 * 2 ** 32
    assert max(m.lds_sums(swept, 1024).values()) < 2 ** 32 // 100
    for n_ref, wraps in ((17, True), (16, False)):                        # by the arithmetic of the issue: about 2 * 16 384 / 8 gaps a bin and workgroup
        per_bin = n_ref * 16384 // 4 * 65535
        assert (per_bin > 2 ** 32) == wraps


def test_lds_sums_by_hand():
    # event i: (depth, inside, w); workgroup (i // 256) % grid
    gaps = [(0, 1, 10)] * 256 + [(1, 1, 7)] * 256 + [(0, 1, 65536), (0, 0, 5), (m.BINS, 1, 5), (0, 1, 0), (0, 1, 65535)] + [(1, 1, 1)] * 251 + [(1, 1, 3)]
    assert m.lds_sums((gaps, 0), 1) == {0: 2560 + 65535, 1: 7 * 256 + 251 + 3}
    assert m.lds_sums((gaps, 0), 2) == {0: 65535 + 2560, 1: 7 * 256 + 3}
    assert m.lds_sums((gaps, 0), 3) == {0: 65535, 1: 7 * 256}
    assert m.lds_sums((gaps, 0), 4) == {0: 65535, 1: 7 * 256}


def test_split_input_has_every_gap_on_both_sides():
    refs, recs, want = m.split_input()
    raw = raw_of(recs, refs)
    hist, dropped, n_pos, n_counted = both(raw)
    assert refs == [(b"s", 1 << 20)] and n_pos == 1 << 20 and n_counted == len(recs) == 3 + 9999 + 3 + 6
    got = {}
    for depth, inside, w in m.sweep(raw)[0]:
        if inside > 0 and 65535 <= w <= 65537:
            got.setdefault(depth, []).append(w)
    assert got == want and sorted(want) == [0, 1, m.BINS - 1, m.BINS]
    assert hist[m.BINS - 1] == dropped == 65535 + 65536 + 65537 and hist[1] == dropped + 1 and hist[9999] == 1
    assert [m.core(r)[1] for r in recs] == sorted(m.core(r)[1] for r in recs)


def test_pow2_inputs():
    sizes = []
    for name, refs, recs in m.pow2_inputs():
        raw = raw_of(recs, refs)
        size = sum(ln for _, ln in refs)
        sizes.append(size)
        last = len(refs) - 1
        ends = [m.runs(r, refs[m.core(r)[0]][1])[0] for r in recs if m.core(r)[0] == last]
        assert any(rs and rs[-1][1] == refs[last][1] and m.core(r)[1] + 12 == refs[last][1] for r, rs in zip([r for r in recs if m.core(r)[0] == last], ends))
        assert any(m.core(r)[:2] == (0, 0) and m.counted(r, len(refs)) for r in recs)
        assert both(raw)[2] == size                                       # every reference has a counted record
        hist, _, n_pos, _ = both(raw, ("region", refs[last][0]))
        assert n_pos == refs[last][1] and sum(hist[1:]) > 0
        assert both(raw, ("region", b"%s:%d-%d" % (refs[last][0], refs[last][1] - 3, refs[last][1] + 9)))[2] == 4
    assert sizes == [(1 << 13) - 1, 1 << 13, (1 << 13) + 1, 1 << 12]


def test_words_input():
    refs, recs, bed, bed2 = m.words_input()
    raw = raw_of(recs, refs)
    assert len(refs) == 70 and all(200 <= ln < 600 for _, ln in refs)
    assert {m.core(r)[0] for r in recs if m.counted(r, 70)} == set(m.WORDS_COUNTED)
    assert {m.core(r)[0] for r in recs if not m.counted(r, 70)} == {t for t, _ in m.WORDS_NOT}
    assert {t >> 5 for t in m.WORDS_COUNTED} == {0, 1, 2} and {t & 31 for t in m.WORDS_COUNTED} >= {0, 31, 1}
    assert both(raw)[2] == sum(refs[t][1] for t in m.WORDS_COUNTED)
    assert sorted(m.targets(raw, ("bed", bed))[0]) == list(m.WORDS_COUNTED) and both(raw, ("bed", bed))[2] == 70 * 7
    assert sorted(m.targets(raw, ("bed", bed2))[0]) == [t for t in m.WORDS_COUNTED if t != 64]
    assert both(raw, ("bed", bed2))[2] == 70 * 6 and refs[64][1] >= 190


def test_deep_bed_cases():
    bed = m.deep_bed()
    merged = {}
    for t, b, e in m.parse_bed(bed, m.DEEP_REFS):
        merged.setdefault(t, []).append((b, e))
    assert sorted(merged) == [0, 2] and len(merged[0]) > m.DEEP_N + 200 and merged[0] != sorted(merged[0])
    assert all(m.merge(v) == [m.deep_iv(k) for k in range(m.DEEP_N)] for v in merged.values())
    cases = m.deep_cases()
    seen = set()
    for name, recs, reported in cases:
        raw = raw_of(recs, m.DEEP_REFS)
        assert sorted(m.targets(raw, ("bed", bed))[0]) == sorted(t for t, yes in reported.items() if yes), name
        assert both(raw, ("bed", bed))[2] == 50 * m.DEEP_N * sum(reported.values()), name
        seen |= {(m.core(r)[0], m.core(r)[1]) for r in recs}
    assert len(cases) == len(m.DEEP_RELATIONS) * len(m.DEEP_KS) + 3 and len(seen) > len(cases)
    assert {yes for _, _, yes in m.DEEP_RELATIONS.values()} == {True, False}
