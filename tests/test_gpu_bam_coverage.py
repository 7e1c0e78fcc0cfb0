"""GPU: sk_bam_file_coverage — `sam coverage histogram` from sorted CIGAR events on the device (mark, emit, radix sort, scan, LDS
histogram) — against the literal statement of tests/bam_coverage_model.py (one counter per position).  The one file whose references
are too long for a counter per position is held to the events statement, which tests/test_bam_coverage_model.py holds to the literal
one.  Every check asserts sum(hist) + n_dropped == n_positions == the size of the targets."""
import random

import numpy as np
import pytest

from tests import bam_coverage_model as m
from tests.bam_coverage_model import D, I, M, S, rec

pytestmark = pytest.mark.gpu

TEXT = b"@HD\tVN:1.6\n"
BED = (b"#comment\nref1\t10\t200\nref1 150 400\nref1\t400\t450\nref3\t0\t99999\nnope\t1\t2\nref5  400\t500\nref7\t50\t50\nref9\t3000\t9000\n"
       b"ref10\t1\t2\nref0\t0\t1\n")
MODES = [("everywhere",), ("region", b"ref2"), ("region", b"ref6:100-1,000"), ("region", b"ref4:5-50"), ("bed", BED)]


def triples(raw, mode):
    """(mode number, the C-ABI's target triples): what the command's host half makes of its options"""
    refs = m.refs_of(raw)
    if mode[0] == "everywhere":
        return 0, []
    if mode[0] == "region":
        reg = m.parse_region(mode[1], refs)
        return 1, [reg] if reg else []
    return 2, m.parse_bed(mode[1], refs)


def check(ctx, path, raw, mode, model=None):
    exp_hist, exp_dropped, exp_pos, exp_counted = (model or m.literal)(raw, mode)
    num, t = triples(raw, mode)
    handled, hist, n_pos, n_drop, n_counted, info = ctx.bam_file_coverage(str(path), num, t)
    assert handled, info
    assert int(hist.sum()) + n_drop == n_pos == m.target_size(raw, mode)
    assert hist.tolist() == exp_hist and (n_drop, n_pos, n_counted) == (exp_dropped, exp_pos, exp_counted)
    assert info[3] == sum(1 for _ in m.records(raw))
    return hist, n_pos, n_drop


def make(tmp, name, recs, refs, piece=0xFF00):
    path = tmp / name
    return path, m.write(path, recs, text=TEXT, refs=refs, piece=piece)


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("coverage")


@pytest.fixture(scope="module")
def bam(tmp):
    """25 000 sorted records on 11 references (none on ref4), every CIGAR op and two codes above 8"""
    refs = m.refs_for()
    return make(tmp, "in.bam", m.sorted_records(25000, refs, skip_refs=(4,)), refs)


@pytest.mark.parametrize("mode", MODES, ids=lambda x: x[0] + (":" + x[1].decode() if x[0] == "region" else ""))
def test_three_modes(ctx, bam, mode):
    path, raw = bam
    hist, n_pos, _ = check(ctx, path, raw, mode)
    if mode[0] != "region" or b"ref4" not in mode[1]:
        assert int(hist[1:].sum()) > 0
    else:
        assert int(hist[0]) == n_pos == 46                                    # a region counts without a record


@pytest.mark.parametrize("n", [50, 999, 1000, 1001, 2300, 4100])
def test_record_counts(ctx, tmp, n):
    refs = m.refs_for(seed=n)
    path, raw = make(tmp, "n%d.bam" % n, m.sorted_records(n, refs, seed=n), refs)
    for mode in MODES:
        check(ctx, path, raw, mode)


def test_many_records_and_their_order(ctx, tmp):
    """300 000 records: the sort and the scans run more than one tile and pass; the same records shuffled give the same histogram"""
    refs = m.refs_for(n_ref=5, seed=9, lo=20000, hi=60000)
    recs = m.sorted_records(300000, refs, seed=9, l_seq=0)
    path, raw = make(tmp, "big.bam", recs, refs)
    hist, n_pos, _ = check(ctx, path, raw, ("everywhere",))
    random.Random(3).shuffle(recs)
    spath, sraw = make(tmp, "shuffled.bam", recs, refs)
    handled, shist, s_pos, s_drop, s_counted, _ = ctx.bam_file_coverage(str(spath), 0, [])
    assert handled and np.array_equal(shist, hist) and (s_pos, s_drop) == (n_pos, 0) and s_counted == sum(1 for r in recs if m.counted(r, 5))


def test_pile_deeper_than_the_last_bin(ctx, tmp):
    """10 002 records on one start with staggered lengths: depths 9 999 and 10 000 are counted, 10 001 and 10 002 dropped"""
    refs = [(b"a", 20000), (b"b", 50)]
    recs = [rec(b"p%d" % i, 0, 100, cigar=((M, i + 1),), l_seq=0) for i in range(10002)]
    path, raw = make(tmp, "pile.bam", recs, refs)
    hist, n_pos, n_drop = check(ctx, path, raw, ("everywhere",))
    assert n_drop == 2 and hist[10000] == 1 and hist[9999] == 1 and hist[1] == 1 and n_pos == 20000
    _, _, n_drop = check(ctx, path, raw, ("region", b"a:101-101"))
    assert n_drop == 1


def test_which_references_are_reported(ctx, tmp):
    refs = [(b"none", 300), (b"skipped", 400), (b"ins", 500), (b"clip", 100)]
    recs = [rec(b"s%d" % f, 1, 10, f) for f in (4, 0x100, 0x200, 0x400, 0x704)]
    recs += [rec(b"i", 2, 7, 0, ((I, 3), (S, 2), (5, 4)))]                     # covers nothing, but its reference is reported
    recs += [rec(b"lo", 3, -1, 0, ((M, 10),)), rec(b"hi", 3, 95, 16, ((M, 5), (D, 2), (M, 20))), rec(b"out", 3, 100, 0, ((M, 5),)), rec(b"neg", 3, -30, 0, ((M, 10),))]
    recs += [rec(b"u", -1, -1, 4, (), l_seq=5, mtid=-1, mpos=-1), rec(b"far", 7, 1, 0)]
    path, raw = make(tmp, "which.bam", recs, refs)
    hist, n_pos, _ = check(ctx, path, raw, ("everywhere",))
    assert n_pos == 600 and hist[1] == 9 + 5 and hist[0] == 500 + 100 - 14
    sup = [rec(b"sup0", 0, 5, 0x800, ((M, 8),)), rec(b"sup1", 1, 5, 0x800 | 16, ((M, 8),))]
    path, raw = make(tmp, "which2.bam", sup + recs, refs)
    hist, n_pos, _ = check(ctx, path, raw, ("everywhere",))
    assert n_pos == 1300 and hist[1] == 14 + 16


def test_references_of_two_to_the_31(ctx, tmp):
    """three references of 2^31 - 1 positions, a few hundred records near both ends of each: the total is above 2^32, so keys and gaps
    need 64 bits.  (No counter per position at this size: the events statement is the reference here.)"""
    L = (1 << 31) - 1
    refs = [(b"x", L), (b"y", L), (b"z", L)]
    rnd = random.Random(5)
    recs = []
    for t in range(3):
        ps = sorted([rnd.randrange(-3, 400) for _ in range(150)] + [rnd.randrange(L - 400, L + 3) for _ in range(150)])
        recs += [rec(b"r%d.%d" % (t, k), t, p if p <= L else L, rnd.choice(m.FLAGS), rnd.choice(m.CIGARS)) for k, p in enumerate(ps)]
    path, raw = make(tmp, "wide.bam", recs, refs)
    hist, n_pos, _ = check(ctx, path, raw, ("everywhere",), model=m.events)
    assert n_pos == 3 * L > 1 << 32 and int(hist[0]) > 1 << 32
    check(ctx, path, raw, ("region", b"z:2,147,483,000-2147483647"), model=m.events)
    check(ctx, path, raw, ("bed", b"y\t2147483000\t4000000000\nz\t0\t100\nx 5 2147483640\n"), model=m.events)
    check(ctx, path, raw, ("region", b"z:2,147,483,000-2147483647"))         # (648 positions: the literal statement serves)


def test_records_that_straddle_blocks(ctx, tmp):
    refs = m.refs_for(seed=4)
    path, raw = make(tmp, "straddle.bam", m.sorted_records(3000, refs, seed=4), refs, piece=0x3000)
    for mode in MODES:
        check(ctx, path, raw, mode)


def test_empty_and_unmapped_only(ctx, tmp):
    refs = m.refs_for(seed=2)
    path, raw = make(tmp, "empty.bam", [], refs)
    for mode in (("everywhere",), ("bed", BED)):
        hist, n_pos, _ = check(ctx, path, raw, mode)
        assert n_pos == 0 and not hist.any()
    path, raw = make(tmp, "unmapped.bam", [rec(b"u%d" % k, 2, 100 + k, 4, ()) for k in range(70)], refs)
    hist, n_pos, _ = check(ctx, path, raw, ("everywhere",))
    assert n_pos == 0
    hist, n_pos, _ = check(ctx, path, raw, ("region", b"ref2:11-110"))
    assert int(hist[0]) == n_pos == 100
    path, raw = make(tmp, "noref.bam", [rec(b"u", -1, -1, 4, (), mtid=-1)], [])
    check(ctx, path, raw, ("everywhere",))


def test_bed_reference_without_an_overlapping_record(ctx, bam, tmp):
    """ref8 has counted records, none of which overlaps its interval (behind the reference's end); ref4 has no record: neither is
    reported; ref2 is"""
    path, raw = bam
    refs = m.refs_of(raw)
    bed = b"ref8\t%d\t%d\nref4\t0\t10\nref2\t0\t30\n" % (refs[8][1] + 200, refs[8][1] + 300)
    _, n_pos, _ = check(ctx, path, raw, ("bed", bed))
    assert n_pos == 30
    lone = [rec(b"a", 0, 50, 0, ((M, 10),)), rec(b"b", 1, 50, 0, ((M, 10),))]
    path, raw = make(tmp, "lone.bam", lone, [(b"p", 200), (b"q", 200)])
    _, n_pos, _ = check(ctx, path, raw, ("bed", b"p\t0\t50\np\t60\t70\nq\t59\t60\n"))
    assert n_pos == 1


def test_arguments(ctx, bam):
    path, raw = bam
    from seqkit_amd.capi import SeqkitHipError
    with pytest.raises(SeqkitHipError):
        ctx.bam_file_coverage(str(path), 3, [])
    handled, hist, n_pos, _, _, info = ctx.bam_file_coverage(str(path) + ".missing", 0, [])
    assert not handled and info[5] < 0 and not hist.any()
    # overlapping targets in any order count once; a refID outside the header is ignored
    handled, hist, n_pos, n_drop, _, _ = ctx.bam_file_coverage(str(path), 1, [(2, 50, 90), (99, 0, 5), (2, 10, 60), (-1, 0, 5), (2, 70, 80)])
    assert handled and n_pos == 80 == int(hist.sum()) + n_drop
    assert hist.tolist() == m.literal(raw, ("region", b"ref2:11-90"))[0]
