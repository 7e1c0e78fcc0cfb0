"""GPU: sk_bam_file_coverage — `sam coverage histogram` from sorted CIGAR events on the device (mark, emit, radix sort, scan, LDS
histogram) — against the literal statement of tests/bam_coverage_model.py (one counter per position).  The one file whose references
are too long for a counter per position is held to the events statement, which tests/test_bam_coverage_model.py holds to the literal
one.  Every check asserts sum(hist) + n_dropped == n_positions == the size of the targets.
The last five tests take the path's fixed-size structures past their capacity — the 32-bit LDS counters of the histogram kernel, its
split at gaps of 2^16, the sort's key width, the bitmaps' second and third word, the search in a long interval list — on inputs that
tests/bam_coverage_model.py generates and tests/test_bam_coverage_model.py holds on the CPU."""
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


# ---- past the capacity of the path's fixed-size structures ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def one_cu(hip_lib):
    """a context that plans for one CU, as `small[1]` of tests/test_gpu_small_grid.py (which imports this file, so it is made here):
    launch_bam_cov_hist gives it four workgroups"""
    from tests.test_gpu_small_grid import planned
    c = planned("1")
    assert c.planned_cus() == 1
    yield c
    c.close()


def known(exp):
    """a model for check(): what the caller has computed already"""
    return lambda raw, mode: exp


def test_lds_counters_wrap(ctx, one_cu, tmp):
    """bam_cov_hist_kernel's carry, `if (old + (u32)w < old) atomicAdd(hist + depth, 1ull << 32)`: 327 680 runs of 65 535 positions, 65 535
    apart, on 20 references of 2^31 - 1.  On the four workgroups of a context planned for one CU the gaps below 2^16 add up to 5.4e9 per
    workgroup and depth, for depth 0 and for depth 1 (asserted from the model's sorted events): both counters wrap.  On the default
    grid none does.  Both equal the sums written out by hand (tests/bam_coverage_model.py: carry_expected) and each other."""
    refs, recs = m.carry_input()
    path = tmp / "carry.bam"
    raw = m.write(path, recs, text=TEXT, refs=refs, level=1)
    swept = m.sweep(raw)
    exp = m.carry_expected()
    assert m.events(raw, swept=swept) == exp and exp[0][1] == 327680 * 65535 and exp[0][0] + exp[0][1] == exp[2] == 20 * ((1 << 31) - 1)
    n_events = len(swept[0]) + 1
    assert m.hist_grid(n_events, 1) == 4 < m.hist_grid(n_events, ctx.planned_cus())
    four, whole = m.lds_sums(swept, 4), m.lds_sums(swept, m.hist_grid(n_events, ctx.planned_cus()))
    assert four[0] > 1 << 32 and four[1] > 1 << 32 and max(whole.values()) < 1 << 32
    got = [check(c, path, raw, ("everywhere",), model=known(exp)) for c in (one_cu, ctx)]
    assert np.array_equal(got[0][0], got[1][0]) and got[0][1:] == got[1][1:] == (exp[2], 0)


def test_gaps_on_both_sides_of_the_lds_split(ctx, one_cu, tmp):
    """bam_cov_hist_kernel's `w >= 65536`: gaps of 65 535 (LDS), 65 536 and 65 537 (the global counter at once) at depth 0, 1, 10 000
    (the last bin) and 10 001 (dropped)"""
    refs, recs, gaps = m.split_input()
    path, raw = make(tmp, "split.bam", recs, refs)
    exp = m.literal(raw)
    assert sorted(gaps) == [0, 1, 10000, 10001] and all(ws == [65535, 65536, 65537] for ws in gaps.values())
    for c in (one_cu, ctx):
        hist, n_pos, n_drop = check(c, path, raw, ("everywhere",), model=known(exp))
        assert n_pos == 1 << 20 and n_drop == 3 * 65536 == hist[10000] and hist[1] == 3 * 65536 + 1


def test_genome_sizes_at_a_power_of_two(ctx, tmp):
    """sk_bam_file_coverage's `bits` loop: the largest sort key is the genome's size itself, the end of a run (and of a target) on the
    last position; at 2^13 and 2^12 it alone needs the top bit"""
    sizes = []
    for name, refs, recs in m.pow2_inputs():
        path, raw = make(tmp, "genome%s.bam" % name, recs, refs)
        last = refs[-1]
        sizes.append(check(ctx, path, raw, ("everywhere",))[1])
        hist, n_pos, _ = check(ctx, path, raw, ("region", last[0]))
        assert n_pos == last[1] and int(hist[1:].sum()) > 0
        assert check(ctx, path, raw, ("region", b"%s:%d-%d" % (last[0], last[1] - 3, last[1] + 9)))[1] == 4
        assert check(ctx, path, raw, ("bed", b"%s\t%d\t%d\ng0\t0\t1\n" % (last[0], last[1] - 1, last[1] + 5)))[1] == 2
    assert sizes == [8191, 8192, 8193, 4096]


def test_bitmap_words_beyond_the_first(ctx, tmp):
    """cov_set_bit's word index and the host's reading of it: 70 references, counted records on 0 31 32 33 63 64 69 alone"""
    refs, recs, bed, bed2 = m.words_input()
    path, raw = make(tmp, "words.bam", recs, refs)
    assert check(ctx, path, raw, ("everywhere",))[1] == sum(refs[t][1] for t in m.WORDS_COUNTED)
    assert check(ctx, path, raw, ("bed", bed))[1] == 70 * 7                   # the seven references alone are reported
    assert check(ctx, path, raw, ("bed", bed2))[1] == 70 * 6                  # ref64's interval lies behind its records
    for t in (1, 31, 32, 64, 65, 69):
        check(ctx, path, raw, ("region", b"ref%d" % t))


def test_deep_bed(ctx, tmp):
    """the binary search of bam_cov_mark_kernel in 1 000 merged intervals a reference, an empty range of `ioff` between two full ones:
    a record in every relation to an interval, one a reference and file, so that each decides whether its reference is reported"""
    bed = m.deep_bed()
    for k, (name, recs, reported) in enumerate(m.deep_cases()):
        path, raw = make(tmp, "deep%d.bam" % k, recs, m.DEEP_REFS)
        _, n_pos, _ = check(ctx, path, raw, ("bed", bed))
        assert n_pos == 50 * m.DEEP_N * sum(reported.values()), name
