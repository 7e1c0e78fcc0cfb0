"""CPU: the two statements of `sam statistics --on-target` in tests/bam_on_target_model.py agree — the reference's sweep over the
sorted regions with its `break` rules, and the prefix-maximum form the device path rests on.  These tests hold the model, not the
feature."""
import random

import pytest

from tests import bam_on_target_model as om


def test_crafted_list_has_the_shapes():
    bed = om.CRAFTED_BED
    assert bed[0] == [] and len(bed[1]) == 1
    assert len({s for s, _ in bed[2]}) == 1 and len(bed[2]) > 3                              # many regions, one start
    long_start, long_end = bed[3][0]
    assert sum(1 for s, e in bed[3][1:] if long_start < s and e < long_end) >= 3            # a long early region over later short ones
    assert any(s == 1 << 31 for s, _ in bed[3])
    assert any(e < s - 1 for s, e in bed[4]) and any(e == s - 1 for s, e in bed[4])         # inverted and zero-length BED lines
    recs = om.crafted_records()
    ivs = [(r[1], om.fragment(r)[3]) for r in recs]
    for tid, regions in enumerate(bed):
        for rs, re in regions:
            if rs >= 1 << 31:
                continue
            for d in (-1, 0, 1):
                assert any(t == tid and iv and iv[0] == re + d for t, iv in ivs), (tid, rs, re, d)     # start at, before and behind r.end
                assert any(t == tid and iv and iv[1] == rs + d for t, iv in ivs), (tid, rs, re, d)     # end at, before and behind r.start
    assert any(iv and iv[1] < iv[0] and not r[0] & 1 for r, (_, iv) in zip(recs, ivs))      # an unpaired record with end < start


def test_crafted_sweep_equals_closed():
    recs = om.crafted_records()
    a, b = om.sweep(recs, om.CRAFTED_BED), om.closed(recs, om.CRAFTED_BED)
    assert a == b
    assert 0 < a[4] < a[3] < a[1] < a[0] and a[2] > 0
    # one record at a time: a difference cannot hide in the sums
    for r in recs:
        assert om.sweep([r], om.CRAFTED_BED) == om.closed([r], om.CRAFTED_BED), r
    # the case a nearest-by-start lookup gets wrong: behind the short region at 5001, inside the long one that began at 101
    assert om.sweep([(0, 3, -1, 6000, 0, 0, 6050)], om.CRAFTED_BED)[4] == 1
    # boundaries (reference 1: [1001, 2000])
    for pos, end_pos, want in ((1999, 2100, 1), (2000, 2100, 0), (900, 1000, 1), (900, 999, 0)):
        assert om.closed([(0, 1, -1, pos, 0, 0, end_pos)], om.CRAFTED_BED)[4] == want, (pos, end_pos)
    assert om.sweep([], om.CRAFTED_BED) == om.closed([], om.CRAFTED_BED) == [0, 0, 0, 0, 0]
    empty = [[] for _ in om.CRAFTED_BED]
    assert om.sweep(recs, empty) == om.closed(recs, empty) == a[:4] + [0]


@pytest.mark.parametrize("seed", range(6))
def test_drawn_sweep_equals_closed(seed):
    rng = random.Random(1000 + seed)
    for _ in range(40):
        n_chr = rng.randrange(1, 5)
        regions = om.drawn_regions(rng, n_chr)
        recs = []
        for _ in range(120):
            tid = rng.randrange(0, n_chr)
            pos = rng.randrange(-2, 3400)
            if rng.random() < 0.5:
                recs.append((rng.choice((0, 16, 1024)), tid, -1, pos, 0, 0, pos + rng.choice((0, 1, 30, 150, -5, -2000))))
            else:
                recs.append((rng.choice((0x41, 0x1, 99, 163)), tid, tid, pos, pos + rng.choice((0, 0, 5, -5)), rng.randrange(-400, 400), pos))
        assert om.sweep(recs, regions) == om.closed(recs, regions)
    recs = om.drawn_records(3000, seed)
    assert om.sweep(recs, om.CRAFTED_BED) == om.closed(recs, om.CRAFTED_BED)


def test_bad_tid_raises_or_is_counted():
    good = (0, 1, -1, 1500, 0, 0, 1600)
    for tid in (-1, len(om.CRAFTED_BED)):
        frag = (0, tid, -1, 10, 0, 0, 20)
        for f in (om.sweep, om.closed):
            with pytest.raises(om.BadTid):
                f([good, frag], om.CRAFTED_BED)
            bad = []
            assert f([good, frag, good], om.CRAFTED_BED, bad=bad) == [3, 3, 0, 3, 2] and bad == [frag]
            # the same tid on records the filters drop: nothing is looked up
            dropped = [(0x4, tid, -1, 10, 0, 0, 20), (0x100, tid, -1, 10, 0, 0, 20), (0x9, tid, tid, 10, 10, 5, 20), (0x41, tid, tid, 10, 10, 5001, 20)]
            assert f(dropped, om.CRAFTED_BED) == [3, 2, 0, 0, 0]


def test_report():
    assert om.report([4, 3, 1, 2, 1]) == (b"Total reads: 4\nAligned reads: 3 (75.0% of all reads)\nDuplicate reads: 1 (33.3% of aligned reads)\n"
                                          b"On-target: 50.0%\n")
    assert om.report([0, 0, 0, 0, 0]) == b"Total reads: 0\nAligned reads: 0 (NaN% of all reads)\nDuplicate reads: 0 (NaN% of aligned reads)\nOn-target: NaN%\n"
    assert om.report([5, 5, 0, 3, 0]).endswith(b"On-target: 0.0%\n")
    assert om.report([5, 5, 0, 3, 0], on_target=False).count(b"\n") == 3
    assert om.parse_bed(b"# c\n\nchr2\t5\t9\n  \nchr1\t0\t1\textra\n", ["chr1", "chr2"]) == [[(1, 1)], [(6, 9)]]
