"""CPU: the streams of tests/bam_decoy.py do what they are named for — they fool the restated guess on the blocks they aim at, the
fooled walk ends as the case says, every stream is a BAM the specification's reader accepts — and the restated rounds reach the plain
walk within the derived bound, whichever way a round's reads and writes are ordered."""
import struct

import numpy as np
import pytest

from tests import bam_decoy as bd
from tests import bam_rewrite_model as rm
from tests import bam_spec

CASES = bd.cases()
N_REFS = (bd.N_REF, -1)


@pytest.fixture(scope="module")
def guesses():
    """{(case, n_ref): {block: its guess}}: a block's guess depends on the stream and n_ref alone"""
    return {(name, n_ref): {} for name in CASES for n_ref in N_REFS}


def test_corpus_size():
    assert sum(len(c.raw) for c in CASES.values()) < 3_000_000
    assert all(len(c.ends) < 600 for c in CASES.values())
    assert all(len(CASES[name].ends) <= 40 and all(d.where == "aux" for d in CASES[name].decoys) for name in bd.FILE_CASES)
    assert len(CASES["long-hop"].ends) > 64 + 40


def test_plain_walk_is_the_searchsorted_statement():
    """what tests/test_gpu_inflate.py computed inline before plain_entries() moved here"""
    for c in CASES.values():
        starts = np.array(c.starts + [len(c.raw)], dtype=np.uint64)
        ends = np.array(c.ends, dtype=np.uint64)
        begins = np.concatenate([[0], ends[:-1]]).astype(np.uint64)
        want = starts[np.searchsorted(starts, np.maximum(begins, c.first))]
        entry, nrec = bd.plain_walk(c.raw, c.first, c.ends)
        assert entry == [int(x) for x in want]
        assert nrec == [int(np.sum((starts[:-1] >= max(int(b), c.first)) & (starts[:-1] < e))) for b, e in zip(begins, ends)]
        assert sum(nrec) == c.n_real


@pytest.mark.parametrize("n_ref", N_REFS)
@pytest.mark.parametrize("name", list(CASES))
def test_the_guess_is_fooled_where_the_case_aims(name, n_ref, guesses):
    c = CASES[name]
    plain = bd.plain_entries(c.raw, c.first, c.ends)
    guessed = bd.guessed_entries(c.raw, c.first, c.ends, n_ref, cache=guesses[name, n_ref])
    for d in c.decoys:
        lo = c.ends[d.block - 1]
        assert lo == d.F and 1 <= d.start - lo <= 300 and not any(c.raw[lo:d.start])          # the block begins in the zeros before the decoy
        assert not bd.plausible(c.raw, lo, n_ref) and c.n_real > d.at
        if d.fools(n_ref):
            assert guessed[d.block] == d.start != plain[d.block]
            assert bd.outcome(c, d, guessed) == d.expect
        else:                                                                                  # the refs contrast: told the count, not fooled
            assert name == "refs" and n_ref == bd.N_REF and guessed[d.block] == plain[d.block]
    assert bd.aimed(c, n_ref) or (name == "refs" and n_ref >= 0)


def test_the_named_outcomes_are_all_there():
    seen = {d.expect if isinstance(d.expect, str) else (d.expect[0], min(d.expect[1], 65), d.expect[2]) for c in CASES.values() for d in c.decoys}
    for want in ("rejoin", "bad record", "truncated", ("hop", 1, "record start"), ("hop", 3, "inside"), ("hop", 3, "record start"),
                 ("hop", 65, "record start"), ("hop", 65, "inside")):
        assert want in seen, want
    assert any(e[0] == "hop" and e[2] == "decoy start" for e in seen if not isinstance(e, str))
    assert {d.block for d in CASES["wave-edge"].decoys} == {63, 64, 255, 256}
    blocks = sorted(d.block for d in CASES["neighbours"].decoys)
    assert blocks[1] == blocks[0] + 1                                                          # two fooled blocks in a row
    c, d = CASES["neighbours"], CASES["neighbours"].decoys[-1]
    sizes = [c.ends[k] - c.ends[k - 1] for k in range(d.block + 1, d.block + 1 + len(d.tiny))]
    assert sizes == list(d.tiny) and c.ends[d.block + len(d.tiny)] < d.host_end                # then blocks of a few bytes inside the host
    for name, n in (("stream-end-2", 2), ("stream-end-3", 3)):                                 # the fake that ends where the stream ends
        (d,) = CASES[name].decoys
        assert d.n_fakes == n and d.end == len(CASES[name].raw)
    assert {d.where for c in CASES.values() for d in c.decoys} == {"aux", "qual"}


@pytest.mark.parametrize("name", list(CASES))
def test_every_stream_is_a_bam(name, tmp_path):
    c = CASES[name]
    path = tmp_path / "c.bam"
    path.write_bytes(rm.bgzf(c.raw, cuts=c.ends))
    assert [len(x) for x in bam_spec.bgzf_blocks(path.read_bytes())] == [b - a for a, b in zip([0] + c.ends[:-1], c.ends)] + [0]
    refs, recs = bam_spec.read_bam(str(path))
    assert refs == [(n.decode(), ln) for n, ln in bd.REFS] and len(recs) == c.n_real == len(c.recs)
    for got, rec in zip(recs, c.recs):
        tid, pos, l_name, mapq, _bin, n_cigar, flag, l_seq, mtid, mpos, tlen = struct.unpack_from("<iiBBHHHiiii", rec, 4)
        assert len(rec) == 4 + struct.unpack_from("<i", rec)[0]
        assert got == dict(refID=tid, pos=pos, mapq=mapq, flag=flag, l_seq=l_seq, next_refID=mtid, next_pos=mpos, tlen=tlen, n_cigar=n_cigar,
                           name=rec[36:36 + l_name - 1])
        assert 0 <= tid < bd.N_REF and rec[36 + l_name - 1] == 0
    assert sum(1 for r in c.recs if r[36:40] == b"host") == len(c.decoys)


@pytest.mark.parametrize("order", ["before", "after"])
@pytest.mark.parametrize("n_ref", N_REFS)
@pytest.mark.parametrize("name", list(CASES))
def test_the_rounds_reach_the_plain_walk_within_the_bound(name, n_ref, order, guesses):
    """the first block whose entry is wrong has a predecessor whose entry is right and is therefore not rewritten in the round: every
    round puts the first wrong block right, so n - 1 rounds correct and one confirms"""
    c = CASES[name]
    got = bd.simulate(c.raw, c.first, c.ends, n_ref, order, cache=guesses[name, n_ref])
    entry, nrec = bd.plain_walk(c.raw, c.first, c.ends)
    assert got["verified"] and got["n_records"] == c.n_real
    assert got["entry"] == entry and got["nrec"] == nrec
    assert got["rounds"] <= len(c.ends) + 1


@pytest.mark.parametrize("n_ref", N_REFS)
@pytest.mark.parametrize("name", bd.BROKEN_OF)
def test_broken_streams_are_not_verified(name, n_ref):
    c = CASES[name]
    for what, raw, length in bd.broken(c):
        ends = c.ends[:-1] + [length]
        for d in c.decoys:
            assert raw[d.start:d.end] == c.raw[d.start:d.end]
        for order in ("before", "after"):
            got = bd.simulate(raw, c.first, ends, n_ref, order, length=length)
            assert not got["verified"] and got["rounds"] <= len(ends) + 1, what


def test_a_long_hop_outlasts_the_cap_when_reads_come_before_writes(guesses):
    """the wrong exit moves one block a round and the correction follows one block behind: more than 64 rounds, so the file call
    declines; taken in order the same stream settles in two"""
    c = CASES["long-hop"]
    assert bd.simulate(c.raw, c.first, c.ends, bd.N_REF, "before", cache=guesses["long-hop", bd.N_REF])["rounds"] > 64
    assert bd.simulate(c.raw, c.first, c.ends, bd.N_REF, "after", cache=guesses["long-hop", bd.N_REF])["rounds"] == 2
    for order in ("before", "after"):
        got = bd.simulate(c.raw, c.first, c.ends, bd.N_REF, order, max_rounds=1, cache=guesses["long-hop", bd.N_REF])
        assert not got["verified"] and got["rounds"] == 1
    got = bd.simulate(c.raw, c.first, c.ends, bd.N_REF, "before", max_rounds=8, cache=guesses["long-hop", bd.N_REF])
    assert not got["verified"] and got["rounds"] == 8


def test_bgzf_cuts_beside_piece():
    raw = bytes(range(256)) * 40
    assert rm.bgzf(raw, piece=1000) == rm.bgzf(raw, cuts=list(range(1000, len(raw), 1000)) + [len(raw)])
    cuts = [1, 7, 5000, len(raw)]
    assert [len(x) for x in bam_spec.bgzf_blocks(rm.bgzf(raw, cuts=cuts))] == [1, 6, 4993, len(raw) - 5000, 0]
    assert b"".join(bam_spec.bgzf_blocks(rm.bgzf(raw, cuts=cuts))) == raw
    with pytest.raises(AssertionError):
        rm.bgzf(raw, cuts=[5, 10])


def test_the_densest_blocks():
    raw, first, ends, recs = bd.dense_stream()
    entry, nrec = bd.plain_walk(raw, first, ends)
    assert [b - a for a, b in zip(ends, ends[1:-1])] == [65536] * 3 and len(recs) == sum(nrec)
    assert nrec[1] == 1821 and entry[1] == ends[0] + 4 and entry[1] + 65520 < ends[1] <= entry[1] + 65520 + 36
    assert nrec[2] == 1820 and nrec[3] == 1821 and entry[3] + 36 * 1820 == entry[3] + 65520 < ends[3]
    assert max(nrec) <= 1824                                                                   # kBlockRecs (sk_bamblock.h)
    recs38 = bd.dense_file_records()
    assert all(len(r) == 38 for r in recs38)
    raw = rm.header(bd.TEXT, bd.REFS) + b"".join(recs38)
    ends = list(range(65536, len(raw), 65536)) + [len(raw)]
    _, nrec = bd.plain_walk(raw, len(raw) - 38 * len(recs38), ends)
    assert len(ends) >= 4 and all(n in (1724, 1725) for n in nrec[1:-1]) and 1725 in nrec[1:-1]
