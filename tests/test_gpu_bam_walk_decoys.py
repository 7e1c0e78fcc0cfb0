"""GPU: the BAM record walk (sk_bam_walk_dev: bam_walk_kernel, bam_walk_guess_kernel, bam_walk_fix_kernel) on the streams of
tests/bam_decoy.py, which fool its guess, and on the densest blocks a BAM can hold — against ONE sequential walk of the block_size
fields (bam_decoy.plain_walk), the oracle and the specification's reader over the real records only.  Then the same streams as BGZF
files through five file calls, each against its existing model.  tests/test_bam_decoy_model.py shows on the CPU that the streams do
fool the guess; nothing expected here comes from the restated kernels."""
import random
import struct

import numpy as np
import pytest

from tests import bam_decoy as bd
from tests import bam_rewrite_model as rm
from tests import bam_spec
from tests.bam_coverage_model import literal as coverage_literal
from tests.test_gpu_bam_columns import expect_from_raw
from tests.test_gpu_bam_coverage import check as coverage_check
from tests.test_gpu_bam_reads import collect as reads_collect
from tests.test_gpu_bam_reads import model as reads_model
from tests.bam_out_util import checked_windows
from tests.test_gpu_inflate import Dev

pytestmark = pytest.mark.gpu

CASES = bd.cases()
N_REFS = (bd.N_REF, -1)
MAX_FRAG = 5000


def core_columns(recs):
    """flag, tid, mtid, tlen of records given as bytes"""
    f = [struct.unpack_from("<H", r, 18)[0] for r in recs]
    t = [struct.unpack_from("<i", r, 4)[0] for r in recs]
    m = [struct.unpack_from("<i", r, 24)[0] for r in recs]
    tl = [struct.unpack_from("<i", r, 32)[0] for r in recs]
    return np.array(f, np.uint16), np.array(t, np.int32), np.array(m, np.int32), np.array(tl, np.int32)


def walk(ctx, d, raw, length, ends, first, n_ref, max_rounds=100000):
    """sk_bam_walk_dev on caller buffers: (verified, n_records, rounds, entry[n], nrec[n], the buffers)"""
    n = len(ends)
    d_stream = d.put(np.frombuffer(raw, dtype=np.uint8))
    d_ends = d.put(np.array(ends, dtype=np.uint64).view(np.uint8))
    d_entry, d_exit, d_nrec = d.empty(8 * (n + 1)), d.empty(8 * (n + 1)), d.empty(4 * (n + 2))
    verified, n_records, rounds = ctx.bam_walk_dev(d_stream, length, d_ends, n, first, d_entry, d_exit, d_nrec, max_rounds=max_rounds, n_ref=n_ref)
    return verified, n_records, rounds, d.get(d_entry, n, np.uint64), d.get(d_nrec, n, np.uint32), (d_stream, d_ends, d_entry)


def check_walk_and_reduce(ctx, oracle, raw, first, ends, n_ref, flag, tid, mtid, tlen, note):
    want_entry, want_nrec = bd.plain_walk(raw, first, ends)
    n = len(ends)
    d = Dev(ctx)
    try:
        verified, n_records, rounds, entry, nrec, (d_stream, d_ends, d_entry) = walk(ctx, d, raw, len(raw), ends, first, n_ref)
        note(rounds)
        assert verified and n_records == len(flag), (verified, n_records, rounds)
        assert np.array_equal(entry, np.array(want_entry, dtype=np.uint64)), np.flatnonzero(entry != np.array(want_entry, dtype=np.uint64))
        assert np.array_equal(nrec, np.array(want_nrec, dtype=np.uint32))
        assert rounds <= n + 1, rounds                      # derived (tests/test_bam_decoy_model.py), not measured
        d_out = d.put(np.zeros(4 + MAX_FRAG + 1, dtype=np.uint64).view(np.uint8))
        ctx.bam_walk_reduce_dev(d_stream, len(raw), d_ends, d_entry, n, MAX_FRAG, d_out)
        got = d.get(d_out, 4 + MAX_FRAG + 1, np.uint64)
    finally:
        d.close()
    e_counters, e_hist, e_total = oracle.bam_flag_tlen(flag, tid, mtid, tlen, MAX_FRAG)
    assert (got[:3] == e_counters).all() and got[3] == e_total and (got[4:] == e_hist).all()
    assert tuple(int(x) for x in got[:3]) == tuple(bam_spec.statistics([dict(flag=int(f)) for f in flag]))


# ---- the stream ----
@pytest.mark.parametrize("n_ref", N_REFS)
@pytest.mark.parametrize("name", list(CASES))
def test_walk_on_decoys_equals_the_plain_walk(ctx, oracle, record_property, name, n_ref):
    c = CASES[name]

    def note(rounds):
        record_property("rounds", rounds)
        print(f"decoy rounds: {name} n_ref={n_ref}: {rounds} rounds over {len(c.ends)} blocks")
    check_walk_and_reduce(ctx, oracle, c.raw, c.first, c.ends, n_ref, *core_columns(c.recs), note)


@pytest.mark.parametrize("n_ref", N_REFS)
@pytest.mark.parametrize("name", bd.BROKEN_OF)
def test_broken_decoy_streams_are_not_verified(ctx, name, n_ref):
    c = CASES[name]
    for what, raw, length in bd.broken(c):
        d = Dev(ctx)
        try:
            verified, n_records, rounds, *_ = walk(ctx, d, raw, length, c.ends[:-1] + [length], c.first, n_ref)
        finally:
            d.close()
        assert not verified and n_records == 0 and rounds <= len(c.ends) + 1, (what, rounds)


@pytest.mark.parametrize("name", ["long-hop", "long-hop-qual"])
def test_the_walk_stops_at_max_rounds(ctx, record_property, name):
    """a hop over more than 64 blocks does not settle in 8 rounds (the wrong exit moves one block a round within a wave): the walk
    stops where it is told to and does not report a half-settled chain"""
    c = CASES[name]
    d = Dev(ctx)
    try:
        verified, n_records, rounds, *_ = walk(ctx, d, c.raw, len(c.raw), c.ends, c.first, bd.N_REF, max_rounds=8)
    finally:
        d.close()
    assert not verified and n_records == 0 and rounds == 8


def test_walk_on_the_densest_blocks(ctx, oracle, record_property):
    """1 821 records of 36 bytes begin in a block of 65 536 bytes whose entry is its 5th byte; the last begins 65 520 bytes behind it"""
    raw, first, ends, recs = bd.dense_stream()
    col = lambda k, dt: np.array([r[k] for r in recs], dtype=dt)

    def note(rounds):
        record_property("rounds", rounds)
        print(f"decoy rounds: densest blocks: {rounds} rounds over {len(ends)} blocks")
    for n_ref in N_REFS:
        check_walk_and_reduce(ctx, oracle, raw, first, ends, n_ref, col("flag", np.uint16), col("refID", np.int32), col("next_refID", np.int32),
                              col("tlen", np.int32), note)


# ---- the file ----
def five_calls(ctx, path, raw, may_decline=False):
    """sk_bam_file_reduce, _columns, _rewrite (trim qnames), _reads (fastq) and _coverage on one file, each against its model; with
    may_decline a call may instead leave the file to the caller at check 20 with nothing written.  Returns how many were handled."""
    path = str(path)
    first = rm.header_end(raw)
    n_real = sum(1 for _ in rm.records(raw))
    _, spec = bam_spec.read_bam(path)
    assert len(spec) == n_real
    served = 0

    def declined(handled, info, outputs_zero):
        if handled:
            return False
        assert may_decline and info[5] == -20 and outputs_zero, info
        return True

    handled, counters, hist, total, info = ctx.bam_file_reduce(path, MAX_FRAG)
    if not declined(handled, info, not counters.any() and not hist.any() and total == 0):
        e_hist = bam_spec.fragment_lengths(spec, MAX_FRAG)
        assert tuple(int(x) for x in counters) == tuple(bam_spec.statistics(spec))
        assert [int(x) for x in hist] == e_hist[0] and total == e_hist[1] and info[3] == n_real
        served += 1
    handled, cols, names, info = ctx.bam_file_columns(path)
    if not declined(handled, info, cols == {} and names == []):
        expect = expect_from_raw(raw, first)
        assert info[3] == n_real == len(expect["flag"]) and names == [n for n, _ in bd.REFS]
        for k in expect:
            assert np.array_equal(cols[k], expect[k]), k
        served += 1
    handled, out, _, _, info = checked_windows(ctx, ctx.bam_file_rewrite(path, "trim qnames", 1, 0), rm)      # (asserts the zeros of a declined call)
    if not declined(handled, info, True):
        exp, code = rm.model(raw, "trim qnames")
        assert code is None and out == exp and info[3] == n_real
        served += 1
    handled, n_kept, text_bytes, info = ctx.bam_file_reads(path, "fastq")
    if not declined(handled, info, n_kept == 0 and text_bytes == 0):
        ok, (rows, _), info = reads_collect(ctx, path, "fastq")
        assert ok and [(k, n, t) for k, n, t, _ in rows] == reads_model(bd.read_dicts(raw), "fastq", True) and info[3] == n_real
        served += 1
    handled, hist, n_pos, n_drop, n_counted, info = ctx.bam_file_coverage(path, 0, [])
    if not declined(handled, info, not hist.any() and (n_pos, n_drop, n_counted) == (0, 0, 0)):
        coverage_check(ctx, path, raw, ("everywhere",), model=coverage_literal)      # (asserts info[3] too)
        served += 1
    return served


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("decoys")
    out = {}
    for name in bd.FILE_CASES + ("long-hop",):
        out[name] = tmp / (name + ".bam")
        out[name].write_bytes(rm.bgzf(CASES[name].raw, cuts=CASES[name].ends))
    return out


@pytest.mark.parametrize("name", bd.FILE_CASES)
def test_file_calls_on_decoys_are_handled(ctx, files, name):
    """at most 40 blocks: the derived bound keeps the rounds under the file calls' cap of 64"""
    assert len(CASES[name].ends) <= 40
    assert five_calls(ctx, files[name], CASES[name].raw) == 5


def test_file_calls_on_the_long_hop(ctx, files, monkeypatch):
    """more rounds than the cap when reads come before writes, two when they come behind: handled and right, or declined at check 20
    with nothing written — and which of the two is not asserted.  With one round allowed it must decline, and nothing of the
    declined call lingers: an ordinary file on the same context is served and right."""
    raw = CASES["long-hop"].raw
    served = five_calls(ctx, files["long-hop"], raw, may_decline=True)
    print(f"decoy long hop: {served} of 5 file calls handled")
    with monkeypatch.context() as m:
        m.setenv("SK_BAMFILE_MAX_ROUNDS", "1")
        handled, counters, hist, total, info = ctx.bam_file_reduce(str(files["long-hop"]), MAX_FRAG)
        assert not handled and info[5] == -20 and not counters.any() and not hist.any() and total == 0
        handled, cols, names, info = ctx.bam_file_columns(str(files["long-hop"]))
        assert not handled and info[5] == -20 and cols == {}
        assert five_calls(ctx, files["long-hop"], raw, may_decline=True) == 0
    p = files["long-hop"].parent / "ordinary.bam"
    raw1 = rm.write(p, [bd.real_record(i, random.Random(i)) for i in range(400)], text=bd.TEXT, refs=bd.REFS, piece=3000)
    assert five_calls(ctx, p, raw1) == 5


def test_file_calls_on_the_densest_blocks(ctx, tmp_path):
    """blocks of exactly 65 536 inflated bytes of 38-byte records: 1 725 records begin in a block, and the lane loops of the block
    passes turn 27 times.  (Whether the device inflater or zlib takes such a block is printed, not asserted.)"""
    recs = bd.dense_file_records()
    path = tmp_path / "dense.bam"
    raw = rm.write(path, recs, text=bd.TEXT, refs=bd.REFS, piece=65536)
    assert [len(x) for x in bam_spec.bgzf_blocks(path.read_bytes())][:3] == [65536] * 3
    assert five_calls(ctx, path, raw) == 5
    info = ctx.bam_file_reduce(str(path), MAX_FRAG)[4]
    print(f"decoy densest file: {int(info[2])} blocks, {int(info[4])} by zlib, {int(info[5])} rounds")
