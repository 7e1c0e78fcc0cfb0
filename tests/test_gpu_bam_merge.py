"""GPU: sk_bam_file_merge / sk_bam_file_rewrite_next — `sam merge` with every input's stream resident, the records of all inputs sorted by
(key, input, place) and the output BGZF-compressed on the device — against the plain-Python loop of tests/bam_merge_model.py."""
import functools
import struct
import zlib

import pytest

from tests import bam_merge_model as m
from tests import bam_minimize_model as mm
from tests import bam_subsample_model as sm
from tests.bam_out_util import checked_windows, zlib_members

pytestmark = pytest.mark.gpu


def write_all(d, files, **kw):
    paths = [d / ("in%d.bam" % (i + 1)) for i in range(len(files))]
    return [str(p) for p in paths], [m.write(p, recs, **kw) for p, recs in zip(paths, files)]


def collect(ctx, paths, suffix=False, level=1, window_bytes=0):
    """(handled, inflated output or info, members, windows, records)"""
    res = ctx.bam_file_merge(paths, suffix, level, window_bytes)
    handled, out, mem, n_win, info = checked_windows(ctx, res, m)
    return handled, out if handled else info, mem, n_win, res[1]


def check(ctx, paths, raws, suffix=False, level=1, window_bytes=0):
    exp, err, code = m.model(raws, suffix)
    assert (err, code) == (b"", 0)
    handled, out, mem, n_win, n_rec = collect(ctx, paths, suffix, level, window_bytes)
    assert handled, out
    assert out == exp and n_rec == sum(len(list(m.records(r))) for r in raws)
    return out, mem, n_win


SIZES = [3000, 0, 1, 2500, 300, 7, 64, 65, 1000, 2, 0, 128, 500, 33, 1, 900]


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """16 files of 0, 1 and up to 3 000 records in 12 KiB pieces (records straddle blocks), half of their keys shared, unmapped tails"""
    d = tmp_path_factory.mktemp("merge")
    return write_all(d, m.served_inputs(16, SIZES, seed=11), piece=0x3000)


@functools.lru_cache(maxsize=None)
def _expected(raws, suffix):
    return m.model(list(raws), suffix)


@pytest.mark.parametrize("suffix", [False, True])
@pytest.mark.parametrize("window", [0, 256, 64 << 10])
@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("k", [2, 3, 16])
def test_merge_matches_model(ctx, inputs, k, level, window, suffix):
    paths, raws = inputs
    exp, err, code = _expected(tuple(raws[:k]), suffix)
    assert (err, code) == (b"", 0)
    handled, out, mem, n_win, n_rec = collect(ctx, paths[:k], suffix, level, window)
    assert handled, out
    assert out == exp and n_rec == sum(SIZES[:k])
    if level == 0:
        assert all(stored for _, stored in mem[:-1])
    elif window != 256:                                                                # (a window of 256 bytes is one member that a dynamic block does not shrink: stored)
        assert not all(stored for _, stored in mem[:-1])                               # (the device deflated what shrinks)
    if window == 256:
        assert n_win > n_rec // 3
    if suffix and k == 16:
        assert {b"1", b"9", b"10", b"16"} <= {r[36:36 + r[12] - 1].rsplit(b".", 1)[1] for r in m.records(out)}


def test_every_member_passes_zlib(ctx, inputs):
    paths, raws = inputs
    for level, suffix in ((0, True), (1, False), (1, True)):
        handled, n_rec, raw_bytes, _ = ctx.bam_file_merge(paths[:5], suffix, level, 1 << 18)
        assert handled
        data = b"".join(w["bgzf"] for w in ctx.bam_file_rewrite_windows())
        out = b"".join(zlib_members(data))
        assert out == _expected(tuple(raws[:5]), suffix)[0] and len(out) == raw_bytes


@pytest.mark.parametrize("shared", [1.0, 0.5, 0.0])
def test_ties(ctx, tmp_path, shared):
    """every record of every input on one key: input 1, then input 2 ..; half the keys shared; none shared: the sort of all records"""
    files = m.served_inputs(4, [1500, 700, 1200, 300], shared=shared, seed=int(shared * 10) + 1)
    paths, raws = write_all(tmp_path, files, piece=0x3000)
    out, _, _ = check(ctx, paths, raws, window_bytes=64 << 10)
    recs = list(m.records(out))
    if shared == 1.0:
        assert recs == files[0] + files[1] + files[2] + files[3]
    if shared == 0.0:
        assert recs == m.sorted_by_key([r for f in files for r in f])
        back = check(ctx, paths[::-1], raws[::-1])[0]
        assert list(m.records(back)) == recs
    check(ctx, paths, raws, suffix=True)


def test_key_edges(ctx, tmp_path):
    """pos = -1 on a mapped reference, pos = 2^31 - 1, refID = -1 behind the highest of 200 references; and a single reference"""
    def rec(tid, pos, name):
        return m.placed(m.rm.record(name, 7), tid, pos)
    refs = [(b"r%d" % i, 1000 + i) for i in range(200)]
    a = [rec(0, -1, b"a0"), rec(0, 0, b"a1"), rec(0, 2**31 - 1, b"a2"), rec(2, 5, b"a3"), rec(199, -1, b"a4"), rec(199, 2**31 - 1, b"a5"), rec(-1, -1, b"a6"),
         rec(-1, -1, b"a7")]
    b = [rec(0, 0, b"b0"), rec(1, -1, b"b1"), rec(2, 2**31 - 1, b"b2"), rec(199, 0, b"b3"), rec(-1, -1, b"b4"), rec(-1, 0, b"b5")]
    c = [rec(-1, -1, b"c0"), rec(-1, 2**31 - 1, b"c1")]
    paths, raws = write_all(tmp_path, [a, b, c], refs=refs, text=b"@HD\tVN:1.6\n")
    out, _, _ = check(ctx, paths, raws)
    assert [r[36:38] for r in m.records(out)] == [b"a0", b"a1", b"b0", b"a2", b"b1", b"a3", b"b2", b"a4", b"b3", b"a5", b"a6", b"a7", b"b4", b"c0", b"b5", b"c1"]
    check(ctx, paths, raws, suffix=True)
    one = [(b"only", 5000)]
    files = m.served_inputs(3, 400, n_refs=1, seed=3)
    paths, raws = write_all(tmp_path, files, refs=one, text=b"")
    check(ctx, paths, raws, suffix=True)


def test_suffix_on_every_name_length_and_record_residue(ctx, tmp_path):
    """names of 1 byte up to the longest that takes ".1" (252) and ".10" (251), record lengths of every residue mod 4 at every place mod 4
    of the output: the edges of the dword copy"""
    files = []
    for f in range(11):
        longest = 252 if f < 9 else 251
        recs = []
        for i in range(260):
            nl = 1 + (i * 7 + f) % longest if i else longest
            recs.append(m.rm.record(bytes(65 + (i + k) % 26 for k in range(nl)), (i + f) % 9, tid=0, pos=10 * i + f, aux=m.rm.aux_z(b"ZZ", b"y" * (i % 5)) if i % 5 else b"", seed=i))
        files.append(recs)
    assert {len(r) % 4 for f in files for r in f} == {0, 1, 2, 3}
    assert {r[12] - 1 for r in files[0]} >= {1, 252} and max(r[12] - 1 for r in files[10]) == 251
    paths, raws = write_all(tmp_path, files)
    for window in (0, 256):
        check(ctx, paths, raws, suffix=True, level=0, window_bytes=window)
    check(ctx, paths, raws, suffix=False, level=0)


def declined(ctx, paths, bits, suffix=False):
    handled, info, _, n_win, n_rec = collect(ctx, paths, suffix)                      # (checked_windows: every count is 0)
    assert not handled and info[5] == -(30 + bits) and n_win == 0 and n_rec == 0
    from seqkit_amd.capi import SeqkitHipError
    with pytest.raises(SeqkitHipError):                                               # no windows were set up
        next(ctx.bam_file_rewrite_windows())


def test_declines(ctx, tmp_path):
    files = m.served_inputs(3, 500, seed=21, unmapped_tail=False)
    paths, raws = write_all(tmp_path, files, piece=0x3000)
    check(ctx, paths, raws)
    # an unsorted input
    bad = list(files[1])
    bad[200], bad[201] = m.placed(bad[200], 1, 500), m.placed(bad[201], 1, 499)
    p = tmp_path / "unsorted.bam"
    m.write(p, bad, piece=0x3000)
    declined(ctx, [paths[0], str(p), paths[2]], 2)
    # the unsorted place exactly at a block boundary: records of equal size, a whole number of them per block
    recs = [m.rm.record(b"n%05d" % i, 10, tid=0, pos=i) for i in range(600)]
    size = len(recs[0])
    assert all(len(r) == size for r in recs)
    hdr = len(m.rm.header(m.rm.TEXT, m.rm.REFS))
    per = 100
    piece = per * size
    pad = (-hdr) % piece                                                              # header and padding text fill whole pieces
    text = m.rm.TEXT + b"\0" * pad
    assert len(m.rm.header(text, m.rm.REFS)) % piece == 0
    at = 3 * per                                                                      # the first record of a block
    recs[at] = m.placed(recs[at], 0, at - 2)
    p2 = tmp_path / "boundary.bam"
    raw = m.write(p2, recs, text=text, piece=piece)
    assert (raw.index(recs[at]) % piece) == 0
    declined(ctx, [paths[0], str(p2)], 2)
    declined(ctx, [str(p2), paths[0]], 2)
    # a name too long only with its suffix
    long = list(files[2])
    long[77] = m.rm.record(b"n" * 253, 10, tid=m.key(long[77])[0], pos=m.key(long[77])[1])
    p3 = tmp_path / "long.bam"
    raw3 = m.write(p3, long, piece=0x3000)
    declined(ctx, [paths[0], str(p3)], 1, suffix=True)
    check(ctx, [paths[0], str(p3)], [raws[0], raw3])
    # reference names that differ, and another count of them
    p4, p5 = tmp_path / "names.bam", tmp_path / "fewer.bam"
    m.write(p4, files[1], refs=m.rm.REFS[:2] + [(b"chrX", 16569)])
    m.write(p5, [r for r in files[1] if m.key(r)[0] < 2], refs=m.rm.REFS[:2])
    declined(ctx, [paths[0], str(p4)], 4)
    declined(ctx, [paths[0], paths[2], str(p5)], 4)
    p6 = tmp_path / "lengths.bam"
    raw6 = m.write(p6, files[1], refs=[(n, ln + 1) for n, ln in m.rm.REFS])
    check(ctx, [paths[0], str(p6)], [raws[0], raw6])                                  # equal names, other lengths: merged
    # an invalid record: l_seq larger than the record holds
    inv = list(files[1])
    b = bytearray(inv[300])
    struct.pack_into("<i", b, 20, 4000)
    inv[300] = bytes(b)
    p7 = tmp_path / "invalid.bam"
    m.write(p7, inv, piece=0x3000)
    declined(ctx, [paths[0], str(p7)], 8)
    # a path that is not a regular file, and one that is not there
    handled, info, _, _, _ = collect(ctx, [paths[0], str(tmp_path)])
    assert not handled and info[5] < 0
    handled, info, _, _, _ = collect(ctx, [str(tmp_path / "none.bam"), paths[0]])
    assert not handled and info[5] < 0
    check(ctx, paths, raws, suffix=True)


def test_invalid_arguments(ctx, inputs):
    from seqkit_amd.capi import SeqkitHipError
    paths, _ = inputs
    for args in ((paths[:1], False, 1), ([], False, 1), (paths[:2], False, 2), (paths[:2], True, -1)):
        with pytest.raises(SeqkitHipError, match=r"failed \(-1\)"):                  # SK_ERR_INVALID
            ctx.bam_file_merge(*args)
    handled, n_rec, raw_bytes, info = ctx.bam_file_merge([paths[i % 16] for i in range(100)])
    assert not handled and info[5] == -21 and (n_rec, raw_bytes) == (0, 0)


def test_the_ctx_is_left_as_found(ctx, inputs, tmp_path):
    """minimize --read-ids and subsample give identical bytes before and after merge calls; a merge started while an earlier merge's
    windows are unread disturbs neither"""
    paths, raws = inputs
    mpath, spath = tmp_path / "min.bam", tmp_path / "sub.bam"
    mm.write(mpath, mm.served_records(4000, seed=3))
    sm.write(spath, sm.served_records(4000, seed=3))

    def others():
        a = ctx.bam_file_minimize(str(mpath), True, False, False, 255, 1, 0)
        wa = [[x for x, _ in m.members(w["bgzf"])] for w in ctx.bam_file_rewrite_windows()]     # (the inflated bytes, window by window)
        b = ctx.bam_file_subsample(str(spath), 0.5, 9, 1, 0)
        wb = [[x for x, _ in m.members(w["bgzf"])] for w in ctx.bam_file_rewrite_windows()]
        assert a[0] and b[0]
        return a[:-1], wa, b[:-1], wb
    before = others()
    exp16, exp3 = _expected(tuple(raws), True)[0], _expected(tuple(raws[:3]), False)[0]
    res = ctx.bam_file_merge(paths, True, 1, 4096)
    assert res[0]
    it = ctx.bam_file_rewrite_windows()
    part = [next(it)["bgzf"] for _ in range(5)]                                       # windows in flight, then another merge on the ctx
    assert exp16.startswith(b"".join(x for x, _ in m.members(b"".join(part))))
    handled, out, _, _, _ = collect(ctx, paths[:3], False, 1, 4096)
    assert handled and out == exp3
    handled, out, _, _, _ = collect(ctx, paths, True, 1, 4096)
    assert handled and out == exp16
    assert others() == before
    res = ctx.bam_file_merge(paths[:3], False, 1, 256)                                # and left with windows unread
    assert res[0] and next(ctx.bam_file_rewrite_windows())["bgzf"]
    assert others() == before


def test_merge_scratch_in_the_first_compressed_files_buffer_or_its_own(ctx, tmp_path, monkeypatch, capfd):
    """the sort's buffers and the columns (29 B per record of all inputs and the sort's own scratch) lie in the idle buffer of input 1's
    compressed file when they fit, else in memory of their own; the placements arise from the files.  Inputs of 3 000 and 2 500 records,
    input 1 under a header text of 4 MiB that does not compress: its buffer.  An input 1 of 300 records in front of the 2 500: memory
    of its own, whatever the sort asks for on top.  (Input 1 under the default header takes 0.30 MB against 0.16 MB of scratch — its
    records do not compress below that — so that pair alone never reaches the second placement; it is merged and compared all the
    same.)  The model's output every time, with and without the suffix, whose input numbers stay in the call's own buffer throughout."""
    import os
    import random
    rnd = random.Random(9)
    text = b"@CO\t" + bytes(rnd.randrange(33, 127) for _ in range(4 << 20)) + b"\n"
    files = m.served_inputs(2, [3000, 2500], seed=5)
    few = m.served_inputs(2, [300, 1], seed=6)[0]
    small, large, tiny, second = tmp_path / "small.bam", tmp_path / "large.bam", tmp_path / "tiny.bam", tmp_path / "second.bam"
    raw_small, raw_large, raw_second = m.write(small, files[0]), m.write(large, files[0], text=text), m.write(second, files[1])
    raw_tiny = m.write(tiny, few)
    assert os.path.getsize(tiny) + 64 < 29 * (300 + 2500)                              # (input 1's buffer against the seven columns alone)
    monkeypatch.setenv("SK_BAMFILE_TRACE", "1")
    capfd.readouterr()
    for first, raw_first, where in ((small, raw_small, None), (tiny, raw_tiny, "its own buffer"), (large, raw_large, "the first compressed file's buffer"),
                                    (tiny, raw_tiny, "its own buffer")):
        for suffix in (False, True):
            check(ctx, [str(first), str(second)], [raw_first, raw_second], suffix)
            lines = [ln for ln in capfd.readouterr().err.split("\n") if "bytes of scratch in" in ln]
            assert len(lines) == 1 and lines[0].startswith("sk_bam_file_merge: 2 inputs, ")
            print(lines[0])
            if where:
                assert lines[0].endswith("bytes of scratch in " + where)
