"""GPU: sk_bam_file_recalc_tlen / sk_bam_file_recalc_tlen_discarded / sk_bam_file_rewrite_next — `sam recalculate tlen` with the records
classified, the mates linked (hash, sort, runs), the pairs' TLENs computed, the written records compacted and BGZF-compressed on the
device — against the plain-Python model of tests/bam_recalc_tlen_model.py."""
import struct

import pytest

from tests import bam_recalc_tlen_model as m
from tests.bam_out_util import checked_windows, zlib_members

pytestmark = pytest.mark.gpu

MAX_LENS = [1, 5000, 1 << 40]


def collect(ctx, path, max_len, level=1, window_bytes=0):
    """(handled, inflated output or info, members, windows, records written, records discarded); the windows are checked by
    tests/bam_out_util.checked_windows (order, first and n over the WRITTEN records, raw_bytes, the EOF block)"""
    res = ctx.bam_file_recalc_tlen(str(path), max_len, level, window_bytes)
    handled, out, mem, n_win, info = checked_windows(ctx, res, m)
    return handled, out if handled else info, mem, n_win, res[1], res[2]


def check(ctx, path, raw, max_len, level=1, window_bytes=0):
    """the call against the model: the output's bytes, both counts, and the discarded names fetched whole after the last window"""
    hdr, written, lone = m.grouped_parts(raw, max_len)
    assert m.literal(raw, max_len) == m.grouped(raw, max_len)
    handled, out, mem, n_win, n_rec, n_disc = collect(ctx, path, max_len, level, window_bytes)
    assert handled, out
    assert out == hdr + b"".join(written) and (n_rec, n_disc) == (len(written), len(lone))
    assert ctx.bam_file_recalc_tlen_discarded(0, n_disc) == lone
    return mem, n_win, len(written), lone


@pytest.fixture(scope="module")
def bam(tmp_path_factory):
    path = tmp_path_factory.mktemp("recalc_tlen") / "in.bam"
    return path, m.write(path, m.served_records(3000, seed=1))


@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("window", [0, 64 << 10])
@pytest.mark.parametrize("max_len", MAX_LENS)
def test_recalc_tlen_matches_model(ctx, bam, level, window, max_len):
    path, raw = bam
    mem, n_win, n_rec, lone = check(ctx, path, raw, max_len, level, window)
    assert n_rec > 2000 and len(lone) > 100
    if level == 0:
        assert all(stored for _, stored in mem[:-1])
    else:
        assert not all(stored for _, stored in mem[:-1])                               # (the device deflated what shrinks)
    if window:
        assert n_win > 3


def test_small_windows_and_input_blocks(ctx, tmp_path):
    """600 records in input blocks of 12 KiB; windows of 256 bytes, so that every window holds a record or two"""
    path = tmp_path / "small.bam"
    raw = m.write(path, m.served_records(600, seed=7), piece=0x3000)
    for max_len in MAX_LENS:
        for level in (0, 1):
            mem, n_win, n_rec, _ = check(ctx, path, raw, max_len, level, 256)
            assert n_win > n_rec // 4


def test_every_member_passes_zlib(ctx, bam):
    path, raw = bam
    for level in (0, 1):
        handled, n_rec, n_disc, raw_bytes, _ = ctx.bam_file_recalc_tlen(str(path), 5000, level, 1 << 20)
        assert handled
        data = b"".join(w["bgzf"] for w in ctx.bam_file_rewrite_windows())
        out = b"".join(zlib_members(data))
        assert out == m.grouped(raw, 5000)[0] and len(out) == raw_bytes


def test_discarded_names_in_ranges(ctx, bam):
    """whole, in ranges cut at odd places, with n = 0, before the first window, between windows and after the last; a range past the
    end is refused and the windows go on"""
    from seqkit_amd.capi import SeqkitHipError
    path, raw = bam
    lone = m.grouped_parts(raw, 5000)[2]
    handled, n_rec, n_disc, _, _ = ctx.bam_file_recalc_tlen(str(path), 5000, 1, 64 << 10)
    assert handled and n_disc == len(lone) > 300
    assert ctx.bam_file_recalc_tlen_discarded(0, n_disc) == lone                       # before any window is taken
    wins = ctx.bam_file_rewrite_windows()
    next(wins)
    next(wins)
    cuts = [0, 1, 2, 67, 68, 199, n_disc - 1, n_disc]
    got = []
    for a, b in zip(cuts, cuts[1:]):
        got += ctx.bam_file_recalc_tlen_discarded(a, b - a)
    assert got == lone
    for first in (0, 5, n_disc):
        assert ctx.bam_file_recalc_tlen_discarded(first, 0) == []
    for first, n in ((0, n_disc + 1), (n_disc, 1), (n_disc + 1, 0), (-1, 1), (3, -1), (1, n_disc)):
        with pytest.raises(SeqkitHipError, match=r"failed \(-1\)"):                    # SK_ERR_INVALID
            ctx.bam_file_recalc_tlen_discarded(first, n)
    rest = list(wins)                                                                  # the windows go on
    assert rest and rest[-1]["bgzf"].endswith(m.EOF_BLOCK)
    assert ctx.bam_file_recalc_tlen_discarded(3, 5) == lone[3:8]                       # after the last window


def test_rewrite_next_after_the_end(ctx, bam):
    path, _ = bam
    assert ctx.bam_file_recalc_tlen(str(path), 5000, 1, 0)[0]
    assert list(ctx.bam_file_rewrite_windows())
    assert list(ctx.bam_file_rewrite_windows()) == []                                  # n == 0 && bytes == 0 again


def test_discarded_needs_a_recalc_tlen_call(ctx, bam, tmp_path):
    from seqkit_amd.capi import SeqkitHipError
    from tests import bam_subsample_model as sm
    path, _ = bam
    assert ctx.bam_file_recalc_tlen(str(path), 5000, 1, 0)[0]
    other = tmp_path / "sub.bam"
    sm.write(other, sm.served_records(300, seed=7))
    assert ctx.bam_file_subsample(str(other), 1.0, 1, 1, 0)[0]
    with pytest.raises(SeqkitHipError, match=r"failed \(-1\)"):
        ctx.bam_file_recalc_tlen_discarded(0, 0)


def test_boundary_files(ctx, tmp_path):
    """a file without records: one window; only lone candidates: one window, everything discarded; no candidates: the input records
    with TLEN 0"""
    empty = tmp_path / "empty.bam"
    raw = m.write(empty, [], text=b"\n\n\0\0")
    handled, out, _, n_win, n_rec, n_disc = collect(ctx, empty, 5000)
    assert handled and n_win == 1 and out == m.out_header(raw) and (n_rec, n_disc) == (0, 0)
    assert ctx.bam_file_recalc_tlen_discarded(0, 0) == []
    lone = tmp_path / "lone.bam"
    names = [b"l%d" % i for i in range(5000)]
    raw = m.write(lone, [m.cand(nm, 0, 100 + i, 150 + i, i & 1, i & 2, m.CIGARS[i % len(m.CIGARS)]) for i, nm in enumerate(names)])
    handled, out, _, n_win, n_rec, n_disc = collect(ctx, lone, 5000)
    assert handled and n_win == 1 and out == m.out_header(raw) and (n_rec, n_disc) == (0, 5000)
    assert ctx.bam_file_recalc_tlen_discarded(0, 5000) == names                        # (more than one chunk of name slots)
    assert ctx.bam_file_recalc_tlen_discarded(4090, 20) == names[4090:4110]
    none = tmp_path / "none.bam"
    recs = [m.md.rec(b"z%d" % (i // 2), i % 3, 100 + i, flag=[0, 0x1 | 0x4, 0x1 | 0x8, 0x1 | 0x10 | 0x20, 0x900][i % 5], cigar=m.CIGARS[i % len(m.CIGARS)],
                     tlen=m.JUNK[i % len(m.JUNK)], mpos=100 + i) for i in range(3000)]
    raw = m.write(none, recs)
    handled, out, _, _, n_rec, n_disc = collect(ctx, none, 5000)
    assert handled and (n_rec, n_disc) == (3000, 0) and out == m.out_header(raw) + b"".join(m.with_tlen(r, 0) for r in recs)


def declined_files():
    """decline bit -> records: a served file with one record (or pair) the device leaves to the caller's reader"""
    base = list(m.served_records(300, seed=4))
    a = m.cand(b"pair", 0, 100, 200, False, True)
    invalid = bytearray(m.cand(b"bad", 0, 100, 200, False, True))
    struct.pack_into("<i", invalid, 20, 4000)                                          # l_seq larger than the record holds
    return {
        1: base[:150] + [m.md.rec(b"sec", 0, 10, flag=0x1 | 0x100 | 0x10, mtid=0, mpos=20)] + base[150:],
        2: base[:150] + [a] + base[150:200] + [m.cand(b"pair", 0, 200, 100, True, True)] + base[200:],
        8: base[:150] + [bytes(invalid)] + base[150:],
        16: base[:150] + [m.md.rec(b"caf\xc3\xa9", 0, 10, flag=0)] + base[150:],       # (valid UTF-8: the conservative side)
        32: base[:150] + [m.md.rec(b"lone", 0, 200, flag=0x1 | 0x80 | 0x10, cigar=((m.M, 10), (9, 3)), l_seq=10, mtid=0, mpos=100)] + base[150:],
    }


@pytest.mark.parametrize("bit", sorted(declined_files()))
def test_declined_files(ctx, tmp_path, bit):
    from seqkit_amd.capi import SeqkitHipError
    path = tmp_path / "in.bam"
    m.write(path, declined_files()[bit])
    handled, info, _, n_win, n_rec, n_disc = collect(ctx, path, 5000)                  # (checked_windows: every count is 0)
    assert not handled and info[5] == -(30 + bit) and n_win == 0
    with pytest.raises(SeqkitHipError):                                                # no windows were set up
        next(ctx.bam_file_rewrite_windows())
    with pytest.raises(SeqkitHipError):
        ctx.bam_file_recalc_tlen_discarded(0, 0)


def test_bits_16_and_32_are_conservative_and_a_nul_in_a_name_declines(ctx, tmp_path):
    """the reference serves a UTF-8 name and a lone candidate with a bad CIGAR operation; the device leaves both to the reader"""
    for bit in (16, 32):
        raw = m.md.rm.header(m.md.rm.TEXT, m.md.rm.REFS) + b"".join(declined_files()[bit])
        assert m.literal(raw, 5000)[2] == 0
    path = tmp_path / "nul.bam"
    m.write(path, [m.md.rec(b"a\0b", 0, 10, flag=0)])
    handled, info, _, _, _, _ = collect(ctx, path, 5000)
    assert not handled and info[5] == -(30 + 16)


def test_key_bits_4_declines_with_bit_64(ctx, tmp_path, monkeypatch):
    """SK_TLEN_KEY_BITS=4: more than 16 distinct names must collide, and the device declines; records of one name have equal hashes and
    equal bytes, and are served"""
    many, one = tmp_path / "many.bam", tmp_path / "one.bam"
    m.write(many, [m.cand(b"key%d" % (i // 2), 0, 100, 150, i & 1, not i & 1) for i in range(400)])
    raw_one = m.write(one, [m.cand(b"same", 0, 100 + i, 150 + i, i & 1, not i & 1) for i in range(401)])
    monkeypatch.setenv("SK_TLEN_KEY_BITS", "4")
    handled, info, _, _, _, _ = collect(ctx, many, 5000)
    assert not handled and info[5] == -(30 + 0x40)
    check(ctx, one, raw_one, 5000)
    monkeypatch.delenv("SK_TLEN_KEY_BITS")
    handled, _, _, _, _, _ = collect(ctx, many, 5000)
    assert handled


@pytest.mark.parametrize("max_len,level", [(0, 1), (-1, 1), (-(1 << 63), 1), (5000, 2), (5000, -1)])
def test_invalid_arguments(ctx, bam, max_len, level):
    from seqkit_amd.capi import SeqkitHipError
    with pytest.raises(SeqkitHipError, match=r"failed \(-1\)"):                        # SK_ERR_INVALID
        ctx.bam_file_recalc_tlen(str(bam[0]), max_len, level, 0)


def test_small_grids(ctx, tmp_path):
    """contexts planned for 1 and 3 CUs: the capped grids of the resolve, gather, name and window kernels stride over 6 000 records;
    the bytes equal the default grid's and the model's"""
    from tests.test_gpu_small_grid import planned
    path = tmp_path / "in.bam"
    raw = m.write(path, m.served_records(6000, seed=3))
    ref = collect(ctx, path, 5000)
    assert ref[0]
    for cus in (1, 3):
        c = planned(str(cus))
        try:
            assert c.planned_cus() == cus
            check(c, path, raw, 5000)
            got = collect(c, path, 5000, window_bytes=1 << 20)
            assert got[0] and got[1] == ref[1] and got[4:] == ref[4:]
            assert c.bam_file_recalc_tlen_discarded(0, got[5]) == m.grouped_parts(raw, 5000)[2]
        finally:
            c.close()


def test_scratch_in_the_compressed_files_buffer_or_its_own(ctx, tmp_path, monkeypatch, capfd):
    """the sort's buffers and the record offsets lie in the idle buffer of the compressed file when they fit, else in memory of their own;
    SK_TLEN_OWN_MEMORY forces the second.  The model's output under every placement."""
    import random
    rnd = random.Random(9)
    text = b"@CO\t" + bytes(rnd.randrange(33, 127) for _ in range(4 << 20)) + b"\n"
    large, tiny = tmp_path / "large.bam", tmp_path / "tiny.bam"
    recs = m.served_records(3000, seed=1)
    raw_large = m.write(large, recs, text=text)
    raw_tiny = m.write(tiny, [m.cand(b"s%d" % (i // 2), 0, 100, 150, i & 1, not i & 1, ((m.M, 1),)) for i in range(8000)])
    import os
    assert os.path.getsize(tiny) + 64 < 32 * 8000                                      # (the file's buffer against the five columns alone)
    monkeypatch.setenv("SK_BAMFILE_TRACE", "1")
    capfd.readouterr()

    def placed():
        lines = [ln for ln in capfd.readouterr().err.split("\n") if "bytes of scratch in" in ln]
        assert len(lines) == 1 and lines[0].startswith("sk_bam_file_recalc_tlen: ")
        return lines[0].split("bytes of scratch in ")[1]
    check(ctx, large, raw_large, 5000)
    assert placed() == "the compressed file's buffer"
    check(ctx, tiny, raw_tiny, 5000)
    assert placed() == "its own buffer"
    monkeypatch.setenv("SK_TLEN_OWN_MEMORY", "1")
    check(ctx, large, raw_large, 5000)
    assert placed() == "its own buffer"
    monkeypatch.delenv("SK_TLEN_OWN_MEMORY")
    check(ctx, large, raw_large, 5000, window_bytes=64 << 10)
    assert placed() == "the compressed file's buffer"
