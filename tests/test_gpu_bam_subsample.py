"""GPU: sk_bam_file_subsample / sk_bam_file_rewrite_next — `sam subsample` with the fragments numbered (hash, sort, runs, scan), drawn
and compacted and the kept records BGZF-compressed on the device — against the plain-Python model of tests/bam_subsample_model.py."""
import struct
import zlib

import pytest

from tests import bam_minimize_model as mm
from tests import bam_subsample_model as m
from tests.bam_out_util import checked_windows, zlib_members

pytestmark = pytest.mark.gpu


def collect(ctx, path, fraction, seed, level=1, window_bytes=0):
    """(handled, inflated output or info, members, windows, records written, records counted); the windows are checked by
    tests/bam_out_util.checked_windows (order, first and n over the WRITTEN records, raw_bytes, the EOF block)"""
    res = ctx.bam_file_subsample(str(path), fraction, seed, level, window_bytes)
    handled, out, mem, n_win, info = checked_windows(ctx, res, m)
    return handled, out if handled else info, mem, n_win, res[1], res[2]


def check(ctx, path, raw, text, seed, level=1, window_bytes=0):
    f = m.parse_fraction(text)
    exp, _, code, kept, total = m.model(raw, seed, f)
    assert code == 0
    handled, out, mem, n_win, n_rec, n_total = collect(ctx, path, float(f), seed, level, window_bytes)
    assert handled, out
    assert out == exp and (n_rec, n_total) == (kept, total)
    return mem, n_win, kept, total


@pytest.fixture(scope="module")
def bam(tmp_path_factory):
    path = tmp_path_factory.mktemp("subsample") / "in.bam"
    return path, m.write(path, m.served_records())


@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("window", [0, 64 << 10])
@pytest.mark.parametrize("text,seed", [("0.5", 0), ("0.5", (1 << 64) - 1), ("0.01", 7), ("0.9", 1 << 63), ("1", 3)])
def test_subsample_matches_model(ctx, bam, level, window, text, seed):
    path, raw = bam
    mem, n_win, kept, total = check(ctx, path, raw, text, seed, level, window)
    if level == 0:
        assert all(stored for _, stored in mem[:-1])
    elif kept > 100:
        assert not all(stored for _, stored in mem[:-1])                               # (the device deflated what shrinks)
    if window and kept > 1000:
        assert n_win > 10
    if text == "1":
        assert kept == total == sum(1 for r in m.records(raw) if not m.flag_of(r) & 0x800)


def test_every_member_passes_zlib(ctx, bam):
    path, raw = bam
    for level in (0, 1):
        handled, n_rec, n_total, raw_bytes, _ = ctx.bam_file_subsample(str(path), 0.5, 11, level, 1 << 20)
        assert handled
        data = b"".join(w["bgzf"] for w in ctx.bam_file_rewrite_windows())
        out = b"".join(zlib_members(data))
        assert out == m.model(raw, 11, m.parse_fraction("0.5"))[0] and len(out) == raw_bytes


def test_subsample_small_windows_and_input_blocks(ctx, tmp_path):
    """records that straddle several input blocks of 12 KiB; windows of 256 bytes, so that runs of dropped records span many windows'
    worth of input"""
    path = tmp_path / "small.bam"
    raw = m.write(path, m.served_records(600, seed=7), piece=0x3000)
    for text, seed in (("0.5", 1), ("0.05", 2), ("1", 0)):
        for level in (0, 1):
            mem, n_win, kept, _ = check(ctx, path, raw, text, seed, level, 256)
            assert n_win > kept // 3


def test_fraction_1_writes_the_input_records(ctx, tmp_path):
    path = tmp_path / "all.bam"
    recs = [r for r in m.served_records(3000, seed=3) if not m.flag_of(r) & 0x800]
    raw = m.write(path, recs)
    handled, out, _, _, n_rec, n_total = collect(ctx, path, 1.0, 99)
    assert handled and n_rec == n_total == len(recs)
    assert out == m.out_header(raw) + b"".join(recs)


def test_everything_dropped_and_nothing_counted(ctx, tmp_path):
    """fraction 0 drops every fragment whose draw is not 0; a file of only 0x800 records counts nothing; a file without records: the
    header's members and the EOF block, one window"""
    path = tmp_path / "in.bam"
    raw = m.write(path, m.served_records(2000, seed=5))
    exp, _, _, kept, total = m.model(raw, 1, 0.0)
    assert kept == 0 and total > 0
    handled, out, _, n_win, n_rec, n_total = collect(ctx, path, 0.0, 1)
    assert handled and n_win == 1 and out == exp == m.out_header(raw) and (n_rec, n_total) == (0, total)
    supp = tmp_path / "supp.bam"
    raw = m.write(supp, [m.rm.record(b"s%d" % (i // 3), 30, flag=0x801 | (0x10 if i & 1 else 0), seed=i) for i in range(700)])
    handled, out, _, n_win, n_rec, n_total = collect(ctx, supp, 1.0, 1)
    assert handled and n_win == 1 and out == m.out_header(raw) and (n_rec, n_total) == (0, 0)
    empty = tmp_path / "empty.bam"
    raw = m.write(empty, [], text=b"\n\n\0\0")
    handled, out, _, n_win, n_rec, n_total = collect(ctx, empty, 0.5, 1)
    assert handled and n_win == 1 and out == m.out_header(raw) and (n_rec, n_total) == (0, 0)


@pytest.fixture(scope="module")
def big(tmp_path_factory):
    """2.1 M short records: the sort takes several passes and tiles, the scans several tiles and more than one round of tile sums;
    names on one record, on two (adjacent and 5 000 records apart) and on three, 0x800 records among them"""
    n = 2_100_000
    path = tmp_path_factory.mktemp("subsample_big") / "big.bam"
    hdr = m.rm.header(b"@HD\tVN:1.6\n", m.rm.REFS)
    body = struct.pack("<iiBBHHHiiii", 0, 100, 0, 30, 4680, 0, 0, 0, 0, 150, 150)
    parts, names, flags = [hdr], [], []
    for i in range(n):
        k = i % 10000
        if k < 5000:
            name, f = b"p%d" % i, 0x41                                                    # its mate 5 000 records on
        else:
            name, f = b"p%d" % (i - 5000), 0x81
        if i % 7 == 3:
            name, f = b"t%d" % (i // 21), 0x101                                           # three records, 7 apart: the third draws anew
        elif i % 97 == 5:
            f |= 0x800                                                                    # between mates, passed over
        elif i % 13 == 0:
            name, f = b"s%d" % i, 0x1                                                     # once (its partner of the p pair stays single)
        nm = name + b"\0"
        b = bytearray(body)
        b[8] = len(nm)
        struct.pack_into("<H", b, 14, f)
        rec = bytes(b) + nm
        parts.append(struct.pack("<i", len(rec)) + rec)
    raw = b"".join(parts)
    comp = []
    for o in range(0, len(raw), 0xFF00):
        data = raw[o:o + 0xFF00]
        c = zlib.compressobj(1, zlib.DEFLATED, -15)
        z = c.compress(data) + c.flush()
        comp.append(struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, len(z) + 25) + z + struct.pack("<II", zlib.crc32(data), len(data)))
    with open(path, "wb") as fh:
        fh.write(b"".join(comp) + m.EOF_BLOCK)
    return path, raw


def test_subsample_two_million_records(ctx, big):
    path, raw = big
    exp, _, code, kept, total = m.model(raw, 42, m.parse_fraction("0.5"))
    assert code == 0 and total > 2_000_000 and 0.45 * total < kept < 0.55 * total
    res = ctx.bam_file_subsample(str(path), 0.5, 42, 1, 0)
    assert res[0] and res[1:4] == (kept, total, len(exp))
    out = b"".join(x for w in ctx.bam_file_rewrite_windows() for x, _ in m.members(w["bgzf"]))
    assert out == exp


def test_key_bits_8_declines_with_bit_64(ctx, tmp_path, monkeypatch):
    """SK_SUBSAMPLE_KEY_BITS=8: more than 256 distinct names must collide, and the device declines; records of one name have equal
    hashes and equal bytes, and are served"""
    many, one = tmp_path / "many.bam", tmp_path / "one.bam"
    m.write(many, [m.rm.record(b"key%d" % (i // 2), 10, flag=0x41 if i & 1 else 0x81, seed=i) for i in range(800)])
    raw_one = m.write(one, [m.rm.record(b"same", 10, flag=0x1 | (0x800 if i % 5 == 2 else 0), seed=i) for i in range(801)])
    monkeypatch.setenv("SK_SUBSAMPLE_KEY_BITS", "8")
    handled, info, _, _, _, _ = collect(ctx, many, 0.5, 1)
    assert not handled and info[5] == -(30 + 0x40)
    check(ctx, one, raw_one, "0.5", 1)
    monkeypatch.delenv("SK_SUBSAMPLE_KEY_BITS")
    handled, _, _, _, _, _ = collect(ctx, many, 0.5, 1)
    assert handled


def test_unpaired_record_declines_and_nothing_is_written(ctx, tmp_path):
    path = tmp_path / "unpaired.bam"
    recs = list(m.served_records(300, seed=7))
    recs[150] = m.rm.record(b"single", 20, flag=0x10)
    m.write(path, recs)
    handled, info, _, n_win, n_rec, n_total = collect(ctx, path, 1.0, 1)           # (checked_windows: every count is 0)
    assert not handled and info[5] == -(30 + 1) and n_win == 0
    from seqkit_amd.capi import SeqkitHipError
    with pytest.raises(SeqkitHipError):                                             # no windows were set up
        next(ctx.bam_file_rewrite_windows())
    recs[150] = m.rm.record(b"single", 20, flag=0x810)                              # with 0x800 it is passed over before the check
    raw = m.write(path, recs)
    check(ctx, path, raw, "1", 1)


def test_invalid_record_declines(ctx, tmp_path):
    """l_seq larger than the record holds: htslib's "Invalid BAM record." """
    path = tmp_path / "bad.bam"
    bad = bytearray(m.rm.record(b"bad", 20, flag=1))
    struct.pack_into("<i", bad, 20, 4000)
    m.write(path, [m.rm.record(b"ok1", 20, flag=1), bytes(bad), m.rm.record(b"ok2", 20, flag=1)])
    handled, info, _, _, _, _ = collect(ctx, path, 0.5, 1)
    assert not handled and info[5] < 0


@pytest.mark.parametrize("fraction,level", [(-0.0001, 1), (1.0001, 1), (float("nan"), 1), (0.5, 2), (0.5, -1)])
def test_invalid_arguments(ctx, bam, fraction, level):
    from seqkit_amd.capi import SeqkitHipError
    with pytest.raises(SeqkitHipError, match=r"failed \(-1\)"):                    # SK_ERR_INVALID
        ctx.bam_file_subsample(str(bam[0]), fraction, 0, level, 0)


def test_minimize_read_ids_before_and_after_on_the_same_ctx(ctx, tmp_path):
    """the id passes are shared: `minimize --read-ids` still matches its model around a subsample call"""
    mpath, spath = tmp_path / "min.bam", tmp_path / "sub.bam"
    mraw = mm.write(mpath, mm.served_records(8000, seed=3))
    sraw = m.write(spath, m.served_records(8000, seed=3))

    def minimize():
        handled, out, _, _, _ = checked_windows(ctx, ctx.bam_file_minimize(str(mpath), True, False, False, 255, 1, 0), mm)
        assert handled and out == mm.model(mraw, "read-ids")[0]
    minimize()
    check(ctx, spath, sraw, "0.5", 9)
    minimize()
    # and on minimize's own input, whose records include unpaired ones and names cut at '/': paired here by flag, whole names as keys
    recs = [r[:18] + bytes([r[18] | 1]) + r[19:] for r in mm.served_records(8000, seed=3)]
    raw = m.write(spath, recs)
    check(ctx, spath, raw, "0.5", 9)
    minimize()


def test_subsample_scratch_in_the_compressed_files_buffer_or_its_own(ctx, tmp_path, monkeypatch, capfd):
    """the sort's buffers and the record offsets (32 B per record and the sort's own scratch) lie in the idle buffer of the compressed
    file when they fit, else in memory of their own; the placements arise from the files.  8 000 served records under a header text of
    4 MiB that does not compress: the file's buffer.  8 000 records of 39 bytes, which compress to 5 bytes each: memory of its own,
    whatever the sort asks for on top.  (The served records under the default header take 1.3 MB against 0.26 MB of scratch: their
    own qualities do not compress, so that file alone never reaches the second placement; it is served and compared all the same.)
    The model's output every time, also after another file has been read into that buffer."""
    import os
    import random
    rnd = random.Random(9)
    text = b"@CO\t" + bytes(rnd.randrange(33, 127) for _ in range(4 << 20)) + b"\n"
    small, large, tiny, other = tmp_path / "small.bam", tmp_path / "large.bam", tmp_path / "tiny.bam", tmp_path / "other.bam"
    recs = m.served_records(8000, seed=3)
    raw_small, raw_large = m.write(small, recs), m.write(large, recs, text=text)
    raw_tiny = m.write(tiny, [m.rm.record(b"s%d" % (i // 2), 0, flag=0x41 if i & 1 else 0x81, seed=i) for i in range(8000)])
    assert os.path.getsize(tiny) + 64 < 32 * 8000                                      # (the file's buffer against the five columns alone)
    raw_other = m.write(other, m.served_records(600, seed=7))
    monkeypatch.setenv("SK_BAMFILE_TRACE", "1")
    capfd.readouterr()

    def placed():
        lines = [ln for ln in capfd.readouterr().err.split("\n") if "bytes of scratch in" in ln]
        assert len(lines) == 1 and lines[0].startswith("sk_bam_file_subsample: ")
        print(lines[0])
        return lines[0].split("bytes of scratch in ")[1]
    check(ctx, small, raw_small, "0.5", 1)
    placed()
    check(ctx, tiny, raw_tiny, "0.5", 1)
    assert placed() == "its own buffer"
    check(ctx, large, raw_large, "0.5", 1)
    assert placed() == "the compressed file's buffer"
    check(ctx, other, raw_other, "0.5", 2)
    placed()
    check(ctx, large, raw_large, "0.5", 1, window_bytes=64 << 10)
    assert placed() == "the compressed file's buffer"
    check(ctx, tiny, raw_tiny, "0.9", 3)
    assert placed() == "its own buffer"
