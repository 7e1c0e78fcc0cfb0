"""GPU: sk_bam_file_minimize / sk_bam_file_rewrite_next — `sam minimize` with the read ids numbered (hash, sort, runs, scan) and the
records rewritten and BGZF-compressed on the device — against the plain-Python model of tests/bam_minimize_model.py."""
import pytest

from tests import bam_minimize_model as m
from tests.bam_out_util import checked_windows

pytestmark = pytest.mark.gpu


def collect(ctx, path, combo, fill=255, level=1, window_bytes=0):
    handled, out, mem, n_win, info = checked_windows(ctx, ctx.bam_file_minimize(str(path), *m.COMBOS[combo], fill, level, window_bytes), m)
    return handled, out if handled else info, mem, n_win


@pytest.fixture(scope="module")
def bam(tmp_path_factory):
    path = tmp_path_factory.mktemp("minimize") / "in.bam"
    return path, m.write(path, m.served_records())


@pytest.mark.parametrize("combo", list(m.COMBOS))
@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("window", [0, 64 << 10])
def test_minimize_matches_model(ctx, bam, combo, level, window):
    path, raw = bam
    for fill in (255, 0, 30) if m.COMBOS[combo][1] else (255,):
        exp, code = m.model(raw, combo, fill)
        assert code is None
        handled, out, mem, n_win = collect(ctx, path, combo, fill, level, window)
        assert handled, out
        assert out == exp
        if level == 0:
            assert all(stored for _, stored in mem[:-1])
        else:
            assert not all(stored for _, stored in mem[:-1])                           # (the device deflated what shrinks)
        if window:
            assert n_win > 10


def test_minimize_many_records(ctx, tmp_path):
    """300 000 records: the sort runs more than one tile and pass, the scans more than one tile and more than one round of tile sums"""
    names = m.served_names(300000, seed=5)
    path = tmp_path / "big.bam"
    raw = m.write(path, [m.record(n, 4 + (i & 3), aux=m.AUX[i % 3], seed=i & 63, pad=i & 15) for i, n in enumerate(names)])
    for combo in ("read-ids", "all"):
        handled, out, _, _ = collect(ctx, path, combo)
        assert handled, out
        assert out == m.model(raw, combo)[0]


def test_minimize_every_name_starts_with_a_slash(ctx, tmp_path):
    """one key, one run of n records: ids 1, 1, 2, 2, 3, 3 .."""
    path = tmp_path / "slash.bam"
    n = 5001
    raw = m.write(path, [m.record(b"/%d" % (i * 7919 % 1000), 9, seed=i & 31, pad=9) for i in range(n)])
    handled, out, _, _ = collect(ctx, path, "read-ids")
    assert handled, out
    assert out == m.model(raw, "read-ids")[0]
    got = [int(r[36:36 + r[12] - 1]) for r in m.records(out)]
    assert got == [i // 2 + 1 for i in range(n)]


def test_minimize_no_records(ctx, tmp_path):
    path = tmp_path / "empty.bam"
    raw = m.write(path, [], text=b"\n\n\0\0")
    for combo in m.COMBOS:
        handled, out, _, n_win = collect(ctx, path, combo)
        assert handled and n_win == 1 and out == m.model(raw, combo)[0]


def test_minimize_small_input_blocks(ctx, tmp_path):
    """records that straddle several input blocks of 12 KiB, and a window of 256 bytes (one or two records each)"""
    path = tmp_path / "small.bam"
    raw = m.write(path, m.served_records(300, seed=7), piece=0x3000)
    for combo in m.COMBOS:
        handled, out, _, n_win = collect(ctx, path, combo, 30, 1, 256)
        assert handled, out
        assert out == m.model(raw, combo, 30)[0] and n_win > 100


def test_minimize_declines_cigar_op_9(ctx, tmp_path):
    path = tmp_path / "cigar.bam"
    recs = list(m.served_records(300, seed=7))
    recs[150] = m.record(b"mid", 20, cigar_op=9)
    raw = m.write(path, recs)
    for combo in m.COMBOS:
        assert m.model(raw, combo)[1] == 101
        handled, info, _, _ = collect(ctx, path, combo)
        assert not handled and info[5] == -(30 + 32)


def test_minimize_declines_invalid_record(ctx, tmp_path):
    """l_seq larger than the record holds: htslib's "Invalid BAM record." """
    import struct
    path = tmp_path / "bad.bam"
    bad = bytearray(m.record(b"bad", 20))
    struct.pack_into("<i", bad, 20, 4000)
    m.write(path, [m.record(b"ok1", 20), bytes(bad), m.record(b"ok2", 20)])
    for combo in m.COMBOS:
        handled, info, _, _ = collect(ctx, path, combo)
        assert not handled and info[5] < 0


def test_minimize_verifies_the_keys_bytes(ctx, tmp_path, monkeypatch):
    """SK_MINIMIZE_KEY_BITS=8: more than 256 distinct keys must collide, and the device declines; names of one key have equal masked
    hashes and equal bytes, and are served"""
    many, one = tmp_path / "many.bam", tmp_path / "one.bam"
    m.write(many, [m.record(b"key%d/1" % (i // 2), 10, seed=i) for i in range(800)])
    raw_one = m.write(one, [m.record(b"same/%d" % i, 10, seed=i) for i in range(801)])
    monkeypatch.setenv("SK_MINIMIZE_KEY_BITS", "8")
    handled, info, _, _ = collect(ctx, many, "read-ids")
    assert not handled and info[5] == -(30 + 64)
    handled, out, _, _ = collect(ctx, many, "tags")                                   # (no ids: nothing to collide)
    assert handled
    handled, out, _, _ = collect(ctx, one, "read-ids+tags")
    assert handled and out == m.model(raw_one, "read-ids+tags")[0]
    monkeypatch.delenv("SK_MINIMIZE_KEY_BITS")
    handled, out, _, _ = collect(ctx, many, "read-ids")
    assert handled


@pytest.mark.parametrize("flags,level", [((False, False, False), 1), ((False, True, False), 1), ((True, True, False), 1), ((True, False, False), 2),
                                         ((True, False, True), -1)])
def test_minimize_invalid_arguments(ctx, bam, flags, level):
    from seqkit_amd.capi import SeqkitHipError
    with pytest.raises(SeqkitHipError, match=r"failed \(-1\)"):                    # SK_ERR_INVALID
        ctx.bam_file_minimize(str(bam[0]), *flags, 255, level, 0)


def test_minimize_unknown_flag_bits_are_invalid(ctx, bam):
    import ctypes as C
    n_rec, raw_bytes, handled = C.c_int64(0), C.c_uint64(0), C.c_int32(0)
    assert ctx._lib.sk_bam_file_minimize(ctx._h, str(bam[0]).encode(), 8, 255, 1, 0, C.byref(n_rec), C.byref(raw_bytes), C.byref(handled), None) == -1
    # (sk_bam_file_rewrite keeps its three ops: 0, minimize's mark inside the library, is no op of its)
    assert ctx._lib.sk_bam_file_rewrite(ctx._h, str(bam[0]).encode(), 0, 1, 0, C.byref(n_rec), C.byref(raw_bytes), C.byref(handled), None) == -1


def test_minimize_windows_end_with_another_file_call(ctx, tmp_path):
    from seqkit_amd.capi import SeqkitHipError
    path = tmp_path / "in.bam"
    m.write(path, m.served_records(50, seed=2))
    assert ctx.bam_file_minimize(str(path), True, False, True)[0]
    assert ctx.bam_file_reads(str(path), "fastq")[0]
    with pytest.raises(SeqkitHipError):
        next(ctx.bam_file_rewrite_windows())
