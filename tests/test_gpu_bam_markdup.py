"""GPU: sk_bam_file_markdup / sk_bam_file_rewrite_next — `sam mark duplicates` with the clusters found (signatures, sort by group,
per-group greedy) and the BAM rewritten and BGZF-compressed on the device — against literal() of tests/bam_markdup_model.py, the
line-by-line statement of the reference's loop."""
import struct

import pytest

from tests import bam_markdup_model as m
from tests.bam_out_util import checked_windows

pytestmark = pytest.mark.gpu


def collect(ctx, path, ignore_umi=False, level=1, window_bytes=0):
    result = ctx.bam_file_markdup(str(path), ignore_umi, level, window_bytes)
    handled, out, mem, n_win, info = checked_windows(ctx, result, m)
    return handled, out if handled else info, mem, n_win, result[2]


def check(ctx, path, raw, ignore_umi=False, level=1, window_bytes=0):
    exp, code, msg = m.literal(raw, ignore_umi)
    assert code == 0
    handled, out, mem, n_win, n_dup = collect(ctx, path, ignore_umi, level, window_bytes)
    assert handled, out
    assert out == exp
    n = len(list(m.records(raw)))
    assert msg == m.summary(n_dup, n)
    return mem, n_win, n_dup


@pytest.fixture(scope="module")
def bam(tmp_path_factory):
    path = tmp_path_factory.mktemp("markdup") / "in.bam"
    return path, m.write(path, m.sorted_records(11, 25000, big=1100))


@pytest.mark.parametrize("ignore_umi", [False, True])
@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("window", [0, 64 << 10])
def test_markdup_matches_literal(ctx, bam, ignore_umi, level, window):
    path, raw = bam
    mem, n_win, n_dup = check(ctx, path, raw, ignore_umi, level, window)
    assert n_dup > 1000
    if level == 0:
        assert all(stored for _, stored in mem[:-1])
    else:
        assert not all(stored for _, stored in mem[:-1])                               # (the device deflated what shrinks)
    if window:
        assert n_win > 10


@pytest.mark.parametrize("seed", range(6))
def test_markdup_other_inputs(ctx, tmp_path, seed):
    """record counts around multiples of 1000, files without UMIs and with UMIs on every group"""
    path = tmp_path / "in.bam"
    raw = m.write(path, m.sorted_records(seed, [50, 999, 1000, 1001, 2300, 4100][seed], big=1100 if seed % 2 else 0, umi_share=[0.7, 0.0, 1.0][seed % 3]))
    check(ctx, path, raw)
    check(ctx, path, raw, ignore_umi=True)


def test_markdup_chains(ctx, tmp_path):
    path = tmp_path / "chain.bam"
    raw = m.write(path, m.chain_records())
    check(ctx, path, raw)


def test_markdup_small_input_blocks(ctx, tmp_path):
    """records that straddle input blocks of 12 KiB, and a window of 256 bytes (one or two records each)"""
    path = tmp_path / "small.bam"
    raw = m.write(path, m.sorted_records(7, 600, big=0), piece=0x3000)
    _, n_win, _ = check(ctx, path, raw, False, 1, 256)
    assert n_win > 100


def test_markdup_many_records(ctx, tmp_path):
    """300 000 records: the sort and the scan run more than one tile and pass"""
    path = tmp_path / "big.bam"
    raw = m.write(path, m.sorted_records(21, 300000, big=1500))
    _, _, n_dup = check(ctx, path, raw)
    assert n_dup > 50000


def test_markdup_one_group_of_all_records(ctx, tmp_path):
    """every read at one start_pos and strand: the strided form of the cluster kernel, many rounds; then as many clusters as reads"""
    import random
    rnd = random.Random(3)
    fams = [m._umi(rnd, 10) for _ in range(40)]
    recs = [m.rec(b"r%d" % i, 0, 700, 0x400 if i % 5 == 0 else 0, ((m.M, 20 + (i * 7) % 13),), aux=m.aux_z(b"RX", m._mutate(rnd, fams[i % 40], i % 2)))
            for i in range(5000)]
    path = tmp_path / "one.bam"
    raw = m.write(path, recs)
    _, _, n_dup = check(ctx, path, raw)
    assert 4000 < n_dup < 5000
    recs = [m.rec(b"r%d" % i, 0, 700, 0, tlen=i + 1) for i in range(700)]          # 700 fragment lengths: 700 clusters of one
    raw = m.write(path, recs)
    assert check(ctx, path, raw)[2] == 0


def test_markdup_no_records(ctx, tmp_path):
    path = tmp_path / "empty.bam"
    raw = m.write(path, [], text=b"\n\n\0\0")
    for ignore_umi in (False, True):
        handled, out, _, n_win, n_dup = collect(ctx, path, ignore_umi)
        assert handled and n_win == 1 and n_dup == 0 and out == m.literal(raw)[0]


def test_markdup_only_unmapped(ctx, tmp_path):
    path = tmp_path / "unmapped.bam"
    raw = m.write(path, [m.rec(b"u%d" % i, -1, -1, 4 | (0x400 if i % 3 == 0 else 0), (), l_seq=20, mtid=-1, mpos=-1) for i in range(100)])
    assert check(ctx, path, raw)[2] == 34


def _declined(ctx, tmp_path, at, bad, bits, literal_code, ignore_umi=False):
    base = m.sorted_records(5, 2300, big=0)
    path = tmp_path / "in.bam"
    raw = m.write(path, base[:at] + [bad] + base[at:])
    if literal_code is not None:
        assert m.literal(raw)[1] == literal_code
    handled, info, _, _, _ = collect(ctx, path, ignore_umi)
    assert not handled and info[5] == -(30 + bits)


@pytest.mark.parametrize("at", [1, 1500])
def test_markdup_declines_what_the_reference_stops_at(ctx, tmp_path, at):
    base = m.sorted_records(5, 2300, big=0)
    tid, pos = m.core(base[at - 1])[:2]
    _declined(ctx, tmp_path, at, m.rec(b"sec", tid, pos, 0x100), 1, 255)
    _declined(ctx, tmp_path, at, m.rec(b"sup", tid, pos, 0x800 | 4), 1, 255)
    _declined(ctx, tmp_path, at, m.rec(b"back", tid, pos - 1), 2, 255)
    _declined(ctx, tmp_path, at, m.rec(b"back", tid, pos - 1, 4, (), l_seq=5), 2, 255)             # an unmapped read out of order
    _declined(ctx, tmp_path, at, m.rec(b"op9", tid, pos, 16, ((m.M, 5), (9, 20)), l_seq=25), 32, 101)


def test_markdup_declines_what_the_grouping_does_not_cover(ctx, tmp_path):
    base = m.sorted_records(5, 2300, big=0)
    tid, pos = m.core(base[99])[:2]
    # a mapped read at pos -1: as u32 the largest position (only the first read of a tid can have it on a sorted file)
    path = tmp_path / "neg.bam"
    m.write(path, [m.rec(b"neg", 2, -1)] + [m.rec(b"x%d" % i, 1, 10 + i) for i in range(50)])
    handled, info, _, _, _ = collect(ctx, path)
    assert not handled and info[5] == -(30 + 4)
    # a reverse read whose CIGAR ends beyond INT32_MAX
    _declined(ctx, tmp_path, 100, m.rec(b"far", tid, pos, 16, ((m.N, (1 << 28) - 1),) * 9, l_seq=0), 4, None)
    # aux data that stop parsing before an RX field is found: a type byte '?', a Z value without its NUL, a B array beyond the record
    for aux in (b"XX?\1", m.aux_i(b"NM", 1) + b"XZZabc", b"ZBBS" + struct.pack("<I", 1000) + b"\0\0", b"RXZACGT", b"X"):
        _declined(ctx, tmp_path, 100, m.rec(b"aux", tid, pos, aux=aux), 16, None)
    # --ignore-umi never reads the aux data, and an unmapped read's are never read
    path = tmp_path / "ok.bam"
    raw = m.write(path, base[:100] + [m.rec(b"aux", tid, pos, aux=b"XX?\1")] + base[100:])
    check(ctx, path, raw, ignore_umi=True)
    raw = m.write(path, base[:100] + [m.rec(b"aux", tid, pos, 4, (), l_seq=5, aux=b"XX?\1")] + base[100:])
    check(ctx, path, raw)
    # bytes behind a complete RX field are not read either
    raw = m.write(path, base[:100] + [m.rec(b"aux", tid, pos, aux=m.aux_z(b"RX", b"ACGT") + b"XX?\1")] + base[100:])
    check(ctx, path, raw)
    # an operation code above 8 on a forward or unmapped read is not looked at
    raw = m.write(path, base[:100] + [m.rec(b"op9", tid, pos, 0, ((9, 20),), l_seq=20), m.rec(b"op9u", tid, pos, 4 | 16, ((9, 20),), l_seq=20)] + base[100:])
    check(ctx, path, raw)


def test_markdup_declines_invalid_record(ctx, tmp_path):
    """l_seq larger than the record holds: htslib's "Invalid BAM record." """
    path = tmp_path / "bad.bam"
    bad = bytearray(m.rec(b"bad", 0, 100))
    struct.pack_into("<i", bad, 20, 4000)
    m.write(path, [m.rec(b"ok1", 0, 100), bytes(bad), m.rec(b"ok2", 0, 100)])
    handled, info, _, _, _ = collect(ctx, path)
    assert not handled and info[5] < 0


def test_markdup_invalid_level(ctx, bam):
    from seqkit_amd.capi import SeqkitHipError
    for level in (-1, 2):
        with pytest.raises(SeqkitHipError, match=r"failed \(-1\)"):                    # SK_ERR_INVALID
            ctx.bam_file_markdup(str(bam[0]), False, level, 0)


def test_markdup_after_and_before_other_file_calls(ctx, bam, tmp_path):
    from seqkit_amd.capi import SeqkitHipError
    path, raw = bam
    assert ctx.bam_file_minimize(str(path), True, False, True)[0]                      # (leaves ids in the working memory markdup takes)
    check(ctx, path, raw)
    assert ctx.bam_file_rewrite(str(path), "trim qnames")[0]
    check(ctx, path, raw, ignore_umi=True, window_bytes=64 << 10)
    assert ctx.bam_file_markdup(str(path))[0]
    assert ctx.bam_file_reads(str(path), "fastq")[0]
    with pytest.raises(SeqkitHipError):
        next(ctx.bam_file_rewrite_windows())


def test_markdup_scratch_in_the_compressed_files_buffer_or_its_own(ctx, tmp_path, monkeypatch, capfd):
    """the sort's buffers and the signatures lie in the idle buffer of the compressed file when they fit (here: a header text of 4 MB
    that does not compress), else in memory of their own; SK_MARKDUP_OWN_MEMORY forces the latter.  The same output either way, also
    after another file has been read into that buffer."""
    import random
    rnd = random.Random(9)
    text = b"@CO\t" + bytes(rnd.randrange(33, 127) for _ in range(4 << 20)) + b"\n"
    path, other = tmp_path / "in.bam", tmp_path / "other.bam"
    raw = m.write(path, m.sorted_records(13, 25000, big=1100), text=text)
    m.write(other, m.sorted_records(14, 3000, big=0))
    monkeypatch.setenv("SK_BAMFILE_TRACE", "1")
    check(ctx, path, raw)
    assert "of scratch in the compressed file's buffer" in capfd.readouterr().err
    check(ctx, path, raw, ignore_umi=True, window_bytes=64 << 10)
    monkeypatch.setenv("SK_MARKDUP_OWN_MEMORY", "1")
    check(ctx, path, raw)
    assert "of scratch in its own buffer" in capfd.readouterr().err
    monkeypatch.delenv("SK_MARKDUP_OWN_MEMORY")
    check(ctx, other, m.write(other, m.sorted_records(14, 3000, big=0)))
    check(ctx, path, raw)
