"""GPU: sk_bam_file_discard_tails / sk_bam_file_discard_tails_loads / sk_bam_file_rewrite_next — `sam discard tail artifacts` with the
genome's chromosomes raw in device memory, both tails of every mapped record walked, the written records compacted and
BGZF-compressed on the device — against the plain-Python model of tests/bam_discard_tails_model.py."""
import functools
import struct

import pytest

from tests import bam_discard_tails_model as m
from tests.bam_out_util import checked_windows, zlib_members

pytestmark = pytest.mark.gpu

UINT32_MAX = (1 << 32) - 1


def ratio_of(T, opt):
    """the f32 ratio of an option as the command makes it, and whether the command accepts it"""
    key, val = opt.split("=")
    thr = m.f32(val) if key == "--threshold" else m.f32(int(val)) / m.f32(T)
    return thr, bool(0.0 <= thr <= 1.0)


def collect(ctx, path, fasta, T, thr, level=1, window_bytes=0, fai=None):
    """(handled, inflated output or info, members, windows, (total, failed, passed), the loads); the windows are checked by
    tests/bam_out_util.checked_windows (order, first and n over the WRITTEN records, raw_bytes, the EOF block), every member by zlib"""
    min_mm = UINT32_MAX if thr != thr else m.check_threshold(T, thr)
    res = ctx.bam_file_discard_tails(str(path), str(fasta), m.fai_entries() if fai is None else fai, T, min_mm, m.co_line(T, thr), level, window_bytes)
    handled, out, mem, n_win, info = checked_windows(ctx, res, m)
    if not handled:
        return False, info, None, 0, None, None
    loads = ctx.bam_file_discard_tails_loads(0, res[5])
    assert res[1] == res[2] - res[3] and res[4] <= res[1]                             # written = total - failed; the passed ones are among them
    return True, out, mem, n_win, (res[2], res[3], res[4]), loads


def check(ctx, path, fasta, raw, expected, T, thr, level=1, window_bytes=0):
    exp_out, _, code, counts, loads, _ = expected
    assert code == 0
    handled, out, mem, n_win, got_counts, got_loads = collect(ctx, path, fasta, T, thr, level, window_bytes)
    assert handled, out
    assert out == exp_out and got_counts == counts and got_loads == loads
    return mem, n_win


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """the genome's two files; the served records in input blocks of 12 KiB, which records straddle; a shorter file for the small windows"""
    d = tmp_path_factory.mktemp("tails")
    fasta, genome = m.write_genome(d)
    path, small = d / "in.bam", d / "small.bam"
    raw = m.write(path, list(m.served_records()), text=m.TEXT, refs=m.REFS, piece=0x3000)
    raw_small = m.write(small, list(m.served_records(500, seed=7)), text=m.TEXT, refs=m.REFS, piece=0x3000)
    return d, fasta, genome, {0: (path, raw), 64 << 10: (path, raw), 256: (small, raw_small)}


@functools.lru_cache(maxsize=None)
def expected_for(which, T, opt):
    """the model's answer, computed once per input and parameter pair and shared by the cases"""
    fasta, fai, _ = m.genome_files()
    recs = m.served_records() if which == "in" else m.served_records(500, seed=7)
    raw = m.rm.header(m.TEXT, m.REFS) + b"".join(recs)
    return m.model(raw, m.Genome(fasta, fai), T, ratio_of(T, opt)[0])


# (--mismatches=3 of a tail of one base is the ratio 3: the command refuses it before any file is opened — tests/test_cli_bam_discard_tails_host.py)
GRID = [(T, opt) for T in (1, 20, 33, 64, 300) for opt in ("--threshold=0", "--threshold=0.15", "--threshold=1", "--mismatches=3") if ratio_of(T, opt)[1]]


@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("window", [0, 64 << 10, 256])
@pytest.mark.parametrize("T,opt", GRID)
def test_discard_tails_matches_model(ctx, files, T, opt, window, level):
    _, fasta, _, inputs = files
    path, raw = inputs[window]
    exp = expected_for("in" if window != 256 else "small", T, opt)
    mem, n_win = check(ctx, path, fasta, raw, exp, T, ratio_of(T, opt)[0], level, window)
    written = exp[3][0] - exp[3][1]
    if level == 0:
        assert all(stored for _, stored in mem[:-1])
    elif written > 100:
        assert not all(stored for _, stored in mem[:-1])                               # (the device deflated what shrinks)
    if window == 256:                                                                  # the header's window, then one per 256 bytes of output in which a record begins
        at, starts = 0, set()
        for r in m.records(exp[0]):
            starts.add(at // 256)
            at += len(r)
        assert n_win == 1 + len(starts)
    elif window and written > 1000:
        assert n_win > 4
    if opt == "--threshold=0":                                                         # every mapped read fails: only the unmapped ones are written
        assert exp[3][2] == 0 and all(r[18] & 4 for r in m.records(exp[0]))


def test_every_member_passes_zlib(ctx, files):
    _, fasta, _, inputs = files
    path, raw = inputs[0]
    exp = expected_for("in", 20, "--threshold=0.15")
    for level in (0, 1):
        res = ctx.bam_file_discard_tails(str(path), str(fasta), m.fai_entries(), 20, 3, m.co_line(20, m.f32(0.15)), level, 1 << 20)
        assert res[0]
        data = b"".join(w["bgzf"] for w in ctx.bam_file_rewrite_windows())
        out = b"".join(zlib_members(data))
        assert out == exp[0] and len(out) == res[6]


def test_nothing_written_and_no_records(ctx, files, tmp_path):
    """a file whose every read is mapped and fails, and a file without records: one window each, the header's members and the EOF block"""
    _, fasta, genome, _ = files
    recs = [r for r in m.served_records(700, seed=5) if not r[18] & 4]
    path = tmp_path / "mapped.bam"
    raw = m.write(path, recs, text=m.TEXT, refs=m.REFS, piece=0x3000)
    exp = m.model(raw, genome, 20, 0.0)
    handled, out, _, n_win, counts, loads = collect(ctx, path, fasta, 20, m.f32(0.0))
    assert handled and n_win == 1 and out == exp[0] == m.out_header(raw, 20, 0.0) and counts == exp[3] == (len(recs), len(recs), 0) and loads == exp[4]
    # a NaN threshold fails no read, whatever its count
    handled, out, _, _, counts, _ = collect(ctx, path, fasta, 20, m.f32("nan"))
    assert handled and counts == (len(recs), 0, len(recs)) and out == m.model(raw, genome, 20, m.f32("nan"))[0]
    empty = tmp_path / "empty.bam"
    raw = m.write(empty, [], text=b"\n\n\0\0", refs=m.REFS)
    handled, out, _, n_win, counts, loads = collect(ctx, empty, fasta, 20, m.f32(0.15))
    assert handled and n_win == 1 and out == m.out_header(raw, 20, 0.15) and counts == (0, 0, 0) and loads == []


def test_tail_longer_than_every_read(ctx, files, tmp_path):
    """LONG TAIL: the walks end with the CIGAR"""
    _, fasta, genome, _ = files
    recs = [r for r in m.served_records(900, seed=4) if len(r) < 1000]
    assert max(struct.unpack_from("<i", r, 20)[0] for r in recs) < 200
    path = tmp_path / "short.bam"
    raw = m.write(path, recs, text=m.TEXT, refs=m.REFS, piece=0x3000)
    for T, thr in ((200, 0.02), (100000, 0.0001), ((1 << 32) - 1, 1e-9)):
        check(ctx, path, fasta, raw, m.model(raw, genome, T, thr), T, m.f32(thr))


def declined(ctx, path, fasta, bits, fai=None):
    handled, info, _, n_win, _, _ = collect(ctx, path, fasta, 20, m.f32(0.15), fai=fai)       # (checked_windows: every count is 0)
    assert not handled and info[5] == -(30 + bits) and n_win == 0, info
    from seqkit_amd.capi import SeqkitHipError
    with pytest.raises(SeqkitHipError):                                                 # no windows were set up
        next(ctx.bam_file_rewrite_windows())
    with pytest.raises(SeqkitHipError):                                                 # and no loads to ask for
        ctx.bam_file_discard_tails_loads(0, 0)


def with_record(tmp_path, name, rec, refs=m.REFS, n=60):
    recs = list(m.served_records(n, seed=9))
    path = tmp_path / (name + ".bam")
    m.write(path, recs[:n // 2] + [rec] + recs[n // 2:], text=m.TEXT, refs=refs, piece=0x3000)
    return path


def test_each_decline_bit(ctx, files, tmp_path):
    """one file per bit, which sets that bit alone; nothing is written"""
    _, fasta, _, _ = files
    cases = m.stop_cases()
    # 1: an operation outside M I D = X — where a walk reaches it, and in the middle of a read whose tails never do
    for label in ("op S left", "op N right", "op H left", "op P right", "op code 9"):
        declined(ctx, with_record(tmp_path, "op", cases[label][1]), fasta, 1)
    declined(ctx, with_record(tmp_path, "spliced", m.record(b"spliced", 0, 100, [(0, 30), (3, 500), (0, 30)], [1] * 60, 0)), fasta, 1)
    # 2: an examined base outside the read, outside the chromosome
    declined(ctx, with_record(tmp_path, "read", cases["read index"][1]), fasta, 2)
    declined(ctx, with_record(tmp_path, "ref", cases["reference index"][1]), fasta, 2)
    declined(ctx, with_record(tmp_path, "neg", m.record(b"neg", 0, -1, [(0, 30)], [1] * 30, 0)), fasta, 2)
    # 4: a refID outside the header, below 0, or one whose name the index lacks; reference 0 without a chromosome; no references at all
    declined(ctx, with_record(tmp_path, "tid", cases["chromosome index"][1]), fasta, 4)
    declined(ctx, with_record(tmp_path, "tidneg", cases["negative chromosome index"][1]), fasta, 4)
    declined(ctx, with_record(tmp_path, "name", m.record(b"z", 3, 5, [(0, 30)], [1] * 30, 0), refs=m.REFS + [(b"chrZ", 900)]), fasta, 4)
    first = tmp_path / "first.bam"
    m.write(first, list(m.served_records(30, seed=9)), text=m.TEXT, refs=[(b"chrZ", 900)] + m.REFS)
    declined(ctx, first, fasta, 4)
    none = tmp_path / "none.bam"
    m.write(none, [m.record(b"u", -1, -1, [], [1, 2], 4)], text=b"", refs=[])
    declined(ctx, none, fasta, 4)
    # (a chromosome whose span ends beyond the FASTA file has none either)
    fai = [e if e[0] != b"chrB" else (e[0], e[1] * 50, e[2], e[3], e[4]) for e in m.fai_entries()]
    declined(ctx, files[3][0][0], fasta, 4, fai=fai)
    # 16: pos + the CIGAR's shift beyond the i32 range
    declined(ctx, with_record(tmp_path, "far", m.record(b"far", 0, (1 << 31) - 1, [(2, 5), (0, 30)], [1] * 30, 0)), fasta, 16)
    # 8: l_seq larger than the record holds
    bad = bytearray(m.record(b"bad", 0, 10, [(0, 20)], [1] * 20, 0))
    struct.pack_into("<i", bad, 20, 4000)
    declined(ctx, with_record(tmp_path, "bad", bytes(bad)), fasta, 8)


def test_an_unmapped_record_is_never_walked(ctx, files, tmp_path):
    """0x4 with a CIGAR the command would stop at, a refID outside the header and a position beyond every chromosome: written"""
    _, fasta, genome, _ = files
    path = with_record(tmp_path, "unmapped", m.record(b"u", 7, 1 << 30, [(4, 5), (0, 5), (9, 1)], [1] * 10, 4))
    raw = open_raw(path)
    check(ctx, path, fasta, raw, m.model(raw, genome), 20, m.f32(0.15))


def open_raw(path):
    return b"".join(x for x, _ in m.members(open(path, "rb").read()))


def test_loads_ranges(ctx, files):
    _, fasta, _, inputs = files
    path, raw = inputs[0]
    exp = expected_for("in", 20, "--threshold=0.15")
    loads = exp[4]
    res = ctx.bam_file_discard_tails(str(path), str(fasta), m.fai_entries(), 20, 3, m.co_line(20, m.f32(0.15)), 1, 0)
    n = res[5]
    assert res[0] and n == len(loads) > 100
    assert ctx.bam_file_discard_tails_loads(0, n) == loads and ctx.bam_file_discard_tails_loads(n, 0) == [] and ctx.bam_file_discard_tails_loads(0, 0) == []
    assert ctx.bam_file_discard_tails_loads(7, 5) == loads[7:12] and ctx.bam_file_discard_tails_loads(n - 1, 1) == loads[-1:]
    from seqkit_amd.capi import SeqkitHipError
    for first, k in ((0, n + 1), (n + 1, 0), (-1, 1), (1, -1), (n, 1), (5, n)):
        with pytest.raises(SeqkitHipError, match=r"failed \(-1\)"):
            ctx.bam_file_discard_tails_loads(first, k)
    out = b"".join(x for w in ctx.bam_file_rewrite_windows() for x, _ in m.members(w["bgzf"]))
    assert out == exp[0]
    assert ctx.bam_file_discard_tails_loads(0, n) == loads                                # after the last window too
    handled = ctx.bam_file_subsample(str(path), 1.0, 1, 1, 0)[0]                          # another file call ends it (this one declines: unpaired records)
    assert not handled
    with pytest.raises(SeqkitHipError):
        ctx.bam_file_discard_tails_loads(0, 1)


def test_scratch_in_its_own_buffer(ctx, files, monkeypatch, capfd):
    _, fasta, _, inputs = files
    path, raw = inputs[0]
    exp = expected_for("in", 33, "--threshold=0.15")
    monkeypatch.setenv("SK_BAMFILE_TRACE", "1")
    for own in (False, True):
        if own:
            monkeypatch.setenv("SK_TAILS_OWN_MEMORY", "1")
        capfd.readouterr()
        check(ctx, path, fasta, raw, exp, 33, m.f32(0.15))
        lines = [ln for ln in capfd.readouterr().err.split("\n") if "bytes of scratch in" in ln]
        assert len(lines) == 1 and lines[0].startswith("sk_bam_file_discard_tails: ")
        assert lines[0].endswith("its own buffer" if own else "the compressed file's buffer")


@pytest.mark.parametrize("T,level,fai", [(0, 1, None), (20, 2, None), (20, -1, None), (20, 1, [(b"chrA", 5000, 22, 0, 61)]), (20, 1, [(b"chrA", 5000, 22, 60, 59)])])
def test_invalid_arguments(ctx, files, T, level, fai):
    from seqkit_amd.capi import SeqkitHipError
    _, fasta, _, inputs = files
    with pytest.raises(SeqkitHipError, match=r"failed \(-1\)"):                        # SK_ERR_INVALID
        ctx.bam_file_discard_tails(str(inputs[0][0]), str(fasta), m.fai_entries() if fai is None else fai, T, 3, b"", level, 0)
