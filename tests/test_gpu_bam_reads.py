"""GPU: sk_bam_file_reads / sk_bam_file_reads_next — the texts of `sam to raw|fasta|fastq`, written on the device from the inflated
BAM file — against a plain-Python statement of src/sam_to_fastq.rs:31-59 (sequence) and :138-149 (write_read)."""
import gzip
import struct

import pytest

from tests import cli_util as cu
from tests.test_cli_gpu import reads_bam

pytestmark = pytest.mark.gpu

FWD = {1: "A", 2: "C", 4: "G", 8: "T"}
REV = {1: "T", 2: "G", 4: "C", 8: "A"}


def sequence(codes, qual, flag, min_baseq=10):
    """src/sam_to_fastq.rs:31-59: reverse reads from l_seq - 1 down, masked by the quality at the stored position"""
    ks = range(len(codes) - 1, -1, -1) if flag & 0x10 else range(len(codes))
    m = REV if flag & 0x10 else FWD
    return "".join("N" if qual[k] < min_baseq else m.get(codes[k], "N") for k in ks).encode()


def text(rec, fmt):
    """write_read (:138-149) for one record: QUAL is 33 + q in u8 arithmetic, stored order"""
    codes = rec.get("codes") or []
    qual = rec.get("qual", [30] * len(codes))
    name = rec["name"] if isinstance(rec["name"], bytes) else rec["name"].encode()
    seq = sequence(codes, qual, rec["flag"])
    if fmt == "fastq":
        return b"@" + name + b"\n" + seq + b"\n+\n" + bytes((33 + q) & 0xFF for q in qual) + b"\n"
    if fmt == "fasta":
        return b">" + name + b"\n" + seq + b"\n"
    return seq + b"\n"


def model(recs, fmt, want_unpaired):
    """the kept records in file order: (kind, name, text)"""
    out = []
    for r in recs:
        f = r["flag"]
        if f & 0x900:
            continue
        kind = 0 if not f & 1 else 1 if f & 0x40 else 2 if f & 0x80 else 3
        if kind == 3 or (kind == 0 and not want_unpaired):
            continue
        name = r["name"] if isinstance(r["name"], bytes) else r["name"].encode()
        out.append((kind, name, text(r, fmt)))
    return out


def collect(ctx, path, fmt, want_unpaired=True, window_bytes=0):
    handled, n_kept, text_bytes, info = ctx.bam_file_reads(str(path), fmt, 10, want_unpaired, window_bytes)
    if not handled:
        return False, None, info
    wins = list(ctx.bam_file_reads_windows())
    at = 0
    for w in wins:                                     # first / n continuous, offsets consistent
        assert w["first"] == at and w["n"] > 0
        at += w["n"]
        assert w["text_off"][0] == 0 and int(w["text_off"][-1]) == len(w["text"])
        assert w["name_off"][0] == 0 and int(w["name_off"][-1]) == len(w["names"])
    assert at == n_kept
    assert sum(len(w["text"]) for w in wins) == text_bytes
    recs = []
    for w in wins:
        for j in range(w["n"]):
            t = w["text"][int(w["text_off"][j]):int(w["text_off"][j + 1])]
            nm = w["names"][int(w["name_off"][j]):int(w["name_off"][j + 1])]
            recs.append((int(w["kind"][j]), nm, t, int(w["key"][j])))
    return True, (recs, wins), info


def check_against_model(ctx, path, recs, fmt, want_unpaired, window_bytes=0):
    ok, got, info = collect(ctx, path, fmt, want_unpaired, window_bytes)
    assert ok, info
    rows, wins = got
    exp = model(recs, fmt, want_unpaired)
    assert [(k, n, t) for k, n, t, _ in rows] == exp
    keys = {}
    for _, n, _, key in rows:                          # equal names, equal keys
        assert keys.setdefault(n, key) == key
    return rows, wins


@pytest.mark.parametrize("fmt", ["raw", "fasta", "fastq"])
@pytest.mark.parametrize("want_unpaired", [True, False])
def test_reads_against_model(ctx, tmp_path, fmt, want_unpaired):
    bam = tmp_path / "r.bam"
    recs = reads_bam(str(bam), 2500, seed=7, sort="shuffled")
    rows, wins = check_against_model(ctx, bam, recs, fmt, want_unpaired)
    assert len(wins) == 1 and len(rows) > 4000
    rows, wins = check_against_model(ctx, bam, recs, fmt, want_unpaired, window_bytes=4096)
    assert len(wins) >= 24


def test_reads_codes_strands_lengths_and_block_spans(ctx, tmp_path):
    recs = []
    for i in range(600):
        ln = [0, 1, 2, 3, 5, 17, 150, 301, 4000][i % 9]
        codes = [(i + k) % 16 for k in range(ln)]       # codes 0 and 3..15 become N
        qual = [(k * 7 + i) % 50 for k in range(ln)]
        if i % 13 == 0:
            qual = [255] * ln                           # absent: 33 + 255 wraps to a space
        flag = [0, 16, 1 | 64, 1 | 128 | 16, 1 | 64 | 16, 1 | 128][i % 6]
        recs.append(dict(tid=0, mtid=0, pos=i, mpos=0, tlen=0, flag=flag, name=f"r{i // 2}", codes=codes, qual=qual))
    bam = tmp_path / "c.bam"
    cu.write_bam(str(bam), [("chr1", 1000)], recs)      # 60 000-byte BGZF blocks: records straddle them
    for fmt in ("raw", "fasta", "fastq"):
        check_against_model(ctx, bam, recs, fmt, True, window_bytes=3000)
    # a reverse read: the mask uses the stored-position quality, QUAL stays in stored order
    r = dict(tid=0, mtid=0, pos=0, mpos=0, tlen=0, flag=16, name="rv", codes=[1, 2, 4, 8], qual=[30, 5, 30, 30])
    cu.write_bam(str(bam), [("chr1", 1000)], [r])
    rows, _ = check_against_model(ctx, bam, [r], "fastq", True)
    assert rows[0][2] == b"@rv\nACNT\n+\n?&??\n"


def test_reads_nothing_kept(ctx, tmp_path):
    bam = tmp_path / "s.bam"
    recs = [dict(tid=0, mtid=0, pos=i, mpos=0, tlen=0, flag=[256, 2048, 1 | 64 | 256][i % 3], name=f"s{i}", codes=[1, 2], qual=[30, 30])
            for i in range(50)]
    cu.write_bam(str(bam), [("chr1", 1000)], recs)
    handled, n_kept, text_bytes, _ = ctx.bam_file_reads(str(bam), "fastq")
    assert handled and n_kept == 0 and text_bytes == 0
    assert list(ctx.bam_file_reads_windows()) == []
    # paired records flagged neither first nor last, and unpaired ones without want_unpaired: nothing either
    recs = [dict(tid=0, mtid=0, pos=i, mpos=0, tlen=0, flag=[1, 0, 16][i % 3], name=f"s{i}", codes=[1], qual=[30]) for i in range(30)]
    cu.write_bam(str(bam), [("chr1", 1000)], recs)
    ok, (rows, wins), _ = collect(ctx, bam, "raw", want_unpaired=False)
    assert ok and rows == [] and wins == []


def test_reads_declines(ctx, tmp_path):
    bam = tmp_path / "d.bam"
    base = dict(tid=0, mtid=0, pos=1, mpos=1, tlen=0)
    good = dict(base, flag=1 | 64, name="ok", codes=[1, 2], qual=[30, 30])
    cases = [
        ([good, dict(base, flag=0, name=b"caf\xc3\xa9", codes=[1], qual=[30])], ("raw", "fasta", "fastq")),            # valid non-ASCII too
        ([good, dict(base, flag=1, name=b"bad\xff", codes=[1], qual=[30])], ("raw", "fasta", "fastq")),                # dropped record, still panics
        ([good, dict(base, flag=0, name="q", codes=[1, 2], qual=[95, 30])], ("fastq",)),
        ([good, dict(base, flag=0, name="q", codes=[1, 2], qual=[30, 222])], ("fastq",)),
        ([good, dict(base, flag=0, name="long", codes=[1] * 65533)], ("raw", "fasta", "fastq")),
    ]
    for recs, fmts in cases:
        cu.write_bam(str(bam), [("chr1", 1000)], recs)
        for fmt in ("raw", "fasta", "fastq"):
            handled, *_ = ctx.bam_file_reads(str(bam), fmt)
            assert handled == (fmt not in fmts), (recs[1]["name"], fmt)
    # q = 94 and 223 (33 + q wraps below 0x80) stay on the device
    recs = [good, dict(base, flag=0, name="q", codes=[1, 2], qual=[94, 223])]
    cu.write_bam(str(bam), [("chr1", 1000)], recs)
    check_against_model(ctx, bam, recs, "fastq", True)
    # a secondary record with a bad name is skipped before the name is read (:102)
    recs = [good, dict(base, flag=256, name=b"x\xff", codes=[1], qual=[30])]
    cu.write_bam(str(bam), [("chr1", 1000)], recs)
    check_against_model(ctx, bam, recs, "fasta", True)
    # a variable part shorter than name + CIGAR + seq + qual: a record htslib rejects
    cu.write_bam(str(bam), [("chr1", 1000)], [good, dict(base, flag=0, name="short", seq_len=10, cigar=[(0, 10)] * 40)])
    raw = bytearray(gzip.decompress(bam.read_bytes()))
    at = raw.rfind(b"short\0") - 36                   # l_seq grows: the record no longer holds its bases and qualities
    struct.pack_into("<i", raw, at + 20, 10 + 200)
    with open(bam, "wb") as f:
        f.write(cu.bgzf_block(bytes(raw)) + cu.bgzf_block(b""))
    for fmt in ("raw", "fasta", "fastq"):
        handled, *_ = ctx.bam_file_reads(str(bam), fmt)
        assert not handled


def test_reads_bad_format_and_no_call(ctx, tmp_path):
    from seqkit_amd import capi
    bam = tmp_path / "b.bam"
    cu.write_bam(str(bam), [("chr1", 1000)], [dict(tid=0, mtid=0, pos=1, mpos=1, tlen=0, flag=0, name="a", codes=[1], qual=[30])])
    with pytest.raises(capi.SeqkitHipError):
        ctx.bam_file_reads(str(bam), 3)
    with pytest.raises(capi.SeqkitHipError):
        ctx.bam_file_reads(str(bam), -1)
    # another file call ends the windows of the last one
    handled, *_ = ctx.bam_file_reads(str(bam), "raw")
    assert handled
    ctx.bam_file_columns(str(bam))
    with pytest.raises(capi.SeqkitHipError):
        list(ctx.bam_file_reads_windows())


def test_reads_windows_left_then_a_larger_range(ctx, tmp_path, monkeypatch):
    """windows left in flight (one being written, one returned), then a file call whose inflated stream needs a larger range than the
    last one reserved: the range is given back and taken again only after the window in flight has ended"""
    small, big = tmp_path / "s.bam", tmp_path / "b.bam"
    recs_s = reads_bam(str(small), 800, seed=11, sort="shuffled")
    recs_b = reads_bam(str(big), 12000, seed=12, sort="shuffled")
    # SK_BAMFILE_OUT_FACTOR sets the inflated stream's room to file size x factor (the range is reserved in 512 MiB pieces)
    assert big.stat().st_size * 1100 > (640 << 20)
    monkeypatch.setenv("SK_BAMFILE_OUT_FACTOR", "1")
    handled, *_ = ctx.bam_file_reads(str(small), "fastq", 10, True, 1024)
    assert handled
    wins = ctx.bam_file_reads_windows()
    next(wins)                                         # window 0 returned, window 1 on its way
    monkeypatch.setenv("SK_BAMFILE_OUT_FACTOR", "1100")
    check_against_model(ctx, big, recs_b, "fastq", True, window_bytes=1 << 16)
    monkeypatch.setenv("SK_BAMFILE_OUT_FACTOR", "1")
    check_against_model(ctx, small, recs_s, "fasta", True, window_bytes=2048)


def test_reads_next_after_another_file_call_is_invalid(ctx, tmp_path):
    """the reads twin of test_gpu_bam_rewrite.py's: a rewrite call between sk_bam_file_reads and its windows ends them"""
    from seqkit_amd.capi import SeqkitHipError
    bam = tmp_path / "r.bam"
    reads_bam(str(bam), 200, seed=13)
    assert ctx.bam_file_reads(str(bam), "fastq")[0]
    assert ctx.bam_file_rewrite(str(bam), "trim qnames", 1, 0)[0]
    with pytest.raises(SeqkitHipError):
        next(ctx.bam_file_reads_windows())
