"""GPU: sk_bam_file_columns — a BAM file to device SoA columns — against what the tests wrote and the specification's reader;
its columns composed with the existing _dev kernels against the oracle."""
import gzip
import struct
import zlib

import numpy as np
import pytest

from seqkit_amd import capi, synth
from tests import bam_spec
from tests import cli_util as cu
from tests.test_gpu_inflate import bam_stream, cut_blocks

pytestmark = pytest.mark.gpu

KNOBS = (None, ("SK_BAMFILE_CHUNK_LOG2", "12"), ("SK_BAMFILE_NO_VMM", "1"))


def end_pos_rule(pos, cigar, l_name, block_size):
    """BamStream::next(..., want_end = true): pos + the lengths of M D N = X, in 64 bits, truncated to int32; pos when the variable
    part is shorter than the read name and the CIGAR."""
    if block_size - 32 < l_name + 4 * len(cigar):
        return pos
    e = pos + sum(ln for op, ln in cigar if op in (0, 2, 3, 7, 8))
    return int(np.array(e, dtype=np.int64).astype(np.int32))


def raw_records(raw, first):
    """(offset, block_size) of every record of an inflated stream"""
    out, o = [], first
    while o < len(raw):
        (bs,) = struct.unpack_from("<I", raw, o)
        out.append((o, bs))
        o += 4 + bs
    return out


def header_end(raw):
    at = 8 + struct.unpack_from("<i", raw, 4)[0]
    (n_ref,) = struct.unpack_from("<i", raw, at)
    at += 4
    for _ in range(n_ref):
        (ln,) = struct.unpack_from("<i", raw, at)
        at += 8 + ln
    return at


def expect_from_raw(raw, first):
    cols = {k: [] for k, _ in capi.BAM_COLUMNS}
    for o, bs in raw_records(raw, first):
        tid, pos, l_name, mapq, _bin, n_cigar, flag, _l_seq, mtid, mpos, tlen = struct.unpack_from("<iiBBHHHiiii", raw, o + 4)
        cig = []
        if bs - 32 >= l_name + 4 * n_cigar:
            for k in range(n_cigar):
                (op,) = struct.unpack_from("<I", raw, o + 36 + l_name + 4 * k)
                cig.append((op & 15, op >> 4))
        for name, v in (("flag", flag), ("mapq", mapq), ("tid", tid), ("mtid", mtid), ("pos", pos), ("mpos", mpos), ("tlen", tlen),
                        ("end_pos", end_pos_rule(pos, cig, l_name, bs) if cig or n_cigar == 0 else pos)):
            cols[name].append(v)
    return {k: np.array(v, dtype=dt) for (k, dt), v in zip(capi.BAM_COLUMNS, cols.values())}


def write_stream(path, raw, ends):
    with open(path, "wb") as f:
        lo = 0
        for e in ends:
            f.write(cu.bgzf_block(raw[lo:int(e)]))
            lo = int(e)
        f.write(cu.bgzf_block(b""))


def check_all_knobs(ctx, monkeypatch, path, expect, names):
    for knob in KNOBS:
        with monkeypatch.context() as m:
            if knob:
                m.setenv(*knob)
            handled, cols, ref_names, info = ctx.bam_file_columns(path)
            assert handled, (knob, info)
            assert info[3] == len(expect["flag"])
            for k, _ in capi.BAM_COLUMNS:
                assert np.array_equal(cols[k], expect[k]), (knob, k)
            assert ref_names == names


def test_columns_blocks_cut_anywhere(ctx, tmp_path, monkeypatch):
    """tests' writer: blocks of 60 000 bytes, records straddle them; CIGARs with every op code, a record too short for its CIGAR"""
    rng = np.random.default_rng(11)
    refs = [("chr1", 100000), ("chr2", 50000), ("chrM", 16000)]
    recs = []
    for i in range(20000):
        cig = [(int(rng.integers(0, 10)), int(rng.integers(0, 1 << 20 if i % 50 == 0 else 200))) for _ in range(int(rng.integers(0, 6)))]
        recs.append(dict(tid=int(rng.integers(-1, 3)), pos=int(rng.integers(-1, 1 << 31)), flag=int(rng.integers(0, 4096)), mtid=int(rng.integers(-1, 3)),
                         mpos=int(rng.integers(-1, 1 << 30)), tlen=int(rng.integers(-(1 << 31), 1 << 31)), mapq=int(rng.integers(0, 256)),
                         name="r%d" % i, cigar=cig, seq_len=int(rng.integers(0, 200))))
    recs.append(dict(tid=0, pos=(1 << 31) - 5, flag=0, mtid=0, mpos=0, tlen=0, cigar=[(0, (1 << 28) - 1), (8, (1 << 28) - 1)], seq_len=1))   # int32 wrap
    path = str(tmp_path / "a.bam")
    cu.write_bam(path, refs, recs)
    raw = b"".join(bam_spec.bgzf_blocks(open(path, "rb").read()))
    # a record whose variable part cannot hold its CIGAR: end_pos = pos (n_cigar of the last record patched upward)
    first = header_end(raw)
    raw = bytearray(raw)
    o_last = raw_records(bytes(raw), first)[-1][0]
    struct.pack_into("<H", raw, o_last + 16, 5000)
    raw = bytes(raw)
    write_stream(path, raw, list(range(60000, len(raw), 60000)) + [len(raw)])
    expect = expect_from_raw(raw, first)
    _, spec = bam_spec.read_bam(path)
    assert [r["flag"] for r in spec] == list(expect["flag"]) and [r["next_pos"] for r in spec] == list(expect["mpos"])
    assert expect["end_pos"][-1] == expect["pos"][-1]
    check_all_knobs(ctx, monkeypatch, path, expect, [b"chr1", b"chr2", b"chrM"])


def test_columns_blocks_on_record_boundaries(ctx, tmp_path, monkeypatch):
    path = str(tmp_path / "s.bam")
    n, flag, tid, mtid, tlen, reps = synth.write_bam_file(path, 20000, seed=3, unit_records=10000)
    _, spec = bam_spec.read_bam(path)
    assert len(spec) == n
    expect = {"flag": np.tile(flag, reps), "tid": np.tile(tid, reps), "mtid": np.tile(mtid, reps), "tlen": np.tile(tlen, reps),
              "mapq": np.full(n, 60, np.uint8), "pos": np.array([r["pos"] for r in spec], np.int32),
              "mpos": np.array([r["next_pos"] for r in spec], np.int32)}
    expect["end_pos"] = expect["pos"] + 150
    check_all_knobs(ctx, monkeypatch, path, expect, [b"chr%d" % (r + 1) for r in range(24)])


@pytest.mark.parametrize("mode", ["records", "anywhere"])
def test_columns_records_longer_than_a_block(ctx, tmp_path, monkeypatch, mode):
    rng = np.random.default_rng(21)
    raw, first, _ = bam_stream(rng, 3000)
    ends = cut_blocks(raw, first, rng, mode)
    path = str(tmp_path / "l.bam")
    write_stream(path, raw, ends)
    check_all_knobs(ctx, monkeypatch, path, expect_from_raw(raw, first), [b"chr1", b"chr2", b"chr3"])


def test_columns_subset_and_header(ctx, tmp_path):
    path = str(tmp_path / "h.bam")
    recs = [dict(tid=0, pos=i, flag=99, mtid=0, mpos=i, tlen=5, name="q%d" % i) for i in range(100)]
    cu.write_bam(path, [("chr1", 1000), ("weird\tname", 5)], recs)
    handled, dev, n, header, info = ctx.bam_file_columns_dev(path, capi.SK_COL["tid"] | capi.SK_COL["end_pos"])
    assert handled and n == 100 and sorted(dev) == ["end_pos", "tid"]
    assert all(p % 16 == 0 for p in dev.values())
    raw = b"".join(bam_spec.bgzf_blocks(open(path, "rb").read()))
    assert header == raw[:len(header)] and capi.bam_header_names(header) == [b"chr1", b"weird\tname"]
    handled, cols, names, _ = ctx.bam_file_columns(path, capi.SK_COL["pos"])
    assert handled and list(cols) == ["pos"] and list(cols["pos"]) == list(range(100))
    cu.write_bam(path, [("chr1", 1000)], [])
    handled, cols, names, info = ctx.bam_file_columns(path)
    assert handled and all(len(v) == 0 for v in cols.values()) and names == [b"chr1"]


def test_columns_not_handled(ctx, tmp_path):
    path = str(tmp_path / "a.bam")
    cu.write_bam(path, [("chr1", 1000)], [dict(tid=0, pos=i, flag=99, mtid=0, mpos=i, tlen=5) for i in range(5000)])
    data = open(path, "rb").read()
    for name, blob in (("cut.bam", data[:len(data) // 2]), ("plain.bam", b"BAM\1" + bytes(100)), ("gz.bam", zlib.compress(b"BAM\1" + bytes(1000))),
                       ("gzip.bam", gzip.compress(b"BAM\1" + bytes(1000)))):
        p = str(tmp_path / name)
        open(p, "wb").write(blob)
        handled, cols, names, info = ctx.bam_file_columns(p)
        assert not handled and cols == {} and names == [], name
    handled, *_ = ctx.bam_file_columns(str(tmp_path / "nope.bam"))
    assert not handled
    handled, cols, _, _ = ctx.bam_file_columns(path)                     # (and the ctx still serves a good file)
    assert handled and len(cols["flag"]) == 5000


def test_columns_compose_with_the_dev_kernels(ctx, oracle, tmp_path):
    path = str(tmp_path / "c.bam")
    rng = np.random.default_rng(9)
    recs = []
    for i in range(30000):
        recs.append(dict(tid=int(rng.integers(0, 3)), pos=i * 10, flag=int(rng.choice([99, 147, 83, 163, 1123, 4, 355, 2147, 65, 129, 0, 16])),
                         mtid=int(rng.integers(0, 3)), mpos=i * 10 + int(rng.integers(-300, 300)), tlen=int(rng.integers(-700, 700)),
                         mapq=int(rng.integers(0, 61)), cigar=[(0, int(rng.integers(1, 100))), (2, 3)], seq_len=5))
    cu.write_bam(path, [("chr1", 1 << 20), ("chr2", 1 << 20), ("chr3", 1 << 20)], recs)
    handled, dev, n, header, _ = ctx.bam_file_columns_dev(path)
    assert handled and n == len(recs)
    col = lambda k, dt: np.array([r[k] if k != "mapq" else r.get("mapq", 60) for r in recs], dtype=dt)
    flag, tid, mtid, tlen = col("flag", np.uint16), col("tid", np.int32), col("mtid", np.int32), col("tlen", np.int32)
    pos, mpos, mapq = col("pos", np.int32), col("mpos", np.int32), col("mapq", np.uint8)
    end_pos = np.array([r["pos"] + r["cigar"][0][1] + 3 for r in recs], dtype=np.int32)
    bits, kept = ctx.malloc_device((n + 7) // 8 + 16), ctx.malloc_device(16)
    try:
        ctx.copy_h2d(kept, np.zeros(2, dtype=np.uint64))
        ctx.bam_fragments_dev(dev["flag"], dev["tid"], dev["mtid"], dev["tlen"], n, 100, 500, bits, kept)
        ctx.sync()
        got = np.empty((n + 7) // 8, dtype=np.uint8)
        ctx.copy_d2h(got, bits)
        e = oracle.fragments_keep(flag, tid, mtid, tlen, 100, 500)
        assert np.array_equal(np.unpackbits(got, bitorder="little")[:n], e)
    finally:
        ctx.free_device(bits)
        ctx.free_device(kept)
    rng = np.random.default_rng(10)
    rchr = rng.integers(0, 3, 500).astype(np.int32)
    rstart = rng.integers(0, 300000, 500).astype(np.uint32)
    rend = rstart + rng.integers(0, 5000, 500).astype(np.uint32)
    order = np.argsort(rchr, kind="stable")
    chr_off = np.searchsorted(rchr[order], np.arange(4)).astype(np.int32)
    for single_end in (False, True):
        ctx.count_set_regions(chr_off, rstart[order], rend[order], order.astype(np.int32), 500)
        ctx.count_add_dev(dev["flag"], dev["mapq"], dev["tid"], dev["mtid"], dev["pos"], dev["mpos"], dev["tlen"], dev["end_pos"] if single_end else 0, n,
                          min_mapq=20, max_frag_len=600, single_end=single_end, center=single_end)
        got = ctx.count_get()
        e, code, _ = oracle.count_batch(flag, mapq, tid, mtid, pos, mpos, tlen, end_pos if single_end else None, 3, rchr, rstart, rend, min_mapq=20,
                                        max_frag_len=600, single_end=single_end, center=single_end)
        assert np.array_equal(got, e), single_end
