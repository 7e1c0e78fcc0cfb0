"""GPU: sk_bam_file_pairs_gz / sk_bam_file_pairs_gz_next — the three streams of `sam to raw|fasta|fastq` deflated and framed on the
device — against tests/bam_pair_model.py and tests/test_gpu_bam_reads.py's text() for what each stream inflates to, zlib itself for
every member, and sk_bam_file_pairs on the same context for the bytes it would have handed out: all comparisons byte for byte."""
import pytest

from seqkit_amd import capi
from tests import cli_util as cu
from tests.bam_out_util import zlib_members
from tests.test_gpu_bam_pairs import FORMATS, F1, F2, collect, expected, mixed_records, ordered, rec
from tests.test_gpu_bam_reads import text

pytestmark = pytest.mark.gpu

BLOCK = 0xFF00                               # SK_DEFLATE_MAX_IN: the most text bytes of one member
REFS = [("chr1", 100000)]


def kinds(data):
    """BTYPE of every member's one DEFLATE block (0 stored, 1 fixed, 2 dynamic): bits 1-2 of the payload's first byte"""
    out, at = [], 0
    while at < len(data):
        out.append((data[at + 18] >> 1) & 3)
        at += int.from_bytes(data[at + 16:at + 18], "little") + 1
    return out


def collect_gz(ctx, path, fmt, level=1, window_bytes=0):
    """(handled, {stream: inflated bytes}, counts, windows, info); the windows of a stream continue one another, the streams come in
    order, every member is zlib's, no member is the empty EOF block, raw_bytes is what the window inflates to"""
    handled, counts, info = ctx.bam_file_pairs_gz(str(path), fmt, 10, level, window_bytes)
    if not handled:
        assert counts == [0] * 8
        return False, None, counts, [], info
    wins = list(ctx.bam_file_pairs_gz_windows())
    streams, at = {0: [], 1: [], 2: []}, {0: 0, 1: 0, 2: 0}
    for k, w in enumerate(wins):
        assert w["n"] > 0 and w["first"] == at[w["stream"]]
        assert k == 0 or wins[k - 1]["stream"] <= w["stream"]
        at[w["stream"]] += w["n"]
        mem = zlib_members(w["bgzf"])
        assert mem and all(0 < len(m) <= BLOCK for m in mem)
        assert all(len(m) == BLOCK for m in mem[:-1])                      # cut wherever the byte count falls
        assert sum(len(m) for m in mem) == w["raw_bytes"]
        if level == 0:
            assert set(kinds(w["bgzf"])) == {0}
        streams[w["stream"]].append(b"".join(mem))
    got = {s: b"".join(v) for s, v in streams.items()}
    assert [len(got[s]) for s in (0, 1, 2)] == counts[5:8]
    pairs, single, left_1, left_2 = counts[:4]
    assert [at[0], at[1], at[2]] == [pairs, pairs, single + left_1 + left_2]
    return True, got, counts, wins, info


@pytest.fixture(scope="module")
def mixed():
    """mixed_records(900, seed=5), the name count enlarged until the first mates' smallest text, raw, takes more than three blocks"""
    n = 900
    while True:
        recs = mixed_records(n, seed=5)
        if len(expected(recs, "raw", False)[0]) > 3 * BLOCK:
            return recs
        n *= 2


@pytest.fixture(scope="module")
def mixed_files(mixed, tmp_path_factory):
    """{order: (path, records, {format: the model's streams})}: written and computed once"""
    d = tmp_path_factory.mktemp("pairs_gz")
    out = {}
    for order in ("name", "position", "shuffled"):
        recs = ordered(mixed, order)
        path = d / (order + ".bam")
        cu.write_bam(str(path), REFS, recs)
        out[order] = (path, recs, {fmt: expected(recs, fmt, False) for fmt in FORMATS})
    return out


@pytest.mark.parametrize("order", ["name", "position", "shuffled"])
def test_pairs_gz_against_model_and_text_windows(ctx, mixed_files, order):
    path, recs, exp = mixed_files[order]
    for fmt in FORMATS:
        assert len(exp[fmt][0]) > 3 * BLOCK
        longest = max(len(text(r, fmt)) for r in recs)
        ok, text_streams, text_counts, _, _ = collect(ctx, path, fmt, False)
        assert ok and text_streams == exp[fmt]
        for window in (0, 4096):
            for level in (0, 1):
                ok, got, counts, wins, info = collect_gz(ctx, path, fmt, level, window)
                assert ok, info
                assert got == exp[fmt], (fmt, level, window)
                assert got == text_streams and counts == text_counts
                if window == 0:
                    assert [w["stream"] for w in wins] == [0, 1, 2]
                    assert len(zlib_members(wins[0]["bgzf"])) >= 4              # a window of several blocks
                else:
                    assert len(wins) >= 60 and all(w["raw_bytes"] < 4096 + longest for w in wins)   # (its records BEGIN in 4096 bytes)
                if level == 1:                                                  # (text that repeats: the deflater is not storing it all)
                    assert {k for w in wins for k in kinds(w["bgzf"])} & {1, 2}


def test_pairs_gz_block_count_edge(ctx, tmp_path):
    """65 280 text bytes are one member; one byte more is a second member of one byte"""
    recs = [rec("u%d" % k, 0, 1019, k) for k in range(64)]
    bam = tmp_path / "e.bam"
    for extra, sizes in ((0, [BLOCK]), (1, [BLOCK, 1])):
        recs[-1] = rec("u63", 0, 1019 + extra, 63)
        cu.write_bam(str(bam), REFS, recs)
        for level in (0, 1):
            ok, got, counts, wins, _ = collect_gz(ctx, bam, "raw", level)
            assert ok and counts[:5] == [0, 64, 0, 0, 0] and counts[7] == BLOCK + extra
            assert len(wins) == 1 and wins[0]["stream"] == 2
            assert [len(m) for m in zlib_members(wins[0]["bgzf"])] == sizes
            assert got == expected(recs, "raw", False)


def test_pairs_gz_record_larger_than_a_block_and_a_window(ctx, tmp_path):
    shorts = [rec("s%d" % (k // 2), F1 if k % 2 == 0 else F2, 5 + k % 40, k) for k in range(400)]
    recs = shorts[:200] + [rec("big", F1, 40000, 7)] + shorts[200:] + [rec("big", F2 | 0x10, 40000, 8)]
    bam = tmp_path / "l.bam"
    cu.write_bam(str(bam), REFS, recs)
    exp = expected(recs, "fastq", False)
    big = len(text(recs[200], "fastq"))
    assert big > BLOCK
    for window in (0, 4096):
        for level in (0, 1):
            ok, got, counts, wins, _ = collect_gz(ctx, bam, "fastq", level, window)
            assert ok and counts[:5] == [201, 0, 0, 0, 0] and got == exp
            if window:
                # (a window holds the records that BEGIN in its 4096 bytes of the stream: a short record may take it a little beyond)
                over = [w for w in wins if w["raw_bytes"] >= big]
                assert [w["stream"] for w in over] == [0, 1]                   # the window of each big mate
                assert all(w["raw_bytes"] < window + 128 for w in wins if w not in over)
                for w in over:
                    assert big <= w["raw_bytes"] < big + window and len(zlib_members(w["bgzf"])) == 2   # the record spans members
            else:
                assert len(wins) == 2 and all(len(zlib_members(w["bgzf"])) >= 2 for w in wins)


def test_pairs_gz_stored_and_deflated_members(ctx, mixed_files, tmp_path):
    """level 1 deflates what shrinks and stores what does not; level 0 stores every member"""
    path = mixed_files["shuffled"][0]
    seen = set()
    ok, _, _, wins, _ = collect_gz(ctx, path, "fastq", 1)
    assert ok
    for w in wins:
        seen.update(kinds(w["bgzf"]))
    assert seen & {1, 2}
    one = [rec("u", 0, 4, 1)]
    bam = tmp_path / "one.bam"
    cu.write_bam(str(bam), REFS, one)
    ok, got, _, wins, _ = collect_gz(ctx, bam, "raw", 1)
    assert ok and len(wins) == 1 and kinds(wins[0]["bgzf"]) == [0]             # five bytes do not shrink: stored
    assert got == expected(one, "raw", False)
    seen.update(kinds(wins[0]["bgzf"]))
    assert 0 in seen and seen & {1, 2}                                          # level 1 has both kinds
    for p, fmt in ((path, "fastq"), (bam, "raw")):                             # (collect_gz asserts it per window, too)
        ok, _, _, wins, _ = collect_gz(ctx, p, fmt, 0)
        assert ok and wins and all(set(kinds(w["bgzf"])) == {0} for w in wins)


def test_pairs_gz_empty_streams(ctx, tmp_path):
    bam = tmp_path / "p.bam"
    pairs = [rec("p%d" % (k // 2), F1 if k % 2 == 0 else F2, 6, k) for k in range(20)]
    cu.write_bam(str(bam), REFS, pairs)
    ok, got, counts, wins, _ = collect_gz(ctx, bam, "fasta")
    assert ok and [w["stream"] for w in wins] == [0, 1] and got == expected(pairs, "fasta", False) and got[2] == b""
    cu.write_bam(str(bam), REFS, [rec("x%d" % k, F1 | (0x100 if k % 2 else 0x800), 5, k) for k in range(30)])
    ok, got, counts, wins, _ = collect_gz(ctx, bam, "fastq")
    assert ok and wins == [] and counts == [0] * 8
    cu.write_bam(str(bam), REFS, [])
    ok, got, counts, wins, _ = collect_gz(ctx, bam, "raw")
    assert ok and wins == [] and counts == [0] * 8


def test_pairs_gz_declines_and_protocol(hip_lib, ctx, mixed_files, tmp_path, monkeypatch):
    import seqkit_amd
    path, recs, exp = mixed_files["shuffled"]
    fresh = seqkit_amd.Context(0)
    try:
        with pytest.raises(capi.SeqkitHipError):                                # before any call on the ctx
            next(fresh.bam_file_pairs_gz_windows())
    finally:
        fresh.close()
    monkeypatch.setenv("SK_PAIR_KEY_BITS", "4")                                 # 16 keys for thousands of names
    ok, _, counts, _, info = collect_gz(ctx, path, "fastq")
    assert not ok and info[5] == -94.0 and counts == [0] * 8
    with pytest.raises(capi.SeqkitHipError):                                    # nothing to take: no window exists
        next(ctx.bam_file_pairs_gz_windows())
    monkeypatch.delenv("SK_PAIR_KEY_BITS")
    small = tmp_path / "s.bam"
    few = [rec("a", F1, 30, 1), rec("a", F2, 30, 2), rec("u", 0, 30, 3)] * 20
    cu.write_bam(str(small), REFS, few)
    assert ctx.bam_file_pairs_gz(str(small), "raw", 10, 1, 256)[0]
    wins = ctx.bam_file_pairs_gz_windows()
    next(wins)                                                                  # one window returned, the next on its way
    ctx.bam_file_columns(str(small))
    with pytest.raises(capi.SeqkitHipError):                                    # another file call ends them
        next(wins)
    assert ctx.bam_file_pairs_gz(str(small), "raw")[0]
    with pytest.raises(capi.SeqkitHipError):                                    # the text windows' call does not take member windows
        next(ctx.bam_file_pairs_windows())
    assert ctx.bam_file_pairs(str(small), "raw")[0]
    with pytest.raises(capi.SeqkitHipError):                                    # nor the other way round
        next(ctx.bam_file_pairs_gz_windows())
    for fmt, level in ((3, 1), (-1, 1), ("raw", 2), ("raw", -1)):
        with pytest.raises(capi.SeqkitHipError):
            ctx.bam_file_pairs_gz(str(small), fmt, 10, level)
    # the ctx again: after a finished series, and after one that was abandoned with a window in flight
    ok, got, *_ = collect_gz(ctx, small, "fastq", 1, 256)
    assert ok and got == expected(few, "fastq", False)
    ok, got, *_ = collect_gz(ctx, path, "fastq", 1, 4096)
    assert ok and got == exp["fastq"]
    assert ctx.bam_file_pairs_gz(str(path), "fasta", 10, 1, 4096)[0]
    wins = ctx.bam_file_pairs_gz_windows()
    next(wins), next(wins)
    ok, got, *_ = collect_gz(ctx, small, "fasta", 1, 256)
    assert ok and got == expected(few, "fasta", False)
    ok, got, *_ = collect_gz(ctx, path, "raw", 0)
    assert ok and got == exp["raw"]
