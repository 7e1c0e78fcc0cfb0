"""GPU: sk_bam_file_pairs / sk_bam_file_pairs_next — the mates of `sam to [interleaved] raw|fasta|fastq` paired on the device and the
texts written in output order — against tests/bam_pair_model.py (src/sam_to_fastq.rs:100-137) for which record goes where, and
tests/test_gpu_bam_reads.py's statement of write_read for each record's text: every stream byte for byte."""
import gzip
import random
import struct

import pytest

from seqkit_amd import capi
from tests import bam_pair_model as pm
from tests import cli_util as cu
from tests.test_gpu_bam_reads import text

pytestmark = pytest.mark.gpu

F1, F2 = 1 | 0x40, 1 | 0x80
FORMATS = ("raw", "fasta", "fastq")
BASE = dict(tid=0, mtid=0, pos=1, mpos=1, tlen=0)


def rec(name, flag, ln=4, seed=0, pos=1):
    """a record with real bases: ambiguity codes, qualities below and above the mask's 10"""
    codes = [(1, 2, 4, 8, 15, 3)[(seed + k) % 6] for k in range(ln)]
    qual = [(seed * 7 + k * 5) % 45 for k in range(ln)]
    return dict(BASE, pos=pos, flag=flag, name=name, codes=codes, qual=qual)


def name_of(r):
    return r["name"] if isinstance(r["name"], bytes) else r["name"].encode()


def expected(recs, fmt, interleaved):
    """{stream: bytes} as the command writes them (interleaved: one stream, the single output discarded)"""
    out_1, out_2, out_single = pm.pair([(r["flag"], name_of(r)) for r in recs])
    cat = lambda idx: b"".join(text(recs[i], fmt) for i in idx)
    if interleaved:
        return {0: cat(pm.interleave(out_1, out_2)), 1: b"", 2: b""}
    return {0: cat(out_1), 1: cat(out_2), 2: cat(out_single)}


def collect(ctx, path, fmt, interleaved, window_bytes=0):
    handled, counts, info = ctx.bam_file_pairs(str(path), fmt, 10, interleaved, window_bytes)
    if not handled:
        assert counts == [0] * 8
        return False, None, counts, [], info
    wins = list(ctx.bam_file_pairs_windows())
    streams, at = {0: [], 1: [], 2: []}, {0: 0, 1: 0, 2: 0}
    for k, w in enumerate(wins):
        assert w["n"] > 0 and w["first"] == at[w["stream"]]                 # each stream's windows continue one another
        assert k == 0 or wins[k - 1]["stream"] <= w["stream"]              # stream 1's first, then stream 2's, then the single stream's
        at[w["stream"]] += w["n"]
        streams[w["stream"]].append(w["text"])
    got = {s: b"".join(v) for s, v in streams.items()}
    assert [len(got[s]) for s in (0, 1, 2)] == counts[5:8]
    pairs, single, left_1, left_2 = counts[:4]
    assert [at[0], at[1], at[2]] == ([2 * pairs, 0, 0] if interleaved else [pairs, pairs, single + left_1 + left_2])
    return True, got, counts, wins, info


def check(ctx, path, recs, window_bytes=0, formats=FORMATS, modes=(False, True)):
    n_wins = 0
    for fmt in formats:
        for interleaved in modes:
            ok, got, counts, wins, info = collect(ctx, path, fmt, interleaved, window_bytes)
            assert ok, info
            assert got == expected(recs, fmt, interleaved), (fmt, interleaved, window_bytes)
            exp = pm.counts([(r["flag"], name_of(r)) for r in recs])
            if interleaved:
                exp[1] = 0                                                  # (unpaired records are not kept then)
            assert counts[:5] == exp
            n_wins = max(n_wins, len(wins))
    return n_wins


def mixed_records(n_names, seed):
    """per name one of: a pair (either mate first, both strands), an orphan of either kind, the same mate twice or three times before
    the other, three and four records of one name, an unpaired read, a paired read with neither mate flag, both mate flags, secondary
    and supplementary records between the mates; l_seq 0, odd and even; names that are prefixes of one another"""
    rnd = random.Random(seed)
    recs = []
    for i in range(n_names):
        name = "n%d" % i if i % 7 else "n%d" % (i // 7)                    # ("n1" .. "n9" are prefixes of "n10" ..; some names come twice)
        ln = rnd.choice([0, 1, 2, 3, 7, 36, 37, 150, 151])
        r = lambda flag: rec(name, flag | (0x10 if rnd.random() < 0.5 else 0), ln if rnd.random() < 0.8 else rnd.choice([0, 5, 64]), rnd.randrange(1000),
                             rnd.randrange(100000))
        shape = rnd.randrange(12)
        flags = ([F1, F2], [F2, F1], [F1], [F2], [F1, F1, F2], [F2, F2, F2, F1], [F1, F2, F1], [F1, F2, F2, F1], [0], [1], [1 | 0x40 | 0x80, F2],
                 [F1, F2 | 0x100, F1 | 0x800, F2])[shape]
        recs += [r(f) for f in flags]
    return recs


def ordered(recs, order, seed=3):
    if order == "name":
        return recs
    if order == "position":
        return sorted(recs, key=lambda r: r["pos"])                         # (stable: mates far apart, equal positions in name order)
    out = list(recs)
    random.Random(seed).shuffle(out)
    return out


@pytest.fixture(scope="module")
def mixed():
    return mixed_records(900, seed=5)


@pytest.mark.parametrize("order", ["name", "position", "shuffled"])
def test_pairs_against_model(ctx, tmp_path, mixed, order):
    recs = ordered(mixed, order)
    assert 1500 < len(recs) < 4000
    bam = tmp_path / "m.bam"
    cu.write_bam(str(bam), [("chr1", 100000)], recs)
    assert check(ctx, bam, recs) <= 3                                       # one window per stream
    assert check(ctx, bam, recs, window_bytes=4096) >= 20                   # mates, groups and rank ranges straddle many windows
    assert check(ctx, bam, recs, window_bytes=256, formats=("fastq",)) >= 100   # windows smaller than one record's text


def test_pairs_scratch_in_its_own_buffer(ctx, tmp_path, mixed, monkeypatch):
    recs = ordered(mixed, "shuffled", seed=9)
    bam = tmp_path / "o.bam"
    cu.write_bam(str(bam), [("chr1", 100000)], recs)
    monkeypatch.setenv("SK_PAIRS_OWN_MEMORY", "1")
    check(ctx, bam, recs, window_bytes=4096, formats=("fasta",))


# the kept-record counts at which a pass takes another path: a wave (64), the pairing kernels' workgroup (capi.PAIR_BLOCK = kPairBlock), and
# around the powers of two up to 8192, among which lie the tile sizes of the library scans and of the radix sort's single-workgroup path
SIZES = sorted({0, 1, 63, 64, 65} | {b + d for b in (capi.PAIR_BLOCK, 1024, 2048, 4096, 8192) for d in (-1, 0, 1)})


@pytest.mark.parametrize("n", SIZES)
def test_pairs_kept_record_counts(ctx, tmp_path, n):
    """n kept records among records that are not kept: pairs whose mates lie n / 2 records apart, a leftover when n is odd"""
    assert {255, 256, 257} <= set(SIZES)
    half = n // 2
    kept = [rec("r%d" % (k % half if half else 0), F1 if k < half else F2, 3 + k % 3, k) for k in range(2 * half)]
    if n & 1:
        kept.append(rec("odd", F2, 5, n))
    recs = []
    for k, r in enumerate(kept):
        recs.append(r)
        if k % 5 == 0:
            recs.append(rec("r%d" % k, F1 | 0x100, 2, k))                    # not kept
    recs.append(rec("tail", F2 | 0x800, 2, 0))
    bam = tmp_path / "k.bam"
    cu.write_bam(str(bam), [("chr1", 100000)], recs)
    ok, got, counts, wins, _ = collect(ctx, bam, "fasta", False, 4096)
    assert ok and counts[:5] == [half, 0, 0, n & 1, 0]
    assert got == expected(recs, "fasta", False)
    ok, got, counts, wins, _ = collect(ctx, bam, "raw", True)
    assert ok and got == expected(recs, "raw", True) and (wins == [] if half == 0 else len(wins) == 1)


def test_pairs_one_name_on_every_record(ctx, tmp_path):
    bam = tmp_path / "s.bam"
    alternating = [rec("same", F1 if k % 2 == 0 else F2, 2 + k % 4, k) for k in range(4096)]
    cu.write_bam(str(bam), [("chr1", 100000)], alternating)
    check(ctx, bam, alternating, window_bytes=4096, formats=("fastq",))
    assert collect(ctx, bam, "raw", False)[2][:5] == [2048, 0, 0, 0, 0]
    firsts = [rec("same", F1, 2 + k % 4, k) for k in range(4095)] + [rec("same", F2, 3, 7)]
    cu.write_bam(str(bam), [("chr1", 100000)], firsts)
    check(ctx, bam, firsts, formats=("fastq",))
    assert collect(ctx, bam, "raw", False)[2][:5] == [1, 0, 0, 0, 4094]      # the last first mate pairs, every other one was replaced
    runs = []                                                               # runs of one kind of every length up to 40, then the other kind
    for k in range(1, 41):
        runs += [rec("same", F1 if k % 2 else F2, 1 + k % 5, k + j) for j in range(k)]
    cu.write_bam(str(bam), [("chr1", 100000)], runs)
    check(ctx, bam, runs, window_bytes=1024)


def test_pairs_names_prefixes_and_lengths(ctx, tmp_path):
    long = b"L" * 254
    names = [b"a", b"ab", b"abc", b"b", long, long[:253], long[:253] + b"x", b"a"]
    recs = [rec(nm, F1, 3 + k, k) for k, nm in enumerate(names)] + [rec(nm, F2, 4 + k, k) for k, nm in reversed(list(enumerate(names)))]
    recs += [rec(b"c", F2, 0, 1), rec(b"c", F1 | 0x10, 0, 2), rec(b"d", F1 | 0x10, 9, 3), rec(b"d", F2 | 0x10, 11, 4)]   # l_seq 0, odd, reverse strand
    bam = tmp_path / "p.bam"
    cu.write_bam(str(bam), [("chr1", 100000)], recs)
    check(ctx, bam, recs)
    check(ctx, bam, recs, window_bytes=256)
    ok, got, *_ = collect(ctx, bam, "fastq", True)
    assert got[0].endswith(text(recs[-2], "fastq") + text(recs[-1], "fastq"))          # the pair completed last is written last


def test_pairs_key_collision_declines(ctx, tmp_path, mixed, monkeypatch):
    bam = tmp_path / "c.bam"
    cu.write_bam(str(bam), [("chr1", 100000)], mixed)
    monkeypatch.setenv("SK_PAIR_KEY_BITS", "4")                             # 16 keys for hundreds of names
    for interleaved in (False, True):
        ok, _, counts, _, info = collect(ctx, bam, "fastq", interleaved)
        assert not ok and info[5] == -94.0 and counts == [0] * 8
        with pytest.raises(capi.SeqkitHipError):                            # nothing to take: no window was written
            next(ctx.bam_file_pairs_windows())
    monkeypatch.setenv("SK_PAIR_KEY_BITS", "64")
    assert collect(ctx, bam, "fastq", False)[0]
    # two records of ONE name under a cut key are no collision
    two = [rec("x", F1, 3, 1), rec("x", F2, 3, 2)]
    cu.write_bam(str(bam), [("chr1", 100000)], two)
    monkeypatch.setenv("SK_PAIR_KEY_BITS", "1")
    check(ctx, bam, two)


def test_pairs_declines_where_reads_declines(ctx, tmp_path):
    bam = tmp_path / "d.bam"
    good = [rec("ok", F1, 2, 1), rec("ok", F2, 2, 2)]
    cases = [
        (dict(BASE, flag=F1, name=b"caf\xc3\xa9", codes=[1], qual=[30]), FORMATS),                 # a qname byte >= 0x80
        (dict(BASE, flag=1, name=b"bad\xff", codes=[1], qual=[30]), FORMATS),                      # ... in a record that is dropped, too
        (dict(BASE, flag=F2, name="q", codes=[1, 2], qual=[94 + 1, 30]), ("fastq",)),              # 33 + q >= 0x80
        (dict(BASE, flag=F1, name="long", codes=[1] * 65533), FORMATS),
    ]
    for bad, fmts in cases:
        cu.write_bam(str(bam), [("chr1", 1000)], good + [bad])
        for fmt in FORMATS:
            for interleaved in (False, True):
                handled, counts, _ = ctx.bam_file_pairs(str(bam), fmt, 10, interleaved)
                assert handled == (fmt not in fmts), (bad["name"], fmt)
                assert handled or counts == [0] * 8
    recs = good + [dict(BASE, flag=F2, name="q", codes=[1, 2], qual=[94, 223])]                  # 33 + q wraps below 0x80: served
    cu.write_bam(str(bam), [("chr1", 1000)], recs)
    check(ctx, bam, recs, formats=("fastq",))
    # a record cut short: its variable part no longer holds its bases and qualities
    cu.write_bam(str(bam), [("chr1", 1000)], good + [dict(BASE, flag=F1, name="short", seq_len=10, cigar=[(0, 10)] * 40)])
    raw = bytearray(gzip.decompress(bam.read_bytes()))
    at = raw.rfind(b"short\0") - 36
    struct.pack_into("<i", raw, at + 20, 10 + 200)
    with open(bam, "wb") as f:
        f.write(cu.bgzf_block(bytes(raw)) + cu.bgzf_block(b""))
    for fmt in FORMATS:
        assert not ctx.bam_file_pairs(str(bam), fmt)[0]


def test_pairs_bad_format_and_call_order(ctx, tmp_path):
    bam = tmp_path / "b.bam"
    recs = [rec("a", F1, 3, 1), rec("a", F2, 3, 2), rec("u", 0, 3, 3)]
    cu.write_bam(str(bam), [("chr1", 1000)], recs)
    for fmt in (3, -1):
        with pytest.raises(capi.SeqkitHipError):
            ctx.bam_file_pairs(str(bam), fmt)
    with pytest.raises(capi.SeqkitHipError):                                # no sk_bam_file_pairs in progress
        next(ctx.bam_file_pairs_windows())
    for other in (lambda: ctx.bam_file_columns(str(bam)), lambda: ctx.bam_file_reads(str(bam), "raw"),
                  lambda: ctx.bam_file_rewrite(str(bam), "trim qnames", 1, 0)):
        assert ctx.bam_file_pairs(str(bam), "raw", 10, False, 256)[0]
        wins = ctx.bam_file_pairs_windows()
        next(wins)                                                          # one window returned, the next on its way
        other()
        with pytest.raises(capi.SeqkitHipError):                            # another file call ends them: SK_ERR_INVALID
            next(wins)
    assert ctx.bam_file_pairs(str(bam), "raw")[0]                           # and a reads call's windows end with a pairs call
    assert ctx.bam_file_reads(str(bam), "raw")[0]
    assert ctx.bam_file_pairs(str(bam), "raw")[0]
    with pytest.raises(capi.SeqkitHipError):
        next(ctx.bam_file_reads_windows())
    check(ctx, bam, recs)
