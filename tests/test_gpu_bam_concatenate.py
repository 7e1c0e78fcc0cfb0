"""GPU: sk_bam_file_concatenate / sk_bam_file_rewrite_next — ONE input of `sam concatenate` per call, '.' and the input's number behind
every name, the header and the EOF block switched by the caller — chained over the inputs and held to the plain-Python loop of
tests/bam_concatenate_model.py.  The windows go through a checker of their own (taken): bam_out_util.checked_windows expects a header
and an EOF block in every call."""
import functools
import os
import struct

import pytest

from tests import bam_concatenate_model as m
from tests import bam_merge_model as merge_m
from tests import bam_minimize_model as mm
from tests import bam_subsample_model as sm
from tests.bam_out_util import zlib_members

pytestmark = pytest.mark.gpu

HEADER, EOF = 1, 2


def taken(ctx, res, flags):
    """the windows of a served call, checked against the protocol: (their bytes, their number)"""
    handled, n_rec, raw_bytes, info = res
    assert handled, info
    wins = list(ctx.bam_file_rewrite_windows())
    recs = [w for w in wins if w["n"]]
    at = 0
    for w in recs:                                                                    # the records, in order
        assert w["first"] == at and w["n"] > 0
        at += w["n"]
    assert at == n_rec
    empty = [i for i, w in enumerate(wins) if not w["n"]]
    if flags & HEADER:                                                                # the header's members first, in a window of their own
        assert empty == [0] and wins[0]["first"] == 0 and wins[0]["raw_bytes"] > 0
    elif flags & EOF and not recs:                                                    # nothing but the EOF block
        assert len(wins) == 1 and wins[0]["bgzf"] == m.EOF_BLOCK and wins[0]["raw_bytes"] == 0
    else:
        assert empty == []
    data = b"".join(w["bgzf"] for w in wins)
    assert data.count(m.EOF_BLOCK) == (1 if flags & EOF else 0) and data.endswith(m.EOF_BLOCK) == bool(flags & EOF)
    mem = m.members(data)
    assert all(0 < len(x) <= 0xFF00 for x, _ in (mem[:-1] if flags & EOF else mem))
    for w in wins:                                                                    # each window's members inflate to its raw bytes
        assert len(b"".join(x for x, _ in m.members(w["bgzf"]))) == w["raw_bytes"]
    assert sum(w["raw_bytes"] for w in wins) == raw_bytes
    return data, len(wins)


def chain(ctx, paths, level=1, window=0, first_number=1):
    """one call per input, HEADER on the first, EOF on the last: (the members of all, the sum of raw_bytes, records, windows)"""
    data, raw, n_rec, n_win = [], 0, 0, 0
    for b, p in enumerate(paths):
        flags = (HEADER if b == 0 else 0) | (EOF if b + 1 == len(paths) else 0)
        res = ctx.bam_file_concatenate(p, first_number + b, flags, level, window)
        d, nw = taken(ctx, res, flags)
        data.append(d)
        raw += res[2]
        n_rec += res[1]
        n_win += nw
    return b"".join(data), raw, n_rec, n_win


SIZES = [3000, 0, 1, 2500, 300, 7, 64, 65, 1000, 2, 0, 128, 500, 33, 1, 900]


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """16 files of 0, 1 and up to 3 000 unsorted records in 12 KiB pieces (records straddle blocks), their reference lists different"""
    d = tmp_path_factory.mktemp("concat")
    return m.write_all(d, m.served_inputs(16, SIZES, seed=11), piece=0x3000)


@functools.lru_cache(maxsize=None)
def _expected(raws):
    return m.model(list(raws))


@pytest.mark.parametrize("window", [0, 256, 64 << 10])
@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("k", [2, 3, 16])
def test_chained_calls_match_model(ctx, inputs, k, level, window):
    paths, raws = inputs
    exp, err, code = _expected(tuple(raws[:k]))
    assert (err, code) == (b"", 0)
    data, raw, n_rec, n_win = chain(ctx, paths[:k], level, window)
    out = b"".join(zlib_members(data))
    assert out == exp and raw == len(out) and n_rec == sum(SIZES[:k])
    mem = m.members(data)
    if level == 0:
        assert all(stored for _, stored in mem[:-1])
    elif window != 256:                                                               # (a window of 256 bytes is one member that a dynamic block does not shrink: stored)
        assert not all(stored for _, stored in mem[:-1])
    if window == 256:
        assert n_win > n_rec // 3
    if k == 16:
        assert {b"1", b"9", b"10", b"16"} <= {r[36:36 + r[12] - 1].rsplit(b".", 1)[1] for r in m.records(out)}


def alone(raw, number, flags):
    """what one call's members inflate to"""
    return (m.out_header(raw) if flags & HEADER else b"") + b"".join(m.with_suffix(r, number) for r in m.records(raw))


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_flags_one_by_one(ctx, inputs, flags):
    paths, raws = inputs
    for f in (4, 1):                                                                  # 300 records; none
        for window in (0, 4096):
            res = ctx.bam_file_concatenate(paths[f], 7, flags, 1, window)
            data, n_win = taken(ctx, res, flags)
            assert b"".join(zlib_members(data)) == alone(raws[f], 7, flags) and res[1] == SIZES[f] and res[2] == len(alone(raws[f], 7, flags))
            if SIZES[f] == 0:
                assert n_win == (0 if flags == 0 else 1)                              # no window at all; the EOF block alone; header members only (and the EOF block behind them)
                if flags == 0:
                    assert data == b""
                if flags == EOF:
                    assert data == m.EOF_BLOCK
                if flags == HEADER:
                    assert b"".join(x for x, _ in m.members(data)) == m.out_header(raws[f])


NUMBERS = [1, 9, 10, 99, 100, 1000, 4294967295]


@pytest.mark.parametrize("number", NUMBERS)
def test_digits_and_edges(ctx, tmp_path, number):
    """names of 1 byte up to exactly the longest that takes the suffix, record lengths of every residue mod 4 at every place mod 4 of the
    output: the edges of the dword copy under a suffix of 2, 3, 4, 5 and 11 bytes; a byte more in one name: declined"""
    sl = 1 + len(str(number))
    assert sl == {1: 2, 9: 2, 10: 3, 99: 3, 100: 4, 1000: 5, 4294967295: 11}[number]
    longest = 254 - sl
    recs = []
    for i in range(260):
        nl = 1 + (i * 7) % longest if i else longest
        recs.append(m.rm.record(bytes(65 + (i + k) % 26 for k in range(nl)), (i + sl) % 9, tid=i % 3 - 1, pos=(977 * i) % 5000,
                                aux=m.rm.aux_z(b"ZZ", b"y" * (i % 5)) if i % 5 else b"", seed=i))
    assert {len(r) % 4 for r in recs} == {0, 1, 2, 3} and {r[12] - 1 for r in recs} >= {1, longest}
    p = tmp_path / "edges.bam"
    raw = m.write(p, recs)
    for window in (0, 256):
        res = ctx.bam_file_concatenate(str(p), number, 3, 0, window)
        data, _ = taken(ctx, res, 3)
        assert b"".join(zlib_members(data)) == alone(raw, number, 3)
    recs[131] = m.rm.record(b"n" * (longest + 1), 5)
    m.write(p, recs)
    declined(ctx, str(p), number, 1)


def declined(ctx, path, number, bits):
    handled, n_rec, raw_bytes, info = ctx.bam_file_concatenate(path, number)
    assert not handled and info[5] == -(30 + bits) and (n_rec, raw_bytes) == (0, 0)
    from seqkit_amd.capi import SeqkitHipError
    with pytest.raises(SeqkitHipError):                                               # no windows were set up
        next(ctx.bam_file_rewrite_windows())


def test_declines_and_invalid_arguments(ctx, inputs, tmp_path):
    from seqkit_amd.capi import SeqkitHipError
    paths, raws = inputs
    inv = list(m.records(raws[4]))
    b = bytearray(inv[200])
    struct.pack_into("<i", b, 20, 4000)                                               # l_seq larger than the record holds
    inv[200] = bytes(b)
    p = tmp_path / "invalid.bam"
    m.write(p, inv, piece=0x3000)
    declined(ctx, str(p), 2, 8)
    for bad in (str(tmp_path), str(tmp_path / "none.bam")):                           # a directory, a missing path: the front half's declines
        handled, n_rec, raw_bytes, info = ctx.bam_file_concatenate(bad, 1)
        assert not handled and info[5] < 0 and (n_rec, raw_bytes) == (0, 0)
    for number, flags, level in ((0, 3, 1), (1, 4, 1), (1, -1, 1), (1, 3, 2), (1, 3, -1)):
        with pytest.raises(SeqkitHipError, match=r"failed \(-1\)"):                  # SK_ERR_INVALID
            ctx.bam_file_concatenate(paths[0], number, flags, level)
    data, raw, n_rec, _ = chain(ctx, paths[:3])                                       # and the ctx serves on
    assert b"".join(zlib_members(data)) == _expected(tuple(raws[:3]))[0]


def planned(value):
    """a context created with SK_PLAN_CUS=value in the environment, which is restored before this returns"""
    import seqkit_amd
    saved = os.environ.get("SK_PLAN_CUS")
    os.environ["SK_PLAN_CUS"] = value
    try:
        return seqkit_amd.Context(0)
    finally:
        if saved is None:
            os.environ.pop("SK_PLAN_CUS", None)
        else:
            os.environ["SK_PLAN_CUS"] = saved


@pytest.mark.parametrize("cus", [1, 3])
def test_capped_grids(ctx, tmp_path, cus):
    """A context that plans for 1 or 3 CUs: the front half's block kernels (a block a wave, 64 blocks a planned CU and trip) and the
    window writer (a record a group of 16 lanes, 256 records a planned CU and trip) loop three times or more over one input and one
    window of it.  (The sizing pass is a wave per block at any CU count, as the merge's key pass is: its grid is not capped.)"""
    files = m.served_inputs(2, [6000, 900], seed=23)
    paths, raws = m.write_all(tmp_path, files, piece=1024)
    n_blocks = len(m.members(open(paths[0], "rb").read())) - 1
    assert n_blocks >= 3 * 64 * cus and len(files[0]) >= 3 * 256 * cus
    exp = m.model(raws)[0]
    small = planned(str(cus))
    try:
        assert small.planned_cus() == cus
        data, raw, n_rec, n_win = chain(small, paths, 1, 0)
        assert n_win == 3                                                             # the header, input 1 in one window, input 2 in one
        got = b"".join(zlib_members(data))
    finally:
        small.close()
    ref = b"".join(zlib_members(chain(ctx, paths, 1, 0)[0]))
    assert got == exp and got == ref and n_rec == 6900


def test_the_ctx_is_left_as_found(ctx, inputs, tmp_path):
    """minimize --read-ids and subsample give identical windows before and after concatenate calls; a concatenate call started while an
    earlier one's windows are unread disturbs neither; a merge call after it is served"""
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
    exp0 = alone(raws[0], 5, 3)
    res = ctx.bam_file_concatenate(paths[0], 5, 3, 1, 4096)
    assert res[0]
    it = ctx.bam_file_rewrite_windows()
    part = [next(it)["bgzf"] for _ in range(5)]                                       # windows in flight, then another call on the ctx
    assert exp0.startswith(b"".join(x for x, _ in m.members(b"".join(part)))) and len(part[0]) > 0
    res = ctx.bam_file_concatenate(paths[3], 12, 2, 1, 4096)
    assert b"".join(zlib_members(taken(ctx, res, 2)[0])) == alone(raws[3], 12, 2)
    data, _, _, _ = chain(ctx, paths, 1, 4096)
    assert b"".join(zlib_members(data)) == _expected(tuple(raws))[0]
    assert others() == before
    res = ctx.bam_file_concatenate(paths[0], 1, 0, 1, 256)                            # and left with windows unread
    assert res[0] and next(ctx.bam_file_rewrite_windows())["bgzf"]
    assert others() == before
    # a merge on the ctx afterwards (sorted inputs with one reference list: its own generator's)
    files = merge_m.served_inputs(2, [400, 300], seed=5)
    mpaths = [str(tmp_path / ("m%d.bam" % i)) for i in range(2)]
    mraws = [merge_m.write(p, f) for p, f in zip(mpaths, files)]
    res = ctx.bam_file_merge(mpaths, True, 1, 0)
    assert res[0]
    out = b"".join(zlib_members(b"".join(w["bgzf"] for w in ctx.bam_file_rewrite_windows())))
    assert out == merge_m.model(mraws, True)[0]
