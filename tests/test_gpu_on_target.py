"""GPU: sk_on_target_set_regions / _add / _add_dev / _get (`sam statistics --on-target`, S1 + S2 over record columns) against the
reference's sweep as tests/bam_on_target_model.py states it."""
import numpy as np
import pytest

from tests import bam_on_target_model as om

pytestmark = pytest.mark.gpu

DTYPES = dict(flag=np.uint16, tid=np.int32, mtid=np.int32, pos=np.int32, mpos=np.int32, tlen=np.int32, end_pos=np.int32)
# around the four-record group (3, 4, 5), the wave and the workgroup (255 .. 257), one workgroup's 1 024 records (1023, 1025), and one
# size above a grid of one workgroup a CU (256 x 1 024 records) so that the grid-stride loop turns over
SIZES = [0, 1, 3, 4, 5, 255, 256, 257, 1023, 1025, 300_000]


def columns(recs):
    return {name: np.array([r[k] for r in recs], dtype=dt) for k, (name, dt) in enumerate(DTYPES.items())}


def set_regions(ctx, regions_by_tid):
    chr_off = np.cumsum([0] + [len(rs) for rs in regions_by_tid]).astype(np.int32)
    flat = [r for rs in regions_by_tid for r in rs]
    ctx.on_target_set_regions(chr_off, np.array([s for s, _ in flat], dtype=np.int64), np.array([e for _, e in flat], dtype=np.int64))


def add(ctx, cols, max_frag_len=om.MAX_FRAG_LEN):
    ctx.on_target_add(*[cols[name] for name in DTYPES], max_frag_len=max_frag_len)


def got(ctx):
    return [int(x) for x in ctx.on_target_get()]


@pytest.fixture(scope="module")
def master():
    """the crafted records, then drawn ones; the model's counters of every prefix the tests use, computed once"""
    recs = om.crafted_records()
    recs += om.drawn_records(max(SIZES) - len(recs), seed=7)
    empty = [[] for _ in om.CRAFTED_BED]
    want = {(n, kind): om.sweep(recs[:n], bed) for n in SIZES for kind, bed in (("crafted", om.CRAFTED_BED), ("empty", empty))}
    return recs, columns(recs), want


class Dev:
    """device copies of host columns at a byte offset; freed at the end"""

    def __init__(self, ctx):
        self.ctx, self.ptrs = ctx, []

    def put(self, a, skip_elems=0):
        a = np.ascontiguousarray(a)
        p = self.ctx.malloc_device(a.nbytes + 64)
        assert p % 16 == 0
        q = p + skip_elems * a.itemsize
        if a.nbytes:
            self.ctx.copy_h2d(q, a)
        self.ptrs.append(p)
        return q

    def close(self):
        self.ctx.sync()
        for p in self.ptrs:
            self.ctx.free_device(p)


@pytest.fixture
def dev(ctx):
    d = Dev(ctx)
    yield d
    d.close()


@pytest.mark.parametrize("kind", ["crafted", "empty"])
@pytest.mark.parametrize("n", SIZES)
def test_column_lengths(ctx, master, n, kind):
    recs, cols, want = master
    set_regions(ctx, om.CRAFTED_BED if kind == "crafted" else [[] for _ in om.CRAFTED_BED])
    add(ctx, {k: v[:n] for k, v in cols.items()})
    assert got(ctx) == want[n, kind] + [0]
    if n >= 1025 and kind == "crafted":
        assert 0 < want[n, kind][4] < want[n, kind][3]


@pytest.mark.parametrize("n", [5, 257, 1025])
def test_host_columns_at_an_odd_element_offset(ctx, master, n):
    recs, cols, want = master
    set_regions(ctx, om.CRAFTED_BED)
    odd = {}
    for name, a in cols.items():
        big = np.zeros(n + 3, dtype=a.dtype)
        big[1:n + 1] = a[:n]
        odd[name] = big[1:n + 1]
        assert odd[name].ctypes.data % 16 != 0
    add(ctx, odd)
    assert got(ctx) == want[n, "crafted"] + [0]


@pytest.mark.parametrize("skip", [0, 1, 3])
@pytest.mark.parametrize("n", [5, 257, 1025, 300_000])
def test_device_columns_narrow_and_wide_loads(ctx, dev, master, n, skip):
    """skip = 0: 16-byte aligned columns, the wide loads; an odd element offset: the narrow-load path"""
    recs, cols, want = master
    set_regions(ctx, om.CRAFTED_BED)
    ptrs = [dev.put(cols[name][:n], skip) for name in DTYPES]
    assert all((p % 16 == 0) == (skip == 0) for p in ptrs)
    ctx.on_target_add_dev(*ptrs, n)
    assert got(ctx) == want[n, "crafted"] + [0]
    # one column off its alignment is enough for the narrow path
    if skip:
        set_regions(ctx, om.CRAFTED_BED)
        ptrs[1:] = [dev.put(cols[name][:n]) for name in list(DTYPES)[1:]]
        ctx.on_target_add_dev(*ptrs, n)
        assert got(ctx) == want[n, "crafted"] + [0]


def test_edge_values_one_record_a_call(ctx):
    """every edge record alone: a wrong answer cannot hide in a sum"""
    recs = om.edge_records()
    set_regions(ctx, om.CRAFTED_BED)
    acc = [0, 0, 0, 0, 0]
    for r in recs:
        add(ctx, columns([r]))
        acc = [a + b for a, b in zip(acc, om.sweep([r], om.CRAFTED_BED))]
        assert got(ctx) == acc + [0], r
    assert acc == om.sweep(recs, om.CRAFTED_BED)
    # the arithmetic is 64-bit: pos = INT32_MAX with tlen = 5000 reaches the region at 2^31, tlen = INT32_MIN is 2^31 > 5000
    set_regions(ctx, om.CRAFTED_BED)
    add(ctx, columns([(0x41, 3, 3, om.I32_MAX, om.I32_MAX, 5000, 0)]))
    assert got(ctx) == [1, 1, 0, 1, 1, 0]
    add(ctx, columns([(0x41, 3, 3, 150, 150, om.I32_MIN, 0)]))
    assert got(ctx) == [2, 2, 0, 1, 1, 0]
    add(ctx, columns([(0x41, 3, 3, 150, 150, 5000, 0), (0x41, 3, 3, 150, 150, -5000, 0), (0x41, 3, 3, 150, 150, 5001, 0), (0x41, 3, 3, 150, 150, -5001, 0)]))
    assert got(ctx) == [6, 6, 0, 3, 3, 0]


def test_max_frag_len_is_the_callers(ctx):
    recs = [(0x41, 1, 1, 1500, 1500, t, 0) for t in (0, 7, -7, 8, -8, om.I32_MIN, om.I32_MAX)]
    for m in (0, 7, 5000, (1 << 31) - 1, 1 << 31, 1 << 40):
        set_regions(ctx, om.CRAFTED_BED)
        add(ctx, columns(recs), max_frag_len=m)
        assert got(ctx) == om.sweep(recs, om.CRAFTED_BED, max_frag_len=m) + [0], m


def test_tid_out_of_range(ctx, master):
    n_chr = len(om.CRAFTED_BED)
    recs = om.drawn_records(5000, seed=11, bad_tids=(-1, -1, n_chr, n_chr, n_chr + 7, om.I32_MIN, om.I32_MAX))
    recs += [(0, -1, -1, 10, 0, 0, 20), (0, n_chr, -1, 10, 0, 0, 20), (0x41, -1, -1, 10, 10, 5, 0), (0x41, n_chr, n_chr, 10, 10, 5, 0)]
    bad = []
    want = om.sweep(recs, om.CRAFTED_BED, bad=bad)
    assert len(bad) > 100 and {r[1] for r in bad} >= {-1, n_chr}
    set_regions(ctx, om.CRAFTED_BED)
    add(ctx, columns(recs))
    assert got(ctx) == want + [len(bad)]
    with pytest.raises(om.BadTid):
        om.sweep(recs, om.CRAFTED_BED)
    # the same tids on records the filters drop
    dropped = [r for t in (-1, n_chr, om.I32_MAX) for r in ((0x4, t, -1, 10, 0, 0, 20), (0x100, t, -1, 10, 0, 0, 20), (0x800, t, -1, 10, 0, 0, 20),
                                                            (0x9, t, t, 10, 10, 5, 20), (0x1, t, 0, 10, 10, 5, 20), (0x1, t, t, 10, 10, 5, 20),
                                                            (0x41, t, t, 11, 10, 5, 20), (0x41, t, t, 10, 10, 5001, 20))]
    set_regions(ctx, om.CRAFTED_BED)
    add(ctx, columns(dropped))
    assert got(ctx) == om.sweep(dropped, om.CRAFTED_BED) + [0]
    # no reference at all: every fragment is out of range
    set_regions(ctx, [])
    add(ctx, columns(recs[:1000]))
    bad = []
    assert got(ctx) == om.sweep(recs[:1000], [], bad=bad) + [len(bad)] and bad


def test_accumulation_and_clear(ctx, master):
    recs, cols, want = master
    n = 1025
    set_regions(ctx, om.CRAFTED_BED)
    add(ctx, {k: v[:400] for k, v in cols.items()})
    assert got(ctx) == om.sweep(recs[:400], om.CRAFTED_BED) + [0]
    add(ctx, {k: v[400:n] for k, v in cols.items()})
    assert got(ctx) == want[n, "crafted"] + [0]
    add(ctx, {k: v[:0] for k, v in cols.items()})
    assert got(ctx) == want[n, "crafted"] + [0]
    set_regions(ctx, om.CRAFTED_BED)                                        # clears
    assert got(ctx) == [0] * 6
    add(ctx, {k: v[:n] for k, v in cols.items()})
    assert got(ctx) == want[n, "crafted"] + [0]


def test_many_chunks_of_the_host_entry(ctx, master, monkeypatch):
    """the host entry's chunk pipeline: both lanes and both workspace halves add to the same six counters"""
    recs, cols, want = master
    monkeypatch.setenv("SK_HOST_CHUNK_LOG2", "7")
    set_regions(ctx, om.CRAFTED_BED)
    add(ctx, {k: v[:1025] for k, v in cols.items()})
    assert got(ctx) == want[1025, "crafted"] + [0]


def test_regions_in_any_order(ctx, master):
    recs, cols, want = master
    shuffled = [list(reversed(rs)) for rs in om.CRAFTED_BED]
    set_regions(ctx, shuffled)
    add(ctx, {k: v[:1025] for k, v in cols.items()})
    assert got(ctx) == want[1025, "crafted"] + [0]


def model_records(recs):
    """the dict records of tests/cli_util.write_bam as the model's tuples (end_pos: pos and the M D N = X operations)"""
    out = []
    for r in recs:
        cigar = r.get("cigar", [(0, r.get("seq_len", 10))])
        end = r["pos"] + sum(ln for op, ln in cigar if op in (0, 2, 3, 7, 8))
        out.append((r["flag"], r["tid"], r["mtid"], r["pos"], r["mpos"], r["tlen"], end))
    return out


@pytest.mark.parametrize("maker", ["make_bam", "sorted_bam"])
def test_composition_with_the_file_columns(ctx, tmp_path, maker):
    from tests import test_cli_gpu as tcg
    bam = tmp_path / "c.bam"
    recs = model_records(getattr(tcg, maker)(str(bam), 30000, seed=23))
    regions = [[(1001, 200000), (500001, 600000), (150001, 150010)], [(1, 450000)], []]
    handled, cols, n, header, _ = ctx.bam_file_columns_dev(str(bam), 1 | 4 | 8 | 16 | 32 | 64 | 128)
    assert handled and n == len(recs)
    set_regions(ctx, regions)
    ctx.on_target_add_dev(*[cols[name] for name in DTYPES], n)
    res = got(ctx)
    want = om.sweep(recs, regions)
    assert res == want + [0] and 0 < want[4] < want[3]
    handled, counters, *_ = ctx.bam_file_reduce(str(bam))
    assert handled and [int(x) for x in counters] == res[:3]
