"""GPU: every kernel whose grid is capped by the CU count, taken past the first trip of its stride loop.

A context created with SK_PLAN_CUS=1 (or 3) plans its launches for that many CUs, so the capped grids loop at test sizes as they do at
production sizes on the whole chip: the stride arithmetic, what a workgroup carries from one trip to the next and the prefetch of the
next tile all run.  Every case holds three properties:
  1. the small-grid result equals the model the kernel's own test file uses (imported from there, not copied);
  2. it equals, byte for byte, what the session's default-grid context returns for the same input;
  3. the input is at least 3 x CAPACITY[kernel] x the planned CU count (trips()): three or more trips, asserted in the case.
The last two tests are the two one-workgroup scans, whose loops do not depend on the CU count; they run on the default context."""
import bisect
import os
import struct
import time
import zlib

import numpy as np
import pytest

from seqkit_amd import synth
from tests import bam_coverage_model as cov_m
from tests import bam_markdup_model as md_m
from tests import bam_merge_model as merge_m
from tests import bam_minimize_model as min_m
from tests import bam_on_target_model as om
from tests import bam_out_util as bu
from tests import bam_rewrite_model as rw_m
from tests import bam_subsample_model as sub_m
from tests import test_gpu_bam_coverage as tg_cov
from tests import test_gpu_bam_markdup as tg_md
from tests import test_gpu_bam_merge as tg_merge
from tests import test_gpu_bam_minimize as tg_min
from tests import test_gpu_bam_pairs as tg_pairs
from tests import test_gpu_bam_reads as tg_reads
from tests import test_gpu_bam_rewrite as tg_rw
from tests import test_gpu_bam_subsample as tg_sub
from tests import test_gpu_deflate_crafted as tg_def
from tests import test_gpu_inflate as tg_inf
from tests import test_gpu_on_target as tg_ot
from tests import test_gpu_parity as tg_par
from tests.bam_out_util import sam  # noqa: F401  (the fixture)
from tests.test_cli_gpu import reads_bam

pytestmark = pytest.mark.gpu

# kernel -> units of work ONE launch covers per planned CU in a single trip of its stride loop (read from the named launcher).  Where a
# launcher asks the occupancy API, the entry is the most it can come to.
CAPACITY = {
    "bam_reads_text_kernel": 256,          # launch_bam_reads_text on group_grid: n_cu * 16 workgroups x 16 groups of 16 lanes, a record a group
    "bam_pair_text_kernel": 256,           # launch_bam_pair_text on group_grid
    "bam_rw_write_kernel": 256,            # launch_bam_rw_write: its own kernel, on group_grid
    "bam_write_kernel<MinRecord>": 256,    # launch_bam_min_write: launch_bam_write, the shared window writer, on group_grid
    "bam_write_kernel<MdRecord>": 256,     # launch_bam_md_write: launch_bam_write
    "bam_copy_write_kernel": 256,          # launch_bam_copy_write: its own kernel, on group_grid
    "bam_write_kernel<MergeRecord>": 256,  # launch_bam_merge_write: launch_bam_write
    "bam_md_cluster_kernel": 2048,         # launch_bam_md_cluster (and bam_md_count_kernel): n_cu * 8 workgroups x 256 sorted positions
    "bam_sub_keep_kernel": 2048,           # launch_bam_sub_keep: n_cu * 8 workgroups x 256 records
    "bam_cov_hist_kernel": 1024,           # launch_bam_cov_hist: n_cu * 4 workgroups x 256 events
    "bam_target_kernel": 1024,             # launch_bam_target: n_cu workgroups x 256 lanes x 4 records
    "bam_count_kernel": 8192,              # launch_bam_count: n_cu * 8 workgroups x 256 lanes x 4 records, aligned columns or not
    "bam_fragments_kernel": 4096,          # launch_bam_fragments: n_cu * 2 workgroups x 2 048 records
    "bam_flag_tlen_kernel": 4096,          # launch_bam_flag_tlen, aligned columns: n_cu * 2 workgroups x 2 048 records
    "bam_flag_tlen_scalar_kernel": 1024,   # launch_bam_flag_tlen, any alignment: n_cu * 4 workgroups x 256 records
    "gc_count_kernel": 32,                 # launch_gc_count: n_cu * 8 workgroups x 4 waves, a segment a wave
    "bam_sequence_tile_kernel": 512,       # launch_bam_sequence: n_cu * 2 workgroups x 4 waves x 64 rows
    "bam_sequence8_kernel": 512,           # launch_bam_sequence: n_cu * 8 (SK_SEQ_WGS) workgroups x 64 rows
    "mask_flat_kernel": 49152,             # launch_mask_flat: n_cu * 3 (SK_MASK_WGS) workgroups x 256 lanes x 4 chunks of 16 BYTES
    "trim_rows_global_kernel": 2048,       # launch_tile_pass, rows longer than an LDS tile: n_cu * 8 workgroups x 256 rows
    "tile_pass_kernel": 1024,              # plan_shape: n_cu * wg workgroups (wg <= 4 by launch_tile_pass) x at most 4 waves x 64 rows
    "tile_blocked_kernel": 1024,           # plan_shape through launch_tile_blocked: wg <= 3, at most 4 waves x 64 rows
    "demux_lut_kernel (table in LDS)": 4096,   # launch_tile_pass, by_table && ldstab: n_cu * 1 workgroup x 16 waves x 256 rows
    "demux_lut8x2_kernel": 4096,           # launch_tile_pass, by_table && rows2 && ldstab: the same shape
    "demux_lut_kernel (table in the vector cache)": 8192,   # launch_tile_pass, by_table && !ldstab: n_cu * wg workgroups (wg <= 8: 32 waves a CU) x 4 waves x 256 rows
    "demux_tile_kernel": 2048,             # plan_shape through launch_tile_pass, the matchers: n_cu * wg workgroups (wg <= 8) x at most 4 waves x 64 rows
    "census front kernel": 2048,           # census_add: n_cu * 1 (SK_CENSUS_WGS) workgroups x 16 waves x at most 2 tiles of 64 rows
    "census_combine_kernel": 2 * 16384,    # census_add: 2 * n_cu workgroups claim items of at most 16 384 RECORDS from a counter
    "census_direct_kernel": 4096,          # census_add: 8 (SK_CENSUS_DIRECT_SPLIT) workgroups x 512 RECORDS for each of the front kernel's n_cu workgroups
    "census table kernels": 2048,          # census_reserve / census_count_hist / census_entries: n_cu * 8 workgroups x 256 SLOTS
    "bgzf_inflate_kernel": 64,             # launch_bgzf_inflate: n_cu * 4 (160 KiB / LDS of a workgroup) * 4 workgroups x 4 waves, a block a wave
    "bgzf_crc_kernel": 64,                 # launch_bgzf_inflate: n_cu * 16 workgroups x 4 waves, a block a wave
    "bgzf_deflate_kernel": 32,             # launch_bgzf_deflate: n_cu * 2 (160 KiB / LDS of a workgroup) * 4 workgroups x 4 waves, a block a wave
    "bgzf_crc_out_kernel": 64,             # launch_bgzf_deflate / launch_bgzf_crc: n_cu * 16 workgroups x 4 waves, a block a wave
    "bam_file_front batches": 32,          # bam_file_front: a batch is at least 2 * 16 * n_cu BLOCKS; six batches are three on either stream
}
# launches that take n_cu and need no case here, or are not capped by it at all
NOT_CAPPED = {
    "bgzf_pack_kernel": "launch_bgzf_pack ignores its n_cu: a workgroup per member",
    "count_order_tile_kernel": "sk_count_order_check_dev launches a workgroup per tile of records; its join is one workgroup",
    "sk_bam_fragments_bed_dev": "its kernels launch a thread per record, uncapped",
    "census_clear_kernel": "census_reset launches a fixed grid that loops over the table's log at any CU count "
                           "(both of its branches, the log's and the whole table's, run in tests/test_gpu_census_log.py)",
}


def trips(kernel, units, cus):
    """property 3: `units` of work in one launch are three trips or more of `kernel`'s loop on a grid planned for `cus` CUs"""
    assert units >= 3 * CAPACITY[kernel] * cus, (kernel, units, cus)


# ---- contexts ------------------------------------------------------------------------------------------------------------
def planned(value, **more):
    """a context created with SK_PLAN_CUS=value (None: unset) in the environment, which is restored before this returns"""
    import seqkit_amd
    env = dict(more)
    env["SK_PLAN_CUS"] = value
    saved = {k: os.environ.get(k) for k in env}
    try:
        for k, v in env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        c = seqkit_amd.Context(0)
        if "SK_CENSUS_SLOTS_LOG2" in more:
            c.census_reset()                                                       # (the census is made on its first call)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return c


@pytest.fixture(scope="module")
def small(hip_lib):
    """{1: a context that plans for one CU, 3: for three (an odd count divides nothing evenly)}"""
    cs = {k: planned(str(k)) for k in (1, 3)}
    for k, c in cs.items():
        assert c.planned_cus() == k
    assert "SK_PLAN_CUS" not in os.environ
    yield cs
    for c in cs.values():
        c.close()


def test_planned_cus_override_and_what_it_ignores(ctx, small):
    real = ctx.planned_cus()
    assert real >= 4 and (small[1].planned_cus(), small[3].planned_cus()) == (1, 3)
    for value in (None, "", "0", "-1", "-3", str(real + 1), "99999999999999999999", "abc", "3x", "1.5", " "):
        c = planned(value)
        try:
            assert c.planned_cus() == real, value
        finally:
            c.close()
    c = planned(str(real))
    try:
        assert c.planned_cus() == real
    finally:
        c.close()


def test_every_capacity_names_its_launcher():
    src = open(__file__, encoding="utf-8").read().split("CAPACITY = {", 1)[1].split("\n}\n", 1)[0]
    rows = [ln for ln in src.split("\n") if ln.strip().startswith('"')]
    assert len(rows) == len(CAPACITY) and all("#" in ln and ("launch_" in ln or "plan_shape" in ln or "census_" in ln or "bam_file_front" in ln) for ln in rows)


class Recording:
    """a context that remembers what a file call's windows held: the helpers of the other test files take it for a context"""

    def __init__(self, c):
        self._c, self.launches, self.bytes, self.info = c, [], [], None

    def __getattr__(self, name):
        f = getattr(self._c, name)
        if name.endswith("_windows"):
            def windows(*a, **kw):
                for w in f(*a, **kw):
                    self.launches.append(int(w["n"]))
                    self.bytes.append(bytes(w["bgzf"]) if "bgzf" in w else bytes(w["text"]))
                    yield w
            return windows
        if name.startswith("bam_file_"):
            def call(*a, **kw):
                self.launches, self.bytes = [], []
                r = f(*a, **kw)
                self.info = r[-1]
                return r
            return call
        return f


CHUNK_LOG2 = 12


@pytest.fixture
def small_chunks(monkeypatch):
    """the front half reads the file in chunks of 4 KiB: a batch of blocks goes to the inflater as soon as 2 * 16 * n_cu are complete"""
    monkeypatch.setenv("SK_BAMFILE_CHUNK_LOG2", str(CHUNK_LOG2))


def front_batches(path, cus):
    """the batches bam_file_front cuts `path` into on a context planned for `cus` CUs, by its rule: after every chunk, the complete blocks not
    yet launched go when they are 2 * 16 * cus or the chunk is the last, rounded down to whole rounds of 16 * cus unless it is"""
    data = open(path, "rb").read()
    ends, at = [], 0
    while at < len(data):
        at += struct.unpack_from("<H", data, at + 16)[0] + 1
        ends.append(at)
    slots, chunk, launched, out = 16 * cus, 1 << CHUNK_LOG2, 0, []
    n_chunks = -(-len(data) // chunk)
    for k in range(n_chunks):
        n_new = bisect.bisect_right(ends, min(len(data), (k + 1) * chunk)) - launched
        last = k + 1 == n_chunks
        if n_new and (n_new >= 2 * slots or last):
            if not last and n_new >= slots:
                n_new -= n_new % slots
            out.append(n_new)
            launched += n_new
    assert launched == len(ends)
    return out


def many_batches(rec, path, cus):
    """the file call `rec` just made read a file of 200 blocks or more; planned for one CU that is six batches or more"""
    assert rec.info[2] >= 200, rec.info
    if cus == 1:
        trips("bam_file_front batches", int(rec.info[2]), 1)
        assert len(front_batches(path, 1)) >= 6
    trips("bgzf_inflate_kernel", int(rec.info[2]), 1)                                # (the default grid takes them in one batch: it loops at one CU's worth)


def window_launches(rec, kernel, cus, windowed):
    """the windows of rec's last call: every one is a launch of `kernel`; the largest loops three times, and of several the second largest too"""
    ns = sorted(rec.launches if rec.launches and rec.launches[0] else rec.launches[1:])      # (a rewrite's first window is the header's)
    trips(kernel, ns[-1], cus)
    if windowed:
        assert len(ns) >= 3 and ns[-2] >= 1000
        trips(kernel, ns[-2], cus)


def windows_of(cus, total_bytes):
    """(window_bytes, several windows?) a case runs with: the default window, and at one CU a third of the output (windows of 1 000 records and
    more; planned for three CUs such a window is no three trips)"""
    return [(0, False)] + ([(total_bytes // 3 + 1, True)] if cus == 1 else [])


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("small_grid")


# ---- the seven 16-lane writers ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def reads_file(tmp):
    path = tmp / "reads.bam"
    return path, reads_bam(str(path), 3500, seed=7, sort="shuffled", piece=2000)


@pytest.mark.parametrize("cus", [1, 3])
@pytest.mark.parametrize("fmt", ["raw", "fasta", "fastq"])
def test_reads_text(ctx, small, small_chunks, reads_file, fmt, cus):
    path, recs = reads_file
    total = sum(len(t) for _, _, t in tg_reads.model(recs, fmt, True))
    for window, several in windows_of(cus, total):
        rec = Recording(small[cus])
        rows, _ = tg_reads.check_against_model(rec, path, recs, fmt, True, window)
        assert rows == tg_reads.check_against_model(ctx, path, recs, fmt, True, window)[0]
        window_launches(rec, "bam_reads_text_kernel", cus, several)
        many_batches(rec, path, cus)


@pytest.mark.parametrize("cus", [1, 3])
@pytest.mark.parametrize("fmt", ["raw", "fasta", "fastq"])
def test_pairs_text(ctx, small, small_chunks, reads_file, fmt, cus):
    path, recs = reads_file
    total = len(tg_pairs.expected(recs, fmt, True)[0])
    for window, several in windows_of(cus, total):
        for interleaved in (False, True):
            rec = Recording(small[cus])
            tg_pairs.check(rec, path, recs, window, formats=(fmt,), modes=(interleaved,))
            ref = Recording(ctx)
            tg_pairs.check(ref, path, recs, window, formats=(fmt,), modes=(interleaved,))
            assert (rec.launches, rec.bytes) == (ref.launches, ref.bytes)
            if interleaved:                                                           # (one stream of both mates: the largest launches)
                window_launches(rec, "bam_pair_text_kernel", cus, several)
            else:
                trips("bam_pair_text_kernel", max(rec.launches), cus)
            many_batches(rec, path, cus)


def out_case(ctx, small, cus, path, kernel, raw_bytes, run, level=1):
    """run(context, level, window_bytes) asserts the model and returns what it likes; the windows' members are compared with the default grid's"""
    for window, several in windows_of(cus, raw_bytes):
        rec, ref = Recording(small[cus]), Recording(ctx)
        assert run(rec, level, window) == run(ref, level, window)
        assert (rec.launches, rec.bytes) == (ref.launches, ref.bytes)
        window_launches(rec, kernel, cus, several)
        many_batches(rec, path, cus)


@pytest.mark.parametrize("cus", [1, 3])
@pytest.mark.parametrize("op", list(rw_m.OPS))
def test_rewrite(ctx, small, small_chunks, tmp, op, cus):
    path = tmp / ("rewrite%d.bam" % rw_m.OPS[op])
    # (blocks of 4 000 bytes; 5 000 for the op whose file the record walk would otherwise need one round a block for, and decline)
    raw = rw_m.write(path, rw_m.served_records(op, 5000, seed=3), piece=5000 if op == "qname from tags" else 4000)
    exp, code = rw_m.model(raw, op)
    assert code is None

    def run(c, level, window):
        handled, out, mem = tg_rw.collect(c, path, op, level, window)
        assert handled and out == exp
        return mem
    out_case(ctx, small, cus, path, "bam_rw_write_kernel", len(exp), run)


@pytest.mark.parametrize("cus", [1, 3])
def test_minimize(ctx, small, small_chunks, tmp, cus):
    path = tmp / "minimize.bam"
    raw = min_m.write(path, min_m.served_records(5000, seed=3), piece=4000)
    exp, code = min_m.model(raw, "all", 30)
    assert code is None

    def run(c, level, window):
        handled, out, mem, _ = tg_min.collect(c, path, "all", 30, level, window)
        assert handled, out
        assert out == exp
        return mem
    out_case(ctx, small, cus, path, "bam_write_kernel<MinRecord>", len(exp), run)


@pytest.mark.parametrize("cus", [1, 3])
def test_markdup(ctx, small, small_chunks, tmp, cus):
    path = tmp / "markdup.bam"
    recs = md_m.sorted_records(11, 7000, big=1100)
    raw = md_m.write(path, recs, piece=2000)
    if cus == 1:
        trips("bam_md_cluster_kernel", len(recs), 1)
    out_case(ctx, small, cus, path, "bam_write_kernel<MdRecord>", len(raw), lambda c, level, window: tg_md.check(c, path, raw, False, level, window))


@pytest.mark.parametrize("cus", [1, 3])
def test_subsample(ctx, small, small_chunks, tmp, cus):
    path = tmp / "subsample.bam"
    recs = sub_m.served_records(9000, seed=3)
    raw = sub_m.write(path, recs, piece=4000)
    exp, _, _, kept, total = sub_m.model(raw, 5, sub_m.parse_fraction("0.5"))
    if cus == 1:
        trips("bam_sub_keep_kernel", len(recs), 1)
    out_case(ctx, small, cus, path, "bam_copy_write_kernel", len(exp), lambda c, level, window: tg_sub.check(c, path, raw, "0.5", 5, level, window))


@pytest.mark.parametrize("cus", [1, 3])
def test_merge(ctx, small, small_chunks, tmp, cus):
    files = merge_m.served_inputs(3, [2600, 1900, 1500], seed=5)
    paths, raws = tg_merge.write_all(tmp, files, piece=1000)
    exp, err, code = merge_m.model(raws, True)
    assert (err, code) == (b"", 0)
    out_case(ctx, small, cus, paths[0], "bam_write_kernel<MergeRecord>", len(exp), lambda c, level, window: tg_merge.check(c, paths, raws, True, level, window)[:2])


def test_rewrite_level_0_is_the_crc_alone(ctx, small, tmp):
    """launch_bgzf_crc without the deflater: one window of 200 stored members and more; then the same window deflated (32 waves take them)"""
    path = tmp / "stored.bam"
    raw = rw_m.write(path, rw_m.served_records("trim qnames", 5000, seed=3) * 13, level=1)
    exp, code = rw_m.model(raw, "trim qnames")
    assert code is None
    for level in (0, 1):
        rec, ref = Recording(small[1]), Recording(ctx)
        mems = []
        for c in (rec, ref):
            handled, out, mem = tg_rw.collect(c, path, "trim qnames", level, 0)
            assert handled and out == exp
            mems.append(mem)
        assert mems[0] == mems[1] and rec.bytes == ref.bytes
        assert len(rec.launches) == 2                                                 # the header's window and one of every record
        members = len(mems[0]) - 2                                                    # (without the header's and the EOF block)
        trips("bgzf_crc_out_kernel", members, 1)
        if level:
            trips("bgzf_deflate_kernel", members, 1)
        assert all(stored for _, stored in mems[0][:-1]) == (level == 0)
        window_launches(rec, "bam_rw_write_kernel", 1, False)


# ---- the two CLI cases -------------------------------------------------------------------------------------------------------
def test_cli_minimize_read_ids(sam, tmp):
    path = tmp / "cli_minimize.bam"
    recs = min_m.served_records(5000, seed=4)
    raw = min_m.write(path, recs)
    trips("bam_write_kernel<MinRecord>", len(recs), 1)
    code, out, err, _ = bu.three(sam, min_m, ["minimize"], path, ["--read-ids"], env={"SK_PLAN_CUS": "1"})
    assert code == 0 and err == b"" and out == min_m.model(raw, "read-ids")[0]
    assert bu.three(sam, min_m, ["minimize"], path, ["--read-ids"])[:3] == (code, out, err)


def test_cli_mark_duplicates(sam, tmp):
    path = tmp / "cli_markdup.bam"
    recs = md_m.sorted_records(13, 5000, big=1100)
    raw = md_m.write(path, recs)
    trips("bam_write_kernel<MdRecord>", len(recs), 1)
    code, out, err, _ = bu.three(sam, md_m, ["mark", "duplicates"], path, env={"SK_PLAN_CUS": "1"})
    exp, stop, msg = md_m.literal(raw)
    assert (code, out, err) == (stop, exp, msg) and stop == 0
    assert bu.three(sam, md_m, ["mark", "duplicates"], path)[:3] == (code, out, err)


# ---- coverage, on-target, the column kernels -----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [tg_cov.MODES[0], tg_cov.MODES[2], tg_cov.MODES[4]], ids=["everywhere", "region", "bed"])
def test_coverage_histogram(ctx, small, small_chunks, tmp, mode):
    refs = cov_m.refs_for()
    path = tmp / "coverage.bam"
    recs = cov_m.sorted_records(8000, refs, seed=3, skip_refs=(4,))
    raw = cov_m.write(path, recs, text=tg_cov.TEXT, refs=refs, piece=1500)
    counted = [r for r in recs if cov_m.counted(r, len(refs))]
    events = 2 * sum(len(cov_m.runs(r, refs[cov_m.core(r)[0]][1])[0]) for r in counted)      # (and two a target interval)
    assert len(counted) >= 4500
    trips("bam_cov_hist_kernel", events, 1)
    rec = Recording(small[1])
    got = tg_cov.check(rec, path, raw, mode)
    ref = tg_cov.check(ctx, path, raw, mode)
    assert np.array_equal(got[0], ref[0]) and got[1:] == ref[1:] and int(got[0][1:].sum()) > 0
    many_batches(rec, path, 1)


@pytest.fixture(scope="module")
def target_records():
    recs = om.crafted_records()
    recs += om.drawn_records(5003 - len(recs), seed=9)
    return recs, tg_ot.columns(recs), om.sweep(recs, om.CRAFTED_BED)


def test_on_target_host_entry(ctx, small, target_records):
    recs, cols, want = target_records
    trips("bam_target_kernel", len(recs), 1)
    got = []
    for c in (small[1], ctx):
        tg_ot.set_regions(c, om.CRAFTED_BED)
        tg_ot.add(c, cols)
        got.append(tg_ot.got(c))
    assert got[0] == want + [0] and got[1] == got[0] and 0 < want[4] < want[3]


@pytest.mark.parametrize("skip", [0, 1], ids=["vector loads", "unaligned columns"])
def test_on_target_device_entry(ctx, small, target_records, skip):
    recs, cols, want = target_records
    trips("bam_target_kernel", len(recs), 1)
    got = []
    for c in (small[1], ctx):
        dev = tg_ot.Dev(c)
        try:
            tg_ot.set_regions(c, om.CRAFTED_BED)
            ptrs = [dev.put(cols[name], skip) for name in tg_ot.DTYPES]
            assert all((p % 16 == 0) == (skip == 0) for p in ptrs)
            c.on_target_add_dev(*ptrs, len(recs))
            got.append(tg_ot.got(c))
        finally:
            dev.close()
    assert got[0] == want + [0] and got[1] == got[0]


N_ROWS = 3 * 8192 + 1237                    # three trips of the widest of the column kernels and a ragged fourth


def test_flag_tlen_and_fragments(ctx, small, oracle):
    n = N_ROWS
    assert n % 4096 and n % 2048 and n % 1024
    trips("bam_flag_tlen_kernel", n, 1)
    trips("bam_fragments_kernel", n, 1)
    flag, tid, mtid, tlen = synth.make_bam_cores(n, seed=15)
    flag ^= (np.random.default_rng(n).random(n) < 0.05).astype(np.uint16) * 0x200
    tlen[3], tlen[4], tlen[n - 1] = -2147483648, 2147483647, 77
    flag[3] = flag[4] = flag[n - 1] = 0x1 | 0x40
    mtid[3], mtid[4], mtid[n - 1] = tid[3], tid[4], tid[n - 1]
    ec, eh, et = oracle.bam_flag_tlen(flag, tid, mtid, tlen, 5000)
    exp = oracle.fragments_keep(flag, tid, mtid, tlen, 0, 5000)
    got = []
    for c in (small[1], ctx):
        cc, h, t = c.bam_flag_tlen(flag, tid, mtid, tlen, 5000)
        keep, kept = c.bam_fragments(flag, tid, mtid, tlen, 0, 5000)
        assert np.array_equal(cc, ec) and np.array_equal(h, eh) and t == et and int(h.sum()) == t
        assert np.array_equal(keep, exp) and kept == int(exp.sum()) > 1000
        got.append((cc.tobytes(), h.tobytes(), t, keep.tobytes(), kept))
    assert got[0] == got[1]


def test_flag_tlen_scalar_form(ctx, small, oracle):
    """columns at an odd element offset: bam_flag_tlen_scalar_kernel (tests/test_gpu_parity.py's test of the _dev entry point, past the first trip)"""
    n, off = 3 * 1024 + 77, 3
    trips("bam_flag_tlen_scalar_kernel", n, 1)
    cols = synth.make_bam_cores(n + 8, seed=16)
    flag, tid, mtid, tlen = [a[off:off + n] for a in cols]
    ec, eh, et = oracle.bam_flag_tlen(flag, tid, mtid, tlen, 5000)
    got = []
    for c in (small[1], ctx):
        dptr = [c.malloc_device(a.nbytes) for a in cols]
        dout = c.malloc_device((4 + 5001) * 8)
        try:
            for a, d in zip(cols, dptr):
                c.copy_h2d(d, a)
            c.copy_h2d(dout, np.zeros(4 + 5001, dtype=np.uint64))
            c.bam_flag_tlen_dev(dptr[0] + 2 * off, dptr[1] + 4 * off, dptr[2] + 4 * off, dptr[3] + 4 * off, n, 5000, dout)
            out = np.empty(4 + 5001, dtype=np.uint64)
            c.copy_d2h(out, dout)
            c.sync()
        finally:
            for d in dptr + [dout]:
                c.free_device(d)
        assert np.array_equal(out[:3], ec) and int(out[3]) == et and np.array_equal(out[4:], eh)
        got.append(out.tobytes())
    assert got[0] == got[1]


@pytest.mark.parametrize("kw", [dict(), dict(single_end=True, center=True, min_mapq=10, max_frag_len=100)], ids=["paired", "single end"])
@pytest.mark.parametrize("form", ["vector loads", "unaligned columns"])
def test_sam_count(ctx, small, oracle, kw, form):
    n, n_chr = N_ROWS, 5
    trips("bam_count_kernel", n, 1)
    cols, rchr, rstart, rend = tg_par.count_inputs(n + 1, n_chr, 3000, seed=19)
    want, code, _ = oracle.count_batch(**{k: v[1:] for k, v in cols.items()}, n_chr=n_chr, rchr=rchr, rstart=rstart, rend=rend, **kw)
    assert code == 0 and want.sum() > 100
    chr_off, gs, ge, gi = tg_par.grouped_regions(rchr, rstart, rend, n_chr)
    names = ("flag", "mapq", "tid", "mtid", "pos", "mpos", "tlen", "end_pos")
    got = []
    for c in (small[1], ctx):
        c.count_set_regions(chr_off, gs, ge, gi, n_regions=3000)
        if form == "vector loads":                                                    # the host entry stages its columns on 16-byte boundaries
            c.count_add(**{k: (None if k == "end_pos" and not kw.get("single_end") else v[1:]) for k, v in cols.items()}, **kw)
        else:                                                                         # every column one element behind such a boundary
            dev = tg_ot.Dev(c)
            try:
                ptrs = [dev.put(cols[k]) + cols[k].itemsize for k in names]
                assert all(p % 16 for p in ptrs)
                c.count_add_dev(*ptrs, n, **kw)
                c.sync()
            finally:
                dev.close()
        res = c.count_get()
        assert len(res) == 3000 and np.array_equal(res[gi], want[gi]) and res[rchr < 0].sum() == 0
        got.append(res.tobytes())
    assert got[0] == got[1]


def test_gc_count(ctx, small, oracle):
    rng = np.random.default_rng(23)
    genome = np.ascontiguousarray(rng.choice(np.frombuffer(b"ACGTNacgtnRYKM-*", dtype=np.uint8), size=2_500_000,
                                             p=[.2, .2, .2, .2, .04, .03, .03, .03, .03, .01] + [.005] * 6))
    starts = [1000 + 65536 * k + k for k in range(16)]                                # every alignment mod 16, longer than a segment
    lens = [65536 * 5 + 17 * k + 1 for k in range(16)]
    starts += [int(s) for s in rng.integers(0, len(genome) - 300_000, size=44)]
    lens += [int(v) for v in rng.choice([0, 1, 15, 16, 17, 100, 1000, 65535, 65536, 65537, 200_000, 200_000, 262_144], size=44)]
    starts, lens = np.array(starts, dtype=np.int64), np.array(lens, dtype=np.int64)
    assert {int(s) % 16 for s in starts[:16]} == set(range(16)) and int((lens > 65536).sum()) >= 16
    segments = int(sum(-(-int(v) // 65536) for v in lens))                            # sk_gc_count cuts a region every 64 KiB
    assert len(starts) == 60 and segments >= 150
    trips("gc_count_kernel", segments, 1)
    raw = genome.tobytes()
    got = []
    for c in (small[1], ctx):
        c.gc_set_genome(genome)
        gc, total = c.gc_count(starts, lens)
        for i in range(len(starts)):
            assert (int(gc[i]), int(total[i])) == oracle.gc_count(raw[starts[i]:starts[i] + lens[i]]), (i, starts[i], lens[i])
        got.append((gc.tobytes(), total.tobytes()))
        c.gc_set_genome(b"")
    assert got[0] == got[1]


# ---- sequence(): the case that consumes a prefetched tile ----------------------------------------------------------------------
SEQ_ROWS = {1: (2111, 3000), 3: (4700,)}     # (planned for three CUs the tile kernel takes 1 536 rows a trip: 3 000 are no three trips)


@pytest.mark.parametrize("kernel,stride,seq4_stride", [("bam_sequence_tile_kernel", 152, 76), ("bam_sequence_tile_kernel", 148, 76),
                                                       ("bam_sequence8_kernel", 152, 76), ("bam_sequence8_kernel", 252, 128)])
@pytest.mark.parametrize("cus", [1, 3])
def test_bam_sequence(ctx, small, oracle, monkeypatch, cus, stride, seq4_stride, kernel):
    if kernel == "bam_sequence8_kernel":                                              # (252 / 128 is a pitch the tile kernel does not serve at all)
        monkeypatch.setenv("SK_SEQ_TILE", "0")
    else:
        assert 64 * stride <= 10 * 1024 and 64 * seq4_stride <= 5 * 1024 and stride % 4 == 0      # launch_bam_sequence: the tile kernel's pitches
    for n in SEQ_ROWS[cus]:
        assert n % 64
        trips(kernel, n, cus)
        seq4, qual, ln, flag = tg_par.bam_rows(n, stride, seed=n + stride, seq4_stride=seq4_stride)
        assert {0, int(stride)} <= set(ln.tolist()) and (flag & 16).any() and not (flag & 16).all()
        for m in (10, 200):                                                           # below and above 128: the kernels' two compares
            want = oracle.bam_sequence_batch(seq4, qual, ln, flag, m)
            got = small[cus].bam_sequence(seq4, qual, ln, flag, m)
            tg_par.assert_rows_equal(got, want, ln)
            tg_par.assert_rows_equal(got, ctx.bam_sequence(seq4, qual, ln, flag, m), ln)
        got = small[cus].bam_sequence(seq4, qual, None, flag, 10)                    # len NULL: every row is full
        assert np.array_equal(got, oracle.bam_sequence_batch(seq4, qual, None, flag, 10))
        assert np.array_equal(got, ctx.bam_sequence(seq4, qual, None, flag, 10))


# ---- mask, trim, demultiplex, the fused pass, the blocked pass -------------------------------------------------------------------
def valid(ln, n, stride):
    return np.arange(stride)[None, :] < ln[:, None].astype(np.int64)


def test_mask_flat(ctx, small, oracle):
    n, stride = 1003, 150
    assert (n * stride) % 16 and (n * stride) % (256 * 4 * 16)
    trips("mask_flat_kernel", n * stride, 1)
    seq, qual = synth.make_reads(n, stride, seed=31)
    ln = synth.ragged_lengths(n, stride, seed=31)
    ok = valid(ln, n, stride)
    want = oracle.mask_batch(seq, qual, ln, 20)
    got = small[1].mask_by_quality(seq, qual, ln, 20)
    assert np.array_equal(got[ok], want[ok]) and np.array_equal(got[ok], ctx.mask_by_quality(seq, qual, ln, 20)[ok])


@pytest.mark.parametrize("stride,kernel", [(150, "tile_pass_kernel"), (1000, "trim_rows_global_kernel")])
def test_trim_alone(ctx, small, oracle, stride, kernel):
    n = 3 * CAPACITY[kernel] + 77
    trips(kernel, n, 1)
    _, qual = synth.make_reads(n, stride, seed=32)
    qual = synth.add_forced_classes(qual, seed=32)
    ln = synth.ragged_lengths(n, stride, seed=32)
    for m in (20, 2):
        want = oracle.trim_batch(qual, ln, m)
        got = small[1].trim_by_quality(qual, ln, m)
        assert np.array_equal(got, want) and np.array_equal(got, ctx.trim_by_quality(qual, ln, m))


@pytest.mark.parametrize("kernel", ["demux_lut_kernel (table in LDS)", "demux_lut_kernel (table in the vector cache)", "demux_lut8x2_kernel", "demux_tile_kernel"])
def test_demux(ctx, small, oracle, monkeypatch, kernel):
    """the decision alone by the sheet's table: in LDS, through the vector cache, two 8-byte rows a lane; every column by the matchers"""
    n = 3 * 8192 + 333
    trips(kernel, n, 1)
    if "vector cache" in kernel:
        monkeypatch.setenv("SK_DEMUX_LDSTAB", "0")
    dual = kernel != "demux_lut8x2_kernel"
    if not dual:
        monkeypatch.setenv("SK_DEMUX_ROWS2", "1")
    table = synth.make_sheet(96 if dual else 16, 8, dual=dual, seed=4)
    bc, _ = synth.observe_barcodes(table, n, seed=33, halves=2 if dual else 1)
    assert dual or bc.shape[1] == 8
    got = []
    for c in (small[1], ctx):
        if kernel == "demux_tile_kernel":
            tg_par.check_demux(c, oracle, table, bc)
            got.append([a.tobytes() for a in c.demux_assign(bc)] + [c.counts().tobytes()])
        else:
            tg_par.check_demux_decision_only(c, oracle, table, bc)
            info = c.barcode_table_info()
            assert info["kind"] != 0 and 0 < info["bytes"] <= 128 << 10, info      # a table, small enough for LDS (launch_tile_pass: ldstab)
            got.append((c.demux_assign(bc, want_detail=False)[0].tobytes(), c.counts().tobytes()))
        c.counts_reset()
    assert got[0] == got[1]


def fused_inputs(n, L, paired, seed):
    table = synth.make_sheet(96, 8, dual=True, seed=4)
    bc, _ = synth.observe_barcodes(table, n, seed=seed, halves=2)
    ln = synth.ragged_lengths(n, L, seed=seed)
    mates = []
    for mi in range(2 if paired else 1):
        seq, qual = synth.make_reads(n, L, seed=seed + 1 + mi)
        mates.append((seq, synth.add_forced_classes(qual, seed=seed + 3 + mi), ln))
    return table, bc, ln, mates


@pytest.mark.parametrize("paired", [False, True], ids=["single", "paired"])
def test_fused_pass(ctx, small, oracle, paired):
    n, L = 3 * 1024 + 77, 101
    trips("tile_pass_kernel", n, 1)
    table, bc, ln, mates = fused_inputs(n, L, paired, seed=40)
    ok = valid(ln, n, L)
    e_assign, e_low, e_first, e_last, e_counts = oracle.demux_batch(table, bc, 1)
    res = []
    for c in (small[1], ctx):
        c.set_barcodes(table, 1)
        r = c.fused_pass(mates, 20, bc=bc, want_detail=True)
        assert np.array_equal(r["assign"], e_assign) and np.array_equal(r["lowest_diff"], e_low)
        assert np.array_equal(r["first_idx"], e_first) and np.array_equal(r["last_idx"], e_last)
        assert np.array_equal(c.counts(), e_counts)
        for mi, (seq, qual, _) in enumerate(mates):
            assert np.array_equal(r["lowest_k"][mi], oracle.trim_batch(qual, ln, 20))
            assert np.array_equal(r["out_seq"][mi][ok], oracle.mask_batch(seq, qual, ln, 20)[ok])
        r2 = c.fused_pass(mates, 2)                                                   # mask + trim without barcodes: the same kernels
        assert np.array_equal(r2["lowest_k"][-1], oracle.trim_batch(mates[-1][1], ln, 2))
        res.append([r["assign"].tobytes(), r["lowest_diff"].tobytes(), r["first_idx"].tobytes(), r["last_idx"].tobytes()]
                   + [r["lowest_k"][mi].tobytes() for mi in range(len(mates))] + [r["out_seq"][mi][ok].tobytes() for mi in range(len(mates))]
                   + [r2["lowest_k"][mi].tobytes() for mi in range(len(mates))] + [r2["out_seq"][mi][ok].tobytes() for mi in range(len(mates))])
    assert res[0] == res[1]


def test_blocked_pass(ctx, small, oracle):
    n, L = 3 * 1024 + 77, 101
    trips("tile_blocked_kernel", n, 1)
    table, bc, ln, mates = fused_inputs(n, L, True, seed=50)
    ok = valid(ln, n, L)
    res = []
    for c in (small[1], ctx):
        tg_par.check_blocked(c, oracle, mates, 20, table, bc)
        tg_par.check_blocked(c, oracle, mates, 30, do_mask=False)                    # trim alone, no barcodes
        r = c.fused_pass_blocked(mates, 20, bc=bc, want_detail=True)
        res.append([r["assign"].tobytes(), r["lowest_diff"].tobytes(), r["first_idx"].tobytes(), r["last_idx"].tobytes()]
                   + [r["lowest_k"][mi].tobytes() for mi in range(2)] + [r["out_seq"][mi][ok].tobytes() for mi in range(2)])
    assert res[0] == res[1]


# ---- census ----------------------------------------------------------------------------------------------------------------------
def census_hist(entries):
    """sk_census_count_hist of the oracle's entries: bin k counts the barcodes seen 2^k .. 2^(k+1) - 1 times"""
    h = np.zeros(64, dtype=np.uint64)
    for _, count, _ in entries:
        h[count.bit_length() - 1] += 1
    return h


def census_case(c, bc, L, want):
    c.census_reset()
    c.census_add(bc, L=L)
    got, total = c.census_entries()
    assert total == len(want) and got == want                                         # as test_census_matches_oracle compares them
    st = c.census_stats()
    assert (st["distinct"], st["counted"], st["rejected"]) == (len(want), len(bc), 0) and sum(k for _, k, _ in got) == len(bc)
    hist = c.census_count_hist()
    assert np.array_equal(hist, census_hist(want))
    few, n_few = c.census_entries(min_count=3)
    assert few == [e for e in want if e[1] >= 3] and n_few == len(few)
    return got, hist.tobytes(), few


@pytest.mark.parametrize("path", ["direct", "partition", "spilled_direct"])
@pytest.mark.parametrize("n,L,stride,n_hot,hot_frac", [(70000, 17, 24, 96, 0.9), (300000, 8, 8, 96, 0.5)])
def test_census(ctx, small, oracle, monkeypatch, path, n, L, stride, n_hot, hot_frac):
    """the shapes of test_census_matches_oracle whose rows meet the front table (hot barcodes), the partition path and its combine kernel"""
    monkeypatch.setenv("SK_CENSUS_SPILL", "0" if path == "direct" else "1")
    if path != "direct":
        monkeypatch.setenv("SK_CENSUS_SPILL_MAX_PCT", "100" if path == "partition" else "0")
    trips("census front kernel", n, 1)
    bc = tg_par.random_barcodes(n, L, stride, n_hot, hot_frac, seed=n + L, alphabet=b"ACGTNacgtn+")
    want = oracle.census(bc, L=L)
    if path != "direct" and n == 300000:                                              # every distinct key reaches the table as a record or more
        trips("census_combine_kernel" if path == "partition" else "census_direct_kernel", len(want), 1)
    got = census_case(small[1], bc, L, want)
    trips("census table kernels", small[1].census_stats()["slots"], 1)
    assert got == census_case(ctx, bc, L, want)


def test_census_grows_between_launches(ctx, oracle, monkeypatch):
    """all-distinct barcodes into a first table of 2^13 slots in launches of 2^14 rows, planned for one CU: the rehash kernel loops too"""
    monkeypatch.setenv("SK_CENSUS_CHUNK_LOG2", "14")
    monkeypatch.setenv("SK_CENSUS_MIN_CHUNK_LOG2", "12")
    n = 40000
    vals = np.random.default_rng(21).permutation(4 ** 10)[:n].astype(np.int64)
    digits = (vals[:, None] >> (2 * np.arange(10))) & 3
    bc = np.zeros((n, 12), dtype=np.uint8)
    bc[:, :10] = np.frombuffer(b"ACGT", dtype=np.uint8)[digits]
    want = oracle.census(bc, L=10)
    c = planned("1", SK_CENSUS_SLOTS_LOG2="13")
    try:
        assert c.planned_cus() == 1 and c.census_stats()["slots"] == 1 << 13
        trips("census table kernels", 1 << 13, 1)
        trips("census front kernel", 1 << 14, 1)
        got = census_case(c, bc, 10, want)
        st = c.census_stats()
        assert st["slots"] >= 2 * n and st["distinct"] == n
    finally:
        c.close()
    assert got == census_case(ctx, bc, 10, want)


# ---- the inflater and the deflater ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cus", [1, 3])
def test_inflate_many_blocks_in_one_call(ctx, small, cus):
    """tests/test_gpu_inflate.py's corpus repeated; among them blocks with a wrong CRC and payloads cut short, reported at their own index"""
    rng = np.random.default_rng(7)
    items = tg_inf.corpus(rng)
    once = [(tg_inf.deflate_raw(raw, **kw), raw) for _, raw, kw in items]
    reps = -(-max(300, 3 * CAPACITY["bgzf_inflate_kernel"] * cus) // len(once))
    payloads, raws, crcs, verdict = [], [], [], []
    for i in range(reps * len(once)):
        p, raw = once[(i + i // len(once)) % len(once)]                               # (each repetition deals the kinds to other waves)
        crc = zlib.crc32(raw) & 0xFFFFFFFF
        if i % 37 == 5:
            crc ^= 0x10
        if i % 41 == 7 and len(p) > 1:
            p = p[:len(p) // 2]
        try:
            dz = zlib.decompressobj(wbits=-15)
            out = dz.decompress(p) + dz.flush()
            ok = dz.eof and len(out) == len(raw) and (zlib.crc32(out) & 0xFFFFFFFF) == crc
        except zlib.error:
            ok = False
        payloads.append(p); raws.append(raw); crcs.append(crc); verdict.append(ok)
    n = len(payloads)
    trips("bgzf_inflate_kernel", n, cus)
    trips("bgzf_crc_kernel", n, cus)
    assert n >= 300 and 10 <= verdict.count(False) < n // 10
    gaps = [int(g) for g in rng.integers(0, 9, n)]
    status, outs = tg_inf.inflate_on_device(small[cus], payloads, raws, gaps, crcs=crcs)
    for i in range(n):
        assert (status[i] == 0) == verdict[i], (i, hex(int(status[i])))
        if verdict[i]:
            assert outs[i] == raws[i], i
    ref_status, ref_outs = tg_inf.inflate_on_device(ctx, payloads, raws, gaps, crcs=crcs)
    assert np.array_equal(status, ref_status)
    assert all(a == b for a, b, ok in zip(outs, ref_outs, verdict) if ok)


def mixed_blocks(n_blocks):
    """text, runs, and random bytes that do not compress, of every size up to a whole block"""
    rng = np.random.default_rng(29)
    words = [rng.integers(65, 91, int(rng.integers(2, 12)), dtype=np.uint8).tobytes() for _ in range(200)]
    out = []
    for i in range(n_blocks):
        n = int(rng.integers(1, tg_def.MAX_IN + 1)) if i % 25 else tg_def.MAX_IN
        if i % 3 == 0:
            out.append(b" ".join(words[int(j)] for j in rng.integers(0, 200, n // 5 + 1))[:n])
        elif i % 3 == 1:
            out.append(bytes(rng.integers(0, 6, n // 7 + 1, dtype=np.uint8).repeat(7))[:n])
        else:
            out.append(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
    return out


def test_deflate_many_blocks_in_one_call(ctx, small):
    datas = mixed_blocks(304)
    trips("bgzf_deflate_kernel", len(datas), 1)
    trips("bgzf_crc_out_kernel", len(datas), 1)
    assert len(datas) >= 300
    aligns = [i % 4 for i in range(len(datas))]
    payloads, ntok, crc = tg_def.deflate_on_device(small[1], datas, aligns)
    for i, (d, p) in enumerate(zip(datas, payloads)):
        assert zlib.decompress(p, wbits=-15) == d, i
        assert crc[i] == (zlib.crc32(d) & 0xFFFFFFFF), i
    assert (payloads, ntok, crc) == tg_def.deflate_on_device(ctx, datas, aligns)
    assert sum(1 for d, p in zip(datas, payloads) if len(p) >= len(d)) >= len(datas) // 3      # (the random third does not shrink)


def test_deflate_framed_entry_point(ctx, small):
    data = b"".join(mixed_blocks(48))
    block = 4097
    n = -(-len(data) // block)
    trips("bgzf_deflate_kernel", n, 1)
    trips("bgzf_crc_out_kernel", n, 1)
    assert n >= 300
    comp = small[1].bgzf_deflate(data, block=block)
    members = bu.zlib_members(comp)                                                   # every member through zlib: CRC-32 and ISIZE checked
    assert b"".join(members) == data and len(members) == n
    assert comp == ctx.bgzf_deflate(data, block=block)


# ---- the two one-workgroup scans (default context) --------------------------------------------------------------------------------
def dict_records(raw):
    """the records of raw BAM bytes as tests/cli_util.write_bam's dicts: what tests/test_gpu_bam_reads.py's model reads"""
    out = []
    for r in rw_m.records(raw):
        lo, nc, flag, l_seq = r[12], struct.unpack_from("<H", r, 16)[0], struct.unpack_from("<H", r, 18)[0], struct.unpack_from("<i", r, 20)[0]
        o = 36 + lo + 4 * nc
        packed = r[o:o + (l_seq + 1) // 2]
        codes = [(packed[k >> 1] >> (0 if k & 1 else 4)) & 15 for k in range(l_seq)]
        out.append(dict(flag=flag, name=r[36:36 + lo - 1], codes=codes, qual=list(r[o + (l_seq + 1) // 2:o + (l_seq + 1) // 2 + l_seq])))
    return out


def test_block_scan_sums_two_entries_a_thread(ctx, tmp):
    """bam_scan_u64_kernel, one workgroup of 1 024 threads, each summing ceil(blocks / 1 024) entries: a file of 1 025 .. 2 048 blocks"""
    path = tmp / "blocks.bam"
    raw = min_m.write(path, min_m.served_records(18000, seed=6), piece=3500, level=1)
    blocks = -(-len(raw) // 3500) + 1                                                 # (and the EOF block)
    assert 1024 < blocks <= 2048 and blocks <= path.stat().st_size // 8192 + 1024   # per == 2; within the front half's block table
    rec = Recording(ctx)
    handled, out, _, _ = tg_min.collect(rec, path, "read-ids")
    assert handled, out
    assert out == min_m.model(raw, "read-ids")[0] and rec.info[2] == blocks > 1024
    handled, out, _ = tg_rw.collect(rec, path, "trim qnames", 1, 0)
    assert handled and out == rw_m.model(raw, "trim qnames")[0] and rec.info[2] == blocks
    assert out != min_m.out_header(raw) + raw[rw_m.header_end(raw):]                 # (names were trimmed)
    rows, _ = tg_reads.check_against_model(rec, path, dict_records(raw), "fastq", True)
    assert rec.info[2] == blocks and len(rows) > 10000


def test_tile_scan_carries_past_1024_tiles(ctx, tmp):
    """min_tile_scan_kernel, tiles of 1 024 elements scanned 1 024 at a trip: 2^20 + 5 000 records, every name twice at a random distance,
    numbered by sk_bam_file_minimize --read-ids at level 0.  Measured on the build machine: 6.9 s of CPU time for the host's side (the
    records 1.3 s, the writer at level 1 1.0 s, the model 4.0 s, the output's members and records 0.5 s)."""
    n = (1 << 20) + 5000
    t0 = time.process_time()
    order = np.random.default_rng(5).permutation(np.repeat(np.arange(n // 2), 2))
    core = struct.pack("<iiBBHHHiiii", 0, 100, 0, 30, 4680, 0, 0x41, 0, 0, 150, 150)
    uniq = []
    for i in range(n // 2):
        nm = b"%x\0" % i
        body = core[:8] + bytes([len(nm)]) + core[9:] + nm
        uniq.append(struct.pack("<i", len(body)) + body)
    assert max(len(u) for u in uniq) <= 4 + 32 + 9
    path = tmp / "tiles.bam"
    raw = min_m.write(path, [uniq[i] for i in order], text=b"@HD\tVN:1.6\n", level=1)
    exp, code = min_m.model(raw, "read-ids")
    assert code is None
    handled, out, mem, n_win = tg_min.collect(ctx, path, "read-ids", 255, 0, 0)
    assert handled, out
    assert out == exp and all(stored for _, stored in mem[:-1])
    assert sum(1 for _ in rw_m.records(out)) == n > 1 << 20
    print("CPU time: %.1f s" % (time.process_time() - t0))
