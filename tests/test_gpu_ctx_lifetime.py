"""GPU: what a ctx owns through its life.  Every setter called again on one ctx, with smaller and then larger tables; the host entry
points around a workspace that grows; contexts made, used in every domain and closed, three times over.  Each test makes its own
Context, because it closes it.  Results only: how much device memory is free is not this process's to assert on."""
import gzip

import numpy as np
import pytest

from seqkit_amd import Context, SeqkitHipError, synth
from tests import bam_on_target_model as om
from tests.test_gpu_on_target import DTYPES, columns
from tests.test_gpu_parity import count_inputs, grouped_regions

pytestmark = pytest.mark.gpu

N = 300                                    # not a multiple of 256: one full and one partial step of the lookup kernels


@pytest.fixture
def own(hip_lib):
    c = Context(0)
    yield c
    c.close()


def demux_case(S, L, seed):
    table = synth.make_sheet(S, L, seed=seed)
    bc, _ = synth.observe_barcodes(table, N, seed=seed + 1)
    return table, bc


def check_demux(c, oracle, table, bc):
    c.set_barcodes(table, 1)
    got = c.demux_assign(bc)
    *want, want_counts = oracle.demux_batch(table, bc, 1)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    assert np.array_equal(c.counts(), want_counts)         # this call's rows alone: the setter left fresh counters
    return [g.copy() for g in got]


def test_set_barcodes_shrinking_then_growing(own, oracle):
    small, large = demux_case(3, 8, seed=5), demux_case(40, 12, seed=7)
    for table, bc in (small, large, small):
        check_demux(own, oracle, table, bc)


COUNT_N_CHR = 3


def count_case(n_regions, seed):
    cols, rchr, rstart, rend = count_inputs(N, COUNT_N_CHR, n_regions, seed=seed, span=20_000)
    rchr[:] = np.arange(n_regions) % COUNT_N_CHR          # every region on a reference the records have,
    rstart[:] = np.arange(n_regions) * 3000               # and wide enough to overlap its neighbour on that reference
    rend[:] = rstart + 12_000
    return cols, rchr, rstart, rend


def check_count(c, oracle, n_regions, seed):
    cols, rchr, rstart, rend = count_case(n_regions, seed)
    want, code, _ = oracle.count_batch(**cols, n_chr=COUNT_N_CHR, rchr=rchr, rstart=rstart, rend=rend)
    assert code == 0 and want.min() > 0
    chr_off, gs, ge, gi = grouped_regions(rchr, rstart, rend, COUNT_N_CHR)
    c.count_set_regions(chr_off, gs, ge, gi, n_regions=n_regions)
    c.count_add(**dict(cols, end_pos=None))
    got = c.count_get()
    assert len(got) == n_regions and np.array_equal(got, want)
    return got


def test_count_set_regions_twice(own, oracle):
    check_count(own, oracle, 2, seed=21)
    check_count(own, oracle, 5, seed=22)


BED_2 = [[], [(1001, 2000)], [(501, 600)], [], []]
BED_5 = [[], [(1001, 2000)], [(501, 600), (501, 900)], [(101, 10000), (201, 210)], []]


def check_on_target(c, bed, recs):
    chr_off = np.cumsum([0] + [len(rs) for rs in bed]).astype(np.int32)
    flat = [r for rs in bed for r in rs]
    c.on_target_set_regions(chr_off, np.array([s for s, _ in flat], dtype=np.int64), np.array([e for _, e in flat], dtype=np.int64))
    cols = columns(recs)
    c.on_target_add(*[cols[name] for name in DTYPES])
    got = [int(x) for x in c.on_target_get()]
    want = om.sweep(recs, bed)
    assert got == want + [0] and want[4] > 0
    return got


def test_on_target_set_regions_twice(own):
    recs = om.drawn_records(N, seed=13)
    two = check_on_target(own, BED_2, recs)
    five = check_on_target(own, BED_5, recs)
    assert five[4] > two[4]                                # the larger table was the one in use


def check_gc(c, oracle, n_bytes, seed):
    rng = np.random.default_rng(seed)
    genome = np.ascontiguousarray(rng.choice(np.frombuffer(b"ACGTNacgt", dtype=np.uint8), size=n_bytes))
    c.gc_set_genome(genome)
    starts = np.array([0, n_bytes // 3, n_bytes - 17], dtype=np.int64)
    lens = np.array([n_bytes, n_bytes // 2, 17], dtype=np.int64)
    gc, total = c.gc_count(starts, lens)
    raw = genome.tobytes()
    got = [(int(g), int(t)) for g, t in zip(gc, total)]
    assert got == [oracle.gc_count(raw[s:s + n]) for s, n in zip(starts, lens)]
    return got


def test_gc_set_genome_twice(own, oracle):
    check_gc(own, oracle, 100, seed=1)
    check_gc(own, oracle, 5000, seed=2)


def test_host_entry_points_around_a_growing_workspace(own, oracle, monkeypatch):
    """64 rows, 5 000 rows, 64 rows in chunks of 256 bytes: both lanes and both halves of a workspace that is made, grows, and stays"""
    monkeypatch.setenv("SK_HOST_CHUNK_LOG2", "8")
    L = 37
    for n, seed in ((64, 3), (5000, 4), (64, 3)):
        _, qual = synth.make_reads(n, L, seed=seed)
        qual = synth.add_forced_classes(qual, seed=seed + 10)
        ln = synth.ragged_lengths(n, L, seed=seed)
        assert np.array_equal(own.trim_by_quality(qual, ln, 20), oracle.trim_batch(qual, ln, 20))


def use_every_domain(c, oracle):
    """every domain of a ctx once; what each gave (checked against its model here), for the rounds to compare"""
    out = []
    table, bc = demux_case(3, 8, seed=5)
    out.append(check_demux(c, oracle, table, bc))
    c.census_reset()
    c.census_add(bc)
    entries, total = c.census_entries()
    assert entries == oracle.census(bc) and total == len(entries)
    out.append(entries)
    out.append(check_count(c, oracle, 2, seed=21).tolist())
    out.append(check_on_target(c, BED_2, om.drawn_records(N, seed=13)))
    out.append(check_gc(c, oracle, 100, seed=1))
    data = bytes(np.random.default_rng(8).integers(65, 70, size=1000, dtype=np.uint8))
    members = c.bgzf_deflate(data)                         # (its compressed slots land in a page-locked buffer the ctx keeps)
    assert gzip.decompress(members) == data
    out.append(members)
    return out


def test_create_use_every_domain_close_three_rounds(hip_lib, oracle):
    rounds = []
    for _ in range(3):
        c = Context(0)
        try:
            rounds.append(use_every_domain(c, oracle))
        finally:
            c.close()
    assert repr(rounds[1]) == repr(rounds[0]) and repr(rounds[2]) == repr(rounds[0])
    Context(0).close()                                     # a ctx on which nothing was set


def test_reading_before_the_setter_keeps_its_message(own):
    """the hand-written messages and codes of the four readers on a ctx whose setter has not run"""
    with pytest.raises(SeqkitHipError) as e:
        own.counts()
    assert str(e.value) == "sk_counts_get failed (-4): sk_set_barcodes has not been called"
    # (Context.count_get sizes its result from what count_set_regions was given: the library itself here)
    out = np.zeros(1, dtype=np.uint32)
    assert own._lib.sk_count_get(own._h, out.ctypes.data) == -1
    assert own._lib.sk_last_error(own._h).decode() == "sk_count_set_regions has not been called"
    with pytest.raises(SeqkitHipError) as e:
        own.on_target_get()
    assert str(e.value) == "sk_on_target_get failed (-1): sk_on_target_set_regions has not been called"
    with pytest.raises(SeqkitHipError) as e:
        own.gc_count(np.array([0]), np.array([0]))
    assert str(e.value) == "sk_gc_count failed (-1): sk_gc_set_genome has not been called"
