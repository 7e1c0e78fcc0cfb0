"""CPU: the two statements of `sam mark duplicates` in tests/bam_markdup_model.py agree — literal(), the reference's deque loop, and
grouped(), the sort-and-greedy statement the device path rests on — and each gives the flags derived by hand for small cases."""
import struct

import pytest

from tests import bam_markdup_model as m
from tests.bam_markdup_model import M, S, D, aux_i, aux_z, aux_h, rec


def raw_of(recs):
    return m.rm.header(m.rm.TEXT, m.rm.REFS) + b"".join(recs)


def flags_of(out):
    return [m.core(r)[4] for r in m.records(out)]


def both(recs, ignore_umi=False):
    """the two statements' outputs, checked equal; every byte but flag bit 0x400 as in the input"""
    raw = raw_of(recs)
    assert m.served(raw)
    lit, grp = m.literal(raw, ignore_umi), m.grouped(raw, ignore_umi)
    assert lit == grp
    out = list(m.records(lit[0]))
    assert len(out) == len(recs)
    for a, b in zip(recs, out):
        assert m.with_flag(a, m.core(a)[4] & ~0x400) == m.with_flag(b, m.core(b)[4] & ~0x400)
    assert lit[0].startswith(m.out_header(raw)) and lit[1] == 0
    return flags_of(lit[0]), lit[2]


@pytest.mark.parametrize("seed", range(24))
@pytest.mark.parametrize("ignore_umi", [False, True])
def test_literal_equals_grouped(seed, ignore_umi):
    n = [50, 999, 1000, 1001, 2300, 4100][seed % 6]
    recs = m.sorted_records(seed, n, big=1100 if seed % 3 == 0 else 0, umi_share=[0.7, 0.0, 1.0][seed % 3])
    flags, err = both(recs, ignore_umi)
    dups = sum(1 for f in flags if f & 0x400)
    assert err == m.summary(dups, len(recs))
    if n >= 999:
        assert 0 < dups < len(recs)


def test_generator_covers_what_it_says():
    recs = m.sorted_records(3, 4100, big=1100)
    raw = raw_of(recs)
    cores = [m.core(r) for r in recs]
    tids = [c[0] for c in cores]
    runs = [t for k, t in enumerate(tids) if k == 0 or t != tids[k - 1]]
    assert runs == [0, 1, 0, 2, 1, -1]
    assert any(c[4] & 4 and c[0] >= 0 and c[4] & 0x400 for c in cores) and any(c[4] & 4 and c[0] == -1 for c in cores)
    assert any(not c[4] & 4 and c[4] & 0x400 for c in cores)
    sizes = {}
    recs2, _ = m.grouped_flags(raw)
    run, prev = -1, None
    for r in recs2:
        tid = m.core(r)[0]
        if tid != prev:
            run += 1
        prev = tid
        start, strand, fraglen, umi, mapped = m.signature(r, False)
        if mapped:
            sizes[(run, start, strand)] = sizes.get((run, start, strand), 0) + 1
    got = set(sizes.values())
    assert 1 in got and 2 in got and max(got) > 1024 and got & {63, 64, 65}
    assert any(not s for (_, _, s) in sizes) and any(s for (_, _, s) in sizes)
    assert any((r, p, True) in sizes and (r, p, False) in sizes for (r, p, _) in sizes)      # both strands at one start_pos


def test_chains_are_not_transitive_in_any_order():
    recs = m.chain_records()
    flags, _ = both(recs)
    by_name = {r[36:36 + r[12] - 1]: f for r, f in zip(recs, flags)}
    for order in ("ABC", "ACB", "BAC", "BCA", "CAB", "CBA"):
        # the l_seq are 20, 21, 22 in the order given: forward reads keep it, reverse reads (sorted by pos = end - length) come reversed
        for who in "ABC":
            assert (b"chain%s.%s" % (order.encode(), who.encode())) in by_name
    # forward, file order A B C: seed A takes B (not C); best of {A: 20, B: 21} is B; C is a cluster of its own
    fw = [f for r, f in zip(recs, flags) if not m.core(r)[4] & 16]
    names_fw = [r[36:36 + r[12] - 1] for r in recs if not m.core(r)[4] & 16]
    got = {n: bool(f & 0x400) for n, f in zip(names_fw, fw)}
    assert (got[b"chainABC.A"], got[b"chainABC.B"], got[b"chainABC.C"]) == (True, False, False)
    # B first: seed B takes A and C — one cluster, the longest (the last) kept
    assert (got[b"chainBAC.B"], got[b"chainBAC.A"], got[b"chainBAC.C"]) == (True, True, False)
    assert (got[b"chainBCA.B"], got[b"chainBCA.C"], got[b"chainBCA.A"]) == (True, True, False)
    # C first, then A: seed C takes B only (B is longer: kept), A is alone
    assert (got[b"chainCAB.C"], got[b"chainCAB.A"], got[b"chainCAB.B"]) == (True, False, False)


def test_hand_derived_cases():
    rx = lambda u: aux_z(b"RX", u)                                                        # noqa: E731
    recs = [
        # pos 100 forward, no UMI: tlen 100, 100, -100 (|tlen|), 0 (wildcard), 200 -> {0, 1, 2, 3} and {4}
        rec(b"a0", 0, 100, 0, ((M, 20),), tlen=100),
        rec(b"a1", 0, 100, 0, ((M, 30),), tlen=100),
        rec(b"a2", 0, 100, 0, ((M, 30),), tlen=-100),                                     # ties with a1: the earlier stays best
        rec(b"a3", 0, 100, 0x400, ((M, 10),), tlen=0),
        rec(b"a4", 0, 100, 0x400, ((M, 20),), tlen=200),                                  # alone: loses the 0x400 it came with
        # the same start on the reverse strand: pos 80 + 20 = 100, a group of its own
        rec(b"b0", 0, 80, 16, ((M, 20),), tlen=100),
        # an unmapped read at pos 100 with 0x400: untouched, counted
        rec(b"u0", 0, 100, 4 | 0x400, (), l_seq=20),
        # pos 200: UMIs.  N matches anything; another length never; RX:i is no UMI (fraglen 0 here: wildcard on tlen, empty UMI matches all)
        rec(b"c0", 0, 200, 0, ((M, 20),), aux=rx(b"ACGTAC")),
        rec(b"c1", 0, 200, 0, ((M, 20),), aux=rx(b"ACGTAA")),                             # 1 mismatch: joins
        rec(b"c2", 0, 200, 0, ((M, 20),), aux=rx(b"ACGTTT")),                             # 2 mismatches: not
        rec(b"c3", 0, 200, 0, ((M, 20),), aux=rx(b"NCGTTT")),                             # N + 2 mismatches against c0: not; joins c2
        rec(b"c4", 0, 200, 0, ((M, 20),), aux=rx(b"ACGTA")),                              # length 5: joins neither; a seed of its own
        rec(b"c5", 0, 200, 0, ((M, 25),), aux=aux_i(b"RX", 5), tlen=0),                   # no UMI, tlen 0: joins the first seed, and is longest
        rec(b"c6", 0, 200, 0, ((S, 5), (M, 20)), aux=aux_h(b"RX", b"ACGTAC")),            # type H counts: joins c0; l_seq 25 ties with c5
        # a reverse read whose CIGAR ends at 300 and a forward read that starts there: different strands
        rec(b"d0", 0, 270, 16, ((M, 10), (D, 10), (M, 10)), tlen=-50),
        rec(b"d1", 0, 300, 0, ((M, 20),), tlen=50),
        rec(b"d2", 0, 280, 16, ((M, 20),), tlen=50),                                      # ends at 300 too: joins d0 (|tlen| equal)
        # a new tid: the same position does not meet tid 0's reads
        rec(b"e0", 1, 100, 0, ((M, 20),), tlen=100),
        rec(b"t0", -1, -1, 4, (), l_seq=20),
    ]
    recs.sort(key=lambda r: (m.core(r)[0] & 0xFFFFFFFF, m.core(r)[1] & 0xFFFFFFFF))        # (stable)
    flags, err = both(recs)
    got = {r[36:36 + r[12] - 1]: bool(f & 0x400) for r, f in zip(recs, flags)}
    assert got == {b"a0": True, b"a1": False, b"a2": True, b"a3": True, b"a4": False, b"b0": False, b"u0": True,
                   b"c0": True, b"c1": True, b"c2": False, b"c3": True, b"c4": False, b"c5": False, b"c6": True,
                   b"d0": False, b"d1": False, b"d2": True, b"e0": False, b"t0": False}
    assert err == b"9 / 19 (47.4%) reads were marked as duplicates.\n"
    # --ignore-umi: the c reads all have tlen 0, a wildcard: one cluster, c5 the first of the two longest
    flags, err = both(recs, ignore_umi=True)
    got = {r[36:36 + r[12] - 1]: bool(f & 0x400) for r, f in zip(recs, flags)}
    assert [got[b"c%d" % k] for k in range(7)] == [True, True, True, True, True, False, True]


def test_no_records_prints_nan():
    out, code, err = m.literal(raw_of([]))
    assert code == 0 and out == m.out_header(raw_of([])) and err == b"0 / 0 (NaN%) reads were marked as duplicates.\n"
    assert m.grouped(raw_of([])) == (out, code, err)


def test_literal_partial_output_on_each_stopping_record():
    base = m.sorted_records(5, 2300, big=0)
    full = m.literal(raw_of(base))[0]
    n_hdr = len(m.out_header(raw_of(base)))
    for at in (10, 1500):
        tid, pos = m.core(base[at - 1])[:2]                                                # (the record before: `bad` follows it)
        for what, bad, code, msg in (("secondary", rec(b"sec", tid, pos, 0x100), 255, m.MSG_SECONDARY),
                                     ("supplementary", rec(b"sup", tid, pos, 0x800), 255, m.MSG_SECONDARY),
                                     ("unsorted", rec(b"back", tid, pos - 1), 255, m.MSG_UNSORTED),
                                     ("cigar", rec(b"op9", tid, pos, 16, ((9, 20),), l_seq=20), 101, b"panicked")):
            recs = base[:at] + [bad] + base[at:]
            raw = raw_of(recs)
            assert not m.served(raw)
            out, c, err = m.literal(raw)
            assert (c, err) == (code, msg), what
            got = list(m.records(out))
            # only what flush_reads wrote before the record: nothing in the first tid's first 1000 records, later a flushed prefix
            if at == 10:
                assert out == m.out_header(raw)
            else:
                assert 0 < len(got) <= at and out[n_hdr:] == full[n_hdr:len(out)]
    # an operation code above 8 on a forward or an unmapped read is never looked at
    tid, pos = m.core(base[10])[:2]
    for flag in (0, 4, 4 | 16):
        recs = base[:10] + [rec(b"op9", tid, pos, flag, ((9, 20),), l_seq=20)] + base[10:]
        assert m.literal(raw_of(recs))[1] == 0
    # the order is compared as u32, and not on the first read of a new tid
    recs = [rec(b"a", 0, 500), rec(b"b", 1, 100), rec(b"c", 1, -1, 4, (), l_seq=5), rec(b"d", 1, 100)]
    assert m.literal(raw_of(recs))[1:] == (255, m.MSG_UNSORTED)
    assert m.literal(raw_of(recs[:3]))[1] == 0


def test_umi_matches():
    assert m.umi_matches(b"", b"ACGT") and m.umi_matches(b"ACGT", b"") and m.umi_matches(b"", b"")
    assert not m.umi_matches(b"ACG", b"ACGT")
    assert m.umi_matches(b"ACGT", b"ACGA") and not m.umi_matches(b"ACGT", b"ACAA")
    assert m.umi_matches(b"NNGT", b"TTGA") and not m.umi_matches(b"NCGT", b"TAAT")


def test_fraglen_saturates():
    for tlen, want in ((0, 0), (-7, 7), (65535, 65535), (65536, 65535), (m.INT32_MIN, 65535)):
        assert m.signature(rec(b"x", 0, 5, tlen=tlen), False)[2] == want
    assert m.signature(rec(b"x", 0, 5, tlen=9, aux=aux_z(b"RX", b"AC")), False)[2:4] == (0, b"AC")
    assert m.signature(rec(b"x", 0, 5, tlen=9, aux=aux_z(b"RX", b"AC")), True)[2:4] == (9, b"")
    assert m.signature(rec(b"x", 0, 5, 4, tlen=9, aux=aux_z(b"RX", b"AC")), False)[:4] == (0, True, 0, b"")
    assert struct.unpack_from("<H", m.with_flag(rec(b"x", 0, 5), 0x410), 18)[0] == 0x410
