"""CPU: tests/bam_minimize_model.py — the id loop on hand-written cases, and that the generator covers what it says and produces only
records the command serves."""
import collections
import struct

from tests import bam_minimize_model as m


def name_of(rec):
    return rec[36:36 + rec[12] - 1]


def test_ids_by_hand():
    ids = m.Ids()
    got = [ids.take(n) for n in [b"a/1", b"b", b"a/2", b"a", b"/x", b"/y", b"/z", b"b/1/2", b"a", b"b", b"c"]]
    assert got == [1, 2, 1, 3, 4, 4, 5, 2, 3, 6, 7]


def test_one_key_counts_in_pairs():
    ids = m.Ids()
    assert [ids.take(b"/%d" % i) for i in range(7)] == [1, 1, 2, 2, 3, 3, 4]


def test_record_shapes():
    rec = m.record(b"read/1", 5, aux=m.rm.aux_i(b"NM", 1), seed=3, pad=7)
    lo, o = rec[12], 36 + rec[12] + 4
    assert rec[o + 2] & 15 == 7
    a = m.minimize(rec, m.Ids(), True, False, False)
    assert name_of(a) == b"1" and a[36 + 2:] == rec[36 + lo:] and struct.unpack_from("<i", a)[0] == len(a) - 4
    b = m.minimize(rec, m.Ids(), False, False, True)
    assert name_of(b) == b"read/1" and len(b) == 36 + lo + 4 + 3 + 5 and b[o + 2] == rec[o + 2] & 0xF0 and b[o + 3:] == rec[o + 3:o + 8]
    c = m.minimize(rec, m.Ids(), True, True, True, fill=30)
    assert name_of(c) == b"1" and c[-5:] == b"\x1e" * 5 and c[4:12] == rec[4:12] and c[13:36] == rec[13:36]
    assert c[36 + 2:36 + 2 + 4 + 3] == rec[36 + lo:36 + lo + 4 + 2] + bytes([rec[o + 2] & 0xF0])


def test_generator_covers_the_cases():
    recs = m.served_records()
    names = [name_of(r) for r in recs]
    keys = [n.split(b"/")[0] if b"/" in n else n for n in names]
    mult = collections.Counter(collections.Counter(keys).values())
    assert all(mult[k] > 0 for k in (1, 2, 3, 4, 5))
    assert {1, 254} <= {len(n) for n in names}
    assert any(n.startswith(b"/") for n in names)
    first = {}
    gaps = []
    for i, k in enumerate(keys):
        if k in first:
            gaps.append(i - first[k])
        first[k] = i
    assert 1 in gaps and max(gaps) > 2000
    byk = collections.defaultdict(set)
    for n, k in zip(names, keys):
        byk[k].add(n)
    assert any(len(v) >= 3 for k, v in byk.items() if k)                # equal up to the '/', different behind it
    ids = m.Ids()
    assert max(ids.take(n) for n in names) >= 10000                     # 1 to 5 digits
    l_seq = [struct.unpack_from("<i", r, 20)[0] for r in recs]
    assert 0 in l_seq and any(x & 1 for x in l_seq) and any(x and not x & 1 for x in l_seq) and sum(len(r) > 65536 for r in recs) >= 2
    pads, aux, ff = set(), set(), 0
    for r, S in zip(recs, l_seq):
        o = 36 + r[12] + 4 * struct.unpack_from("<H", r, 16)[0]
        if S & 1:
            pads.add(r[o + S // 2] & 15)
        aux.add(r[o + (S + 1) // 2 + S:])
        ff += S > 0 and r[o + (S + 1) // 2:o + (S + 1) // 2 + S] == b"\xff" * S
    assert len(pads - {0}) >= 2 and b"" in aux and len(aux) >= 5 and ff > 100


def test_generator_records_are_all_served():
    raw = m.rm.header(m.rm.TEXT, m.rm.REFS) + b"".join(m.served_records())
    n = len(m.served_records())
    for combo in m.COMBOS:
        out, code = m.model(raw, combo, 30)
        assert code is None                                             # Stop is raised for none of them
        assert len(list(m.records(out))) == n


def test_model_stops_at_cigar_op_9():
    raw = m.rm.header(m.rm.TEXT, m.rm.REFS) + m.record(b"a", 10) + m.record(b"b", 10, cigar_op=9) + m.record(b"c", 10)
    for combo in m.COMBOS:
        out, code = m.model(raw, combo)
        assert code == 101 and len(list(m.records(out))) == 1
