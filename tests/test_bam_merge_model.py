"""CPU: the properties of tests/bam_merge_model.py — the loop `sam merge` is held to on both paths."""
import struct

import pytest

from tests import bam_merge_model as m


def raws(files):
    return [m.rm.header(m.rm.TEXT, m.rm.REFS) + b"".join(recs) for recs in files]


def merged(files, suffix=False):
    out, err, code = m.model(raws(files), suffix)
    assert (err, code) == (b"", 0)
    return list(m.records(out))


@pytest.mark.parametrize("n_files,shared", [(2, 0.5), (3, 0.0), (5, 1.0), (12, 0.3)])
def test_every_input_keeps_its_order_and_the_output_is_sorted(n_files, shared):
    files = m.served_inputs(n_files, 300, shared=shared, seed=n_files)
    assert all(recs == m.sorted_by_key(recs) for recs in files)                       # (the generator's promise)
    out = merged(files)
    assert len(out) == sum(len(f) for f in files)
    assert sorted(out) == sorted(r for f in files for r in f)
    place = {r: k for k, r in enumerate(out)}                                         # (records are distinct: their names say file and index)
    assert len(place) == len(out)
    for recs in files:
        places = [place[r] for r in recs]
        assert places == sorted(places)
    keys = [m.key(r) for r in out]
    assert keys == sorted(keys)
    assert [m.key64(r) for r in out] == sorted(m.key64(r) for r in out)               # the device's one-number key orders alike


def test_tie_free_inputs_merge_to_the_sort_in_any_order_of_the_files():
    files = m.served_inputs(4, 250, shared=0.0, seed=9)
    keys = [set(m.key(r) for r in f) for f in files]
    assert not any(keys[a] & keys[b] for a in range(4) for b in range(a + 1, 4))
    expect = m.sorted_by_key([r for f in files for r in f])
    for order in ([0, 1, 2, 3], [3, 2, 1, 0], [2, 0, 3, 1]):
        assert merged([files[i] for i in order]) == expect


def test_with_ties_the_earlier_input_comes_first():
    files = m.served_inputs(3, 120, shared=1.0, seed=2)
    assert merged(files) == files[0] + files[1] + files[2]
    assert merged(files[::-1]) == files[2] + files[1] + files[0]
    half = m.served_inputs(3, 400, shared=0.5, seed=3)
    out = merged(half)
    where = {r: f for f, recs in enumerate(half) for r in recs}
    shared_keys = 0
    for a, b in zip(out, out[1:]):
        if m.key(a) == m.key(b):
            assert where[a] <= where[b]
            shared_keys += where[a] < where[b]
    assert shared_keys > 50


def test_key_edges():
    def rec(tid, pos, name):
        return m.placed(m.rm.record(name, 5), tid, pos)
    a = [rec(0, -1, b"a0"), rec(0, 0, b"a1"), rec(0, 2**31 - 1, b"a2"), rec(2, 5, b"a3"), rec(-1, -1, b"a4")]
    b = [rec(0, 0, b"b0"), rec(1, -1, b"b1"), rec(2, 2**31 - 1, b"b2"), rec(-1, -1, b"b3"), rec(-1, 7, b"b4")]
    assert a == m.sorted_by_key(a) and b == m.sorted_by_key(b)
    assert [r[36:38] for r in merged([a, b])] == [b"a0", b"a1", b"b0", b"a2", b"b1", b"a3", b"b2", b"a4", b"b3", b"b4"]


def test_an_unsorted_input_is_still_the_loop():
    def rec(pos, name):
        return m.rm.record(name, 5, tid=0, pos=pos)
    a = [rec(10, b"a0"), rec(5, b"a1"), rec(30, b"a2")]
    b = [rec(7, b"b0"), rec(20, b"b1")]
    assert [r[36:38] for r in merged([a, b])] == [b"b0", b"a0", b"a1", b"b1", b"a2"]


def test_suffix():
    files = m.served_inputs(12, 20, seed=4)
    plain, out = merged(files), merged(files, suffix=True)
    where = {r: f for f, recs in enumerate(files) for r in recs}
    assert len(plain) == len(out)
    for r, s in zip(plain, out):
        sfx = b".%d" % (where[r] + 1)
        lo = r[12]
        assert s[12] == lo + len(sfx) and struct.unpack_from("<i", s)[0] == struct.unpack_from("<i", r)[0] + len(sfx)
        assert s[4:12] == r[4:12] and s[13:36] == r[13:36]
        assert s[36:36 + s[12]] == r[36:36 + lo - 1] + sfx + b"\0" and s[36 + s[12]:] == r[36 + lo:]
    assert {where[r] for r in plain} == set(range(12))


def test_a_name_too_long_with_its_suffix_stops_with_101():
    a = [m.rm.record(b"ok", 5, pos=1), m.rm.record(b"n" * 253, 5, pos=3), m.rm.record(b"late", 5, pos=9)]
    b = [m.rm.record(b"b", 5, pos=2), m.rm.record(b"c", 5, pos=4)]
    rs = raws([a, b])
    out, err, code = m.model(rs, True)
    assert code == 101 and err == m.PANIC
    assert [r[36:36 + r[12] - 1] for r in m.records(out)] == [b"ok.1", b"b.2"]
    assert m.model(rs, False) == (m.out_header(rs[0]) + a[0] + b[0] + a[1] + b[1] + a[2], b"", 0)
    ok = [m.rm.record(b"n" * 252, 5, pos=3)]
    assert m.model(raws([ok, b]), True)[2] == 0                                       # 254 bytes with ".1"


def test_headers():
    recs = m.served_inputs(2, 10, seed=5)
    h = m.rm.header
    base = h(b"@HD\tVN:1.6\n\n", m.rm.REFS) + b"".join(recs[0])
    other_text = h(b"@CO\tother\n", m.rm.REFS) + b"".join(recs[1])
    out, err, code = m.model([base, other_text], False)
    assert code == 0 and out.startswith(m.out_header(base))                           # input 1's header
    lengths = h(m.rm.TEXT, [(n, ln + 1) for n, ln in m.rm.REFS]) + b"".join(recs[1])
    assert m.model([base, lengths], False)[2] == 0                                    # names are compared, lengths are not
    renamed = h(m.rm.TEXT, m.rm.REFS[:2] + [(b"chrX", 5)]) + b"".join(recs[1])
    fewer = h(m.rm.TEXT, m.rm.REFS[:2])
    assert m.model([base, lengths, renamed], False, ["a", "b", "c"]) == (b"", m.sq_error("a", "c"), 255)
    assert m.model([base, fewer, renamed], False, ["a", "b", "c"]) == (b"", m.sq_error("a", "b"), 255)
    assert m.model([base], False) == (b"", m.TWO_ERROR, 255)
