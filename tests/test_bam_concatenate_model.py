"""CPU: tests/bam_concatenate_model.py against a hand-spelled expectation, and its properties on generated inputs."""
import struct

from tests import bam_concatenate_model as m


def hand_record(tid, pos, name, tail):
    """a record spelled field by field: refID, pos, l_read_name, mapq 30, bin 4680, no CIGAR, flag 4, l_seq 0, next refID -1, next pos -1, tlen 0"""
    body = struct.pack("<iiBBHHHiiii", tid, pos, len(name) + 1, 30, 4680, 0, 4, 0, -1, -1, 0) + name + b"\0" + tail
    return struct.pack("<i", len(body)) + body


def test_two_inputs_of_two_records_spelled_out(tmp_path):
    aux = b"NMC\x05"
    one = [hand_record(1, 700, b"r", b""), hand_record(0, 5, b"read/1", aux)]                 # (not sorted)
    two = [hand_record(-1, -1, b"r", aux), hand_record(0, 9, b"x.y", b"")]
    raw1 = m.write(tmp_path / "a.bam", one, text=b"@HD\tVN:1.6\n\n\0\0", refs=[(b"chr1", 1000), (b"chr2", 900)])
    raw2 = m.write(tmp_path / "b.bam", two, text=b"@CO\tother\n", refs=[(b"zz", 7)])
    header = (b"BAM\1" + struct.pack("<i", 11) + b"@HD\tVN:1.6\n" + struct.pack("<i", 2)
              + struct.pack("<i", 5) + b"chr1\0" + struct.pack("<i", 1000) + struct.pack("<i", 5) + b"chr2\0" + struct.pack("<i", 900))
    core = struct.pack("<BHHHiiii", 30, 4680, 0, 4, 0, -1, -1, 0)                             # mapq .. tlen, the same in all four
    exp = (header
           + struct.pack("<iiiB", 32 + 4, 1, 700, 4) + core + b"r.1\0"
           + struct.pack("<iiiB", 32 + 9 + 4, 0, 5, 9) + core + b"read/1.1\0" + aux
           + struct.pack("<iiiB", 32 + 4 + 4, -1, -1, 4) + core + b"r.2\0" + aux
           + struct.pack("<iiiB", 32 + 6, 0, 9, 6) + core + b"x.y.2\0")
    assert m.model([raw1, raw2]) == (exp, b"", 0)


def test_properties_on_generated_inputs(tmp_path):
    sizes = [300, 0, 1, 120, 7, 0, 64, 65, 2, 33, 50, 20]
    files = m.served_inputs(12, sizes, seed=4)
    assert any(sorted(f, key=lambda r: struct.unpack_from("<Ii", r, 4)) != f for f in files)   # not sorted by position
    assert {len(m.refs_of(f)) for f in range(12)} == {1, 3, 4}
    assert {r[12] - 1 for f in files for r in f} >= {1, 2, 60}
    assert {struct.unpack_from("<i", r, 20)[0] % 4 for f in files for r in f} == {0, 1, 2, 3}
    paths, raws = m.write_all(tmp_path, files)
    out, err, code = m.model(raws)
    assert (err, code) == (b"", 0)
    assert out.startswith(m.out_header(raws[0]))
    got = list(m.records(out))
    assert len(got) == sum(sizes)
    at = 0
    for b, f in enumerate(files):                                                             # order kept within and across inputs
        for src in f:
            rec = got[at]
            at += 1
            assert rec[36:36 + rec[12] - 1].endswith(b".%d" % (b + 1))
            assert m.strip_suffix(rec, b + 1) == src
    assert at == len(got)
    assert len(out) == len(m.out_header(raws[0])) + sum(len(r) + 1 + len(str(b + 1)) for b, f in enumerate(files) for r in f)


def test_one_input_is_the_two_files_error(tmp_path):
    raw = m.write(tmp_path / "a.bam", m.served_inputs(1, 5)[0])
    assert m.model([raw]) == (b"", m.TWO_ERROR, 255)
    assert m.model([]) == (b"", m.TWO_ERROR, 255)


def test_a_name_too_long_with_its_suffix(tmp_path):
    one = m.served_inputs(1, 40, seed=2)[0]
    two = m.served_inputs(1, 30, seed=3)[0]
    two[11] = m.rm.record(b"n" * 253, 5)
    raw1, raw2 = m.write(tmp_path / "a.bam", one), m.write(tmp_path / "b.bam", two)
    out, err, code = m.model([raw1, raw2])
    assert (err, code) == (m.PANIC, 101)
    assert out == m.out_header(raw1) + b"".join(m.with_suffix(r, 1) for r in one) + b"".join(m.with_suffix(r, 2) for r in two[:11])
    two[11] = m.rm.record(b"n" * 252, 5)                                                      # 254 bytes with ".2": served
    raw2 = m.write(tmp_path / "b.bam", two)
    out, err, code = m.model([raw1, raw2])
    assert (err, code) == (b"", 0) and len(list(m.records(out))) == 70
    assert m.model([raw1] * 9 + [raw2])[2] == 101                                              # ".10" is a byte more


def test_a_file_that_cannot_be_opened(tmp_path):
    one = m.served_inputs(1, 10, seed=2)[0]
    raw = m.write(tmp_path / "a.bam", one)
    out, err, code = m.model([raw, raw, None], ["a", "b", "/none/c.bam"])
    assert (err, code) == (b"ERROR: Cannot open BAM file '/none/c.bam'\n", 255)
    assert out == m.out_header(raw) + b"".join(m.with_suffix(r, 1) for r in one) + b"".join(m.with_suffix(r, 2) for r in one)
    assert m.model([None, raw], ["/none/a.bam", "b"]) == (b"", b"ERROR: Cannot open BAM file '/none/a.bam'\n", 255)
