"""CPU: tests/bam_discard_tails_model.py against the reference's own self-test expectations (src/sam_discard_tail_artifacts.rs:458-531,
held here as a table), check_threshold's f32 values, and a six-record file whose header, output and stderr are spelled out by hand."""
import struct

import numpy as np
import pytest

from tests import bam_discard_tails_model as m

CODE = {"A": 1, "C": 2, "G": 4, "T": 8, "N": 15}
M, I, D = 0, 1, 2


def self_test():
    """the reference's test() over the model's functions: [(label, got)] in its order"""
    got = []
    seq = ["A"] * 50
    ref = bytearray(b"A" * 50)
    cigar = [(M, 50)]

    def run(T, seq_index, ref_offset, step):
        ops = cigar if step > 0 else cigar[::-1]
        return m.count_mismatches(T, ops, [CODE[b] for b in seq], seq_index, m.as_usize(ref_offset), bytes(ref), step)

    def both(left, right, T):
        got.append((left, run(T, 0, 0, 1)))
        got.append((right, run(T, 49, 0, -1)))
    both("IDENTICAL LEFT: ", "IDENTICAL RIGHT", 20)
    both("LONG TAIL LEFT", "LONG TAIL RIGHT", 100)
    ref[0] = ord("N")
    got.append(("REF N", run(1, 0, 0, 1)))
    seq[1] = "N"
    got.append(("SEQ N", run(1, 0, 0, 1)))
    seq[1] = "A"
    ref[0] = ref[49] = ord("a")
    both("LOWER CASE LEFT", "LOWER CASE RIGHT", 20)
    ref[0] = ref[49] = ord("C")
    both("MISMATCH LEFT", "MISMATCH RIGHT", 20)
    ref[19], ref[30] = ord("G"), ord("T")
    both("2 MISMATCH LEFT", "2 MISMATCH RIGHT", 20)
    ref[20], ref[29] = ord("G"), ord("T")
    both("NON-TAIL MISMATCH LEFT", "NON-TAIL MISMATCH RIGHT", 20)
    ref = bytearray(b"F" * 50)
    both("NONSENSE LEFT", "NONSENSE RIGHT", 20)
    both("OVERLAP LEFT", "OVERLAP RIGHT", 50)
    ref = bytearray(b"A" * 20 + b"C" * 20 + b"A" * 20)
    got.append(("REF OFFSET MATCH", m.count_right_end_offset(cigar)))
    cigar = [(M, 20), (D, 10), (M, 20)]
    offset = m.count_right_end_offset(cigar)
    got.append(("REF OFFSET DEL", offset))
    got.append(("DELETION LEFT", run(20, 0, 0, 1)))
    got.append(("DELETION LEFT (2)", run(21, 0, 0, 1)))
    got.append(("INDEL RIGHT", run(40, 49, offset, -1)))
    cigar = [(M, 20), (I, 10), (M, 20)]
    offset = m.count_right_end_offset(cigar)
    got.append(("REF OFFSET INS", offset))
    got.append(("INSERTION LEFT", run(21, 0, 0, 1)))
    got.append(("INSERTION RIGHT", run(50, 49, offset, -1)))                 # (offset as usize: -10 wraps, and the sum wraps back)
    cigar = [(M, 20), (I, 5), (D, 5), (M, 20)]
    offset = m.count_right_end_offset(cigar)
    got.append(("REF OFFSET INS-DEL", offset))
    got.append(("INS-DEL LEFT", run(23, 0, 0, 1)))
    got.append(("INS-DEL RIGHT", run(50, 49, offset, -1)))
    return got


# :458-531: the label and the value each ftr() call expects
EXPECTED = [("IDENTICAL LEFT: ", 0), ("IDENTICAL RIGHT", 0), ("LONG TAIL LEFT", 0), ("LONG TAIL RIGHT", 0), ("REF N", 0), ("SEQ N", 0),
            ("LOWER CASE LEFT", 0), ("LOWER CASE RIGHT", 0), ("MISMATCH LEFT", 1), ("MISMATCH RIGHT", 1), ("2 MISMATCH LEFT", 2),
            ("2 MISMATCH RIGHT", 2), ("NON-TAIL MISMATCH LEFT", 2), ("NON-TAIL MISMATCH RIGHT", 2), ("NONSENSE LEFT", 20), ("NONSENSE RIGHT", 20),
            ("OVERLAP LEFT", 50), ("OVERLAP RIGHT", 50), ("REF OFFSET MATCH", 0), ("REF OFFSET DEL", 10), ("DELETION LEFT", 0),
            ("DELETION LEFT (2)", 2), ("INDEL RIGHT", 11), ("REF OFFSET INS", -10), ("INSERTION LEFT", 2), ("INSERTION RIGHT", 21),
            ("REF OFFSET INS-DEL", 0), ("INS-DEL LEFT", 5), ("INS-DEL RIGHT", 17)]


def test_the_references_self_test_expectations():
    assert self_test() == EXPECTED


@pytest.mark.parametrize("T,thr,want", [(20, 0.15, 3), (20, 0.0, 0), (20, 1.0, 20), (33, 0.15, 5), (20, np.float32(3) / np.float32(20), 3)])
def test_check_threshold(T, thr, want):
    assert m.check_threshold(T, np.float32(thr)) == want
    # a count fails a tail iff it reaches that value: the integer the device compares
    for count in range(T + 3):
        assert (np.float32(count) / np.float32(T) >= np.float32(thr)) == (count >= want)


def test_threshold_prints_as_f32():
    assert m.fmt(np.float32(0.15), 1) == "0.2" and m.fmt(np.float32(0.15) * np.float32(100.0), 1) == "15.0"
    assert m.fmt(np.float32("nan"), 1) == "NaN" and m.fmt(np.float32(3) / np.float32(20), 2) == "0.15"
    assert m.check_threshold(20, np.float32("nan")) == 21                    # (no ratio reaches NaN: no read fails)


FASTA = b">c1 first\nACGTACGTAC\nGTACGTACGT\nAC\n>c2\nTTTTTTTTTT\n"
FAI = b"c1\t22\t10\t10\t11\nc2\t10\t39\t10\t11\n"


def rec(name, tid, pos, bases, flag=0, cigar=None):
    return m.record(name, tid, pos, [(M, len(bases))] if cigar is None else cigar, [CODE[b] for b in bases], flag)


def test_six_records_by_hand():
    assert FASTA[10:20] == b"ACGTACGTAC" and FASTA[39:49] == b"TTTTTTTTTT"
    g = m.Genome(FASTA, FAI, "g.fa")
    recs = [rec(b"r1", 0, 0, "ACGTACGT"),                                     # matches: passes
            rec(b"r2", -1, -1, "GGGG", flag=4),                               # unmapped: written
            rec(b"r3", 1, 0, "AATTTT"),                                       # chromosome 2 is loaded; two mismatches in the left tail: fails
            rec(b"r4", 1, 2, "TTTTT"),                                        # no load; passes
            rec(b"r5", 0, 3, "CCCC", flag=4),                                 # unmapped with a refID: no load
            rec(b"r6", 0, 4, "ACGTAA")]                                       # chromosome 1 again; one mismatch in the right tail: passes
    raw = m.rm.header(b"@HD\tVN:1.6\n\n\0\0", [(b"c1", 22), (b"c2", 10)]) + b"".join(recs)
    out, err, code, counts, loads, discarded = m.model(raw, g, 4, 0.5)
    text = b"@HD\tVN:1.6\n@CO\tProcessed with discard tail artifacts (ver 0.5) TAIL_LEN:4 THRESHOLD:0.5\n"
    header = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", 2) + struct.pack("<i", 3) + b"c1\0" + struct.pack("<i", 22) \
        + struct.pack("<i", 3) + b"c2\0" + struct.pack("<i", 10)
    assert out == header + recs[0] + recs[1] + recs[3] + recs[4] + recs[5]
    assert (code, counts, loads, discarded) == (0, (6, 1, 3), [1, 0], [recs[2]])
    assert err == (b"INFO: 2 mismatches in 4 read tail bases will cause read to be discarded.\n"
                   b"INFO: Loaded chromosome c1 of length 22 bp\n"
                   b"INFO: Running DISCARD TAIL ARTIFACTS...\n"
                   b"INFO: Loaded chromosome c2 of length 10 bp\n"
                   b"INFO: Loaded chromosome c1 of length 22 bp\n"
                   b"\nDISCARD TAIL ARTIFACT RESULTS\n"
                   b"Total number of reads processed: 6\n"
                   b"Number of reads with 50.0% or more tail artifacts: 1 [FAILED]\n"
                   b"Number of reads with less than 50.0% tail artifacts: 3 [PASSED]\n"
                   b"\n"
                   b"Percentage of processed records discarded 16.7%\n"
                   b"\n"
                   b"Processing took N seconds.\n"
                   b"ALL DONE.\n")
    assert m.record_tails(recs[2], 4, b"TTTTTTTTTT") == (2, 0) and m.record_tails(recs[5], 4, b"ACGTACGTACGTACGTACGTAC") == (0, 1)
    # --mismatches=1 is the ratio 1/4: the line of :66, and r6 fails too
    out, err, code, counts, _, _ = m.model(raw, g, 4, 0.15, mismatches=1)
    assert err.startswith(b"INFO: Mismatch threshold ratio set to 0.25\nINFO: 1 mismatches in 4 read tail bases") and counts == (6, 2, 2)
    assert b"THRESHOLD:0.2\n" in out                                          # (0.25 to one place, half to even)


def test_no_records_and_the_errors_before_the_first():
    g = m.Genome(FASTA, FAI, "g.fa")
    raw = m.rm.header(b"", [(b"c1", 22)])
    out, err, code, counts, _, _ = m.model(raw, g)
    assert code == 0 and counts == (0, 0, 0) and b"discarded NaN%\n" in err and out == m.out_header(raw, 20, 0.15)
    assert struct.unpack_from("<i", out, 4)[0] == len(m.co_line(20, 0.15))    # (an empty text: the @CO line alone)
    assert m.model(m.rm.header(b"", []), g)[1:3] == (b"INFO: 3 mismatches in 20 read tail bases will cause read to be discarded.\n" + m.NO_REFERENCES_PANIC, 101)
    assert m.model(raw, m.Genome(FASTA, None, "g.fa"))[1:3] == (b"INFO: 3 mismatches in 20 read tail bases will cause read to be discarded.\n" + m.open_error("g.fa"), 255)
    assert m.model(m.rm.header(b"", [(b"c9", 5)]), g)[1].endswith(m.not_found_error(b"c9", "g.fa"))
    assert m.model(raw, g, 20, 1.5)[:3] == (b"", m.THRESHOLD_RANGE_ERROR, 255)
    assert m.model(raw, g, 20, 0.15, mismatches=21)[1:3] == (b"INFO: Mismatch threshold ratio set to 1.05\n" + m.THRESHOLD_RANGE_ERROR, 255)


def test_fai_lines():
    assert m.parse_fai(FAI) == [(b"c1", 22, 10, 10, 11), (b"c2", 10, 39, 10, 11)]
    assert m.parse_fai(b"c1\t22\t10\t10\t11\r\n") == [(b"c1", 22, 10, 10, 11)]
    for bad in (b"c1\t22\t10\t10\n", b"c1\t22\t10\t10\t11\t5\n", b"\t22\t10\t10\t11\n", b"c1\t-2\t10\t10\t11\n", b"c1\t22\t10\t0\t11\n",
                b"c1\t22\t10\t12\t11\n", b"c1\t22\t10\t10\t11\n\nc2\t10\t39\t10\t11\n", b"c1 22 10 10 11\n"):
        assert m.parse_fai(bad) is None, bad


def test_served_records_cover_what_they_say():
    recs = m.served_records()
    assert 2900 < len(recs) < 3100 and sum(1 for r in recs if len(r) > 65536) >= 3
    cigars = [m.cigar_of(r) for r in recs]
    assert any(len(c) == 300 for c in cigars) and any(c and c[0][0] == I for c in cigars) and any(c and c[-1][0] == D for c in cigars)
    assert {code for c in cigars for code, _ in c} == {0, 1, 2, 7, 8}
    assert any(struct.unpack_from("<i", r, 8)[0] == 0 for r in recs)
    assert {struct.unpack_from("<i", r, 20)[0] & 1 for r in recs} == {0, 1}
    fasta, fai, _ = m.genome_files()
    raw = m.rm.header(m.TEXT, m.REFS) + b"".join(recs)
    for T in (1, 20, 300):
        _, _, code, (total, failed, passed), loads, _ = m.model(raw, m.Genome(fasta, fai), T, 0.15)
        assert code == 0 and total == len(recs) and failed > 50 and passed > 500 and len(loads) > 100 and set(loads) == {0, 1, 2}
