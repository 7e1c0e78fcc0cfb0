"""A plain-Python statement of `sam discard tail artifacts` (src/sam_discard_tail_artifacts.rs:44-240 with count_right_end_offset
:243-255, count_mismatches :257-348 and check_threshold :386-398, and src/genome_reader.rs) over raw BAM bytes, on
tests/bam_rewrite_model.py's reader and writer: the f32 threshold, the two walks with the release build's casts, the chromosome loads,
the header's @CO line, every stderr line, and a generator of a genome and of records the command serves.

The casts (as tests/bam_minimize_model.py states `highest_id`): the reference is built in release mode, so `usize` arithmetic wraps mod
2^64, `x as i32` keeps the low 32 bits and `i32 as usize` sign-extends them.  USIZE, as_i32 and as_usize below are those three.

bio::io::fasta::IndexedReader as this build reads it (UNPINNED, as DESIGN.md §5: the crate is not available here): `<path>.fai` holds
per line name, length, offset, line_bases, line_width; base p of a chromosome is the file's byte offset + p / line_bases * line_width +
p % line_bases; of two lines with one name the later counts; a FASTA file or an index that is missing or does not parse fails
`from_file`.  Seq::encoded_base is read here as refusing an index outside [0, l_seq) (status 101)."""
import functools
import random
import struct

import numpy as np

from tests import bam_rewrite_model as rm
from tests.bam_rewrite_model import EOF_BLOCK, Stop, members, records, write  # noqa: F401  (what the tests use)

f32 = np.float32
USIZE = (1 << 64) - 1
UNMAPPED = 0x4

USAGE = (b"\nUsage:\n  sam discard tail artifacts [options] <ref_genome.fa> <bam_file>\n  sam discard tail artifacts --test\n\nOptions:  \n"
         b"  --tail-length=N    The tail length of the read that is examined [default: 20].\n"
         b"                     The tail length specifies the number of bases that are \n"
         b"                     examined from each end of the read. Indels encountered do\n"
         b"                     not affect this number.\n"
         b"  --threshold=FLOAT  Threshold ratio (0.0-1.0, inclusive) of variations that\n"
         b"                     will cause the read to be discarded [default: 0.15].\n"
         b"  --mismatches=N     Number of mismatches (inclusive) in a tail that will cause \n"
         b"                     the read to be discarded.\n"
         b"                     This number will be converted to a threshold ratio.\n"
         b"  --debug            Print information and save discarded reads to a separate \n"
         b"                     file.\n"
         b"  --test             Run tests and exit.\n\nDescription:\n\n"
         b"This script processes all the reads in a bam-file and removes reads that have \n"
         b"a number of mismatching bases in the tails (ends) of the reads that is above \n"
         b"the specified threshold ratio. Output (new bam file) is written to stdout.\n\n")
INVALID = b"ERROR: Invalid arguments.\n" + USAGE + b"\n"
TAIL_LENGTH_ERROR = b"ERROR: --tail-length requires a positive integer argument.\n"                                  # :53, :60
THRESHOLD_PARSE_ERROR = b"ERROR: --threshold requires a floating point number argument (default: 0.10).\n"         # :54
MISMATCHES_ERROR = b"ERROR: --mismatches requires a positive integer argument.\n"                                   # :64
THRESHOLD_RANGE_ERROR = b"ERROR: --threshold requires a floating point number between 0.0 and 1.0.\n"              # :70
INDEX_ERROR = b"ERROR: Chromosome index error!\n"                                                                   # :159
NO_REFERENCES_PANIC = b"thread 'main' panicked: index out of bounds: the len is 0 but the index is 0\n"              # :119 chr_names[0]
BAD_CIGAR_PANIC = b"thread 'main' panicked: Unexpected cigar operation\n"                                           # read.cigar(), as DESIGN.md §10 reads it
READ_INDEX_PANIC = b"thread 'main' panicked: index out of bounds: the read's bases\n"                               # :283
REF_INDEX_PANIC = b"thread 'main' panicked: index out of bounds: the chromosome's bases\n"                          # :285
SECONDS = b"Processing took N seconds.\n"                                                                           # :236, the number masked


def op_panic(letter):
    return b"thread 'main' panicked: Unexpected CIGAR type: " + letter + b"\n"                                      # :339-343


def open_error(path):
    return b"ERROR: Could not open genome FASTA file '%s'.\n" % str(path).encode()                                 # src/genome_reader.rs:15


def not_found_error(name, path):
    return b"ERROR: Chromosome %s not found in %s.\n" % (name, str(path).encode())                                 # src/genome_reader.rs:22


def mask_seconds(err):
    """stderr with the number of `Processing took N seconds.` replaced by N"""
    return b"".join(SECONDS if ln.startswith(b"Processing took ") and ln.endswith(b" seconds.\n") else ln for ln in err.splitlines(True))


def as_i32(v):
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v & 0x80000000 else v


def as_usize(v):
    """an i32 (or any signed value) `as usize`"""
    return v & USIZE


def fmt(v, digits):
    """"{:.N}" of an f32"""
    v = float(f32(v))
    return "NaN" if v != v else "%.*f" % (digits, v)


# ---- the threshold (:386-398) ----
def check_threshold(tail_length, threshold_ratio):
    thr = f32(threshold_ratio)
    n = 0
    while n <= tail_length:
        if f32(n) / f32(tail_length) >= thr:
            break
        n += 1
    return n


# ---- the genome (src/genome_reader.rs) ----
def parse_fai(text):
    """[(name, length, offset, line_bases, line_width)], or None where a line does not parse"""
    out = []
    lines = text.split(b"\n")
    if lines[-1] == b"":                                                # (an empty last line is no line)
        lines.pop()
    for ln in lines:
        if ln.endswith(b"\r"):
            ln = ln[:-1]
        cols = ln.split(b"\t")
        if len(cols) != 5 or not cols[0] or not all(c.isdigit() and len(c) <= 20 for c in cols[1:]):
            return None
        vals = [int(c) for c in cols[1:]]
        if any(v > USIZE for v in vals) or vals[2] < 1 or vals[3] < vals[2]:
            return None
        out.append((cols[0],) + tuple(vals))
    return out


class Genome:
    """fasta: the FASTA file's bytes; fai: its index's bytes.  Either None: the file is missing."""

    def __init__(self, fasta, fai, path="genome.fa"):
        self.fasta, self.path = fasta, path
        self.index = None if fasta is None or fai is None else parse_fai(fai)
        self.by_name = {e[0]: e for e in self.index} if self.index is not None else {}

    def ok(self):
        return self.index is not None

    def load(self, name):
        """load_chromosome_seq: (chromosome, its INFO line); Stop(255) with .err where the index lacks the name"""
        e = self.by_name.get(name)
        if e is None:
            s = Stop(255)
            s.err = not_found_error(name, self.path)
            raise s
        _, length, offset, lb, lw = e
        seq = bytearray()
        for p in range(length):                                        # (byte by byte: the test genomes are small)
            at = offset + p // lb * lw + p % lb
            if at >= len(self.fasta):
                break
            seq.append(self.fasta[at])
        return bytes(seq), b"INFO: Loaded chromosome %s of length %d bp\n" % (name, len(seq))


# ---- the walks ----
def cigar_of(rec):
    lo, nc = rec[12], struct.unpack_from("<H", rec, 16)[0]
    return [(v & 15, v >> 4) for v in struct.unpack_from("<%dI" % nc, rec, 36 + lo)]


def seq_codes(rec):
    lo, nc, S = rec[12], struct.unpack_from("<H", rec, 16)[0], struct.unpack_from("<i", rec, 20)[0]
    o = 36 + lo + 4 * nc
    return [(rec[o + (k >> 1)] >> (0 if k & 1 else 4)) & 15 for k in range(S)]


def count_right_end_offset(cigar):
    """:243-255, in wrapping i32"""
    offset = 0
    for code, ln in cigar:
        if code == 1:
            offset = as_i32(offset - as_i32(ln))
        elif code == 2:
            offset = as_i32(offset + as_i32(ln))
    return offset


READ_BASE = {1: "A", 2: "C", 4: "G", 8: "T"}                            # :410-412, every other code N
OP_LETTER = {3: b"N", 4: b"S", 5: b"H", 6: b"P", 9: b"9"}               # :339-343 (rust-htslib's Back is code 9)


def stop101(err):
    s = Stop(101)
    s.err = err
    return s


def count_mismatches(tail_length, cigar, codes, seq_index, ref_offset, chr_seq, step):
    """:257-348.  cigar: the operations in the order the walk takes them; seq_index, ref_offset: usize"""
    n_bases_examined = tail_mismatches = 0
    for code, ln in cigar:
        if n_bases_examined >= tail_length:                             # :270, at the top of every op
            break
        if code in (0, 7, 8):                                           # :273-311
            for _ in range(ln):
                n_bases_examined += 1
                if not 0 <= seq_index < len(codes):                     # :283 seq.encoded_base(seq_index)
                    raise stop101(READ_INDEX_PANIC)
                read_acgt = READ_BASE.get(codes[seq_index], "N")
                ri = (ref_offset + seq_index) & USIZE                   # :285 (usize: wraps)
                if ri >= len(chr_seq):
                    raise stop101(REF_INDEX_PANIC)
                ref_acgt = chr(chr_seq[ri])
                if "a" <= ref_acgt <= "z":                              # to_ascii_uppercase
                    ref_acgt = ref_acgt.upper()
                if not (read_acgt == ref_acgt or ref_acgt == "N" or read_acgt == "N"):      # :288
                    tail_mismatches += 1
                seq_index = as_usize(as_i32(as_i32(seq_index) + step))  # :300
                if n_bases_examined >= tail_length:                     # :309, after every base
                    return tail_mismatches
        elif code == 1:                                                 # :312-324: one mismatch whatever its length, no base examined
            tail_mismatches += 1
            ls = as_i32(as_i32(ln) * step)
            seq_index = as_usize(as_i32(as_i32(seq_index) + ls))
            ref_offset = as_usize(as_i32(as_i32(ref_offset) - ls))
        elif code == 2:                                                 # :325-338
            tail_mismatches += 1
            ref_offset = as_usize(as_i32(as_i32(ref_offset) + as_i32(as_i32(ln) * step)))
        else:
            raise stop101(op_panic(OP_LETTER[code]))
    return tail_mismatches


def record_tails(rec, tail_length, chr_seq):
    """(left, right) of a mapped record (:170-193); Stop(101) where cigar() or a walk ends the command"""
    cigar, codes = cigar_of(rec), seq_codes(rec)
    if any(code > 8 for code, _ in cigar):                              # read.cigar(): an operation code above 8
        raise stop101(BAD_CIGAR_PANIC)
    (pos,) = struct.unpack_from("<i", rec, 8)
    ref_offset = as_usize(pos)                                          # :179 read.pos() as usize
    left = count_mismatches(tail_length, cigar, codes, 0, ref_offset, chr_seq, 1)
    ref_offset = as_usize(as_i32(as_i32(ref_offset) + count_right_end_offset(cigar)))      # :189
    right = count_mismatches(tail_length, cigar[::-1], codes, (len(codes) - 1) & USIZE, ref_offset, chr_seq, -1)   # :191 read_len - 1
    return left, right


# ---- the command ----
def ref_names(raw):
    (l_text,) = struct.unpack_from("<i", raw, 4)
    o = 8 + l_text
    (n_ref,) = struct.unpack_from("<i", raw, o)
    o += 4
    names = []
    for _ in range(n_ref):
        (ln,) = struct.unpack_from("<i", raw, o)
        nm = raw[o + 4:o + 4 + ln]
        names.append(nm[:-1] if nm.endswith(b"\0") else nm)
        o += 4 + ln + 4
    return names


def co_line(tail_length, thr):
    return b"@CO\tProcessed with discard tail artifacts (ver 0.5) TAIL_LEN:%d THRESHOLD:%s\n" % (tail_length, fmt(thr, 1).encode())   # :82


def out_header(raw, tail_length, thr):
    """bam_rewrite_model.out_header's text rule, one @CO line behind the text; the binary reference list kept"""
    h = rm.out_header(raw)
    (l_text,) = struct.unpack_from("<i", h, 4)
    text = h[8:8 + l_text] + co_line(tail_length, thr)
    return b"BAM\1" + struct.pack("<i", len(text)) + text + h[8 + l_text:]


def results(total, failed, passed, thr, debug_filename=None):
    """:229-239"""
    pct = fmt(f32(thr) * f32(100.0), 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        share = fmt(f32(failed) / f32(total) * f32(100.0), 1)         # (an empty file: NaN)
    err = "\nDISCARD TAIL ARTIFACT RESULTS\nTotal number of reads processed: %d\n" % total
    err += "Number of reads with %s%% or more tail artifacts: %d [FAILED]\n" % (pct, failed)
    err += "Number of reads with less than %s%% tail artifacts: %d [PASSED]\n\n" % (pct, passed)
    err += "Percentage of processed records discarded %s%%\n\n" % share
    err = err.encode() + SECONDS
    if debug_filename is not None:
        err += b"Reads with tail artifacts written to file: '%s'\n" % debug_filename
    return err + b"ALL DONE.\n"


def model(raw, genome, tail_length=20, threshold=0.15, mismatches=None, debug_filename=None):
    """(inflated stdout, stderr with the seconds masked, status, (total, failed, passed), the refIDs loaded after the first, the
    discarded records); where the reference ends mid-file the records before that are written, by DESIGN.md §10's rule"""
    thr = f32(threshold)
    err = b""
    if mismatches is not None:                                          # :63-67
        thr = f32(mismatches) / f32(tail_length)
        err += b"INFO: Mismatch threshold ratio set to %s\n" % fmt(thr, 2).encode()
    if thr < 0.0 or thr > 1.0:                                          # :69-71
        return b"", err + THRESHOLD_RANGE_ERROR, 255, (0, 0, 0), [], []
    err += b"INFO: %d mismatches in %d read tail bases will cause read to be discarded.\n" % (check_threshold(tail_length, thr), tail_length)   # :73
    out = [out_header(raw, tail_length, thr)]                           # :77-83
    if debug_filename is not None:
        err += b"DEBUG: Writing discarded reads to file '%s'. (debug)\n" % debug_filename      # :89
    total = passed = failed = 0
    loads, discarded = [], []
    try:
        if not genome.ok():                                             # :100
            s = Stop(255)
            s.err = open_error(genome.path)
            raise s
        names = ref_names(raw)
        if not names:                                                   # :119 chr_names[0] of an empty list
            raise stop101(NO_REFERENCES_PANIC)
        chr_index = 0
        chr_seq, line = genome.load(names[0])                           # :119: before the first record
        err += line + b"INFO: Running DISCARD TAIL ARTIFACTS...\n"      # :126
        for rec in records(raw):
            total += 1
            tid, flag = struct.unpack_from("<i", rec, 4)[0], struct.unpack_from("<H", rec, 18)[0]
            if flag & UNMAPPED:                                         # :141-146: written, counted in the total alone, the chromosome untouched
                out.append(rec)
                continue
            if tid != as_i32(chr_index):                                # :149-162
                chr_index = as_usize(tid)
                if chr_index >= len(names):
                    s = Stop(255)
                    s.err = INDEX_ERROR
                    raise s
                chr_seq, line = genome.load(names[chr_index])
                err += line
                loads.append(tid)
            left, right = record_tails(rec, tail_length, chr_seq)
            if f32(left) / f32(tail_length) >= thr or f32(right) / f32(tail_length) >= thr:      # :195-211
                failed += 1
                discarded.append(rec)
            else:
                passed += 1
                out.append(rec)
    except Stop as s:
        return b"".join(out), err + s.err, s.code, (total, failed, passed), loads, discarded
    return b"".join(out), err + results(total, failed, passed, thr, debug_filename), 0, (total, failed, passed), loads, discarded


# ---- inputs ----
CHROMS = [(b"chrA", 5000, 60, 61), (b"chrB", 700, 7, 9), (b"chrC", 61, 61, 61)]       # name, bases, line_bases, line_width
REFS = [(name, n) for name, n, _, _ in CHROMS]
TEXT = b"@HD\tVN:1.6\tSO:unsorted\n" + b"".join(b"@SQ\tSN:%s\tLN:%d\n" % r for r in REFS) + b"\n\n" + b"\0" * 3


@functools.lru_cache(maxsize=None)
def genome_files(seed=1):
    """(FASTA bytes, .fai bytes, {name: the bases as the file holds them}): three chromosomes of 5 000, 700 and 61 bases; lines of
    60 bases and '\\n', of 7 bases and '\\r\\n', and one single line without an end; lower-case stretches, runs of N, R and F"""
    rnd = random.Random(seed)
    fasta, fai, seqs = b"", b"", {}
    for name, n, lb, lw in CHROMS:
        s = bytearray(rnd.choice(b"ACGT") for _ in range(n))
        for _ in range(max(1, n // 400)):                               # lower-case stretches
            a = rnd.randrange(n)
            s[a:a + 37] = bytes(s[a:a + 37]).lower()
        for _ in range(max(1, n // 900)):                               # runs of N (and n)
            a = rnd.randrange(n)
            s[a:a + 11] = (b"N" * 6 + b"n" * 5)[:len(s[a:a + 11])]
        for _ in range(max(2, n // 300)):                               # bytes outside ACGTN
            s[rnd.randrange(n)] = rnd.choice(b"RFrf")
        s = bytes(s[:n])
        fasta += b">" + name + b" test chromosome\n"
        fai += b"%s\t%d\t%d\t%d\t%d\n" % (name, n, len(fasta), lb, lw)
        end = b"\r\n" if lw == lb + 2 else b"\n" if lw == lb + 1 else b""
        fasta += b"".join(s[a:a + lb] + end for a in range(0, n, lb))
        seqs[name] = s
    return fasta, fai, seqs


def write_genome(d, seed=1, fai=True):
    """the genome's two files under d: (path of the FASTA, Genome)"""
    fasta, index, _ = genome_files(seed)
    path = d / "genome.fa"
    path.write_bytes(fasta)
    if fai:
        (d / "genome.fa.fai").write_bytes(index)
    return path, Genome(fasta, index if fai else None, path)


def fai_entries(seed=1):
    """the index as seqkit_amd.capi's bam_file_discard_tails takes it"""
    return parse_fai(genome_files(seed)[1])


CODE = {65: 1, 67: 2, 71: 4, 84: 8}                                     # A C G T


def record(name, tid, pos, cigar, codes, flag=0, aux=b"", mapq=30):
    """one record's bytes: cigar [(code, length)], codes one 4-bit base code per base"""
    nm = name + b"\0"
    S = len(codes)
    body = struct.pack("<iiBBHHHiiii", tid, pos, len(nm), mapq, 4680, len(cigar), flag, S, -1, -1, 0)
    body += nm + b"".join(struct.pack("<I", (ln << 4) | code) for code, ln in cigar)
    cs = list(codes) + [0]
    body += bytes((cs[2 * k] << 4) | cs[2 * k + 1] for k in range((S + 1) // 2)) + bytes([30 + k % 10 for k in range(S)]) + aux
    return struct.pack("<i", len(body)) + body


def aligned(rnd, ref, pos, cigar):
    """the base codes of a read that matches ref from pos on under cigar (a base of the reference outside ACGT is read as A; an
    insertion's bases are drawn), and the read index of every M = X base in order"""
    codes, at, idx = [], pos, []
    for code, ln in cigar:
        if code in (0, 7, 8):
            for _ in range(ln):
                idx.append(len(codes))
                codes.append(CODE.get(ref[at] & 0xDF, 1))
                at += 1
        elif code == 1:
            codes += [rnd.choice([1, 2, 4, 8]) for _ in range(ln)]
        elif code == 2:
            at += ln
    assert at <= len(ref)
    return codes, idx


def other(code):
    return {1: 2, 2: 4, 4: 8, 8: 1}.get(code, 2)


@functools.lru_cache(maxsize=None)
def served_records(n=3000, seed=1, T=20):
    """n records every one of which the command serves against genome_files(1), for any tail length: ops M = X I D; I as first op
    and D as last; I next to D; an I or D exactly at tail length T's end, on either side; 300-op CIGARs; reads at position 0 and reads
    that end on a chromosome's last base; a right walk whose pos + D - I is negative; l_seq odd and even; read codes N and ambiguity
    codes; planted mismatches at tail positions 0, T - 1 and T of either end; unmapped records with refID -1 and with a refID of the
    header; refIDs that go back and forth; two records over 64 KiB, one of them mapped"""
    rnd = random.Random(seed)
    _, _, seqs = genome_files(1)
    refs = [seqs[name] for name, _, _, _ in CHROMS]
    aux = [b"", rm.aux_i(b"NM", 3), rm.aux_z(b"RX", b"ACGT")]
    recs = []
    tid = 0
    for i in range(n):
        kind = i % 24
        if i % 97 == 0:
            tid = rnd.randrange(3)                                      # back and forth
        elif i % 11 == 0:
            tid = (tid + 1) % 3 if i % 22 else 0
        if i in (100, n * 2 // 3):
            tid = 0                                                     # (the long mapped records lie on the long chromosome)
        ref = refs[tid]
        L = len(ref)
        name = b"r%d" % i
        if kind == 0:                                                   # unmapped, refID -1, bases that match nothing
            recs.append(record(name, -1, -1, [], [rnd.choice([1, 2, 4, 8, 15]) for _ in range(rnd.choice([0, 1, 30, 75]))], UNMAPPED | 1))
            continue
        if kind == 1:                                                   # unmapped with a refID of the header, and one of another chromosome than the reads around it
            recs.append(record(name, (tid + 1) % 3, 5, [(0, 10)], [1] * 10, UNMAPPED | 0x10, aux[i % 3]))
            continue
        span = min(rnd.choice([25, 40, 41, 50, 61]), L)
        pos = None
        if kind == 3:
            cigar = [(7, span // 2), (8, span - span // 2)]
        elif kind == 4:
            cigar = [(1, 3), (0, span - 4), (2, 4)]                     # I first, D last
        elif kind == 5:
            cigar = [(0, 10), (1, 2), (2, 3), (0, span - 13)]           # I next to D
        elif kind == 6 and span > 2 * T:
            cigar = [(0, T), (1, 2), (0, span - 2 * T), (2, 1), (0, T)]  # an I exactly where the left tail ends, a D where the right one does
        elif kind == 7 and span > 2 * T:
            cigar = [(0, T), (2, 2), (0, span - 2 * T), (1, 1), (0, T)]
        elif kind == 8:
            cigar = [(0, 1), (1, 1)] * 149 + [(0, 1), (2, 1)]           # 300 ops: the walks stop early
        elif kind == 9:
            cigar = [(0, 2), (1, 12), (0, span - 2)]                    # pos + D - I below 0, every index valid
            pos = rnd.randrange(0, 8)
        elif kind == 10:
            cigar = [(0, 5), (2, rnd.randrange(1, 6)), (0, 9), (1, rnd.randrange(1, 6)), (0, span - 14)]
        else:
            cigar = [(0, span)]
        need = sum(ln for code, ln in cigar if code in (0, 2, 7, 8))    # the reference bases the alignment spans
        if need > L or (pos is not None and pos + need > L):
            cigar, need, pos = [(0, span)], span, None
        if kind == 2:
            pos = 0                                                     # at position 0
        elif kind == 3:
            pos = L - need                                              # ends on the chromosome's last base
        elif pos is None:
            pos = rnd.randrange(0, L - need + 1)
        if i in (100, n * 2 // 3) and L >= 5000:                        # over 64 KiB, mapped: a long insertion between two tails
            cigar = [(0, 30), (1, 50000 + (i & 1)), (0, 30)]
            pos = rnd.randrange(0, L - 60)
        codes, idx = aligned(rnd, ref, pos, cigar)
        m = len(idx)
        plant = []
        if kind in (11, 12, 13):                                        # one mismatch at tail position 0, T - 1 or T, from the left and from the right
            p = (0, T - 1, T)[kind - 11]
            plant = [p, m - 1 - p]
        elif kind in (14, 15):                                          # enough of them to fail a tail
            plant = list(range(0, 8, 2)) if kind == 14 else [m - 1 - k for k in range(0, 9, 3)]
        elif kind == 16:
            plant = [rnd.randrange(m) for _ in range(rnd.randrange(0, 6))]
        for p in plant:
            if 0 <= p < m:
                codes[idx[p]] = other(codes[idx[p]])
        if kind == 17:                                                  # read codes N and ambiguity codes: a match, whatever the genome holds
            for p in (0, 1, m - 1):
                codes[idx[p]] = rnd.choice([15, 0, 3, 5, 10])
        recs.append(record(name, tid, pos, cigar, codes, rnd.choice([0, 0x10, 0x63, 0x93, 0x100, 0x800]), aux[i % 3]))
    recs.append(record(b"big-unmapped", 1, 3, [], [rnd.choice([1, 2, 4, 8]) for _ in range(50001)], UNMAPPED))
    return tuple(recs)


def stop_cases():
    """{label: (the records before, the stopping record, status, the stderr line)}: what ends the reference mid-file"""
    _, _, seqs = genome_files(1)
    ref = seqs[b"chrA"]
    rnd = random.Random(5)

    def rec(cigar, pos=100, tid=0, drop=0):
        codes, _ = aligned(rnd, ref, pos, [c for c in cigar if c[0] in (0, 1, 2, 7, 8)])
        codes = codes + [1] * sum(ln for code, ln in cigar if code == 4)
        return record(b"stop", tid, pos, cigar, codes[:len(codes) - drop], 0)
    before = list(served_records(40, seed=9))
    cases = {}
    for code, letter in OP_LETTER.items():
        if code <= 8:
            cases["op %s left" % letter.decode()] = (before, rec([(code, 3), (0, 40)]), 101, op_panic(letter))
            cases["op %s right" % letter.decode()] = (before, rec([(0, 40), (code, 3)]), 101, op_panic(letter))
    cases["op code 9"] = (before, rec([(0, 40), (9, 3)]), 101, BAD_CIGAR_PANIC)
    cases["read index"] = (before, rec([(0, 40)], drop=30), 101, READ_INDEX_PANIC)
    cases["reference index"] = (before, record(b"stop", 0, 4990, [(0, 40)], [1] * 40, 0), 101, REF_INDEX_PANIC)
    cases["chromosome index"] = (before, record(b"stop", 3, 10, [(0, 40)], [1] * 40, 0), 255, INDEX_ERROR)
    cases["negative chromosome index"] = (before, record(b"stop", -1, 10, [(0, 40)], [1] * 40, 0), 255, INDEX_ERROR)
    return cases
