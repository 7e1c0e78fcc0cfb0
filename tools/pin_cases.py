#!/usr/bin/env python3
"""The corpus of tools/pin_with_cargo.sh: run the reference's binaries and the oracle's on the same inputs, compare everything
observable (stdout, stderr, exit code, decompressed *.gz outputs).  Never run here (no Rust toolchain); see the shell script.
Known, documented differences are normalised: a Rust panic's message text (exit 101: only the code is compared), and the order
of equal counts in the dry run's table (a HashMap's iteration order)."""
import argparse
import gzip
import os
import shutil
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
from hypothesis import HealthCheck, given, settings  # noqa: E402

from oracle import oracle as orc  # noqa: E402
from seqkit_amd import synth  # noqa: E402
from tests import cli_util as cu  # noqa: E402
from tests.test_text_model import cases  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--ref-fasta", required=True)
ap.add_argument("--ref-sam", required=True)
args = ap.parse_args()
failures = 0


def run_both(ref_bin, orc_bin, argv, files, label):
    global failures
    outs = []
    for binary in (ref_bin, orc_bin):
        d = tempfile.mkdtemp(prefix="sk_pin_")
        try:
            for name, data in files.items():
                with open(os.path.join(d, name), "wb") as f:
                    f.write(data)
            r = subprocess.run([binary] + argv, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
            gz = {f: gzip.open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d)) if f.endswith(".gz")}
        finally:
            shutil.rmtree(d, ignore_errors=True)
        outs.append((r.returncode % 256, r.stdout, r.stderr, gz))
    a, b = outs
    same = a[0] == b[0] and (a[0] == 101 or (sorted(a[1].splitlines()) == sorted(b[1].splitlines()) and a[2] == b[2] and a[3] == b[3]))
    if not same:
        failures += 1
        print(f"DIFFERENT: {label}: {' '.join(argv)}\n  reference rc={a[0]} stderr={a[2][-300:]!r}\n  oracle    rc={b[0]} stderr={b[2][-300:]!r}")


# cfg 1-3 shaped inputs
seq, qual = synth.make_reads(2000, 150, seed=1)
qual = synth.add_forced_classes(qual, seed=2)
fq = synth.fastq_text(seq, qual, prefix="SIM:1")
for m in ("0", "2", "20", "30", "41", "255", "256", "x"):
    run_both(args.ref_fasta, orc.FASTA_BIN, ["trim", "by", "quality", "r.fq", m], {"r.fq": fq}, "trim")
    run_both(args.ref_fasta, orc.FASTA_BIN, ["mask", "by", "quality", "r.fq", m], {"r.fq": fq}, "mask")
table = synth.make_sheet(16, 8, seed=3)
bc, _ = synth.observe_barcodes(table, 2000, seed=3)
headers = [f"@SIM:3:{i} 1:N:0 BC:".encode() + bc[i].tobytes() for i in range(2000)]
sheet = b"".join(f"S{i}\t".encode() + table[i].tobytes() + b"\n" for i in range(16))
run_both(args.ref_fasta, orc.FASTA_BIN, ["demultiplex", "sheet.tsv", "r.fq"], {"sheet.tsv": sheet, "r.fq": synth.fastq_text(seq, qual, headers=headers)}, "demultiplex cfg3")
run_both(args.ref_fasta, orc.FASTA_BIN, ["demultiplex", "--dry-run=1500", "sheet.tsv", "r.fq"], {"sheet.tsv": sheet, "r.fq": synth.fastq_text(seq, qual, headers=headers)}, "dry run")


# the text layer
@settings(max_examples=400, deadline=None, derandomize=True, suppress_health_check=list(HealthCheck))
@given(cases())
def text_cases(case):
    files, argv, *_ = case
    run_both(args.ref_fasta, orc.FASTA_BIN, ["demultiplex"] + argv, files, "text layer")


text_cases()
# BAM
rng = np.random.default_rng(5)
recs = [dict(tid=int(rng.integers(0, 2)), pos=i, flag=int(rng.choice([99, 147, 83, 163, 1123, 4, 355, 2147, 65, 129])), mtid=int(rng.integers(0, 2)), mpos=i + 3,
             tlen=int(rng.integers(-6000, 6000)), name=f"r{i}", seq_len=int(rng.integers(1, 200))) for i in range(20000)]
d = tempfile.mkdtemp(prefix="sk_pin_bam_")
cu.write_bam(os.path.join(d, "a.bam"), [("chr1", 100000), ("chr2", 50000)], recs)
bam = open(os.path.join(d, "a.bam"), "rb").read()
shutil.rmtree(d)
for argv in (["statistics", "a.bam"], ["fragment", "lengths", "a.bam"], ["fragment", "lengths", "--max-frag-size=300", "--reads=1000", "a.bam"], ["fragments", "a.bam"]):
    run_both(args.ref_sam, orc.SAM_BIN, argv, {"a.bam": bam}, "sam")


# sam minimize (no oracle binary has it: the reference against tests/bam_minimize_model.py, which the hosts are tested against).  Three
# statements about rust-htslib 0.31's Record::set and cigar() are unpinned: set() drops the aux data and writes the
# unused low nibble of an odd l_seq's last base byte as 0, and cigar() panics (exit 101) on an operation code above 8.
def minimize_cases():
    global failures
    from tests import bam_minimize_model as mm
    served = [mm.record(b"pair/1", 7, aux=mm.AUX[2], seed=1, pad=9), mm.record(b"pair/2", 8, aux=mm.AUX[1], seed=2),
              mm.record(b"/x", 1, seed=3, pad=15), mm.record(b"pair", 0, aux=mm.AUX[3], seed=4), mm.record(b"/y", 33, seed=5, pad=1, qual=0xFF)]
    files = {"odd l_seq, pad nibbles, aux data": served + list(mm.served_records(2000, seed=9)),
             "CIGAR op code 9": served + [mm.record(b"stop", 12, cigar_op=9), mm.record(b"never", 12)]}
    for label, recs in files.items():
        d = tempfile.mkdtemp(prefix="sk_pin_min_")
        try:
            raw = mm.write(os.path.join(d, "m.bam"), recs)
            for combo in mm.COMBOS:
                for fill in (None, 0):
                    argv = ["minimize", "--uncompressed"] + mm.args(combo, fill) + ["m.bam"]
                    r = subprocess.run([args.ref_sam] + argv, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
                    exp, code = mm.model(raw, combo, 255 if fill is None else fill)
                    got = b"".join(x for x, _ in mm.members(r.stdout)) if r.stdout else b""
                    if r.returncode % 256 != (code or 0) or got != exp:
                        failures += 1
                        print(f"DIFFERENT: sam minimize, {label}: {' '.join(argv)}\n  reference rc={r.returncode} stderr={r.stderr[-300:]!r}, model rc={code or 0}")
        finally:
            shutil.rmtree(d, ignore_errors=True)
    for argv in (["minimize", "m.bam"], ["minimize", "--base-qualities", "m.bam"], ["minimize", "--tags", "--baseq-fill=256", "m.bam"], ["minimize"]):
        outs = [subprocess.run([b] + argv, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60) for b in (args.ref_sam, cu.SAM)]
        if (outs[0].returncode, outs[0].stdout, outs[0].stderr) != (outs[1].returncode, outs[1].stdout, outs[1].stderr):
            failures += 1
            print(f"DIFFERENT: sam minimize messages: {' '.join(argv)}\n  reference {outs[0].stderr[-300:]!r}\n  host      {outs[1].stderr[-300:]!r}")


minimize_cases()


# sam subsample.  The reference's generator is unseeded, so no run of it can be held to particular records; what every run must show is
# what tests/bam_subsample_model.py shows for any seed: the counts of its stderr lines, an output that is an in-order subset of the
# counted records (those without 0x800) and closed under the pairing (the 2nd, 4th .. counted record of a name shares the fate of the one
# before it), fractions 1 and an unparsable one exactly, and the status and partial output at a record without 0x1.  That rand 0.5's
# random::<f32>() is (u32 >> 8) * 2^-24 compared with <= is unpinned: a share test of one run would not tell it apart.
def subsample_cases():
    global failures
    import re
    from tests import bam_subsample_model as sm

    def differs(what, detail=""):
        global failures
        failures += 1
        print(f"DIFFERENT: sam subsample: {what} {detail}")
    d = tempfile.mkdtemp(prefix="sk_pin_sub_")
    try:
        raw = sm.write(os.path.join(d, "s.bam"), sm.served_records(4000, seed=9))
        counted = [r for r in sm.records(raw) if not sm.flag_of(r) & 0x800]
        for text in ("0.5", "1", ".25", "0"):
            r = subprocess.run([args.ref_sam, "subsample", "s.bam", text], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
            got = list(sm.records(b"".join(x for x, _ in sm.members(r.stdout)))) if r.stdout else []
            mt = re.fullmatch(rb"Total reads: (\d+)\nKept reads: (\d+) \(([0-9.]+)% of all reads\)\n", r.stderr)
            if r.returncode != 0 or not mt or int(mt.group(1)) != len(counted) or int(mt.group(2)) != len(got):
                differs("counts", f"fraction {text}: rc={r.returncode} stderr={r.stderr[-300:]!r}, {len(got)} records written")
                continue
            if mt.group(3) != b"%.1f" % (len(got) / len(counted) * 100.0):
                differs("percentage", f"fraction {text}: {r.stderr!r}")
            at, pending, closed = 0, {}, True
            for rec in counted:
                kept = at < len(got) and got[at] == rec
                name = sm.qname(rec)
                if name in pending:
                    closed = closed and pending.pop(name) == kept
                else:
                    pending[name] = kept
                at += kept
            if at != len(got) or not closed:
                differs("subset in order / mate closure", f"fraction {text}: {at} of {len(got)} written records matched, closed={closed}")
            if text == "1" and len(got) != len(counted):
                differs("fraction 1 keeps every counted record", f"{len(got)} of {len(counted)}")
        recs = list(sm.served_records(200, seed=4))
        recs[120] = sm.rm.record(b"single", 21, flag=0x10)
        raw = sm.write(os.path.join(d, "u.bam"), recs)
        r = subprocess.run([args.ref_sam, "subsample", "u.bam", "1"], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        exp_out, exp_err, code, _, _ = sm.model(raw, 0, sm.parse_fraction("1"))
        got = b"".join(x for x, _ in sm.members(r.stdout)) if r.stdout else b""
        if r.returncode % 256 != code or r.stderr != exp_err or got != exp_out:
            differs("a record without 0x1", f"rc={r.returncode} stderr={r.stderr[-300:]!r}")
        for text in ("abc", "1.5", "nan", " 0.5", "0x1p-1"):
            r = subprocess.run([args.ref_sam, "subsample", "s.bam", text], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
            if (r.returncode % 256, r.stdout, r.stderr) != (255, b"", sm.FRACTION_ERROR):
                differs("fraction message", f"{text!r}: rc={r.returncode} stderr={r.stderr[-300:]!r}")
    finally:
        shutil.rmtree(d, ignore_errors=True)


subsample_cases()


# sam coverage histogram.  The reference shells out to `samtools depth -a`: these cases need a host that has samtools (1.13 or later) on
# its PATH, and hold the reference to tests/bam_coverage_model.py's literal statement, which the hosts are tested against.  One case per
# unpinned statement of DESIGN.md §10: which records count and what they cover (all nine CIGAR ops, a code above 8, 0x800 counted, the
# 0x704 flags not, clipping at both ends), references without a counted record are not reported (-a, not -aa), depths above 10 000 are
# passed over (and not capped at 8 000), REGION forms and a BED file (both need "c.bam.bai": the cases write a sorted file and index it
# with `samtools index`; this build needs no index), an unknown region (zeros, status 0), both options together, and the long-CIGAR CG
# placeholder, which this build reads by its in-record CIGAR (a known difference: reported, not counted as a failure).
def coverage_cases():
    global failures
    from tests import bam_coverage_model as cm
    if not shutil.which("samtools"):
        print("sam coverage histogram: no samtools on this host, cases not run")
        return

    def differs(what, detail=""):
        global failures
        failures += 1
        print(f"DIFFERENT: sam coverage histogram: {what} {detail}")
    d = tempfile.mkdtemp(prefix="sk_pin_cov_")
    try:
        refs = cm.refs_for() + [(b"odd:1-5", 500)]
        pile = [cm.rec(b"p%d" % i, 10, 100, cigar=((cm.M, (i % 200) + 1),), l_seq=0) for i in range(10400)]
        raw = cm.write(os.path.join(d, "c.bam"), cm.sorted_records(6000, refs, skip_refs=(4, 10)) + pile, text=b"@HD\tVN:1.6\tSO:coordinate\n", refs=refs)
        subprocess.run(["samtools", "index", "c.bam"], cwd=d, check=False)
        bed = b"ref1\t10\t200\nref1\t150\t400\nref3\t0\t99999\nnope\t1\t2\nref5\t400\t500\n"
        with open(os.path.join(d, "r.bed"), "wb") as f:
            f.write(bed)
        for argv, mode in ((["c.bam"], ("everywhere",)), (["--region=ref2", "c.bam"], ("region", b"ref2")), (["--region=ref2:100-1,000", "c.bam"], ("region", b"ref2:100-1,000")),
                           (["--region=ref2:100", "c.bam"], ("region", b"ref2:100")), (["--region=odd:1-5", "c.bam"], ("region", b"odd:1-5")),
                           (["--region=ref4:5-50", "c.bam"], ("region", b"ref4:5-50")), (["--region=nope", "c.bam"], ("region", b"nope")),
                           (["--regions=r.bed", "c.bam"], ("bed", bed))):
            r = subprocess.run([args.ref_sam, "coverage", "histogram"] + argv, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
            hist, dropped, _, _ = cm.literal(raw, mode)
            if r.returncode != 0 or r.stdout != cm.stdout_of(hist):
                differs(" ".join(argv), f"rc={r.returncode} stderr={r.stderr[-300:]!r}; the model drops {dropped} positions above the last bin")
        r = subprocess.run([args.ref_sam, "coverage", "histogram", "--region=ref1", "--regions=r.bed", "c.bam"], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        if (r.returncode % 256, r.stdout, r.stderr) != (255, b"", cm.MSG_BOTH):
            differs("both options", f"rc={r.returncode} stderr={r.stderr[-300:]!r}")
        # the CG placeholder: kSmN in the record, the real CIGAR in CG:B,I
        real = [(cm.M, 30), (cm.D, 2), (cm.M, 20)]
        cg = b"CGBI" + len(real).to_bytes(4, "little") + b"".join(((ln << 4) | op).to_bytes(4, "little") for op, ln in real)
        recs = [cm.rec(b"long", 0, 10, 0, ((cm.S, 50), (cm.N, 52)), l_seq=50, aux=cg)]
        raw = cm.write(os.path.join(d, "g.bam"), recs, text=b"@HD\tVN:1.6\n", refs=[(b"a", 200)])
        r = subprocess.run([args.ref_sam, "coverage", "histogram", "g.bam"], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        if r.stdout != cm.stdout_of(cm.literal(raw)[0]):
            print("known difference: sam coverage histogram reads a CG placeholder record by its in-record CIGAR (DESIGN.md §10)")
    finally:
        shutil.rmtree(d, ignore_errors=True)


coverage_cases()

# sam merge.  The reference's heap fixes everything but the order of records of different inputs with one key: a
# case without such ties must match tests/bam_merge_model.py byte for byte, with and without --suffix, for sorted and unsorted inputs
# and in any order of the files; a case with ties is the known deviation — there the reference must still write the same records, every
# input's in its own order, sorted by the key (reported, not counted as a failure, when only the tie order differs).  And the messages.
def merge_cases():
    global failures
    from tests import bam_merge_model as gm

    def differs(what, detail=""):
        global failures
        failures += 1
        print(f"DIFFERENT: sam merge: {what} {detail}")

    def ref(argv, d):
        r = subprocess.run([args.ref_sam, "merge"] + argv, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        return r.returncode % 256, (b"".join(x for x, _ in gm.members(r.stdout)) if r.stdout else b""), r.stderr
    d = tempfile.mkdtemp(prefix="sk_pin_merge_")
    try:
        free = gm.served_inputs(4, 1500, shared=0.0, seed=9)
        free[3] = free[3][700:] + free[3][:700]                               # an unsorted input: the same loop
        tied = gm.served_inputs(3, 1500, shared=0.5, seed=3)
        for label, files, known in (("no ties", free, False), ("ties", tied, True)):
            names = ["%s%d.bam" % (label[0], i) for i in range(len(files))]
            raws = [gm.write(os.path.join(d, n), recs) for n, recs in zip(names, files)]
            for order in (list(range(len(files))), list(range(len(files)))[::-1]):
                for extra in ([], ["--suffix"], ["--uncompressed", "--suffix"]):
                    argv = extra + [names[i] for i in order]
                    code, out, err = ref(argv, d)
                    exp = gm.model([raws[i] for i in order], "--suffix" in extra, [names[i] for i in order])
                    if (out, err, code) == exp:
                        continue
                    got, want = list(gm.records(out)), list(gm.records(exp[0]))
                    same_but_ties = code == 0 and sorted(got) == sorted(want) and [gm.key(r) for r in got] == [gm.key(r) for r in want]
                    if known and same_but_ties:
                        print(f"known difference: sam merge writes records of different inputs with one key in the inputs' order (DESIGN.md §10): {' '.join(argv)}")
                    else:
                        differs(label, f"{' '.join(argv)}: rc={code} stderr={err[-300:]!r}")
        raw = [gm.write(os.path.join(d, "n%d.bam" % i), tied[i], refs=rf) for i, rf in enumerate([gm.rm.REFS, [(n, ln + 1) for n, ln in gm.rm.REFS],
                                                                                                 gm.rm.REFS[:2] + [(b"chrX", 16569)]])]
        for argv, idx in ((["n0.bam", "n1.bam"], [0, 1]), (["n0.bam", "n1.bam", "n2.bam"], [0, 1, 2]), (["n0.bam"], [0])):
            code, out, err = ref(argv, d)
            exp = gm.model([raw[i] for i in idx], False, argv)
            if (code, err) != (exp[2], exp[1]) or (exp[2] and out != exp[0]):
                differs("headers and messages", f"{' '.join(argv)}: rc={code} stderr={err[-300:]!r}")
        long = [gm.rm.record(b"ok", 5, pos=1), gm.rm.record(b"n" * 253, 5, pos=3), gm.rm.record(b"late", 5, pos=9)]
        raws = [gm.write(os.path.join(d, "l0.bam"), long), gm.write(os.path.join(d, "l1.bam"), [gm.rm.record(b"b", 5, pos=2)])]
        code, out, err = ref(["--suffix", "l0.bam", "l1.bam"], d)
        if (code, out) != (101, gm.model(raws, True)[0]):
            differs("a name of 253 bytes with --suffix", f"rc={code} stderr={err[-300:]!r}")
    finally:
        shutil.rmtree(d, ignore_errors=True)


merge_cases()

# sam concatenate.  src/sam_concatenate.rs is a source file that the reference's src/sam_main.rs does not declare: these cases need a
# host with Rust, on which the reference was built with that module declared and dispatched (--ref-sam names that binary); any other
# reference binary answers with its top-level usage, and the cases are not run.  They hold it to tests/bam_concatenate_model.py byte for
# byte: unsorted inputs with different reference lists under the first header, the suffixes up to ".12", --uncompressed, the two-files
# message, and the two readings of DESIGN.md §10: the stop at a new name of 255 bytes, and "-" in first place, which the reference,
# opening its first path twice, cannot serve (reported, not counted as a failure).
def concatenate_cases():
    global failures
    from tests import bam_concatenate_model as cc

    def differs(what, detail=""):
        global failures
        failures += 1
        print(f"DIFFERENT: sam concatenate: {what} {detail}")

    def ref(argv, d, stdin=None):
        r = subprocess.run([args.ref_sam, "concatenate"] + argv, cwd=d, input=stdin, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        return r.returncode % 256, (b"".join(x for x, _ in cc.members(r.stdout)) if r.stdout else b""), r.stderr
    d = tempfile.mkdtemp(prefix="sk_pin_concat_")
    try:
        sizes = [700, 500, 0, 300, 1, 200, 150, 100, 80, 60, 40, 20]
        names = ["c%d.bam" % i for i in range(len(sizes))]
        raws = [cc.write(os.path.join(d, n), recs, refs=cc.refs_of(i)) for i, (n, recs) in enumerate(zip(names, cc.served_inputs(len(sizes), sizes, seed=6)))]
        code, out, err = ref(names[:1], d)
        if b"sam concatenate" not in err:
            print("sam concatenate: this reference binary does not declare the command (src/sam_main.rs), cases not run")
            return
        if (code, out, err) != (255, b"", cc.TWO_ERROR):
            differs("one path", f"rc={code} stderr={err[-300:]!r}")
        for k in (2, 3, 12):
            for extra in ([], ["--uncompressed"]):
                code, out, err = ref(extra + names[:k], d)
                if (out, err, code) != cc.model(raws[:k], names[:k]):
                    differs(f"{k} inputs", f"{' '.join(extra)}: rc={code} stderr={err[-300:]!r}")
        long = [cc.rm.record(b"ok", 5), cc.rm.record(b"n" * 253, 5), cc.rm.record(b"late", 5)]
        lraws = [cc.write(os.path.join(d, "l0.bam"), [cc.rm.record(b"b", 5)]), cc.write(os.path.join(d, "l1.bam"), long)]
        code, out, err = ref(["l0.bam", "l1.bam"], d)
        if (code, out) != (101, cc.model(lraws)[0]):
            differs("a name of 253 bytes", f"rc={code} stderr={err[-300:]!r}")
        code, out, err = ref(["-", names[1]], d, stdin=open(os.path.join(d, names[0]), "rb").read())
        if (out, err, code) != cc.model(raws[:2], ["-", names[1]]):
            print("known difference: sam concatenate reads \"-\" in first place once and serves it (DESIGN.md §10)")
    finally:
        shutil.rmtree(d, ignore_errors=True)


concatenate_cases()


# sam discard tail artifacts.  src/sam_discard_tail_artifacts.rs and src/genome_reader.rs are source files that the reference's
# src/sam_main.rs does not declare: these cases need a host with Rust, on which the reference was built from a copy with `mod
# sam_discard_tail_artifacts; mod genome_reader;`, a dispatch arm for "discard tail artifacts", `use crate::genome_reader::RefGenomeReader`
# at :11 and the crates bio and ansi_term (--ref-sam names that binary); any other reference binary answers with its top-level usage, and
# the cases are not run.  They hold it to tests/bam_discard_tails_model.py: the served records over the parameter grid, every stop
# (status, and for an ERROR: the message; a panic's text is not compared), the header's @CO line, the argument errors, --test's 30
# lines, and the readings of DESIGN.md §10 (the .fai arithmetic on the three line shapes, an index that does not parse, a base index
# at l_seq, ansi_term's bytes).  After a stop the reference may lose its last block: only a prefix is asked for there.
def discard_tails_cases():
    global failures
    from pathlib import Path

    from tests import bam_discard_tails_model as tm
    words = ["discard", "tail", "artifacts"]

    def differs(what, detail=""):
        global failures
        failures += 1
        print(f"DIFFERENT: sam discard tail artifacts: {what} {detail}")

    def ref(argv, d, stdin=None):
        r = subprocess.run([args.ref_sam] + words + argv, cwd=d, input=stdin, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        try:
            out = b"".join(x for x, _ in tm.members(r.stdout)) if r.stdout else b""
        except Exception:
            out = None                                                  # (a stream the reference left unfinished)
        return r.returncode % 256, out, tm.mask_seconds(r.stderr)
    d = tempfile.mkdtemp(prefix="sk_pin_tails_")
    try:
        fasta, genome = tm.write_genome(Path(d))
        genome.path = "genome.fa"
        code, out, err = ref([], d)
        if b"sam discard tail artifacts" not in err:
            print("sam discard tail artifacts: this reference binary does not declare the command (src/sam_main.rs), cases not run")
            return
        if (code, err) != (255, tm.INVALID):
            differs("usage", f"rc={code} stderr={err[-300:]!r}")
        raw = tm.write(os.path.join(d, "in.bam"), list(tm.served_records()), text=tm.TEXT, refs=tm.REFS)
        for T in (1, 20, 33, 64, 300):
            for opt in ("--threshold=0", "--threshold=0.15", "--threshold=1", "--mismatches=3"):
                key, val = opt.split("=")
                exp = tm.model(raw, genome, T, float(val)) if key == "--threshold" else tm.model(raw, genome, T, 0.15, mismatches=int(val))
                code, out, err = ref(["--tail-length=%d" % T, opt, "genome.fa", "in.bam"], d)
                if (out, err, code) != exp[:3]:
                    differs("served records", f"T={T} {opt}: rc={code} stderr={err[-300:]!r}")
        for label, (before, stop, status, line) in sorted(tm.stop_cases().items()):
            sraw = tm.write(os.path.join(d, "stop.bam"), before + [stop] + before, text=tm.TEXT, refs=tm.REFS)
            exp = tm.model(sraw, genome)
            code, out, err = ref(["genome.fa", "stop.bam"], d)
            if code != status or (status == 255 and err != exp[1]) or (out is not None and not exp[0].startswith(out)):
                differs("stop: " + label, f"rc={code} stderr={err[-300:]!r}")
        odd = tm.record(b"odd", 0, 100, [(0, 7)], [1] * 7, 0)            # T = 8 over 7M of an odd l_seq: no base index reaches l_seq
        oraw = tm.write(os.path.join(d, "odd.bam"), [odd, tm.record(b"pad", 0, 100, [(0, 8)], [1] * 7, 0)], text=tm.TEXT, refs=tm.REFS)
        code, out, err = ref(["--tail-length=8", "genome.fa", "odd.bam"], d)
        if code != tm.model(oraw, genome, 8)[2]:
            print("known difference: a base index equal to an odd l_seq reads the pad nibble in the reference (DESIGN.md §10)")
        for argv, message in ((["--tail-length=x"], tm.TAIL_LENGTH_ERROR), (["--tail-length=0"], tm.TAIL_LENGTH_ERROR), (["--threshold=abc"], tm.THRESHOLD_PARSE_ERROR),
                              (["--mismatches=x"], tm.MISMATCHES_ERROR), (["--threshold=1.01"], tm.THRESHOLD_RANGE_ERROR)):
            code, out, err = ref(argv + ["genome.fa", "in.bam"], d)
            if (code, err) != (255, message):
                differs("argument error", f"{argv}: rc={code} stderr={err[-300:]!r}")
        with open(os.path.join(d, "bad.fa"), "wb") as f:
            f.write(tm.genome_files()[0])
        with open(os.path.join(d, "bad.fa.fai"), "wb") as f:
            f.write(b"chrA\t5000\t22\t60\n")
        code, out, err = ref(["bad.fa", "in.bam"], d)
        if (code, err[-len(tm.open_error("bad.fa")):]) != (255, tm.open_error("bad.fa")):
            differs("an index that does not parse", f"rc={code} stderr={err[-300:]!r}")
        r = subprocess.run([args.ref_sam] + words + ["--test"], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        lines = r.stderr.split(b"\n")
        if r.returncode != 0 or len(lines) != 32 or not all(ln.startswith(b"[\x1b[32mPASS\x1b[0m] ") for ln in lines[:30]):
            differs("--test", f"rc={r.returncode} stderr={r.stderr[-300:]!r}")
    finally:
        shutil.rmtree(d, ignore_errors=True)


discard_tails_cases()
print(f"{failures} differences")
sys.exit(1 if failures else 0)
