#!/usr/bin/env python3
"""`sam fragments`, `sam count`, `sam count --single-end --center`, `sam to interleaved fastq` and `sam to fastq <prefix>` from a BAM
FILE: the device path (sk_bam_file_columns / sk_bam_file_reads and the kernels behind them) against the host reader (SEQKIT_HOST_INFLATE=1), alternating, several runs each: wall time and CPU-seconds of
every run, outputs of both paths and of the oracle command line checked identical (the .gz files of `sam to fastq` decompressed).  Then sk_bam_file_columns' library-call time next
to sk_bam_file_reduce's on the same file in one process.

The fragments file is tools/bam_e2e.py's (100 k paired records, one in two kept, repeated); the count file is the same unit once per
reference, with tid = the repeat's index, so it is coordinate-sorted with positions restarting per reference; the BED file holds
about 20 k regions over those references.  usage: bam_cmd_e2e.py [million records (20)] [runs per path (3)] [--lib-only: the library
calls alone, e.g. under rocprofv3 --kernel-trace --stats] [--no-gz: without the `sam to fastq <prefix>` row] [--markdup: only the
`sam mark duplicates` rows, see below] [--markdup-file=PATH: only write that row's file to PATH, for a profiler run of the command] [--coverage: only the `sam coverage histogram` rows, see below] [--coverage-file=PATH: only
write that row's file to PATH; with --human the one under the human-sized header]
[--subsample: only the `sam subsample` rows, see below] [--yardstick-sam=PATH: with --subsample, another build's `sam` (the parent
commit's) whose `trim qnames` is the yardstick row instead of this build's] [--subsample-file=PATH: only write that row's file to
PATH, for a profiler run of the command] [--merge: only the `sam merge` rows, see below] [--merge-files=DIR: only write the undealt file
and the parts to DIR (in.bam, p2_0.bam .., p8_0.bam ..), for a profiler run of the command] [--pairing: only the `sam to` pairing rows,
see below] [--pairing-file=PATH: only write that row's file to PATH, for a profiler run of the command] [--on-target: only the `sam
statistics --on-target` rows, see below] [--on-target-files=DIR: only write that row's file and BED to DIR (in.bam, t.bed), for a profiler
run of the command] [--recalc-tlen: only the `sam recalculate tlen` rows, see below] [--use-file=PATH: with --recalc-tlen, the file
--markdup-file wrote to PATH instead of a new one; it is left there] [--concatenate: only the `sam concatenate` rows, see below]
[--concatenate-files=DIR: only write those rows' two files to DIR (a.bam, b.bam), for a profiler run of the command]
[--tails: only the `sam discard tail artifacts` rows, see below] [--tails-files=DIR: only write that row's file and the smaller genome
to DIR (in.bam, genome.fa, genome.fa.fai), for a profiler run of the command]

--tails: the subsample file with bases that match a generated genome: one chromosome per reference, every reference the same 50 400
bases that the reads lie on and then filler up to the genome's size; five reads in eight are 150M, one has an insertion and one a
deletion behind base 70, one has four mismatches in its left tail and fails at the defaults.  Two genomes, about 0.4 GB and about 3 GB
of FASTA in lines of 60 bases, so that the cost per GB of bringing the genome in separates from the cost per record.  Rows, all to
/dev/null: `sam subsample --seed=1 <file> 1.0` on the device path (--yardstick-sam: another build's, the parent commit's) — it writes
every record through the same windows —, `sam discard tail artifacts` on the device path with either genome and, twice, through the host
reader with the smaller one.  The ratios to the yardstick are printed run for run next to the spread (max - min) of the yardstick's
repeats, and the library's own line on the genome (bytes, milliseconds).  With --check the device path and the host reader also write a
file each, and the inflated outputs and stderr (the seconds masked) are compared.

--concatenate: the mark duplicates file cut in two: the first half of its repeats and the second, each position-sorted, under one
header.  Rows, all to /dev/null: `sam merge --suffix a b` on the device path (--yardstick-sam: another build's, the parent commit's) —
it writes the same records under the same names, and keys, sorts and gathers them besides —, `sam concatenate a b` on the device
path and, twice, through the host reader.  The ratio concatenate / merge --suffix is printed run for run and by the medians next to the
spread (max - min) of the merge repeats.  With --check the device path and the host reader also write a file each, and the inflated
outputs are compared with each other and with merge --suffix's (the halves do not interleave: the two commands write the same stream).

--recalc-tlen: the mark duplicates file (position-sorted; every record a candidate, the mates adjacent: every pair is found, nothing is
discarded, and every TLEN is rewritten).  Rows, all to /dev/null: `sam trim qnames` on the device path (--yardstick-sam: another
build's, the parent commit's) — it reads and writes the same bytes —, `sam recalculate tlen` on the device path and, twice, through the
host reader.  The ratio recalculate tlen / trim qnames is printed run for run next to the spread (max - min) of the trim qnames
repeats.  With --check the device path and the host reader also write a file each, and the inflated outputs and stderr are compared.

--on-target: the subsample file (position-sorted, 200 references) and a BED of 4 000 regions over its references, a fifth of them short
ones under a long one.  Rows, all to /dev/null: `sam count --single-end <file> <bed>` on the device path (--yardstick-sam: another
build's, the parent commit's) — it makes the same columns call (with mapq besides) and runs the heavier kernel: an order check, the
search, a walk over the regions and an atomic per hit —, `sam statistics --on-target=<bed>` on the device path and through the host
reader.  Wall and CPU-seconds of every run, and statistics / count run for run next to the spread (max - min) of the count repeats.
The stdout and stderr of both paths are compared on every run.

--pairing: the fragments file (name-sorted in effect: mates adjacent).  Rows: `sam to interleaved fastq` to /dev/null and, without
--no-gz, `sam to fastq <prefix>` to files, each with the mates paired on the device (SEQKIT_DEVICE_PAIRING=1), paired on the host over the device's
texts (SEQKIT_HOST_PAIRING=1) and, with --yardstick-sam, by another build's `sam` (the parent commit's), alternating.  Wall and CPU-seconds
of every run, each row's spread (max - min), and default / yardstick run for run.  The .gz files of the first run of every row are
compared decompressed.  To files the device pairing also deflates and frames the outputs there (sk_bam_file_pairs_gz); one more row, device
pairing with SEQKIT_GPU_DEFLATE=0, separates the pairing from the deflate.  Then sk_bam_file_pairs' and sk_bam_file_pairs_gz's library-call
times and their windows drained, next to sk_bam_file_reads'.

--merge: the subsample file, and its records dealt alternately (record j of a repeat to part j mod P) into P = 2 and P = 8 position-
sorted parts.  Mates share a position, so every key occurs in two parts: with ties by input the merge writes the undealt file's records
in their order.  Rows, all to /dev/null: `sam trim qnames` on the undealt file on the device path (--yardstick-sam: another build's, the
parent commit's) — it reads and writes the same bytes —, `sam merge` of the 2 and of the 8 parts on the device path and through the
host reader.  The ratios merge / trim qnames are printed run for run next to the spread of the trim qnames repeats.  With --check the
inflated output of every merge row on both paths is compared with trim qnames' on the undealt file.

--markdup: the count file (position-sorted, one reference per repeat) with duplicates: every fourth pair lies at the position and has
the fragment length of the pair before it, and the pairs of every second group of four carry an RX:Z UMI (a duplicate pair its
original's).  So half of the records are in groups of two and a quarter are marked; the other groups have one member.  Rows: `sam
mark duplicates` to /dev/null, device path against the host reader, and `sam trim qnames` to /dev/null on the same file (no name
has a space: every record passes unchanged through the same inflate, window, deflate and pack pipeline, without signatures, sort and
clusters).  With --check both paths also write a file each, and the inflated outputs and the stderr lines are compared.

--subsample: the same file without the duplicates (position-sorted, paired, mates adjacent; a name recurs once per reference).  Rows,
all to /dev/null: `sam subsample --seed=1 <file> 1.0` and `0.5` on the device path, `0.5` through the host reader, and `sam trim
qnames` on the device path — at fraction 1.0 the command writes what trim qnames writes (no name has a space), plus the id passes, the
keep pass and the compaction.  The ratio 1.0 / trim qnames is printed run for run next to the spread (max - min) of the trim qnames
repeats.  With --check the device path and the host reader also write a file each at 0.5, and the inflated outputs and the stderr
lines are compared.

--coverage: the subsample file (200 references of 2^28 positions: 53.7 G positions, of which the records cover 50 k per reference) and
the same records under a human-sized header: 25 references of 124 M positions, 3.1 G in all, record k's reference its repeat's index
mod 25 (no longer sorted: the command does not ask for order).  Rows per file, all to /dev/null: `sam statistics` on the device path
(--yardstick-sam: another build's, the parent commit's) — the same front half plus a reduction —, `sam coverage histogram` on the
device path and through the host reader.  The ratio coverage / statistics is printed run for run next to the spread of the statistics
repeats.  With --check the stdout of both paths is compared.

The `sam to interleaved fastq` row is also run with stdout to /dev/null (no oracle there: the row before checked the outputs), which
takes the writer's cost out of both paths."""
import os
import struct
import subprocess
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor
from hashlib import sha256

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from oracle import oracle as orc  # noqa: E402
from seqkit_amd import build  # noqa: E402

orc.build()
build.build_all()
SAM = os.path.join(build.BINDIR, "sam")
lib_only = "--lib-only" in sys.argv
no_gz = "--no-gz" in sys.argv
markdup = "--markdup" in sys.argv
markdup_check = "--check" in sys.argv
subsample = "--subsample" in sys.argv
yardstick_sam = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--yardstick-sam=")), None)
coverage = "--coverage" in sys.argv
human = "--human" in sys.argv
coverage_file = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--coverage-file=")), None)
subsample_file = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--subsample-file=")), None)
merge = "--merge" in sys.argv
pairing = "--pairing" in sys.argv
pairing_file = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--pairing-file=")), None)
on_target = "--on-target" in sys.argv
on_target_files = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--on-target-files=")), None)
recalc_tlen = "--recalc-tlen" in sys.argv
concatenate = "--concatenate" in sys.argv
concatenate_files = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--concatenate-files=")), None)
tails_files = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--tails-files=")), None)
tails = "--tails" in sys.argv or tails_files is not None
use_file = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--use-file=")), None)
merge_files = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--merge-files=")), None)
markdup_file = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--markdup-file=")), None)
argv = [a for a in sys.argv[1:] if not a.startswith("--")]
millions = int(argv[0]) if len(argv) > 0 else 20
runs = int(argv[1]) if len(argv) > 1 else 3
PAIRS = 50_000
reps = millions * 1_000_000 // (2 * PAIRS)
rng = np.random.default_rng(3)
codes = np.array([1, 2, 4, 8], dtype=np.uint8)
d = tempfile.mkdtemp(prefix="sk_bamcmd_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
bam, bed, out = os.path.join(d, "in.bam"), os.path.join(d, "r.bed"), os.path.join(d, "out.txt")


def bgzf(data, level=1):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    comp = c.compress(data) + c.flush()
    return struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, len(comp) + 25) + comp + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data))


unit = bytearray()
starts, ends = [], []
dup_mode = markdup or markdup_file is not None or recalc_tlen or concatenate or concatenate_files is not None
tl_prev, umi_prev = 0, b""
chrom = rng.integers(0, 4, size=PAIRS + 400).astype(np.uint8) if tails else None          # --tails: the bases the reads lie on (0 .. 3 = A C G T)
for i in range(PAIRS):
    tl = int(rng.lognormal(np.log(170), 0.35))
    pos, aux = i, b""
    if dup_mode:
        umi = bytes(b"ACGT"[k] for k in rng.integers(0, 4, size=8)) if (i & 4) == 0 else b""
        if i % 4 == 3:                                                      # a duplicate of the pair before it
            pos, tl, umi = i - 1, tl_prev, umi_prev
        tl_prev, umi_prev = tl, umi
        aux = b"RXZ" + umi + b"\0" if umi else b""
    for mate in (0, 1):
        name = b"read%d\0" % i
        nib = codes[rng.integers(0, 4, size=150)]
        cigar = struct.pack("<I", 150 << 4)
        if tails:
            kind = i % 8
            if kind == 5:                                                       # 70M 2I 78M
                nib = codes[np.concatenate([chrom[pos:pos + 70], rng.integers(0, 4, size=2).astype(np.uint8), chrom[pos + 70:pos + 148]])]
                cigar = struct.pack("<III", 70 << 4, (2 << 4) | 1, 78 << 4)
            elif kind == 6:                                                     # 70M 3D 80M
                nib = codes[np.concatenate([chrom[pos:pos + 70], chrom[pos + 73:pos + 153]])]
                cigar = struct.pack("<III", 70 << 4, (3 << 4) | 2, 80 << 4)
            else:
                nib = codes[chrom[pos:pos + 150]]
                if kind == 7:                                                   # four mismatches in the left tail
                    nib[2:18:4] = codes[(chrom[pos + 2:pos + 18:4] + 1) & 3]
        packed = ((nib[0::2] << 4) | nib[1::2]).astype(np.uint8).tobytes()
        q = rng.integers(2, 41, size=150, dtype=np.uint8).tobytes()
        flag = 1 | 2 | (64 | 32 if mate == 0 else 128 | 16)
        body = struct.pack("<iiBBHHHiiii", 0, pos, len(name), 60 if i % 7 else 10, 4680, len(cigar) // 4, flag, 150, 0, pos + (tl if mate == 0 else -tl),
                           tl if mate == 0 else -tl) + name + cigar + packed + q + aux
        starts.append(len(unit))
        unit += struct.pack("<i", len(body)) + body
        ends.append(len(unit))
unit = bytes(unit)


def blocks_of(u):
    # what htslib writes: a block is flushed rather than a record split
    out_, lo, prev = [], 0, 0
    for e in ends:
        if e - lo > 0xff00:
            out_.append(bgzf(u[lo:prev]))
            lo = prev
        prev = e
    out_.append(bgzf(u[lo:]))
    return b"".join(out_)


def header(n_ref, l_ref=1 << 28):
    text = b"@HD\tVN:1.6\tSO:coordinate\n"
    h = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", n_ref)
    for r in range(n_ref):
        nm = b"chr%d\0" % (r + 1)
        h += struct.pack("<i", len(nm)) + nm + struct.pack("<i", l_ref)
    return bgzf(h)


def with_tid(t):
    u = np.frombuffer(unit, dtype=np.uint8).copy()
    o = np.array(starts, dtype=np.int64)
    tb = np.frombuffer(struct.pack("<i", t), dtype=np.uint8)
    for k in range(4):
        u[o + 4 + k] = tb[k]
        u[o + 24 + k] = tb[k]
    return blocks_of(u.tobytes())


def timed(args, env=None, sink=None):
    """one run: (wall s, CPU s of the child, rc, sha256 of stdout, stderr); sink: where stdout goes instead (not hashed)"""
    e = dict(os.environ)
    e.pop("SEQKIT_HOST_INFLATE", None)
    if env:
        e.update(env)
    with open(sink or out, "wb") as fo:
        t0 = time.perf_counter()
        p = subprocess.Popen(args, stdout=fo, stderr=subprocess.PIPE, env=e)
        err = p.stderr.read()
        _, status, ru = os.wait4(p.pid, 0)
        dt = time.perf_counter() - t0
    p.returncode = os.waitstatus_to_exitcode(status)
    h = sha256(open(out, "rb").read()).hexdigest()[:16] if not sink else None
    return dt, ru.ru_utime + ru.ru_stime, p.returncode, h, err


def gz_digest(prefix):
    """sha256 of the decompressed .gz files that begin with prefix (sorted by name)"""
    h = sha256()
    for f in sorted(os.listdir(d)):
        if f.startswith(os.path.basename(prefix)) and f.endswith(".gz"):
            zc = subprocess.run(["gzip", "-dc", os.path.join(d, f)], stdout=subprocess.PIPE, check=True).stdout
            h.update(f.encode() + sha256(zc).digest())
            os.remove(os.path.join(d, f))
    return h.hexdigest()[:16]


def compare_to(label, args, prefix=None, sink=None):
    """compare() for `sam to`: with a prefix, the decompressed .gz files are the output (checked on the first run of each path); with
    a sink (/dev/null), the times alone"""
    rows = {"device": [], "host": []}
    seen = set()
    for k in range(runs):
        for path, env in (("device", None), ("host", {"SEQKIT_HOST_INFLATE": "1"})):
            dt, cpu, rc, h, err = timed([SAM] + args, env, sink)
            rows[path].append((dt, cpu))
            if sink:
                h = None
            elif prefix:
                h = gz_digest(prefix) if k == 0 else None
            if h is not None:
                seen.add((rc, h, err))
    if sink:
        dt = cpu = float("nan")
        seen.add((0, "not compared", b""))
    else:
        dt, cpu, rc, h, err = timed([orc.SAM_BIN] + args)
        seen.add((rc, gz_digest(prefix) if prefix else h, err))
    assert len(seen) == 1, f"{label}: outputs differ: {seen}"
    tr = subprocess.run([SAM] + args, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, env=dict(os.environ, SK_BAMFILE_TRACE="1")).stderr
    if prefix:
        gz_digest(prefix)
    served = [ln for ln in tr.decode(errors="replace").split("\n") if ln.startswith("sam ")]
    for path in ("device", "host"):
        w = [r[0] for r in rows[path]]
        c = [r[1] for r in rows[path]]
        print(f"{label:34s} {path:6s} wall {min(w):6.2f} s (median {float(np.median(w)):6.2f})  CPU {float(np.median(c)):6.2f} s   "
              + " ".join(f"{x:.2f}" for x in w), flush=True)
    print(f"{label:34s} oracle wall {dt:6.2f} s  CPU {cpu:6.2f} s; outputs identical (rc {rc}, output sha256 {next(iter(seen))[1]}); trace: {served}", flush=True)
    dev, host = float(np.median([r[0] for r in rows['device']])), float(np.median([r[0] for r in rows['host']]))
    print(f"{label:34s} device / host wall (medians) = {dev / host:.2f}", flush=True)


def compare(label, args):
    rows = {"device": [], "host": []}
    seen = set()
    for _ in range(runs):
        for path, env in (("device", None), ("host", {"SEQKIT_HOST_INFLATE": "1"})):
            dt, cpu, rc, h, err = timed([SAM] + args, env)
            rows[path].append((dt, cpu))
            seen.add((rc, h, err))
    dt, cpu, rc, h, err = timed([orc.SAM_BIN] + args)
    seen.add((rc, h, err))
    assert len(seen) == 1, f"{label}: outputs differ: {seen}"
    tr = subprocess.run([SAM] + args, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, env=dict(os.environ, SK_BAMFILE_TRACE="1")).stderr
    served = [ln for ln in tr.decode(errors="replace").split("\n") if ln.startswith("sam ")]
    for path in ("device", "host"):
        w = [r[0] for r in rows[path]]
        c = [r[1] for r in rows[path]]
        print(f"{label:34s} {path:6s} wall {min(w):6.2f} s (median {float(np.median(w)):6.2f})  CPU {float(np.median(c)):6.2f} s   "
              + " ".join(f"{x:.2f}" for x in w), flush=True)
    print(f"{label:34s} oracle wall {dt:6.2f} s  CPU {cpu:6.2f} s; outputs identical (rc {rc}, stdout sha256 {h}); trace: {served}", flush=True)
    dev, host = float(np.median([r[0] for r in rows['device']])), float(np.median([r[0] for r in rows['host']]))
    print(f"{label:34s} device / host wall (medians) = {dev / host:.2f}", flush=True)


n = reps * 2 * PAIRS


def pairing_rows():
    variants = [("device pairing", SAM, {"SEQKIT_DEVICE_PAIRING": "1"}), ("host pairing  ", SAM, {"SEQKIT_HOST_PAIRING": "1"})]
    if yardstick_sam:
        variants.append(("yardstick     ", yardstick_sam, None))
    modes = [("sam to interleaved fastq >/dev/null", ["to", "interleaved", "fastq", bam], None)]
    if not no_gz:
        modes.append(("sam to fastq <prefix>", ["to", "fastq", bam, os.path.join(d, "o")], os.path.join(d, "o")))
    for label, args, prefix in modes:
        rows, seen = {}, set()
        # to files, the device pairing deflates there too (sk_bam_file_pairs_gz): one more row separates the pairing from the deflate
        more = [("device pairing, SEQKIT_GPU_DEFLATE=0", SAM, {"SEQKIT_DEVICE_PAIRING": "1", "SEQKIT_GPU_DEFLATE": "0"})] if prefix else []
        for k in range(runs):
            for name, binary, env in variants + more:
                dt, cpu, rc, _, err = timed([binary] + args, env, sink=os.devnull)
                assert rc == 0, (label, name, rc, err[-400:])
                rows.setdefault(name, []).append((dt, cpu))
                if prefix and k == 0:
                    seen.add(gz_digest(prefix))
                elif prefix:                                                # (the later runs' files are only removed)
                    for f in os.listdir(d):
                        if f.startswith(os.path.basename(prefix)) and f.endswith(".gz"):
                            os.remove(os.path.join(d, f))
        assert len(seen) <= 1, f"{label}: outputs differ: {seen}"
        for name, r in rows.items():
            w = [x[0] for x in r]
            print(f"{label:36s} {name} wall median {float(np.median(w)):5.2f} s, max - min {max(w) - min(w):.2f} s, CPU median "
                  f"{float(np.median([x[1] for x in r])):5.2f} s   " + " ".join(f"{dt:.2f}/{cpu:.1f}" for dt, cpu in r), flush=True)
        if yardstick_sam:
            a, b = [x[0] for x in rows["device pairing"]], [x[0] for x in rows["yardstick     "]]
            print(f"{label:36s} device pairing / yardstick, run for run: " + " ".join(f"{x / y:.2f}x" for x, y in zip(a, b))
                  + f"; medians {float(np.median(a)) / float(np.median(b)):.2f}x; median difference {float(np.median(b)) - float(np.median(a)):+.2f} s "
                  f"against the yardstick's max - min {max(b) - min(b):.2f} s" + ("; decompressed outputs identical" if prefix else ""), flush=True)
            print(f"{label:36s} yardstick - device pairing, run for run: " + " ".join(f"{y - x:+.2f}" for x, y in zip(a, b)) + " s", flush=True)
    tr = subprocess.run([SAM, "to", "interleaved", "fastq", bam], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, env=dict(os.environ, SK_BAMFILE_TRACE="1")).stderr
    print("trace of the default: " + str([ln for ln in tr.decode(errors="replace").split("\n") if ln.startswith("sam ")]), flush=True)


def write_count_file(path, n_ref=None, l_ref=1 << 28):
    """n_ref: the header's references, repeat r's records on reference r mod n_ref (None: one reference per repeat)"""
    with open(path, "wb") as f:
        f.write(header(n_ref or reps, l_ref))
        with ThreadPoolExecutor(16) as ex:
            for blob in ex.map(with_tid, [r % (n_ref or reps) for r in range(reps)]):
                f.write(blob)
        f.write(bgzf(b""))


def inflated_digest(path):
    """sha256 of the BGZF file's inflated bytes"""
    p = subprocess.Popen(["gzip", "-dc", path], stdout=subprocess.PIPE)
    h = sha256()
    for chunk in iter(lambda: p.stdout.read(1 << 24), b""):
        h.update(chunk)
    assert p.wait() == 0
    return h.hexdigest()[:16]


def markdup_rows():
    t0 = time.perf_counter()
    write_count_file(bam)
    print(f"mark duplicates file: {n} BAM records on {reps} references, sorted, {os.path.getsize(bam) / 1e6:.0f} MB, written in {time.perf_counter() - t0:.1f} s; "
          f"1 pair in 4 duplicates the pair before it (half of the records in groups of two, the others alone), RX:Z on every second group of four pairs; "
          f"{runs} runs per path, alternating", flush=True)
    rows = {}
    for k in range(runs):
        for label, args, env in (("sam mark duplicates  device", ["mark", "duplicates", bam], None),
                                 ("sam mark duplicates  host  ", ["mark", "duplicates", bam], {"SEQKIT_HOST_INFLATE": "1"}),
                                 ("sam trim qnames      device", ["trim", "qnames", bam], None)):
            dt, cpu, rc, _, err = timed([SAM] + args, dict(env or {}, SK_BAMFILE_TRACE="1"), sink=os.devnull)
            served = [ln for ln in err.decode(errors="replace").split("\n") if ln.startswith("sam ")]
            assert rc == 0 and served and ("host reader" if env else "device path") in served[0], (label, rc, err[-400:])
            rows.setdefault(label, []).append((dt, cpu, [ln for ln in err.decode(errors="replace").split("\n") if "reads were marked" in ln]))
    for label, r in rows.items():
        print(f"{label} > /dev/null: " + ", ".join(f"{dt:.2f} s / {cpu:.1f} CPU-s" for dt, cpu, _ in r) + ("  " + r[0][2][0] if r[0][2] else ""), flush=True)
    md = [x[0] for x in rows["sam mark duplicates  device"]]
    tq = [x[0] for x in rows["sam trim qnames      device"]]
    print("mark duplicates / trim qnames, device wall, run for run: " + " ".join(f"{a / b:.2f}x" for a, b in zip(md, tq))
          + f"; medians {float(np.median(md)) / float(np.median(tq)):.2f}x", flush=True)
    if markdup_check:
        got = []
        for env in (None, {"SEQKIT_HOST_INFLATE": "1"}):
            dt, cpu, rc, _, err = timed([SAM, "mark", "duplicates", bam], env, sink=out)
            got.append((rc, inflated_digest(out), err))
        assert got[0] == got[1], got
        print(f"sam mark duplicates > file: inflated outputs and stderr identical on both paths ({got[0][1]})", flush=True)
        os.remove(out)
    os.remove(bam)
    os.rmdir(d)


def subsample_rows():
    t0 = time.perf_counter()
    write_count_file(bam)
    print(f"subsample file: {n} BAM records on {reps} references, sorted, paired, mates adjacent, {os.path.getsize(bam) / 1e6:.0f} MB, written in "
          f"{time.perf_counter() - t0:.1f} s; {runs} runs per row, alternating", flush=True)
    trim_sam = yardstick_sam or SAM
    trim_label = "sam trim qnames        device" + (" (yardstick build)" if yardstick_sam else "")
    rows = {}
    for k in range(runs):
        for label, cmd, env in ((trim_label, [trim_sam, "trim", "qnames", bam], None),
                                ("sam subsample 1.0      device", [SAM, "subsample", "--seed=1", bam, "1.0"], None),
                                ("sam subsample 0.5      device", [SAM, "subsample", "--seed=1", bam, "0.5"], None),
                                ("sam subsample 0.5      host  ", [SAM, "subsample", "--seed=1", bam, "0.5"], {"SEQKIT_HOST_INFLATE": "1"})):
            dt, cpu, rc, _, err = timed(cmd, dict(env or {}, SK_BAMFILE_TRACE="1"), sink=os.devnull)
            lines = err.decode(errors="replace").split("\n")
            served = [ln for ln in lines if ln.startswith("sam ")]
            assert rc == 0 and served and ("host reader" if env else "device path") in served[0], (label, rc, err[-400:])
            rows.setdefault(label, []).append((dt, cpu, [ln for ln in lines if ln.startswith("Kept reads")]))
    for label, r in rows.items():
        print(f"{label} > /dev/null: " + ", ".join(f"{dt:.2f} s / {cpu:.1f} CPU-s" for dt, cpu, _ in r) + ("  " + r[0][2][0] if r[0][2] else ""), flush=True)
    one = [x[0] for x in rows["sam subsample 1.0      device"]]
    tq = [x[0] for x in rows[trim_label]]
    print("subsample 1.0 / trim qnames, device wall, run for run: " + " ".join(f"{a / b:.2f}x" for a, b in zip(one, tq))
          + f"; medians {float(np.median(one)) / float(np.median(tq)):.2f}x; trim qnames max - min {max(tq) - min(tq):.2f} s = "
          f"{(max(tq) - min(tq)) / float(np.median(tq)):.2f} of its median", flush=True)
    if markdup_check:
        got = []
        for env in (None, {"SEQKIT_HOST_INFLATE": "1"}):
            dt, cpu, rc, _, err = timed([SAM, "subsample", "--seed=1", bam, "0.5"], env, sink=out)
            got.append((rc, inflated_digest(out), err))
        assert got[0] == got[1], got
        print(f"sam subsample --seed=1 0.5 > file: inflated outputs and stderr identical on both paths ({got[0][1]})", flush=True)
        os.remove(out)
    os.remove(bam)
    os.rmdir(d)


def recalc_tlen_rows():
    global bam
    t0 = time.perf_counter()
    if use_file:
        bam = use_file
    else:
        write_count_file(bam)
    print(f"recalculate tlen file: {n} BAM records on {reps} references, sorted, every record a candidate, mates adjacent, {os.path.getsize(bam) / 1e6:.0f} MB, "
          + ("as given" if use_file else f"written in {time.perf_counter() - t0:.1f} s") + f"; {runs} runs per device row, alternating, 2 through the host reader", flush=True)
    trim_sam = yardstick_sam or SAM
    trim_label = "sam trim qnames        device" + (" (yardstick build)" if yardstick_sam else "")
    rows = {}
    for k in range(runs):
        for label, cmd, env in ((trim_label, [trim_sam, "trim", "qnames", bam], None),
                                ("sam recalculate tlen   device", [SAM, "recalculate", "tlen", bam], None),
                                ("sam recalculate tlen   host  ", [SAM, "recalculate", "tlen", bam], {"SEQKIT_HOST_INFLATE": "1"})):
            if env and k >= 2:
                continue
            dt, cpu, rc, _, err = timed(cmd, dict(env or {}, SK_BAMFILE_TRACE="1"), sink=os.devnull)
            lines = err.decode(errors="replace").split("\n")
            served = [ln for ln in lines if ln.startswith("sam ")]
            assert rc == 0 and served and ("host reader" if env else "device path") in served[0], (label, rc, err[-400:])
            rows.setdefault(label, []).append((dt, cpu, [ln for ln in lines if ln.startswith("sk_bam_file_recalc_tlen:")]))
    for label, r in rows.items():
        w, c = [x[0] for x in r], [x[1] for x in r]
        print(f"{label} > /dev/null: " + ", ".join(f"{dt:.2f} s / {cpu:.1f} CPU-s" for dt, cpu, _ in r)
              + f"  (wall {min(w):.2f}-{max(w):.2f} s, CPU {min(c):.1f}-{max(c):.1f} s)", flush=True)
    for ln in rows["sam recalculate tlen   device"][-1][2]:
        print("  " + ln, flush=True)
    rt = [x[0] for x in rows["sam recalculate tlen   device"]]
    tq = [x[0] for x in rows[trim_label]]
    host = [x[0] for x in rows["sam recalculate tlen   host  "]]
    print("recalculate tlen / trim qnames, device wall, run for run: " + " ".join(f"{a / b:.2f}x" for a, b in zip(rt, tq))
          + f"; medians {float(np.median(rt)) / float(np.median(tq)):.2f}x; median difference {float(np.median(rt)) - float(np.median(tq)):+.2f} s against trim qnames' "
          f"max - min {max(tq) - min(tq):.2f} s = {(max(tq) - min(tq)) / float(np.median(tq)):.2f} of its median; device / host reader (medians) = "
          f"{float(np.median(rt)) / float(np.median(host)):.2f}", flush=True)
    if markdup_check:
        got = []
        for env in (None, {"SEQKIT_HOST_INFLATE": "1"}):
            dt, cpu, rc, _, err = timed([SAM, "recalculate", "tlen", bam], env, sink=out)
            got.append((rc, inflated_digest(out), err))
        assert got[0] == got[1], got
        print(f"sam recalculate tlen > file: inflated outputs and stderr identical on both paths ({got[0][1]})", flush=True)
        os.remove(out)
    if not use_file:
        os.remove(bam)
    os.rmdir(d)


def write_genome(path, total_bytes):
    """one chromosome per reference of the count file, every one the reads' bases and filler, in lines of 60 bases; path.fai beside it"""
    per = max(len(chrom) + 60, total_bytes // reps // 61 * 60) // 60 * 60
    grng = np.random.default_rng(11)
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)[np.concatenate([chrom, grng.integers(0, 4, size=per - len(chrom)).astype(np.uint8)])]
    body = np.concatenate([bases.reshape(-1, 60), np.full((per // 60, 1), 10, dtype=np.uint8)], axis=1).tobytes()
    at, fai = 0, []
    with open(path, "wb") as f:
        for r in range(reps):
            head = b">chr%d\n" % (r + 1)
            f.write(head)
            f.write(body)
            fai.append(b"chr%d\t%d\t%d\t60\t61\n" % (r + 1, per, at + len(head)))
            at += len(head) + len(body)
    with open(path + ".fai", "wb") as f:
        f.write(b"".join(fai))
    return at


def mask_seconds(err):
    return b"".join(b"Processing took N seconds.\n" if ln.startswith(b"Processing took ") else ln for ln in err.splitlines(True)
                    if not ln.startswith(b"sk_bam") and not ln.startswith(b"sam discard tail artifacts: "))


def tails_rows():
    t0 = time.perf_counter()
    write_count_file(bam)
    genomes = []
    for label, size in (("0.4 GB", 400_000_000), ("3 GB  ", 3_000_000_000)):
        g = os.path.join(d, "genome%d.fa" % len(genomes))
        genomes.append((label, g, write_genome(g, size)))
    print(f"tails file: {n} BAM records on {reps} references, sorted, paired, {os.path.getsize(bam) / 1e6:.0f} MB; genomes of "
          + " and ".join(f"{b / 1e6:.0f} MB" for _, _, b in genomes) + f" of FASTA, written in {time.perf_counter() - t0:.1f} s; {runs} runs per device row, "
          "alternating, 2 through the host reader", flush=True)
    yard_sam = yardstick_sam or SAM
    yard = "sam subsample 1.0              device" + (" (yardstick build)" if yardstick_sam else "")
    cmds = [(yard, [yard_sam, "subsample", "--seed=1", bam, "1.0"], None)]
    for label, g, _ in genomes:
        cmds.append((f"sam discard tail artifacts {label} device", [SAM, "discard", "tail", "artifacts", g, bam], None))
    cmds.append((f"sam discard tail artifacts {genomes[0][0]} host  ", [SAM, "discard", "tail", "artifacts", genomes[0][1], bam], {"SEQKIT_HOST_INFLATE": "1"}))
    rows = {}
    for k in range(runs):
        for label, cmd, env in cmds:
            if env and k >= 2:
                continue
            dt, cpu, rc, _, err = timed(cmd, dict(env or {}, SK_BAMFILE_TRACE="1"), sink=os.devnull)
            lines = err.decode(errors="replace").split("\n")
            served = [ln for ln in lines if ln.startswith("sam ")]
            assert rc == 0 and served and ("host reader" if env else "device path") in served[0], (label, rc, err[-400:])
            rows.setdefault(label, []).append((dt, cpu, [ln for ln in lines if "genome:" in ln or "[FAILED]" in ln]))
    for label, r in rows.items():
        w, c = [x[0] for x in r], [x[1] for x in r]
        print(f"{label} > /dev/null: " + ", ".join(f"{dt:.2f} s / {cpu:.1f} CPU-s" for dt, cpu, _ in r)
              + f"  (wall {min(w):.2f}-{max(w):.2f} s, CPU {min(c):.1f}-{max(c):.1f} s)", flush=True)
        for ln in r[-1][2]:
            print("  " + ln, flush=True)
    ys = [x[0] for x in rows[yard]]
    for label, _, _ in genomes:
        ts = [x[0] for x in rows[f"sam discard tail artifacts {label} device"]]
        print(f"discard tail artifacts ({label.strip()}) / subsample 1.0, device wall, run for run: " + " ".join(f"{a / b:.2f}x" for a, b in zip(ts, ys))
              + f"; medians {float(np.median(ts)) / float(np.median(ys)):.2f}x; median difference {float(np.median(ts)) - float(np.median(ys)):+.2f} s against the "
              f"yardstick's max - min {max(ys) - min(ys):.2f} s = {(max(ys) - min(ys)) / float(np.median(ys)):.2f} of its median", flush=True)
    if markdup_check:
        got = []
        for env in (None, {"SEQKIT_HOST_INFLATE": "1"}):
            dt, cpu, rc, _, err = timed([SAM, "discard", "tail", "artifacts", genomes[0][1], bam], env, sink=out)
            got.append((rc, inflated_digest(out), mask_seconds(err)))
        assert got[0] == got[1], got
        print(f"sam discard tail artifacts > file: inflated outputs and stderr (the seconds masked) identical on both paths ({got[0][1]})", flush=True)
        os.remove(out)
    for _, g, _ in genomes:
        os.remove(g)
        os.remove(g + ".fai")
    os.remove(bam)
    os.rmdir(d)


def write_half_files(dirname):
    """the mark duplicates file cut in two: the first half of its repeats in a.bam, the second in b.bam; the paths"""
    halves = [os.path.join(dirname, "a.bam"), os.path.join(dirname, "b.bam")]
    for path, tids in zip(halves, (range(0, reps // 2), range(reps // 2, reps))):
        with open(path, "wb") as f:
            f.write(header(reps))
            with ThreadPoolExecutor(16) as ex:
                for blob in ex.map(with_tid, tids):
                    f.write(blob)
            f.write(bgzf(b""))
    return halves


def concatenate_rows():
    t0 = time.perf_counter()
    halves = write_half_files(d)
    print(f"concatenate files: the mark duplicates file of {n} BAM records on {reps} references cut in two, each half sorted ("
          + ", ".join(f"{os.path.getsize(p) / 1e6:.0f}" for p in halves) + f" MB), written in {time.perf_counter() - t0:.1f} s; {runs} runs per device row, "
          "alternating, 2 through the host reader", flush=True)
    merge_sam = yardstick_sam or SAM
    merge_label = "sam merge --suffix  device" + (" (yardstick build)" if yardstick_sam else "")
    rows = {}
    for k in range(runs):
        for label, cmd, env in ((merge_label, [merge_sam, "merge", "--suffix"] + halves, None),
                                ("sam concatenate     device", [SAM, "concatenate"] + halves, None),
                                ("sam concatenate     host  ", [SAM, "concatenate"] + halves, {"SEQKIT_HOST_INFLATE": "1"})):
            if env and k >= 2:
                continue
            dt, cpu, rc, _, err = timed(cmd, dict(env or {}, SK_BAMFILE_TRACE="1"), sink=os.devnull)
            lines = err.decode(errors="replace").split("\n")
            served = [ln for ln in lines if ln.startswith("sam ")]
            assert rc == 0 and served and all(("host reader" if env else "device path") in ln for ln in served), (label, rc, err[-400:])
            rows.setdefault(label, []).append((dt, cpu, [ln for ln in lines if ln.startswith("sk_bam_file_concatenate:")]))
    for label, r in rows.items():
        w, c = [x[0] for x in r], [x[1] for x in r]
        print(f"{label} > /dev/null: " + ", ".join(f"{dt:.2f} s / {cpu:.1f} CPU-s" for dt, cpu, _ in r)
              + f"  (wall median {float(np.median(w)):.2f} s, {min(w):.2f}-{max(w):.2f} s, CPU {min(c):.1f}-{max(c):.1f} s)", flush=True)
    for ln in rows["sam concatenate     device"][-1][2]:
        print("  " + ln, flush=True)
    cc = [x[0] for x in rows["sam concatenate     device"]]
    mg = [x[0] for x in rows[merge_label]]
    host = [x[0] for x in rows["sam concatenate     host  "]]
    print("concatenate / merge --suffix, device wall, run for run: " + " ".join(f"{a / b:.2f}x" for a, b in zip(cc, mg))
          + f"; medians {float(np.median(cc)) / float(np.median(mg)):.2f}x; median difference {float(np.median(cc)) - float(np.median(mg)):+.2f} s against merge's "
          f"max - min {max(mg) - min(mg):.2f} s = {(max(mg) - min(mg)) / float(np.median(mg)):.2f} of its median; device / host reader (medians) = "
          f"{float(np.median(cc)) / float(np.median(host)):.2f}", flush=True)
    if markdup_check:
        got = []
        for cmd, env in (([merge_sam, "merge", "--suffix"] + halves, None), ([SAM, "concatenate"] + halves, None),
                         ([SAM, "concatenate"] + halves, {"SEQKIT_HOST_INFLATE": "1"})):
            dt, cpu, rc, _, err = timed(cmd, env, sink=out)
            got.append((rc, inflated_digest(out), err))
        assert got[0] == got[1] == got[2], got
        print(f"sam concatenate > file: inflated outputs identical on both paths and to merge --suffix's ({got[0][1]})", flush=True)
        os.remove(out)
    for p in halves:
        os.remove(p)
    os.rmdir(d)


def write_part_files(dirname, parts):
    """the count file's records dealt alternately into `parts` files: record j of every repeat goes to part j mod parts; the paths"""
    u = np.frombuffer(unit, dtype=np.uint8)
    paths = []
    for p in range(parts):
        idx = range(p, len(starts), parts)
        pu = np.concatenate([u[starts[j]:ends[j]] for j in idx])
        lens = np.array([ends[j] - starts[j] for j in idx], dtype=np.int64)
        pe = np.cumsum(lens)
        ps = pe - lens

        def blob(t, pu=pu, ps=ps, pe=pe):
            v = pu.copy()
            tb = np.frombuffer(struct.pack("<i", t), dtype=np.uint8)
            for k in range(4):
                v[ps + 4 + k] = tb[k]
                v[ps + 24 + k] = tb[k]
            raw, out_, lo, prev = v.tobytes(), [], 0, 0
            for e in pe:                                                     # (blocks_of's rule: a block is flushed rather than a record split)
                if e - lo > 0xff00:
                    out_.append(bgzf(raw[lo:prev]))
                    lo = prev
                prev = int(e)
            out_.append(bgzf(raw[lo:]))
            return b"".join(out_)
        path = os.path.join(dirname, f"p{parts}_{p}.bam")
        with open(path, "wb") as f:
            f.write(header(reps))
            with ThreadPoolExecutor(16) as ex:
                for b in ex.map(blob, range(reps)):
                    f.write(b)
            f.write(bgzf(b""))
        paths.append(path)
    return paths


def merge_rows():
    t0 = time.perf_counter()
    write_count_file(bam)
    parts = {P: write_part_files(d, P) for P in (2, 8)}
    print(f"merge files: {n} BAM records on {reps} references, sorted, {os.path.getsize(bam) / 1e6:.0f} MB, and dealt alternately into 2 parts ("
          + ", ".join(f"{os.path.getsize(p) / 1e6:.0f}" for p in parts[2]) + " MB) and 8 parts (" + ", ".join(f"{os.path.getsize(p) / 1e6:.0f}" for p in parts[8])
          + f" MB), written in {time.perf_counter() - t0:.1f} s; {runs} runs per row, alternating", flush=True)
    trim_sam = yardstick_sam or SAM
    trim_label = "sam trim qnames   device" + (" (yardstick build)" if yardstick_sam else "")
    rows = {}
    for k in range(runs):
        for label, cmd, env in ((trim_label, [trim_sam, "trim", "qnames", bam], None),
                                ("sam merge 2      device", [SAM, "merge"] + parts[2], None),
                                ("sam merge 2      host  ", [SAM, "merge"] + parts[2], {"SEQKIT_HOST_INFLATE": "1"}),
                                ("sam merge 8      device", [SAM, "merge"] + parts[8], None),
                                ("sam merge 8      host  ", [SAM, "merge"] + parts[8], {"SEQKIT_HOST_INFLATE": "1"})):
            dt, cpu, rc, _, err = timed(cmd, dict(env or {}, SK_BAMFILE_TRACE="1"), sink=os.devnull)
            lines = err.decode(errors="replace").split("\n")
            served = [ln for ln in lines if ln.startswith("sam ")]
            assert rc == 0 and served and ("host reader" if env else "device path") in served[0], (label, rc, err[-400:])
            rows.setdefault(label, []).append((dt, cpu, [ln for ln in lines if ln.startswith("sk_bam_file_merge:")]))
    for label, r in rows.items():
        print(f"{label} > /dev/null: " + ", ".join(f"{dt:.2f} s / {cpu:.1f} CPU-s" for dt, cpu, _ in r), flush=True)
    tq = [x[0] for x in rows[trim_label]]
    for P in (2, 8):
        dev, host = [x[0] for x in rows[f"sam merge {P}      device"]], [x[0] for x in rows[f"sam merge {P}      host  "]]
        for ln in rows[f"sam merge {P}      device"][-1][2]:
            print("  " + ln, flush=True)
        print(f"merge {P} / trim qnames, device wall, run for run: " + " ".join(f"{a / b:.2f}x" for a, b in zip(dev, tq))
              + f"; medians {float(np.median(dev)) / float(np.median(tq)):.2f}x; trim qnames max - min {max(tq) - min(tq):.2f} s = "
              f"{(max(tq) - min(tq)) / float(np.median(tq)):.2f} of its median; device / host reader (medians) = {float(np.median(dev)) / float(np.median(host)):.2f}", flush=True)
    if markdup_check:
        dt, cpu, rc, _, err = timed([trim_sam, "trim", "qnames", bam], None, sink=out)
        want = (rc, inflated_digest(out), err)
        for P in (2, 8):
            for env in (None, {"SEQKIT_HOST_INFLATE": "1"}):
                dt, cpu, rc, _, err = timed([SAM, "merge"] + parts[P], env, sink=out)
                assert (rc, inflated_digest(out), err) == want, (P, env, rc, err[-400:])
        print(f"sam merge > file: inflated outputs of 2 and 8 parts on both paths identical to trim qnames' on the undealt file ({want[1]})", flush=True)
        os.remove(out)
    os.remove(bam)
    for ps in parts.values():
        for p in ps:
            os.remove(p)
    os.rmdir(d)


def write_target_bed(path, regions=4000):
    """regions over the count file's references (positions 0 .. PAIRS + a fragment): four in five 50-3 000 long anywhere, one in five a
    short one under a long one that begins before it"""
    brng = np.random.default_rng(7)
    with open(path, "w") as f:
        f.write("# targets\n")
        for k in range(regions // 5):
            c = int(brng.integers(1, reps + 1))
            for _ in range(3):
                s0 = int(brng.integers(0, PAIRS))
                f.write(f"chr{c}\t{s0}\t{s0 + int(brng.integers(50, 3000))}\n")
            s0 = int(brng.integers(0, PAIRS - 6000))
            f.write(f"chr{c}\t{s0}\t{s0 + 6000}\n")
            s1 = s0 + int(brng.integers(100, 5000))
            f.write(f"chr{c}\t{s1}\t{s1 + 20}\n")


def on_target_rows():
    t0 = time.perf_counter()
    write_count_file(bam)
    write_target_bed(bed)
    print(f"on-target file: {n} BAM records on {reps} references, sorted, {os.path.getsize(bam) / 1e6:.0f} MB, written in {time.perf_counter() - t0:.1f} s; "
          f"BED of {sum(1 for ln in open(bed) if not ln.startswith('#'))} regions; {runs} runs per row, alternating", flush=True)
    count_sam = yardstick_sam or SAM
    count_label = "sam count --single-end          device" + (" (yardstick build)" if yardstick_sam else "")
    rows, seen = {}, set()
    for k in range(runs):
        for label, cmd, env in ((count_label, [count_sam, "count", "--single-end", bam, bed], None),
                                ("sam statistics --on-target      device", [SAM, "statistics", f"--on-target={bed}", bam], None),
                                ("sam statistics --on-target      host  ", [SAM, "statistics", f"--on-target={bed}", bam], {"SEQKIT_HOST_INFLATE": "1"})):
            stat = label.startswith("sam statistics")
            dt, cpu, rc, h, err = timed(cmd, dict(env or {}, SK_BAMFILE_TRACE="1"), sink=None if stat else os.devnull)
            lines = err.decode(errors="replace").split("\n")
            served = [ln for ln in lines if ln.startswith("sam ")]
            assert rc == 0 and len(served) == 1 and ("host reader" if env else "device path") in served[0], (label, rc, err[-400:])
            if stat:
                seen.add((rc, h, "\n".join(ln for ln in lines if not ln.startswith(("sam ", "sk_bam_file_")))))     # (without the trace's own lines)
            rows.setdefault(label, []).append((dt, cpu))
            if stat and not env:
                stages = [ln for ln in lines if ln.startswith("sk_bam_file_columns:")]
    assert len(seen) == 1, f"sam statistics --on-target: outputs differ: {seen}"
    for label, r in rows.items():
        w = [x[0] for x in r]
        print(f"{label} : " + ", ".join(f"{dt:.2f} s / {cpu:.1f} CPU-s" for dt, cpu in r) + f"  (median {float(np.median(w)):.2f} s, max - min {max(w) - min(w):.2f} s)", flush=True)
    print("sam statistics --on-target: stdout and stderr identical on both paths in every run (stdout sha256 " + next(iter(seen))[1] + "): "
          + open(out).read().replace("\n", " | "), flush=True)
    for ln in stages:
        print("  " + ln, flush=True)
    st = [x[0] for x in rows["sam statistics --on-target      device"]]
    ct = [x[0] for x in rows[count_label]]
    host = [x[0] for x in rows["sam statistics --on-target      host  "]]
    print("statistics --on-target / count --single-end, device wall, run for run: " + " ".join(f"{a / b:.2f}x" for a, b in zip(st, ct))
          + f"; medians {float(np.median(st)) / float(np.median(ct)):.2f}x; median difference {float(np.median(st)) - float(np.median(ct)):+.2f} s against count's max - min "
          f"{max(ct) - min(ct):.2f} s; device / host reader (medians) = {float(np.median(st)) / float(np.median(host)):.2f}", flush=True)
    for f_ in (bam, bed, out):
        os.remove(f_)
    os.rmdir(d)


HUMAN_REFS, HUMAN_LEN = 25, 124_000_000


def coverage_rows():
    stat_sam = yardstick_sam or SAM
    stat_label = "sam statistics          device" + (" (yardstick build)" if yardstick_sam else "")
    for what, n_ref, l_ref in ((f"{reps} references of 2^28 positions, sorted", None, 1 << 28),
                               (f"{HUMAN_REFS} references of {HUMAN_LEN} positions ({HUMAN_REFS * HUMAN_LEN / 1e9:.1f} G), repeat r on reference r mod {HUMAN_REFS}", HUMAN_REFS, HUMAN_LEN)):
        t0 = time.perf_counter()
        write_count_file(bam, n_ref, l_ref)
        print(f"coverage file: {n} BAM records on {what}, {os.path.getsize(bam) / 1e6:.0f} MB, written in {time.perf_counter() - t0:.1f} s; "
              f"{runs} runs per row, alternating", flush=True)
        rows = {}
        for k in range(runs):
            for label, cmd, env in ((stat_label, [stat_sam, "statistics", bam], None),
                                    ("sam coverage histogram  device", [SAM, "coverage", "histogram", bam], None),
                                    ("sam coverage histogram  host  ", [SAM, "coverage", "histogram", bam], {"SEQKIT_HOST_INFLATE": "1"})):
                dt, cpu, rc, _, err = timed(cmd, dict(env or {}, SK_BAMFILE_TRACE="1"), sink=os.devnull)
                lines = err.decode(errors="replace").split("\n")
                served = [ln for ln in lines if ln.startswith("sam ")]
                assert rc == 0 and served and (("host reader" if env else "device path") in served[-1] or "sk_bam_file_reduce" in served[-1]), (label, rc, err[-400:])
                rows.setdefault(label, []).append((dt, cpu, [ln for ln in lines if ln.startswith("sk_bam_file_coverage:")]))
        for label, r in rows.items():
            print(f"{label} > /dev/null: " + ", ".join(f"{dt:.2f} s / {cpu:.1f} CPU-s" for dt, cpu, _ in r), flush=True)
        for ln in rows["sam coverage histogram  device"][-1][2]:
            print("  " + ln, flush=True)
        cov = [x[0] for x in rows["sam coverage histogram  device"]]
        st = [x[0] for x in rows[stat_label]]
        host = [x[0] for x in rows["sam coverage histogram  host  "]]
        print("coverage histogram / statistics, device wall, run for run: " + " ".join(f"{a / b:.2f}x" for a, b in zip(cov, st))
              + f"; medians {float(np.median(cov)) / float(np.median(st)):.2f}x; statistics max - min {max(st) - min(st):.2f} s = "
              f"{(max(st) - min(st)) / float(np.median(st)):.2f} of its median; device / host reader (medians) = {float(np.median(cov)) / float(np.median(host)):.2f}", flush=True)
        if markdup_check:
            got = []
            for env in (None, {"SEQKIT_HOST_INFLATE": "1"}):
                dt, cpu, rc, h, err = timed([SAM, "coverage", "histogram", bam], env)
                got.append((rc, h, err))
            assert got[0] == got[1], got
            print(f"sam coverage histogram > file: stdout identical on both paths ({got[0][1]}); first lines: "
                  + " ".join(open(out).read().split("\n")[:3]).replace("\t", ":"), flush=True)
            os.remove(out)
        os.remove(bam)
    os.rmdir(d)


if merge_files is not None:
    write_count_file(os.path.join(merge_files, "in.bam"))
    for P in (2, 8):
        write_part_files(merge_files, P)
    print(f"wrote {merge_files}/in.bam and its 2 and 8 parts: {n} records", flush=True)
    os.rmdir(d)
    sys.exit(0)
if merge:
    merge_rows()
    sys.exit(0)
if on_target_files is not None:
    write_count_file(os.path.join(on_target_files, "in.bam"))
    write_target_bed(os.path.join(on_target_files, "t.bed"))
    print(f"wrote {on_target_files}/in.bam ({n} records) and t.bed", flush=True)
    os.rmdir(d)
    sys.exit(0)
if on_target:
    on_target_rows()
    sys.exit(0)
if coverage_file is not None:
    write_count_file(coverage_file, HUMAN_REFS if human else None, HUMAN_LEN if human else 1 << 28)
    print(f"wrote {coverage_file}: {n} records, {os.path.getsize(coverage_file) / 1e6:.0f} MB", flush=True)
    os.rmdir(d)
    sys.exit(0)
if coverage:
    coverage_rows()
    sys.exit(0)
if markdup_file is not None or subsample_file is not None:
    markdup_file = markdup_file or subsample_file
    write_count_file(markdup_file)
    print(f"wrote {markdup_file}: {n} records, {os.path.getsize(markdup_file) / 1e6:.0f} MB", flush=True)
    os.rmdir(d)
    sys.exit(0)
if markdup:
    markdup_rows()
    sys.exit(0)
if recalc_tlen:
    recalc_tlen_rows()
    sys.exit(0)
if tails_files is not None:
    write_count_file(os.path.join(tails_files, "in.bam"))
    write_genome(os.path.join(tails_files, "genome.fa"), 400_000_000)
    print(f"wrote {tails_files}/in.bam ({n} records), genome.fa and genome.fa.fai", flush=True)
    os.rmdir(d)
    sys.exit(0)
if tails:
    tails_rows()
    sys.exit(0)
if concatenate_files is not None:
    write_half_files(concatenate_files)
    print(f"wrote {concatenate_files}/a.bam and b.bam: {n} records", flush=True)
    os.rmdir(d)
    sys.exit(0)
if concatenate:
    concatenate_rows()
    sys.exit(0)
if subsample:
    subsample_rows()
    sys.exit(0)
t0 = time.perf_counter()
with open(bam, "wb") as f:
    f.write(header(1))
    body = blocks_of(unit)
    for _ in range(reps):
        f.write(body)
    f.write(bgzf(b""))
print(f"fragments file: {n} BAM records, {os.path.getsize(bam) / 1e6:.0f} MB, written in {time.perf_counter() - t0:.1f} s; {runs} runs per path", flush=True)
if pairing_file is not None:
    os.replace(bam, pairing_file)
    print(f"wrote {pairing_file}", flush=True)
    os.rmdir(d)
    sys.exit(0)
if pairing and not lib_only:
    pairing_rows()
if not lib_only and not pairing:
    compare("sam fragments", ["fragments", bam])
    compare_to("sam to interleaved fastq", ["to", "interleaved", "fastq", bam])
    compare_to("sam to interleaved fastq >/dev/null", ["to", "interleaved", "fastq", bam], sink=os.devnull)
    if not no_gz:
        compare_to("sam to fastq <prefix>", ["to", "fastq", bam, os.path.join(d, "o")], prefix=os.path.join(d, "o"))

# the library calls on the same file, one process
import seqkit_amd  # noqa: E402
from seqkit_amd import capi  # noqa: E402
with seqkit_amd.Context(0) as ctx:
    tc, tr_ = [], []
    for _ in range(runs + 1):
        t0 = time.perf_counter()
        h, _, _, _, info = ctx.bam_file_reduce(bam, 5000)
        tr_.append(time.perf_counter() - t0)
        assert h
        t0 = time.perf_counter()
        h, dev, nn, _, info = ctx.bam_file_columns_dev(bam, capi.SK_COL_ALL)
        tc.append(time.perf_counter() - t0)
        assert h and nn == n
    tr_, tc = tr_[1:], tc[1:]                                               # (the first pair: the buffers are taken)
    print(f"library call, {n} records: sk_bam_file_reduce {1e3 * min(tr_):.0f} ms (median {1e3 * float(np.median(tr_)):.0f}), "
          f"sk_bam_file_columns (all 8 fields) {1e3 * min(tc):.0f} ms (median {1e3 * float(np.median(tc)):.0f}): "
          f"columns / reduce = {float(np.median(tc)) / float(np.median(tr_)):.2f}", flush=True)
    # sk_bam_file_reads (fastq) and its windows, the text left in the page-locked buffers: the device side of `sam to fastq`
    t0 = time.perf_counter()
    h, kept, tb, _ = ctx.bam_file_reads(bam, "fastq")
    t1 = time.perf_counter()
    w = capi._ReadsWindow()
    nw = 0
    while True:
        ctx._check(ctx._lib.sk_bam_file_reads_next(ctx._h, capi.C.byref(w)), "sk_bam_file_reads_next")
        if w.n == 0:
            break
        nw += 1
    t2 = time.perf_counter()
    assert h
    print(f"library call, {n} records: sk_bam_file_reads (fastq) {1e3 * (t1 - t0):.0f} ms, {kept} kept, {tb / 1e9:.2f} GB of text; "
          f"{nw} windows drained in {1e3 * (t2 - t1):.0f} ms", flush=True)
    # sk_bam_file_pairs (fastq, interleaved and not) and its windows: the device side of `sam to fastq` with the mates paired there
    for inter in (True, False):
        t0 = time.perf_counter()
        h, counts, _ = ctx.bam_file_pairs(bam, "fastq", 10, inter)
        t1 = time.perf_counter()
        pw = capi._PairsWindow()
        nw = 0
        while True:
            ctx._check(ctx._lib.sk_bam_file_pairs_next(ctx._h, capi.C.byref(pw)), "sk_bam_file_pairs_next")
            if pw.n == 0:
                break
            nw += 1
        t2 = time.perf_counter()
        assert h
        print(f"library call, {n} records: sk_bam_file_pairs (fastq{', interleaved' if inter else ''}) {1e3 * (t1 - t0):.0f} ms, {counts[0]} pairs, "
              f"{sum(counts[5:]) / 1e9:.2f} GB of text; {nw} windows drained in {1e3 * (t2 - t1):.0f} ms", flush=True)
    # sk_bam_file_pairs_gz (fastq, level 1) and its windows: the three streams deflated and framed on the device, the members copied back
    t0 = time.perf_counter()
    h, counts, _ = ctx.bam_file_pairs_gz(bam, "fastq", 10, 1)
    t1 = time.perf_counter()
    gw = capi._PairsGzWindow()
    nw = packed = 0
    while True:
        ctx._check(ctx._lib.sk_bam_file_pairs_gz_next(ctx._h, capi.C.byref(gw)), "sk_bam_file_pairs_gz_next")
        if gw.n == 0:
            break
        nw += 1
        packed += gw.bytes
    t2 = time.perf_counter()
    assert h
    print(f"library call, {n} records: sk_bam_file_pairs_gz (fastq, level 1) {1e3 * (t1 - t0):.0f} ms, {counts[0]} pairs, "
          f"{sum(counts[5:]) / 1e9:.2f} GB of text in {packed / 1e9:.2f} GB of members; {nw} windows drained in {1e3 * (t2 - t1):.0f} ms", flush=True)
os.remove(bam)
if lib_only or pairing:
    os.rmdir(d)
    sys.exit(0)

t0 = time.perf_counter()
write_count_file(bam)
brng = np.random.default_rng(5)
with open(bed, "w") as f:
    for k in range(20_000):
        s = int(brng.integers(0, PAIRS))
        f.write(f"chr{int(brng.integers(1, reps + 1))}\t{s}\t{s + int(brng.integers(50, 3000))}\n")
print(f"count file: {n} BAM records on {reps} references, sorted, {os.path.getsize(bam) / 1e6:.0f} MB, written in {time.perf_counter() - t0:.1f} s; "
      f"20000 BED regions", flush=True)
compare("sam count", ["count", bam, bed])
compare("sam count --single-end --center", ["count", "--single-end", "--center", bam, bed])
os.remove(bam)
os.remove(bed)
if os.path.exists(out):
    os.remove(out)
os.rmdir(d)
