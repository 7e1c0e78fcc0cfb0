#!/usr/bin/env python3
"""`sam tags from qname`, `sam qname from tags`, `sam trim qnames` and `sam minimize` (--read-ids; --read-ids --tags; --read-ids --tags
--base-qualities) from a BAM FILE: the device path (sk_bam_file_rewrite, sk_bam_file_minimize) against the host reader
(SEQKIT_HOST_INFLATE=1), alternating: wall time and CPU-seconds of every run, stdout to a file on local disk and to /dev/null; the
inflated outputs of both paths are checked identical.

The file: paired records of 150 drawn bases and qualities whose names carry a "/1" or "/2" suffix and a " UMI:" field
("readN/1 UMI:ACGTACGT"); for `qname from tags` the output of `tags from qname` (names without the field, an RX tag).
usage: bam_rewrite_e2e.py [million records (20)] [runs per path (2)] [--lib-only: the library calls alone, e.g. under rocprofv3
--kernel-trace --stats] [--only=minimize: `trim qnames`, the minimize rows' yardstick, and the minimize rows] [--trim-sam=PATH: the
`trim qnames` row from another build's sam binary, e.g. the parent commit's]"""
import os
import resource
import struct
import subprocess
import sys
import tempfile
import time
import zlib
from hashlib import sha256

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from seqkit_amd import build  # noqa: E402

build.build_all()
SAM = os.path.join(build.BINDIR, "sam")
lib_only = "--lib-only" in sys.argv
only_minimize = "--only=minimize" in sys.argv
TRIM_SAM = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--trim-sam=")), SAM)
argv = [a for a in sys.argv[1:] if not a.startswith("--")]
millions = int(argv[0]) if len(argv) > 0 else 20
runs = int(argv[1]) if len(argv) > 1 else 2
PAIRS = 50_000
reps = max(1, millions * 1_000_000 // (2 * PAIRS))
rng = np.random.default_rng(5)
codes = np.array([1, 2, 4, 8], dtype=np.uint8)
d = tempfile.mkdtemp(prefix="sk_bamrw_", dir=os.environ.get("SK_E2E_DIR"))
bam, tagged, out = os.path.join(d, "in.bam"), os.path.join(d, "tagged.bam"), os.path.join(d, "out.bam")


def bgzf(data):
    c = zlib.compressobj(1, zlib.DEFLATED, -15)
    comp = c.compress(data) + c.flush()
    return struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, len(comp) + 25) + comp + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data))


unit = bytearray()
for i in range(PAIRS):
    umi = bytes(b"ACGT"[k] for k in rng.integers(0, 4, size=8))
    for mate in (0, 1):
        name = b"read%d/%d UMI:%s\0" % (i, mate + 1, umi)
        nib = codes[rng.integers(0, 4, size=150)]
        packed = ((nib[0::2] << 4) | nib[1::2]).astype(np.uint8).tobytes()
        q = rng.integers(2, 41, size=150, dtype=np.uint8).tobytes()
        body = struct.pack("<iiBBHHHiiii", 0, i, len(name), 60, 4680, 1, 1 | 2 | (64 if mate == 0 else 128), 150, 0, i, 170) + name + struct.pack("<I", 150 << 4) + packed + q
        unit += struct.pack("<i", len(body)) + body
unit = bytes(unit)
comp = b"".join(bgzf(unit[o:o + 0xff00]) for o in range(0, len(unit), 0xff00))   # (a record may straddle blocks: the walk takes it)
text = b"@HD\tVN:1.6\n@SQ\tSN:chr1\tLN:248956422\n"
head = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", 1) + struct.pack("<i", 5) + b"chr1\0" + struct.pack("<i", 248956422)
with open(bam, "wb") as f:
    f.write(bgzf(head))
    for _ in range(reps):
        f.write(comp)
    f.write(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))
n_rec = reps * 2 * PAIRS
print(f"# {n_rec / 1e6:.0f} M records, {os.path.getsize(bam) / 1e9:.2f} GB compressed, {len(unit) * reps / 1e9:.2f} GB inflated")

if lib_only:
    import seqkit_amd
    with seqkit_amd.Context(0) as ctx:
        for _ in range(2):
            t = time.perf_counter()
            handled, n, raw, info = ctx.bam_file_rewrite(bam, "tags from qname", 1, 0)
            tot = sum(len(w["bgzf"]) for w in ctx.bam_file_rewrite_windows())
            print(f"sk_bam_file_rewrite + windows: {time.perf_counter() - t:.3f} s, handled {handled}, {n} records, {raw / 1e9:.2f} GB -> {tot / 1e9:.2f} GB")
        for flags in ((True, False, False), (True, False, True), (True, True, True)):
            for _ in range(2):
                t = time.perf_counter()
                handled, n, raw, info = ctx.bam_file_minimize(bam, *flags)
                tot = sum(len(w["bgzf"]) for w in ctx.bam_file_rewrite_windows())
                print(f"sk_bam_file_minimize {flags} + windows: {time.perf_counter() - t:.3f} s, handled {handled}, {n} records, {raw / 1e9:.2f} GB -> {tot / 1e9:.2f} GB")
    sys.exit(0)


def inflate_digest(path):
    h, data, at = sha256(), open(path, "rb").read(), 0
    while at < len(data):
        (xlen,) = struct.unpack_from("<H", data, at + 10)
        (bsize,) = struct.unpack_from("<H", data, at + 16)
        h.update(zlib.decompress(data[at + 12 + xlen:at + bsize + 1 - 8], wbits=-15))
        at += bsize + 1
    return h.hexdigest()[:16]


def run(words, path, env, dest):
    r0 = resource.getrusage(resource.RUSAGE_CHILDREN)
    t = time.perf_counter()
    with open(dest, "wb") as o:
        p = subprocess.run([TRIM_SAM if words[0] == "trim" else SAM] + words + [path], stdout=o, stderr=subprocess.PIPE,
                           env=dict(os.environ, SK_BAMFILE_TRACE="1", **env))
    wall = time.perf_counter() - t
    r1 = resource.getrusage(resource.RUSAGE_CHILDREN)
    assert p.returncode == 0, p.stderr[-500:]
    who = ("sam " + " ".join(w for w in words if not w.startswith("--")) + ": ").encode()
    assert (who + (b"host reader" if env else b"device path")) in p.stderr, p.stderr[-500:]       # (a collision would say "host reader")
    return wall, (r1.ru_utime - r0.ru_utime) + (r1.ru_stime - r0.ru_stime)


ROWS = [(["tags", "from", "qname"], bam), (["qname", "from", "tags"], tagged), (["trim", "qnames"], bam),
        (["minimize", "--read-ids"], bam), (["minimize", "--read-ids", "--tags"], bam), (["minimize", "--read-ids", "--tags", "--base-qualities"], bam)]
if only_minimize:
    ROWS = ROWS[2:]
else:
    subprocess.run([SAM, "tags", "from", "qname", bam], stdout=open(tagged, "wb"), check=True)
if TRIM_SAM != SAM:
    print(f"# the trim qnames row: {TRIM_SAM}")
for words, path in ROWS:
    res = {}
    for dest in (out, "/dev/null"):
        for k in range(runs):
            for name, env in (("device", {}), ("host", {"SEQKIT_HOST_INFLATE": "1"})):
                wall, cpu = run(words, path, env, dest)
                res.setdefault((name, dest), []).append((wall, cpu))
                if dest == out and k == 0:
                    res[(name, "digest")] = inflate_digest(out)
    assert res[("device", "digest")] == res[("host", "digest")]
    for dest in (out, "/dev/null"):
        line = " | ".join(f"{name} " + ", ".join(f"{w:.2f} s / {c:.1f} CPU-s" for w, c in res[(name, dest)]) for name in ("device", "host"))
        print(f"sam {' '.join(words)} > {'file' if dest == out else '/dev/null'}: {line}  (inflated outputs identical: {res[('device', 'digest')]})")
