"""A plain-Python statement of `sam merge` (src/sam_merge.rs:58-103) over raw BAM bytes, on tests/bam_subsample_model.py's helpers: the
header check, the loop that takes the smallest current first record one at a time — among equal keys the lowest input, which is the one
thing this build fixes where the reference leaves it to its heap —, the suffix, and a generator of inputs the command serves."""
import random
import struct

from tests import bam_rewrite_model as rm
from tests.bam_subsample_model import EOF_BLOCK, members, out_header, records, write  # noqa: F401  (what the tests use)

TWO_ERROR = b"ERROR: At least two BAM files must be provided for concatenation.\n"
PANIC = b"thread 'main' panicked: assertion failed: new_qname.len() < 255\n"


def key(rec):
    """((u32) refID, pos as a signed 32-bit value): refID -1 sorts last, pos -1 before 0"""
    tid, pos = struct.unpack_from("<ii", rec, 4)
    return tid & 0xFFFFFFFF, pos


def key64(rec):
    """the same order in one unsigned 64-bit number, as the device sorts it"""
    tid, pos = key(rec)
    return tid << 32 | ((pos & 0xFFFFFFFF) ^ 0x80000000)


def placed(rec, tid, pos):
    """the record with another refID and pos (rm.record derives the mate's position from pos, which pos = 2^31 - 1 overflows)"""
    return rec[:4] + struct.pack("<ii", tid, pos) + rec[12:]


def sorted_by_key(recs):
    return sorted(recs, key=key)


def ref_names(raw):
    """target_names(): every reference's name, its final NUL dropped"""
    (l_text,) = struct.unpack_from("<i", raw, 4)
    o = 8 + l_text
    (n_ref,) = struct.unpack_from("<i", raw, o)
    o += 4
    names = []
    for _ in range(n_ref):
        (ln,) = struct.unpack_from("<i", raw, o)
        name = raw[o + 4:o + 4 + ln]
        names.append(name[:-1] if name.endswith(b"\0") else name)
        o += 4 + ln + 4
    return names


def sq_error(path_1, path_b):
    return b"ERROR: Input BAM files %s and %s have different SQ fields.\n" % (str(path_1).encode(), str(path_b).encode())


def with_suffix(rec, number):
    """the record with '.' and the decimal input number behind its name; raises rm.Stop(101) at a new name of more than 254 bytes"""
    lo = rec[12]
    new = rec[36:36 + lo - 1] + b".%d" % number
    if len(new) > 254:
        raise rm.Stop(101)
    body = rec[4:12] + bytes([len(new) + 1]) + rec[13:36] + new + b"\0" + rec[36 + lo:]
    return struct.pack("<i", len(body)) + body


def model(raws, suffix, paths=None):
    """(inflated stdout, stderr, status) of `sam merge [--suffix] paths...` over the inputs' raw BAM bytes"""
    paths = paths or ["%d.bam" % (i + 1) for i in range(len(raws))]
    if len(raws) < 2:
        return b"", TWO_ERROR, 255
    names = ref_names(raws[0])
    for b in range(1, len(raws)):
        if ref_names(raws[b]) != names:
            return b"", sq_error(paths[0], paths[b]), 255
    out = [out_header(raws[0])]
    its = [records(raw) for raw in raws]
    heads = [next(it, None) for it in its]
    while True:
        best = None
        for b, h in enumerate(heads):                                       # the smallest key, among equal keys the lowest input
            if h is not None and (best is None or key(h) < key(heads[best])):
                best = b
        if best is None:
            return b"".join(out), b"", 0
        rec = heads[best]
        heads[best] = next(its[best], None)
        if suffix:
            try:
                rec = with_suffix(rec, best + 1)
            except rm.Stop as s:
                return b"".join(out), PANIC, s.code
        out.append(rec)


# ---- inputs ----
def served_inputs(n_files, n_records, n_refs=3, shared=0.5, seed=1, unmapped_tail=True, names=None):
    """n_files lists of records, each sorted by the key; n_records per file (an int, or one per file); a share `shared` of every file's
    records carries a key that another file has too (1.0: every record of every file on one key; 0.0: no key in two files).  Names of 1 to
    `names` bytes (default 60), l_seq of every residue, aux data of several kinds; with unmapped_tail some records of every file with
    refID = -1 and pos = -1 at its end, which all share one key."""
    rnd = random.Random(seed)
    counts = [n_records] * n_files if isinstance(n_records, int) else list(n_records)
    aux = [b"", rm.aux_i(b"NM", 3), rm.aux_z(b"RX", b"ACGT") + rm.aux_a(b"XA", b"Q"), rm.aux_b(b"ZB", [1, 2, 3])]
    pool = [(rnd.randrange(n_refs), rnd.randrange(0, 1 << 20)) for _ in range(max(counts) // 3 + 1)]     # the keys files share
    files = []
    for f, n in enumerate(counts):
        keys = []
        for i in range(n):
            if shared >= 1.0:
                keys.append((0, 1000))
            elif rnd.random() < shared:
                keys.append(rnd.choice(pool))
            else:                                                           # this file's own: pos = a multiple of n_files plus f, above the pool's
                keys.append((rnd.randrange(n_refs), (1 << 21) + rnd.randrange(1 << 20) * n_files + f))
        n_tail = min(n, 1 + n // 20) if unmapped_tail and shared < 1.0 and (shared > 0.0 or f == 0) else 0
        keys = sorted(keys[:n - n_tail]) + [(-1, -1)] * n_tail
        recs = []
        for i, (tid, pos) in enumerate(keys):
            name = b"f%d:%d:" % (f, i) + rm._word(rnd, rnd.randrange(0, names or 60))
            name = name[:names] if names else name
            l_seq = rnd.choice([0, 1, 2, 3, 7, 36, 100, 151])
            recs.append(rm.record(name, l_seq, flag=rnd.choice([0, 0x10, 0x63, 0x93]) | (4 if tid < 0 else 0), tid=tid, pos=pos, aux=aux[(i + f) % len(aux)],
                                  seed=f * 100003 + i))
        files.append(recs)
    return files
