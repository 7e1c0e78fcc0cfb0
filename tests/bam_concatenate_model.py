"""A plain-Python statement of `sam concatenate` (src/sam_concatenate.rs:21-50) over raw BAM bytes, on the helpers of
tests/bam_merge_model.py and tests/bam_subsample_model.py: the first input's header, then every input's records in command-line and
file order with '.' and the input's number behind the name, the stop at a new name of more than 254 bytes, and a generator of inputs
that `sam merge` would not take: unsorted, with reference lists that differ."""
import random

from tests import bam_rewrite_model as rm
from tests.bam_merge_model import PANIC, TWO_ERROR, with_suffix  # noqa: F401  (what the tests use)
from tests.bam_subsample_model import EOF_BLOCK, members, out_header, records, write  # noqa: F401

USAGE = (b"\nUsage:\n  sam concatenate [options] <bam_files>...\n\nOptions:\n  --uncompressed    Output in uncompressed BAM format\n\n"
         b"Concatenates two or more BAM files together, ensuring that read\nidentifiers do not clash. Currently we simply add a '.1' suffix to all\n"
         b"read identifiers found in the first BAM file, a '.2' suffix to all all\nread identifiers found in the second BAM file, and so forth.\n")
INVALID = b"ERROR: Invalid arguments.\n" + USAGE + b"\n"


def open_error(path):
    return b"ERROR: Cannot open BAM file '%s'\n" % str(path).encode()


def model(raws, paths=None):
    """(inflated stdout, stderr, status) of `sam concatenate paths...` over the inputs' raw BAM bytes; an entry of raws that is None is
    a file that cannot be opened: the command ends there in the reader's words, the inputs before it written"""
    paths = paths or ["%d.bam" % (i + 1) for i in range(len(raws))]
    if len(raws) < 2:
        return b"", TWO_ERROR, 255
    if raws[0] is None:
        return b"", open_error(paths[0]), 255
    out = [out_header(raws[0])]                                             # the first input's; the others' are read and skipped, not compared
    for b, raw in enumerate(raws):
        if raw is None:
            return b"".join(out), open_error(paths[b]), 255
        for rec in records(raw):
            try:
                out.append(with_suffix(rec, b + 1))
            except rm.Stop as s:
                return b"".join(out), PANIC, s.code
    return b"".join(out), b"", 0


def strip_suffix(rec, number):
    """the record without the '.number' behind its name, l_read_name and block_size restored; None: its name does not end so"""
    lo = rec[12]
    name, sfx = rec[36:36 + lo - 1], b".%d" % number
    if not name.endswith(sfx) or rec[36 + lo - 1] != 0:
        return None
    body = rec[4:12] + bytes([lo - len(sfx)]) + rec[13:36] + name[:-len(sfx)] + b"\0" + rec[36 + lo:]
    return len(body).to_bytes(4, "little") + body


# ---- inputs ----
REF_LISTS = [rm.REFS, [(b"chrM", 16569)], rm.REFS[:2] + [(b"chrX", 156040895), (b"chrY", 57227415)], [(b"only", 5000)]]


def refs_of(f):
    """file f's reference list: they differ from file to file"""
    return REF_LISTS[f % len(REF_LISTS)]


def served_inputs(n_files, n_records, seed=1, names=None):
    """n_files lists of records NOT sorted by position, refIDs within file f's own reference list (refs_of(f)) and -1; n_records per file
    (an int, or one per file: 0 and 1 among them as the caller likes).  Names of 1 byte up to `names` bytes (default 60), l_seq of every
    residue, aux data of several kinds, secondary and supplementary records."""
    rnd = random.Random(seed)
    counts = [n_records] * n_files if isinstance(n_records, int) else list(n_records)
    aux = [b"", rm.aux_i(b"NM", 3), rm.aux_z(b"RX", b"ACGT") + rm.aux_a(b"XA", b"Q"), rm.aux_b(b"ZB", [1, 2, 3])]
    files = []
    for f, n in enumerate(counts):
        n_refs = len(refs_of(f))
        recs = []
        for i in range(n):
            tid = rnd.randrange(-1, n_refs) if n_refs else -1
            name = rm._word(rnd, 1 + rnd.randrange(0, names or 60)) if i % 7 else bytes([65 + (i // 7) % 26])
            l_seq = rnd.choice([0, 1, 2, 3, 7, 36, 100, 151])
            recs.append(rm.record(name, l_seq, flag=rnd.choice([0, 0x10, 0x63, 0x93, 0x100, 0x800]) | (4 if tid < 0 else 0), tid=tid,
                                  pos=rnd.randrange(0, 1 << 20) if tid >= 0 else -1, aux=aux[(i + f) % len(aux)], seed=f * 100003 + i))
        files.append(recs)
    return files


def write_all(d, files, **kw):
    """the files as in1.bam, in2.bam .. under d, file f with refs_of(f): (paths, raw BAM bytes)"""
    paths = [d / ("in%d.bam" % (i + 1)) for i in range(len(files))]
    return [str(p) for p in paths], [write(p, recs, refs=refs_of(i), **kw) for i, (p, recs) in enumerate(zip(paths, files))]
