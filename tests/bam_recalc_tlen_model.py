"""Two plain-Python statements of `sam recalculate tlen` (src/sam_recalculate_tlen.rs) over raw BAM bytes, on
tests/bam_rewrite_model.py's reader and writer, and a generator of inputs the command serves.

literal() follows the reference's loop line by line: the FIFO deque of reads, the map from a name to the place of the read that waits
for its mate, the flush of the ready reads at the deque's front after every record, and the partial output, stderr and exit code when
a record stops the loop.
grouped() is the statement the device path rests on: every record is Z (written with TLEN 0), S (the reference stops) or C (a
candidate); among the candidates of one name, in file order, the 1st and 2nd are a pair, the 3rd and 4th, and so on; an odd last one is
discarded.  It returns None where it sees a record the loop may stop at: there literal() decides."""
import collections
import functools
import random
import struct

from tests import bam_markdup_model as md
from tests.bam_markdup_model import CIGARS, D, EQ, H, I, M, N, P, S, X  # noqa: F401  (the operations, for the tests)
from tests.bam_rewrite_model import EOF_BLOCK, Stop, members, out_header, records, write  # noqa: F401  (what the tests use)

MSG_SECONDARY = b"ERROR: Secondary and supplementary read alignments are not supported.\n"
MSG_MAX_LEN = b"ERROR: --max-len must be a positive integer.\n"
# a Rust panic as this build's host reader words it (status 101)
PANIC_UTF8 = b"thread 'main' panicked: called `Result::unwrap()` on an `Err` value: Utf8Error\n"
PANIC_ASSERT = b"thread 'main' panicked: assertion failed: read.is_first_in_template() != mate.is_first_in_template()\n"
PANIC_CIGAR = b"thread 'main' panicked: Unexpected cigar operation\n"


# ---- one record's fields ----
def fields(rec):
    """tid, pos, flag, mtid, mpos"""
    tid, pos = struct.unpack_from("<ii", rec, 4)
    (flag,) = struct.unpack_from("<H", rec, 18)
    mtid, mpos = struct.unpack_from("<ii", rec, 24)
    return tid, pos, flag, mtid, mpos


def qname(rec):
    return rec[36:36 + rec[12] - 1]


def tlen_of(rec):
    return struct.unpack_from("<i", rec, 32)[0]


def with_tlen(rec, t):
    """`as i32`: the low 32 bits of t at record offset 32"""
    return rec[:32] + struct.pack("<I", t & 0xFFFFFFFF) + rec[36:]


def parse_max_len(text):
    """args.get_str("--max-len").parse::<i64>().unwrap_or(0) (:29): [+-]digits within i64, anything else 0"""
    body = text[1:] if text[:1] in ("+", "-") else text
    if not body or not all(c in "0123456789" for c in body):
        return 0
    v = int(text)
    return v if -(1 << 63) <= v < (1 << 63) else 0


def classify(rec, max_len):
    """:44-55 — "Z" written with TLEN 0, "S" the reference stops, "C" a candidate"""
    tid, pos, flag, mtid, mpos = fields(rec)
    if not flag & 0x1 or flag & 0x4 or flag & 0x8:
        return "Z"
    if flag & 0x900:
        return "S"
    if tid != mtid or abs(pos - mpos) > max_len or bool(flag & 0x10) == bool(flag & 0x20):
        return "Z"
    return "C"


def start(rec):
    """:60-61 — the 5' end: pos, or for a reverse read cigar().end_pos() - 1; Stop(101) where cigar() panics"""
    _, pos, flag, _, _ = fields(rec)
    return md.end_pos(rec) - 1 if flag & 0x10 else pos


def pair_tlen(a, b):
    """:59-73 for the earlier record a and the later b: t, of which b gets the low 32 bits and a those of -t; Stop(101) at the assert
    (first) and where cigar() panics (b's, then a's)"""
    if (fields(a)[2] ^ fields(b)[2]) & 0x40 == 0:
        s = Stop(101)
        s.msg = PANIC_ASSERT
        raise s
    try:
        sb = start(b)
        sa = start(a)
    except Stop as s:
        s.msg = PANIC_CIGAR
        raise
    t = abs(sb - sa) + 1
    if fields(b)[1] > fields(a)[1]:
        t = -t
    rev = bool(fields(b)[2] & 0x10)
    if (sb < sa and rev) or (sb > sa and not rev):
        t = 0
    return t


def discard_line(name):
    return b"Read " + name + b" discarded due to missing mate.\n"


# ---- the reference's loop ----
def literal(raw, max_len):
    """(inflated stdout, stderr, exit code): on a stop the records already flushed from the FIFO, the message, 255 or 101"""
    out, err = [out_header(raw)], []
    reads = collections.deque()                                         # [ready, tlen, record]
    mates = {}
    written = 0
    for rec in records(raw):
        name = qname(rec)
        try:
            name.decode("utf-8")
        except UnicodeDecodeError:
            return b"".join(out), PANIC_UTF8, 101
        cls = classify(rec, max_len)
        if cls == "S":
            return b"".join(out), MSG_SECONDARY, 255
        if cls == "Z":
            reads.append([True, 0, rec])
        elif name in mates:
            mate = reads[mates.pop(name) - written]
            try:
                t = pair_tlen(mate[2], rec)
            except Stop as s:
                return b"".join(out), s.msg, s.code
            reads.append([True, t, rec])
            mate[0], mate[1] = True, -t
        else:
            mates[name] = written + len(reads)
            reads.append([False, 0, rec])
        while reads and reads[0][0]:
            _, t, r = reads.popleft()
            out.append(with_tlen(r, t))
            written += 1
    for ready, t, r in reads:
        if not ready:
            err.append(discard_line(qname(r)))
            continue
        out.append(with_tlen(r, t))
    return b"".join(out), b"".join(err), 0


# ---- the grouped statement ----
def grouped_parts(raw, max_len):
    """(header, written records with their new TLENs, discarded names) in file order, or None: a record the loop may stop at"""
    recs = list(records(raw))
    tl = [0] * len(recs)
    waiting = {}                                                        # name -> the candidate of odd rank that has no mate yet
    for k, rec in enumerate(recs):
        name = qname(rec)
        try:
            name.decode("utf-8")
        except UnicodeDecodeError:
            return None
        cls = classify(rec, max_len)
        if cls == "S":
            return None
        if cls == "C":
            if name in waiting:
                a = waiting.pop(name)
                try:
                    t = pair_tlen(recs[a], rec)
                except Stop:
                    return None
                tl[a], tl[k] = -t, t
            else:
                waiting[name] = k
    lone = set(waiting.values())
    return (out_header(raw), [with_tlen(r, tl[k]) for k, r in enumerate(recs) if k not in lone], [qname(recs[k]) for k in sorted(lone)])


def grouped(raw, max_len):
    """(inflated stdout, stderr, 0), or None as grouped_parts"""
    parts = grouped_parts(raw, max_len)
    if parts is None:
        return None
    hdr, recs, lone = parts
    return hdr + b"".join(recs), b"".join(discard_line(n) for n in lone), 0


# ---- inputs ----
JUNK = [7, -7, 123456, -(1 << 31), 0x7FFFFFFF, 1, -1, 99999]              # what the input TLENs hold: never 0, so a pass-through shows
DISTS = [1, 2, 5000, 5001, 37, 300, 0]                                   # |pos - mpos|: at and just above the max_len the tests use
# end_pos more than 2^31 beyond the mate: nine N runs of 2^28 - 1
LONG_N = ((M, 5),) + ((N, (1 << 28) - 1),) * 9 + ((M, 5),)


def cand(name, tid, pos, mpos, rev, first, cigar=((M, 20),), junk=7, extra=0):
    """a record that is a candidate whenever |pos - mpos| <= max_len: paired, both mapped, one tid, 0x20 the opposite of 0x10"""
    flag = 0x1 | (0x40 if first else 0x80) | (0x10 if rev else 0x20) | extra
    return md.rec(name, tid, pos, flag=flag, cigar=cigar, tlen=junk, mtid=tid, mpos=mpos)


@functools.lru_cache(maxsize=None)
def served_records(n=3000, seed=1):
    """n records every one of which the command serves, for every max_len: names with 1, 2, 3 and 4 candidates, mates adjacent and about
    700 records apart, every reason for Z, 0x100 / 0x800 records that are Z by their first line, one mate a candidate and the other Z,
    reverse reads with CIGARs of every operation, converging, diverging and same-start pairs, pos(b) below, equal to and above pos(a),
    both mates reverse and both forward, one pair whose N runs carry end_pos more than 2^31 beyond its mate, a name many records carry,
    and junk in every input TLEN"""
    rnd = random.Random(seed)
    out, far = [], []                                                   # far: (the number of records after which it is due, record)
    shared = 0
    k = 0
    while len(out) < n:
        k += 1
        out += [r for due, r in far if due <= len(out)]
        far = [(due, r) for due, r in far if due > len(out)]
        kind = k % 16
        name = b"q%d:" % k + bytes(rnd.choice(b"ACGTacgt0123456789_:-.") for _ in range(rnd.randrange(0, 12)))
        tid, p = rnd.randrange(0, 3), rnd.randrange(0, 1_000_000)
        d = DISTS[k % len(DISTS)]
        j = JUNK[k % len(JUNK)]
        cg = CIGARS[k % len(CIGARS)]
        cg2 = CIGARS[(k // 3) % len(CIGARS)]
        if kind == 0:                                                   # one candidate: discarded
            out.append(cand(name, tid, p, p + d, k & 32, True, cg, j))
        elif kind == 1:                                                 # converging, b to the right: pos(b) > pos(a) unless d == 0
            out += [cand(name, tid, p, p + d, False, True, cg, j), cand(name, tid, p + d, p, True, False, cg2, j)]
        elif kind == 2:                                                 # converging, b to the left
            out += [cand(name, tid, p + d, p, True, k & 32, cg, j), cand(name, tid, p, p + d, False, not k & 32, cg2, j)]
        elif kind == 3:                                                 # diverging, either order: TLEN 0 for both
            if k & 16:
                out += [cand(name, tid, p, p + 300, True, True, cg, j), cand(name, tid, p + 300, p, False, False, cg2, j)]
            else:
                out += [cand(name, tid, p + 300, p, False, True, cg, j), cand(name, tid, p, p + 300, True, False, cg2, j)]
        elif kind == 4:                                                 # the same 5' end: b reverse over one base at a's pos
            out += [cand(name, tid, p, p, False, True, cg, j), cand(name, tid, p, p, True, False, ((S, 4), (M, 1)), j)]
        elif kind == 5:                                                 # pos(b) == pos(a), the 5' ends apart
            out += [cand(name, tid, p, p, k & 16, True, cg, j), cand(name, tid, p, p, not k & 16, False, cg2, j)]
        elif kind == 6:                                                 # three candidates: the third is discarded
            out += [cand(name, tid, p, p + d, False, True, cg, j), cand(name, tid, p + d, p, True, False, cg2, j)]
            third = cand(name, tid, p, p + d, False, True, cg, j)
            if k & 16:
                far.append((len(out) + 700, third))
            else:
                out.append(third)
        elif kind == 7:                                                 # four candidates: two pairs, the second far away
            out += [cand(name, tid, p, p + d, False, True, cg, j), cand(name, tid, p + d, p, True, False, cg2, j)]
            far += [(len(out) + 700, cand(name, tid, p + 1, p + d, True, False, cg2, j)), (len(out) + 702, cand(name, tid, p + d, p + 1, False, True, cg, j))]
        elif kind == 8:                                                 # the mate about 700 records later
            out.append(cand(name, tid, p, p + d, k & 16, True, cg, j))
            far.append((len(out) + 700, cand(name, tid, p + d, p, not k & 16, False, cg2, j)))
        elif kind == 9:                                                 # every reason for Z
            why = (k // 16) % 7
            flag, mtid, mpos = [(0x40, tid, p), (0x1 | 0x4 | 0x40, tid, p), (0x1 | 0x8 | 0x80, tid, p), (0x1 | 0x10, (tid + 1) % 3, p),
                                (0x1 | 0x20, tid, p + (1 << 30)), (0x1 | 0x10 | 0x20, tid, p), (0x1 | 0x80, tid, p)][why]
            out.append(md.rec(name, tid, p, flag=flag, cigar=cg, tlen=j, mtid=mtid, mpos=mpos))
        elif kind == 10:                                                # 0x100 / 0x800 records that are Z by their first line
            flag = [0x100, 0x800 | 0x1 | 0x4, 0x100 | 0x1 | 0x8 | 0x10, 0x900, 0x800 | 0x10][(k // 16) % 5]
            out.append(md.rec(name, tid, p, flag=flag, cigar=cg, tlen=j, mtid=tid, mpos=p + d))
        elif kind == 11:                                                # one mate a candidate, the other Z: the candidate is discarded
            out += [cand(name, tid, p, p + d, False, True, cg, j), md.rec(name, tid, p + d, flag=0x1 | 0x8 | 0x80 | 0x10, cigar=cg2, tlen=j, mtid=tid, mpos=p)]
        elif kind == 12:                                                # a Z record of the same name between two mates takes no part
            out += [cand(name, tid, p, p + d, True, True, cg, j), md.rec(name, tid, p, flag=0x100, cigar=cg2, tlen=j, mtid=tid, mpos=p),
                    cand(name, tid, p + d, p, False, False, cg2, j)]
        elif kind == 13:                                                # both reverse, both forward
            r = bool(k & 16)
            out += [cand(name, tid, p, p + d, r, True, cg, j), cand(name, tid, p + d, p, r, False, cg2, j)]
        elif kind == 14:                                                # a name many records carry, far apart: pairs by rank
            out.append(cand(b"X", tid, p, p + (shared >> 2 & 1), shared & 2, not shared & 1, cg, j))     # (a candidate for every max_len)
            shared += 1
        else:                                                           # soft clips, insertions and pads around the 5' end
            out += [cand(name, tid, p + 7, p, True, False, cg, j), cand(name, tid, p, p + 7, False, True, cg2, j)]
        if k == 40:                                                     # `as i32` cuts: |t| is above 2^31
            out += [cand(b"long", 0, 100, 101, False, True, ((M, 10),), 5), cand(b"long", 0, 101, 100, True, False, LONG_N, 5)]
    return tuple(out[:n])


def stop_files():
    """what -> (records, the index of the stopping record, status, stderr): a served file with one record the reference's loop stops at"""
    base = list(served_records(400, seed=2))
    a = cand(b"pair", 0, 100, 200, False, True)
    same = cand(b"pair", 0, 200, 100, True, True)                        # 0x40 like its mate
    bad_op = md.rec(b"pair", 0, 200, flag=0x1 | 0x80 | 0x10, cigar=((M, 10), (9, 3)), l_seq=10, mtid=0, mpos=100)
    bad_first = md.rec(b"pair", 0, 100, flag=0x1 | 0x40 | 0x10, cigar=((M, 10), (12, 1)), l_seq=10, mtid=0, mpos=200)
    secondary = md.rec(b"sec", 0, 10, flag=0x1 | 0x100 | 0x10, mtid=0, mpos=20)
    return {
        "secondary": (base[:150] + [secondary] + base[150:], 150, 255, MSG_SECONDARY),
        "supplementary": (base[:150] + [md.rec(b"sup", 0, 10, flag=0x1 | 0x800 | 0x20, mtid=1, mpos=20)] + base[150:], 150, 255, MSG_SECONDARY),
        "utf8": (base[:90] + [md.rec(b"bad\xff\xfe", 0, 10, flag=0)] + base[90:], 90, 101, PANIC_UTF8),
        "assert": (base[:200] + [a] + base[200:260] + [same] + base[260:], 261, 101, PANIC_ASSERT),
        "cigar": (base[:200] + [a] + base[200:260] + [bad_op] + base[260:], 261, 101, PANIC_CIGAR),
        "cigar of the waiting mate": (base[:200] + [bad_first] + base[200:260] + [cand(b"pair", 0, 200, 100, False, False)] + base[260:], 261, 101, PANIC_CIGAR),
        "first record": ([secondary] + base, 0, 255, MSG_SECONDARY),
    }
