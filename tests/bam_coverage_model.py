"""Two plain-Python statements of `sam coverage histogram` (src/sam_coverage_histogram.rs over this build's reading of `samtools depth
-a`) over raw BAM bytes, on tests/bam_rewrite_model.py's reader and tests/bam_markdup_model.py's record builder.

literal() keeps one counter per position, from the first to the last target position of a reference: for small references or targets.
events() is the form the device path rests on: two events per covering run and per target interval on one global axis, sorted, and
one sweep that adds the gap behind an event to the bin of the running depth wherever the running `inside` is positive.

Both return (hist[10001], n_dropped, n_positions, n_counted).  mode: ("everywhere",) | ("region", text) | ("bed", text of the file)."""
import random
import re
import struct

import numpy as np

from tests import bam_rewrite_model as rm
from tests.bam_markdup_model import D, EQ, H, I, M, N, P, S, X, core, rec  # noqa: F401
from tests.bam_rewrite_model import header, records, write  # noqa: F401

BINS = 10001
SKIP = 0x704
MSG_BOTH = b"ERROR: Only one of --region or --regions can be provided.\n"
MSG_BED = b"ERROR: Invalid region in BED file:\n"


def refs_of(raw):
    """[(name without its NUL, l_ref read unsigned)]"""
    (l_text,) = struct.unpack_from("<i", raw, 4)
    o = 8 + l_text
    (n_ref,) = struct.unpack_from("<i", raw, o)
    o += 4
    out = []
    for _ in range(n_ref):
        (ln,) = struct.unpack_from("<i", raw, o)
        name = raw[o + 4:o + 4 + ln]
        out.append((name[:-1] if name.endswith(b"\0") else name, struct.unpack_from("<I", raw, o + 4 + ln)[0]))
        o += 4 + ln + 4
    return out


def counted(r, n_ref):
    tid, pos, lo, nc, flag, l_seq, tlen = core(r)
    return 0 <= tid < n_ref and not flag & SKIP


def runs(r, l_ref):
    """([the covering runs [s, e) cut to [0, l_ref), adjacent M = X fused], end): ops 0 7 8 cover and advance, 2 3 advance, the others
    (9 .. 15 too) do neither; end = the position behind the last reference-consuming op"""
    tid, pos, lo, nc, flag, l_seq, tlen = core(r)
    p, out, start = pos, [], None
    for k in range(nc):
        (op,) = struct.unpack_from("<I", r, 36 + lo + 4 * k)
        code, ln = op & 15, op >> 4
        if code in (0, 7, 8):
            if start is None:
                start = p
            p += ln
        elif code in (2, 3):
            if start is not None:
                out.append((start, p))
                start = None
            p += ln
    if start is not None:
        out.append((start, p))
    cut = [(max(s, 0), min(e, l_ref)) for s, e in out]
    return [(s, e) for s, e in cut if s < e], p


# ---- the options ----
def _digits(s):
    return int(s) if re.fullmatch(rb"[0-9]{1,18}", s) else None


def parse_region(text, refs):
    """(refID, beg, end) 0-based half-open, not yet cut to the reference, or None: it names no reference or does not parse"""
    names = [n for n, _ in refs]
    if text in names:
        r = names.index(text)
        return r, 0, refs[r][1]
    if b":" not in text:
        return None
    name, rest = text.rsplit(b":", 1)
    if name not in names:
        return None
    r = names.index(name)
    rest = rest.replace(b",", b"")
    b, dash, e = rest.partition(b"-")
    beg = _digits(b)
    end = _digits(e) if dash else refs[r][1]
    if beg is None or end is None:
        return None
    return r, max(beg, 1) - 1, end


class BadBed(Exception):
    def __init__(self, line):
        super().__init__(line)
        self.line = line


def parse_bed(text, refs):
    """[(refID, beg, end)] of the lines whose name is in the header; BadBed(line) for a line with fewer than three fields or a
    non-numeric field"""
    names = [n for n, _ in refs]
    out = []
    for line in text.splitlines(keepends=True):
        if line.startswith((b"#", b"track", b"browser")):
            continue
        f = line.split()
        if not f:
            continue
        if len(f) < 3 or _digits(f[1]) is None or _digits(f[2]) is None:
            raise BadBed(line)
        if f[0] in names:
            out.append((names.index(f[0]), _digits(f[1]), _digits(f[2])))
    return out


def merge(ivs):
    """sorted, disjoint, empty ones dropped; adjacent intervals join"""
    out = []
    for b, e in sorted(iv for iv in ivs if iv[0] < iv[1]):
        if out and b <= out[-1][1]:
            out[-1][1] = max(out[-1][1], e)
        else:
            out.append([b, e])
    return [tuple(x) for x in out]


def targets(raw, mode):
    """{refID: merged target intervals cut to the reference} and whether the region is known"""
    refs = refs_of(raw)
    recs = [r for r in records(raw) if counted(r, len(refs))]
    if mode[0] == "everywhere":
        has = {core(r)[0] for r in recs}
        return {t: [(0, refs[t][1])] for t in has if refs[t][1]}, True
    if mode[0] == "region":
        reg = parse_region(mode[1], refs)
        if reg is None:
            return {}, False
        t, b, e = reg
        e = min(e, refs[t][1])
        return ({t: [(b, e)]} if b < e else {}), True
    per = {}
    for t, b, e in parse_bed(mode[1], refs):
        per.setdefault(t, []).append((b, e))
    per = {t: merge(v) for t, v in per.items()}
    out = {}
    for r in recs:
        tid, pos = core(r)[:2]
        if tid in out or tid not in per:
            continue
        end = runs(r, refs[tid][1])[1]
        if end <= pos:
            end = pos + 1
        if any(b < end and pos < e for b, e in per[tid]):
            out[tid] = merge((b, min(e, refs[tid][1])) for b, e in per[tid])
    return {t: v for t, v in out.items() if v}, True


def literal(raw, mode=("everywhere",)):
    refs = refs_of(raw)
    tg, _ = targets(raw, mode)
    lo = {t: min(b for b, _ in ivs) for t, ivs in tg.items()}           # one counter per position, from a reference's first target
    depth = {t: np.zeros(max(e for _, e in ivs) - lo[t], dtype=np.int64) for t, ivs in tg.items()}     # position to its last
    n_counted = 0
    for r in records(raw):
        if not counted(r, len(refs)):
            continue
        n_counted += 1
        tid = core(r)[0]
        if tid in depth:
            for s, e in runs(r, refs[tid][1])[0]:
                depth[tid][max(s - lo[tid], 0):max(e - lo[tid], 0)] += 1
    hist, dropped, n_pos = [0] * BINS, 0, 0
    for t, ivs in tg.items():
        for b, e in ivs:
            d = depth[t][b - lo[t]:e - lo[t]]
            n_pos += len(d)
            dropped += int((d >= BINS).sum())
            for k, v in enumerate(np.bincount(d[d < BINS], minlength=1)):
                hist[k] += int(v)
    return hist, dropped, n_pos, n_counted


def sweep(raw, mode=("everywhere",)):
    """([(depth, inside, w) behind sorted event i, for every event but the last], n_counted): the running sums behind the event and
    the gap to the next one.  Events of one coordinate stand in any order; whatever it is, the last of them alone has w > 0 and the
    sums of them all, so the entries with w > 0 and their indices do not depend on it."""
    refs = refs_of(raw)
    base = [0]
    for _, ln in refs:
        base.append(base[-1] + ln)
    tg, _ = targets(raw, mode)
    ev, n_counted = [], 0
    for r in records(raw):
        if not counted(r, len(refs)):
            continue
        n_counted += 1
        tid = core(r)[0]
        for s, e in runs(r, refs[tid][1])[0]:
            ev += [(base[tid] + s, 1, 0), (base[tid] + e, -1, 0)]
    for t, ivs in tg.items():
        for b, e in ivs:
            ev += [(base[t] + b, 0, 1), (base[t] + e, 0, -1)]
    ev.sort(key=lambda x: x[0])                                         # (ties in any order: the gap between them is zero)
    out, depth, inside = [], 0, 0
    for k in range(len(ev) - 1):
        depth += ev[k][1]
        inside += ev[k][2]
        out.append((depth, inside, ev[k + 1][0] - ev[k][0]))
    return out, n_counted


def events(raw, mode=("everywhere",), swept=None):
    """swept: sweep(raw, mode) where the caller has it already"""
    gaps, n_counted = swept or sweep(raw, mode)
    hist, dropped, n_pos = [0] * BINS, 0, 0
    for depth, inside, w in gaps:
        if inside > 0 and w:
            n_pos += w
            if depth < BINS:
                hist[depth] += w
            else:
                dropped += w
    return hist, dropped, n_pos, n_counted


LDS_BELOW = 1 << 16      # bam_cov_hist_kernel: a gap of this many positions or more goes to the global counter at once
HIST_THREADS = 256       # ... event i is workgroup (i // 256) % grid's
HIST_WGS_PER_CU = 4      # launch_bam_cov_hist: ceil(events / 256) workgroups, at most four a planned CU


def hist_grid(n_events, cus):
    return min(-(-n_events // HIST_THREADS), HIST_WGS_PER_CU * cus)


def lds_sums(swept, grid):
    """{depth: the most any one workgroup of a grid of `grid` adds to its 32-bit LDS counter of that depth}: the gaps below 2^16
    positions at depths below BINS, event i with workgroup (i // 256) % grid.  Above 2^32 - 1 that counter wraps."""
    per = {}
    for i, (depth, inside, w) in enumerate(swept[0]):
        if inside > 0 and 0 < w < LDS_BELOW and depth < BINS:
            key = (depth, (i // HIST_THREADS) % grid)
            per[key] = per.get(key, 0) + w
    out = {}
    for (depth, _), v in per.items():
        out[depth] = max(out.get(depth, 0), v)
    return out


def stdout_of(hist):
    return b"".join(b"%d\t%d\n" % (k, v) for k, v in enumerate(hist))


def target_size(raw, mode):
    return sum(e - b for ivs in targets(raw, mode)[0].values() for b, e in ivs)


# ---- inputs ----
# CIGARs with all nine ops and a code above 8: (ops); several covering runs, runs split by D and N, I S H P between M ops (one run)
CIGARS = [((M, 20),), ((S, 3), (M, 17)), ((M, 10), (I, 2), (M, 8)), ((M, 10), (D, 5), (M, 10)), ((M, 8), (N, 300), (M, 12)),
          ((H, 4), (M, 20), (H, 2)), ((M, 10), (P, 1), (I, 1), (M, 9)), ((EQ, 12), (X, 1), (EQ, 7)), ((S, 2), (EQ, 10), (D, 1), (X, 2), (M, 6), (S, 5)),
          ((M, 5), (9, 7), (M, 5)), ((M, 4), (D, 2), (M, 4), (N, 9), (M, 4), (D, 1), (EQ, 3)), ((I, 5), (S, 5)), ((D, 4), (M, 6)), ((M, 0), (D, 3), (M, 7)),
          ((M, 30), (15, 3)), ((M, 150),)]
FLAGS = [0, 0, 0, 1 | 0x40, 1 | 0x80, 16, 0x800, 4, 0x100, 0x200, 0x400, 0x800 | 16]


def refs_for(n_ref=11, seed=1, lo=300, hi=4000):
    rnd = random.Random(seed)
    return [(b"ref%d" % k, rnd.randrange(lo, hi)) for k in range(n_ref)]


def sorted_records(n, refs, seed=1, skip_refs=(), l_seq=None):
    """n position-sorted records over the references (none on skip_refs), a tail without a reference; starts from -3 to past l_ref;
    l_seq: every record's, instead of what its CIGAR consumes (0: small records, many to a block)"""
    rnd = random.Random(seed)
    use = [t for t in range(len(refs)) if t not in skip_refs]
    out = []
    per = max(1, n // max(1, len(use)))
    k = 0
    for t in use:
        ps = sorted(rnd.randrange(-3, refs[t][1] + 5) for _ in range(per))
        for p in ps:
            out.append(rec(b"r%d" % k, t, p, rnd.choice(FLAGS), rnd.choice(CIGARS), l_seq=l_seq, tlen=rnd.choice([0, 100, -100])))
            k += 1
    while len(out) < n:
        out.append(rec(b"u%d" % len(out), -1, -1, 4, (), l_seq=20, mtid=-1, mpos=-1))
    return out


def by_position(recs):
    """position-sorted (stable), the records without a reference last"""
    return sorted(recs, key=lambda r: (core(r)[0] < 0, core(r)[0], core(r)[1]))


# ---- inputs that take a fixed-size structure of the device path past its capacity (tests/test_bam_coverage_model.py holds each) ----
CARRY_REF = (1 << 31) - 1
CARRY_PER_REF = 16384
CARRY_RUN = 65535


def carry_input(n_ref=20):
    """(refs, records): n_ref references of 2^31 - 1 positions, on each 16 384 runs of 65 535 positions at k * 131 070: every gap of
    either depth is 65 535 positions (the LDS side of the histogram kernel) but the one behind a reference's last run, 98 302"""
    refs = [(b"c%d" % t, CARRY_REF) for t in range(n_ref)]
    recs = [rec(b"%x" % k, t, 2 * CARRY_RUN * k, 0, ((M, CARRY_RUN),), l_seq=0) for t in range(n_ref) for k in range(CARRY_PER_REF)]
    return refs, recs


def carry_expected(n_ref=20):
    """(hist, n_dropped, n_positions, n_counted) of carry_input(n_ref) everywhere, by arithmetic"""
    n = n_ref * CARRY_PER_REF
    hist = [0] * BINS
    hist[1] = n * CARRY_RUN
    hist[0] = n_ref * CARRY_REF - hist[1]
    return hist, 0, n_ref * CARRY_REF, n


SPLIT_WIDTHS = (65535, 65536, 65537)
SPLIT_PILE = 9999


def split_input():
    """(refs, records, {depth: [gap widths]}): one reference of 2^20 positions; gaps of 65 535, 65 536 and 65 537 positions at depth 1
    (a run of that length by itself), at depth 0 (behind it), at depth 10 000 (one run of that length on a pile of 9 999) and at depth
    10 001 (two).  The pile's records start together and end a position apart, as test_pile_deeper_than_the_last_bin's do."""
    refs = [(b"s", 1 << 20)]
    recs, p = [], 100
    for w in SPLIT_WIDTHS:
        recs.append(rec(b"one%d" % w, 0, p, 0, ((M, w),), l_seq=0))
        p += 2 * w
    start, span = p, 2 * sum(SPLIT_WIDTHS)
    recs += [rec(b"p%d" % i, 0, start, 0, ((M, span + i + 1),), l_seq=0) for i in range(SPLIT_PILE)]
    for extra in (1, 2):
        for w in SPLIT_WIDTHS:
            recs += [rec(b"x%d.%d.%d" % (extra, w, j), 0, p, 0, ((M, w),), l_seq=0) for j in range(extra)]
            p += w
    assert p == start + span and p + SPLIT_PILE < refs[0][1]
    return refs, by_position(recs), {0: list(SPLIT_WIDTHS), 1: list(SPLIT_WIDTHS), SPLIT_PILE + 1: list(SPLIT_WIDTHS), SPLIT_PILE + 2: list(SPLIT_WIDTHS)}


def pow2_inputs():
    """[(name, refs, records)]: genomes of 2^13 - 1, 2^13 and 2^13 + 1 positions on three references and one of 2^12 on one; in each a
    record whose last run ends on the genome's last position (the largest sort key: the genome's size), one that would run past
    it, and one that starts at position 0 of the first reference"""
    out = []
    for name, lens in (("8191", (3000, 2000, 3191)), ("8192", (3000, 2000, 3192)), ("8193", (3000, 2000, 3193)), ("4096", (4096,))):
        refs = [(b"g%d" % k, ln) for k, ln in enumerate(lens)]
        last = len(refs) - 1
        recs = [r for r in sorted_records(40 * len(refs), refs, seed=len(name) + lens[-1]) if core(r)[0] >= 0]
        recs += [rec(b"first", 0, 0, 0, ((M, 20),)), rec(b"last", last, lens[-1] - 12, 16, ((M, 5), (D, 2), (M, 5))),
                 rec(b"past", last, lens[-1] - 7, 0, ((M, 20),))]
        out.append((name, refs, by_position(recs)))
    return out


WORDS_COUNTED = (0, 31, 32, 33, 63, 64, 69)
WORDS_NOT = ((1, 0x4), (30, 0x100), (34, 0x200), (65, 0x400))


def words_input():
    """(refs, records, bed, bed2): 70 references (three words of the device's bitmaps); counted records on WORDS_COUNTED alone, each
    over positions 100 .. 139, records that are not counted on WORDS_NOT.  bed: [90, 160) on every reference.  bed2: the same, but
    [180, 190) on ref64, behind its records"""
    refs = refs_for(n_ref=70, seed=70, lo=200, hi=600)
    recs = []
    for t in WORDS_COUNTED:
        recs += [rec(b"a%d" % t, t, 100, 0, ((M, 20),)), rec(b"b%d" % t, t, 110, 16, ((M, 10), (D, 5), (M, 15)))]
    recs += [rec(b"n%d" % t, t, 100, f, ((M, 20),)) for t, f in WORDS_NOT]
    line = lambda t, b, e: b"ref%d\t%d\t%d\n" % (t, b, e)                # noqa: E731
    bed = b"".join(line(t, 90, 160) for t in range(70))
    bed2 = b"".join(line(t, 180, 190) if t == 64 else line(t, 90, 160) for t in range(70))
    return refs, by_position(recs), bed, bed2


DEEP_N = 1000
DEEP_LEN = 100 * DEEP_N + 100


def deep_iv(k):
    return 100 * k + 10, 100 * k + 60


def deep_bed(seed=7):
    """DEEP_N disjoint intervals [100 k + 10, 100 k + 60) on `a` and on `c`, none on `b` between them; the lines shuffled, every
    seventh interval as two lines that overlap and every eleventh as two that touch"""
    rnd = random.Random(seed)
    lines = []
    for name in (b"a", b"c"):
        for k in range(DEEP_N):
            b, e = deep_iv(k)
            pieces = [(b, b + 30), (b + 20, e)] if k % 7 == 3 else [(b, b + 25), (b + 25, e)] if k % 11 == 5 else [(b, e)]
            lines += [b"%s\t%d\t%d\n" % (name, pb, pe) for pb, pe in pieces]
    rnd.shuffle(lines)
    return b"".join(lines)


DEEP_REFS = [(b"a", DEEP_LEN), (b"b", 5000), (b"c", DEEP_LEN)]
# relation -> (position from interval k's (ibeg, iend), CIGAR, does its span overlap an interval?).  A span is [pos, end), end behind
# the last reference-consuming op; without one it is [pos, pos + 1).
DEEP_RELATIONS = {
    "end == ibeg": (lambda b, e: b - 20, ((M, 20),), False),
    "end == ibeg + 1": (lambda b, e: b - 19, ((M, 20),), True),
    "pos == iend - 1": (lambda b, e: e - 1, ((M, 20),), True),
    "pos == iend": (lambda b, e: e, ((M, 20),), False),
    "spans two": (lambda b, e: e - 5, ((M, 70),), True),                # (20 positions do not reach from one interval to the next)
    "in a gap": (lambda b, e: e + 10, ((M, 20),), False),
    "nothing at ibeg - 1": (lambda b, e: b - 1, ((I, 3),), False),
    "nothing at ibeg": (lambda b, e: b, ((I, 3),), True),
    "nothing at iend - 1": (lambda b, e: e - 1, ((I, 3),), True),
    "nothing at iend": (lambda b, e: e, ((I, 3),), False),
}
DEEP_KS = (0, 1, 499, 500, 750, 998)                                   # (interval 999 has no next one to span to: the ends are cases of their own)


def deep_cases():
    """[(name, records, {refID: is it reported?})]: in each file one counted record on `a`, one on `c` in another relation to
    another interval, and one on `b`, so that every relation decides by itself whether its reference is reported"""
    names = list(DEEP_RELATIONS)
    one = lambda tid, rel, k: rec(b"r", tid, DEEP_RELATIONS[rel][0](*deep_iv(k)), 0, DEEP_RELATIONS[rel][1])      # noqa: E731
    out = []
    for i, rel in enumerate(names):
        for j, k in enumerate(DEEP_KS):
            other, k2 = names[(i + 1 + j) % len(names)], DEEP_KS[(j + 3) % len(DEEP_KS)]
            recs = [one(0, rel, k), rec(b"mid", 1, 100, 0, ((M, 20),)), one(2, other, k2)]
            out.append(("%s @%d | %s @%d" % (rel, k, other, k2), recs, {0: DEEP_RELATIONS[rel][2], 1: False, 2: DEEP_RELATIONS[other][2]}))
    last_b, last_e = deep_iv(DEEP_N - 1)
    ends = [("before the first | behind the last", [rec(b"r", 0, 1, 0, ((M, 8),)), rec(b"r", 2, last_e + 10, 0, ((M, 20),))], {0: False, 2: False}),
            ("the first | the last", [rec(b"r", 0, 1, 0, ((M, 10),)), rec(b"r", 2, last_e - 1, 0, ((M, 20),))], {0: True, 2: True}),
            ("behind the last at iend | nothing in the last", [rec(b"r", 0, last_e, 0, ((M, 20),)), rec(b"r", 2, last_e - 1, 0, ((I, 3),))], {0: False, 2: True})]
    return out + ends
