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


def events(raw, mode=("everywhere",)):
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
    hist, dropped, n_pos, depth, inside = [0] * BINS, 0, 0, 0, 0
    for k in range(len(ev) - 1):
        depth += ev[k][1]
        inside += ev[k][2]
        w = ev[k + 1][0] - ev[k][0]
        if inside > 0 and w:
            n_pos += w
            if depth < BINS:
                hist[depth] += w
            else:
                dropped += w
    return hist, dropped, n_pos, n_counted


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
