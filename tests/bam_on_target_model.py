"""Two plain-Python statements of `sam statistics --on-target=BED` (src/sam_statistics.rs:63-106) over record columns.

A record is (flag, tid, mtid, pos, mpos, tlen, end_pos), end_pos = the cigar's end as SK_COL_END gives it.  regions_by_tid[tid] is
that reference's list of (start, end), 1-based inclusive as :44-47 keep them (start = BED column 2 + 1, end = BED column 3), in BED
order; both statements sort it by start (:51-53).

sweep() is the reference's loop with its `break` rules as written.  closed() is the form the device path rests on:
with k = the regions with start <= end and pmax[i] = the largest region end among regions 0 .. i, a fragment is on target iff
k > 0 and pmax[k - 1] >= start.

Both return [total_reads, aligned_reads, duplicate_reads, total_fragments, on_target_fragments] and raise BadTid at a fragment whose
tid has no entry in regions_by_tid, where the reference panics (target_regions[tid]).  With bad=[] such fragments are counted as
fragments, appended to the list and not looked up: what sk_on_target_add does with them."""
import random

MAX_FRAG_LEN = 5000
REC_FIELDS = ("flag", "tid", "mtid", "pos", "mpos", "tlen", "end_pos")
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


class BadTid(IndexError):
    pass


def fragment(rec, max_frag_len=MAX_FRAG_LEN):
    """(reads, aligned, duplicate, interval): what one record adds to the S1 counters, and its fragment's (start, end) or None (:64-92)"""
    flag, tid, mtid, pos, mpos, tlen, end_pos = rec
    if flag & 0x100 or flag & 0x800:                                        # :64
        return 0, 0, 0, None
    if flag & 0x4:                                                          # :66
        return 1, 0, 0, None
    dup = 1 if flag & 0x400 else 0                                          # :69
    if flag & 0x1:
        if flag & 0x8:                                                      # :76
            return 1, 1, dup, None
        if tid != mtid:                                                     # :77
            return 1, 1, dup, None
        if pos > mpos or (pos == mpos and not flag & 0x40):                 # :81
            return 1, 1, dup, None
        tl = abs(tlen)                                                      # :83 (i64 in the reference: -2^31 is 2^31)
        if tl > max_frag_len:                                               # :84
            return 1, 1, dup, None
        start = pos + 1                                                     # :86
        end = start + tl                                                    # :87
    else:
        start = pos + 1                                                     # :90
        end = end_pos + 1                                                   # :91
    return 1, 1, dup, (start, end)


def _count(records, regions_by_tid, hit, prepared, max_frag_len, bad):
    c = [0, 0, 0, 0, 0]
    tables = [prepared(sorted(rs, key=lambda r: r[0])) for rs in regions_by_tid]        # :51-53
    for rec in records:
        reads, aligned, dup, iv = fragment(rec, max_frag_len)
        c[0] += reads
        c[1] += aligned
        c[2] += dup
        if iv is None:
            continue
        c[3] += 1                                                           # :94
        tid = rec[1]
        if tid < 0 or tid >= len(tables):                                   # :97 target_regions[tid as usize]
            if bad is None:
                raise BadTid(tid)
            bad.append(rec)
            continue
        c[4] += hit(tables[tid], iv[0], iv[1])
    return c


def _sweep_hit(regions, start, end):
    for rs, re in regions:                                                  # :97-106
        if start <= re and end >= rs:
            return 1
        if rs > end:
            break
    return 0


def _closed_table(regions):
    starts, pmax, run = [], [], None
    for rs, re in regions:
        run = re if run is None or re > run else run
        starts.append(rs)
        pmax.append(run)
    return starts, pmax


def _closed_hit(table, start, end):
    starts, pmax = table
    lo, hi = 0, len(starts)                                                 # k = the first index with starts[k] > end
    while lo < hi:
        mid = (lo + hi) // 2
        if starts[mid] <= end:
            lo = mid + 1
        else:
            hi = mid
    return 1 if lo > 0 and pmax[lo - 1] >= start else 0


def sweep(records, regions_by_tid, max_frag_len=MAX_FRAG_LEN, bad=None):
    return _count(records, regions_by_tid, _sweep_hit, lambda rs: rs, max_frag_len, bad)


def closed(records, regions_by_tid, max_frag_len=MAX_FRAG_LEN, bad=None):
    return _count(records, regions_by_tid, _closed_hit, _closed_table, max_frag_len, bad)


def _pct(num, den):
    """Rust's `{:.1}` of num as f64 / den as f64 * 100.0"""
    if den == 0:
        return "NaN" if num == 0 else "inf"
    return "%.1f" % (num / den * 100.0)


def report(counters, on_target=True):
    """the command's stdout (:109-115); on_target=False: without the option, or with a header that has no reference"""
    total, aligned, dup, frags, on = counters
    out = "Total reads: %d\n" % total
    out += "Aligned reads: %d (%s%% of all reads)\n" % (aligned, _pct(aligned, total))
    out += "Duplicate reads: %d (%s%% of aligned reads)\n" % (dup, _pct(dup, aligned))
    if on_target:
        out += "On-target: %s%%\n" % _pct(on, frags)
    return out.encode()


def parse_bed(text, names):
    """regions_by_tid of a well-formed BED text (:34-48): blank lines and lines that begin with '#' are skipped"""
    regions = [[] for _ in names]
    for line in text.split(b"\n"):
        if not line.strip() or line.startswith(b"#"):
            continue
        cols = line.strip().split(b"\t")
        regions[names.index(cols[0].decode())].append((int(cols[1]) + 1, int(cols[2])))
    return regions


# ---- inputs both test files share ------------------------------------------------------------------------------------------
# Reference 0: no region.  1: one region.  2: many regions with one start.  3: a long early region over later short ones (what a
# nearest-by-start lookup gets wrong) and a region that begins at 2^31.  4: inverted lines (chr 100 50), zero-length lines (start ==
# end in BED terms: (s + 1, s)), touching neighbours, out of order.
CRAFTED_BED = [
    [],
    [(1001, 2000)],
    [(501, 600), (501, 520), (501, 900), (501, 501), (501, 700)],
    [(101, 10000), (201, 210), (301, 310), (5001, 5010), (20001, 20010), ((1 << 31), (1 << 31) + 10)],
    [(101, 50), (301, 300), (401, 400), (801, 900), (601, 700), (701, 800), (1201, 1100), (1001, 1000)],
]


def boundary_records(regions_by_tid):
    """For every region: unpaired and paired fragments whose start is the region's end and whose end is the region's start, and the same
    one position to either side."""
    recs = []
    for tid, regions in enumerate(regions_by_tid):
        for rs, re in regions:
            for d in (-1, 0, 1):
                for start, end in ((re + d, re + d + 30), (rs + d - 30, rs + d), (rs + d, rs + d), (re + d, re + d)):
                    pos = start - 1
                    if not (I32_MIN <= pos <= I32_MAX and I32_MIN <= end - 1 <= I32_MAX):
                        continue
                    recs.append((0, tid, -1, pos, 0, 0, end - 1))                             # unpaired: end = end_pos + 1
                    if 0 <= end - start <= MAX_FRAG_LEN:
                        recs.append((0x1 | 0x40, tid, tid, pos, pos, end - start, pos))       # paired: end = start + |tlen|
    return recs


def edge_records():
    """The values the arithmetic and the filters turn on."""
    recs = [
        (0x41, 3, 3, I32_MAX, I32_MAX, 5000, 0),              # start = 2^31, end = 2^31 + 5000: inside the region at 2^31
        (0x41, 3, 3, I32_MAX - 1, I32_MAX, -4, 0),
        (0x41, 1, 1, 1500, 1500, I32_MIN, 0),                  # |tlen| = 2^31 > 5000
        (0x41, 1, 1, 1500, 1500, 5000, 0), (0x41, 1, 1, 1500, 1500, -5000, 0),
        (0x41, 1, 1, 1500, 1500, 5001, 0), (0x41, 1, 1, 1500, 1500, -5001, 0),
        (0x41, 1, 1, 1500, 1500, 10, 0), (0x01, 1, 1, 1500, 1500, 10, 0), (0x81, 1, 1, 1500, 1500, 10, 0),   # pos == mpos with and without 0x40
        (0x01, 1, 1, 1500, 1501, 10, 0), (0x01, 1, 1, 1501, 1500, 10, 0),
        (0x41, 1, 1, -1, -1, 1000, 0), (0x00, 1, -1, -1, 0, 0, 1000), (0x00, 1, -1, -1, 0, 0, -1),           # pos = -1
        (0x00, 1, -1, 1500, 0, 0, 100), (0x00, 1, -1, 1500, 0, 0, I32_MIN), (0x00, 3, -1, I32_MAX, 0, 0, I32_MIN),   # unpaired, end < start
        (0x00, 3, -1, 150, 0, 0, I32_MAX), (0x00, 3, -1, I32_MAX, 0, 0, I32_MAX),
        (0x00, 4, -1, 10, 0, 0, 60), (0x00, 4, -1, 10, 0, 0, 10),
    ]
    for bits in range(1 << 7):                                  # every combination of 0x1 0x4 0x8 0x40 0x100 0x400 0x800
        flag = sum(b for k, b in enumerate((0x1, 0x4, 0x8, 0x40, 0x100, 0x400, 0x800)) if bits >> k & 1)
        recs.append((flag, 1, 1, 1500, 1500, 100, 1600))
        recs.append((flag, 2, 2, 100, 300, 100, 200))
    return recs


def drawn_records(n, seed, n_chr=len(CRAFTED_BED), bad_tids=()):
    """n records drawn around the crafted regions' coordinates; bad_tids: tids without a reference, drawn now and then"""
    rng = random.Random(seed)
    flags = (99, 147, 83, 163, 65, 129, 0, 16, 4, 1024 + 99, 1024, 256 + 99, 2048 + 99, 73, 1, 0x41, 0x441)
    tids = list(range(n_chr)) * 8 + list(bad_tids)
    recs = []
    for _ in range(n):
        flag = rng.choice(flags)
        tid = rng.choice(tids)
        pos = rng.choice((rng.randrange(0, 1400), rng.randrange(0, 1400), rng.randrange(0, 25000), I32_MAX - rng.randrange(0, 20)))
        tlen = rng.choice((rng.randrange(-300, 300), rng.randrange(-6000, 6000)))
        mtid = tid if rng.random() < 0.9 else rng.randrange(-1, n_chr)
        mpos = pos if rng.random() < 0.2 else pos + rng.randrange(-50, 300)
        end_pos = min(pos + rng.randrange(0, 200), I32_MAX)
        recs.append((flag, tid, mtid, pos, min(mpos, I32_MAX), tlen, end_pos))
    return recs


def drawn_regions(rng, n_chr, max_regions=12, span=3000):
    """region lists with nesting, equal starts, inverted and zero-length lines"""
    out = []
    for _ in range(n_chr):
        regions = []
        for _ in range(rng.randrange(0, max_regions + 1)):
            s = rng.randrange(0, span)
            e = s + rng.choice((0, 1, 5, 40, 40, 300, 2000, -1, -30))
            regions.append((s + 1, e))
        out.append(regions)
    return out


def crafted_records():
    return boundary_records(CRAFTED_BED) + edge_records()
