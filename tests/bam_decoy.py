"""BAM streams built to fool the record walk's guess (sk_inflate.hip: bam_walk_kernel, bam_walk_guess_kernel, bam_walk_fix_kernel),
and the plain statements they are held to.  Plain Python, no GPU.

A DECOY is a run of well-formed fake records inside a real record's B:C aux array (or its quality bytes), behind a run of zeros; a
block end is placed inside the zeros, so the block that begins there finds the decoy before it finds a real record.  What the walk
must give is plain_walk(): one sequential walk of the block_size fields.  plausible() / guessed_entries() / simulate() restate the
three kernels; they serve as WITNESSES only (that an input fools the guess, that the rounds are bounded): no expected value of a GPU
test comes from them."""
import random
import struct

from tests import bam_rewrite_model as rm

BAD_RECORD = (1 << 64) - 2            # kWalkBadRecord
TRUNCATED = (1 << 64) - 3             # kWalkTruncated
REFS = [(b"ref0", 6000), (b"ref1", 5000), (b"ref2", 4000)]
N_REF = len(REFS)
TEXT = b"@HD\tVN:1.6\tSO:unsorted\n"
# a counted decoy would change every counter: 0x400 = total, aligned and duplicates; 0x41 with tid == mtid and tlen 9 = the histogram
DECOY_FLAGS = (0x400, 0x41)
REAL_FLAGS = (0, 16, 99, 147, 0x41, 0x81, 4, 0x100, 0x800 | 16, 0x400, 0x441)


def le32(raw, o):
    return struct.unpack_from("<I", raw, o)[0]


# ---- the plain walk: the expected value ----
def record_starts(raw, first, length=None):
    """the offset of every record, by one sequential walk; the walk must end where the stream ends"""
    length = len(raw) if length is None else length
    out, o = [], first
    while o < length:
        out.append(o)
        o += 4 + le32(raw, o)
    assert o == length, "the stream does not end where its last record ends"
    return out


def plain_walk(raw, first, ends):
    """(entry[n], nrec[n]): for every block the first record that begins at or behind max(begin, first) (the stream's length when
    there is none), and the number of records that begin in the block"""
    starts = record_starts(raw, first) + [len(raw)]
    entry, nrec, k = [], [], 0
    begin = 0
    for e in ends:
        e = int(e)
        lo = max(begin, first)
        while starts[k] < lo:
            k += 1
        entry.append(starts[k])
        j = k
        while j < len(starts) - 1 and starts[j] < e:
            j += 1
        nrec.append(j - k)
        begin = e
    return entry, nrec


def plain_entries(raw, first, ends):
    return plain_walk(raw, first, ends)[0]


# ---- the kernels restated: witnesses ----
def plausible(raw, o, n_ref, length=None):
    """bam_plausible: three records in a row from o look like records (or the stream ends first)"""
    length = len(raw) if length is None else length
    for _ in range(3):
        if o == length:
            return True
        if o + 36 > length:
            return False
        bs = le32(raw, o)
        if bs < 32 or bs > (1 << 28) or o + 4 + bs > length:
            return False
        tid, pos, w8, w12, l_seq, mtid, mpos = struct.unpack_from("<iiIIiii", raw, o + 4)
        l_name, n_cigar = w8 & 0xFF, w12 & 0xFFFF
        if tid < -1 or mtid < -1 or pos < -1 or mpos < -1 or l_seq < 0 or l_name == 0:
            return False
        if n_ref >= 0 and (tid >= n_ref or mtid >= n_ref):
            return False
        if 32 + l_name + 4 * n_cigar + ((l_seq + 1) >> 1) + l_seq > bs:
            return False
        if raw[o + 36 + l_name - 1] != 0:
            return False
        o += 4 + bs
    return True


def walk_one(raw, length, o, end):
    """bam_walk_one: (exit, records) of the walk from o to the block's end"""
    n = 0
    while o < end:
        if o + 4 > length:
            return TRUNCATED, n
        bs = le32(raw, o)
        if bs < 32:
            return BAD_RECORD, n
        if o + 4 + bs > length:
            return TRUNCATED, n
        n += 1
        o += 4 + bs
    return o, n


def _guess(raw, length, begin, end, n_ref):
    for o in range(begin, end):
        if plausible(raw, o, n_ref, length):
            return o
    return end


class _Walk:
    """the state of sk_bam_walk_dev; order "before": every lane reads its predecessor's exit before any lane of the launch writes
    (the lanes of one wave); "after": the blocks are taken in order and see what the ones before them wrote"""

    def __init__(self, raw, first, ends, n_ref, order, length=None):
        self.raw, self.first, self.ends, self.n_ref, self.order = raw, first, [int(e) for e in ends], n_ref, order
        self.length = len(raw) if length is None else length
        self.n = len(self.ends)
        self.begin = [0] + self.ends[:-1]
        self.entry = [max(b, first) for b in self.begin]
        self.exit, self.nrec = [0] * self.n, [0] * self.n
        for c in range(self.n):
            self.walk(c)

    def walk(self, c):
        self.exit[c], self.nrec[c] = walk_one(self.raw, self.length, self.entry[c], self.ends[c])

    def guess_round(self, cache=None):
        seen = list(self.exit) if self.order == "before" else self.exit
        for c in range(1, self.n):
            want = seen[c - 1]
            if want < TRUNCATED and self.entry[c] == max(want, self.first):
                continue
            if cache is not None and c in cache:
                self.entry[c] = cache[c]
            else:
                self.entry[c] = _guess(self.raw, self.length, max(self.begin[c], self.first), self.ends[c], self.n_ref)
                if cache is not None:
                    cache[c] = self.entry[c]
            self.walk(c)

    def fix_round(self):
        seen = list(self.exit) if self.order == "before" else self.exit
        changed = 0
        for c in range(1, self.n):
            want = seen[c - 1]
            if want >= TRUNCATED:
                continue
            want = max(want, self.first)
            if self.entry[c] == want:
                continue
            self.entry[c] = want
            self.walk(c)
            changed += 1
        return changed


def guessed_entries(raw, first, ends, n_ref, length=None, cache=None):
    """entry[] behind the first walk and the guess, before any fix round"""
    w = _Walk(raw, first, ends, n_ref, "before", length)
    w.guess_round(cache)
    return w.entry


def simulate(raw, first, ends, n_ref, order, max_rounds=100000, length=None, cache=None):
    """sk_bam_walk_dev restated: dict(verified, n_records, rounds, entry, nrec).  cache: {block: its guess}, shared between runs
    over one stream, length and n_ref (a block's guess depends on nothing else)"""
    w = _Walk(raw, first, ends, n_ref, order, length)
    r = 1
    while True:
        if r == 1:
            w.guess_round(cache)
        if w.fix_round() == 0:
            break
        if r >= max_rounds:
            return dict(verified=False, n_records=0, rounds=r, entry=w.entry, nrec=w.nrec)
        r += 1
    ok = all(x < TRUNCATED for x in w.exit) and max(w.exit[-1], first) == w.length
    return dict(verified=ok, n_records=sum(w.nrec) if ok else 0, rounds=r, entry=w.entry, nrec=w.nrec)


# ---- the builder ----
def aux_bc(tag, data):
    """a B:C array (rm.aux_b writes B:S)"""
    return tag + b"BC" + struct.pack("<I", len(data)) + data


def fake(tid, flag, size=38):
    """a well-formed record of `size` bytes: name "d", no CIGAR, no bases, zeros behind the name"""
    name = b"d\0"
    body = struct.pack("<iiBBHHHiiii", tid, 7, len(name), 0, 4680, 0, flag, 0, tid, 7, 9) + name
    return struct.pack("<I", size - 4) + body + bytes(size - 4 - len(body))


def qual_host(name, flag, tid, pos, payload, seed):
    """a record whose quality bytes are `payload` (the last bytes of the record); no CIGAR"""
    rnd = random.Random(seed)
    nm = name + b"\0"
    body = struct.pack("<iiBBHHHiiii", tid, pos, len(nm), 30, 4680, 0, flag, len(payload), tid, pos + 50, 150) + nm
    body += bytes(rnd.getrandbits(8) for _ in range((len(payload) + 1) // 2)) + payload
    return struct.pack("<i", len(body)) + body


class Decoy:
    """at: the index of the real record that hosts it.  Payload: `lead` zeros, `n_fakes` fakes, `after`, `tail` zeros.  The block that
    is to be fooled begins `gap` bytes before the first fake and ends `tail_cut` bytes behind `after` (None: at the next decoy's
    block); `tiny`: sizes of further blocks behind it.  land: where the last fake's block_size makes the chain go on:
    None (the fakes keep their 38 bytes), "host end", ("record", index, delta) or ("decoy", index).  pin: the fooled block's index.
    expect: what outcome() must say of it."""

    def __init__(self, at, n_fakes=3, tid=0, lead=300, gap=40, tail=200, tail_cut=100, after=b"", land=None, where="aux", tiny=(), pin=None,
                 expect=None):
        self.at, self.n_fakes, self.tid, self.lead, self.gap, self.tail, self.tail_cut = at, n_fakes, tid, lead, gap, tail, tail_cut
        self.after, self.land, self.where, self.tiny, self.pin, self.expect = after, land, where, tuple(tiny), pin, expect

    def payload(self):
        fakes = b"".join(fake(self.tid, DECOY_FLAGS[k % 2]) for k in range(self.n_fakes))
        return bytes(self.lead) + fakes + self.after + bytes(self.tail)

    def fools(self, n_ref):
        return n_ref < 0 or self.tid < n_ref


class Case:
    pass


def real_record(i, rnd):
    name = b"r%d" % i if i % 7 else b"r%d/1 tail%d" % (i, i)
    return rm.record(name, rnd.choice([0, 1, 20, 50, 100, 151]), flag=rnd.choice(REAL_FLAGS), tid=rnd.randrange(N_REF), pos=rnd.randrange(3500), seed=i)


def build(name, n_records, decoys, piece=1000, seed=1):
    """the case: raw, first, ends, decoys (with .start, .end, .F, .block), starts and recs (of the real records), n_real"""
    rnd = random.Random(seed)
    by_at = {d.at: d for d in decoys}
    assert len(by_at) == len(decoys)
    raw = bytearray(rm.header(TEXT, REFS))
    first = len(raw)
    starts, lens = [], []
    for i in range(n_records):
        starts.append(len(raw))
        d = by_at.get(i)
        if d is None:
            raw += real_record(i, rnd)
            lens.append(len(raw) - starts[-1])
            continue
        p = d.payload()
        flag, tid, pos = rnd.choice(REAL_FLAGS), rnd.randrange(N_REF), rnd.randrange(3500)
        if d.where == "aux":
            rec = rm.record(b"host%d" % i, 10, flag=flag, tid=tid, pos=pos, aux=aux_bc(b"ZD", p), seed=i)
        else:
            rec = qual_host(b"host%d" % i, flag, tid, pos, p, seed=i)
        assert rec.endswith(p)
        raw += rec
        lens.append(len(rec))
        d.host_end = len(raw)
        d.start = d.host_end - len(p) + d.lead
        d.end = d.start + 38 * d.n_fakes + len(d.after)
        d.F = d.start - d.gap
        d.E = None if d.tail_cut is None else d.end + d.tail_cut
        assert d.gap <= d.lead and (d.E is None or d.E + sum(d.tiny) < d.host_end)
    decoys = sorted(decoys, key=lambda d: d.start)
    for d in decoys:                                     # where the last fake says the next record begins
        if d.land is None:
            continue
        last = d.start + 38 * (d.n_fakes - 1)
        to = d.host_end if d.land == "host end" else starts[d.land[1]] + d.land[2] if d.land[0] == "record" else by_at[d.land[1]].start
        assert to >= d.end
        struct.pack_into("<I", raw, last, to - last - 4)
    # the block ends
    ends, prev, fill = [], 0, True
    for d in decoys:
        if d.pin is not None:
            m = d.pin - 1 - len(ends)
            assert 0 <= m < d.F - prev, (name, d.pin, len(ends))
            ends += [prev + (d.F - prev) * j // (m + 1) for j in range(1, m + 1)]
        elif fill:
            ends += list(range(prev + piece, d.F, piece))
        assert d.F > prev
        ends.append(d.F)
        prev, fill = d.F, d.E is not None
        if d.E is not None:
            ends.append(d.E)
            prev = d.E
        for t in d.tiny:
            prev += t
            ends.append(prev)
    ends += list(range(prev + piece, len(raw), piece)) + [len(raw)]
    assert all(a < b for a, b in zip(ends, ends[1:]))
    for d in decoys:
        d.block = ends.index(d.F) + 1
        assert d.pin is None or d.block == d.pin
    c = Case()
    c.name, c.raw, c.first, c.ends, c.decoys, c.starts, c.n_real = name, bytes(raw), first, ends, decoys, starts, n_records
    c.recs = [c.raw[s:s + n] for s, n in zip(starts, lens)]              # the real records' bytes, as the builder laid them down
    assert record_starts(c.raw, first) == starts
    return c


def block_of(ends, o):
    """the block that holds stream offset o"""
    lo, hi = 0, len(ends) - 1
    while lo < hi:
        mid = (lo + hi) // 2
        if ends[mid] > o:
            hi = mid
        else:
            lo = mid + 1
    return lo


def outcome(case, d, guessed):
    """what the walk from the fooled block's guess comes to: "bad record", "truncated", "rejoin" (the plain exit, from a wrong
    entry), or ("hop", blocks ahead, "record start" | "decoy start" | "inside")"""
    ex, _ = walk_one(case.raw, len(case.raw), guessed[d.block], case.ends[d.block])
    if ex == BAD_RECORD:
        return "bad record"
    if ex == TRUNCATED:
        return "truncated"
    plain = plain_entries(case.raw, case.first, case.ends) + [len(case.raw)]
    if ex == plain[d.block + 1]:
        return "rejoin"
    where = "record start" if ex in set(case.starts) else "decoy start" if ex in {x.start for x in case.decoys} else "inside"
    return ("hop", block_of(case.ends, ex) - d.block, where)


# ---- the named cases ----
def _rec_in_block(case_ends, starts, block, which):
    """the index of the first (0) or last (-1) real record that begins in `block`, which must hold two at least"""
    lo = case_ends[block - 1]
    inside = [i for i, s in enumerate(starts) if lo <= s < case_ends[block]]
    assert len(inside) >= 2
    return inside[which]


def _hop_case(name, n_records, specs, where="aux", seed=3, piece=1000):
    """specs: [(host record, blocks ahead, landing)]; landing "record start" (the block's last), "inside" (8 bytes into it) or
    ("decoy", host record).  Two passes: the layout does not depend on where the last fakes point."""
    mk = lambda land: [Decoy(at, land=land(k), where=where, expect=None) for k, (at, _, _) in enumerate(specs)]
    probe = build(name, n_records, mk(lambda k: None), piece, seed)
    lands = []
    for d, (at, k, landing) in zip(sorted(probe.decoys, key=lambda x: x.at), specs):
        if isinstance(landing, tuple):
            lands.append(landing)
        else:
            j = _rec_in_block(probe.ends, probe.starts, d.block + k, -1)
            lands.append(("record", j, 0 if landing == "record start" else 8))
    case = build(name, n_records, mk(lambda k: lands[k]), piece, seed)
    at_of = {d.at: d for d in case.decoys}
    for d, (at, k, landing) in zip(sorted(case.decoys, key=lambda x: x.at), specs):
        if isinstance(landing, tuple):                  # (a relay lands where the other decoy lies: the distance follows from the layout)
            d.expect = ("hop", block_of(case.ends, at_of[landing[1]].start) - d.block, "decoy start")
        else:
            d.expect = ("hop", k, landing)
    assert case.ends == probe.ends
    return case


def cases():
    """{name: case}.  Every case is run with the header's reference count and with -1."""
    out = {}

    def add(c):
        out[c.name] = c
    add(build("rejoin", 90, [Decoy(20, land="host end", gap=5, expect="rejoin"), Decoy(55, n_fakes=4, land="host end", gap=250, expect="rejoin")]))
    add(build("rejoin-qual", 90, [Decoy(30, land="host end", where="qual", gap=17, expect="rejoin")], seed=2))
    add(build("garbage", 120, [Decoy(25, gap=3, expect="bad record"), Decoy(70, n_fakes=5, gap=120, expect="bad record")], seed=4))
    add(build("garbage-qual", 90, [Decoy(40, where="qual", gap=64, expect="bad record")], seed=5))
    add(build("truncated", 90, [Decoy(35, after=b"\xff\xff\xff\x0f", gap=33, expect="truncated")], seed=6))
    # hops over blocks of about 1 KB: one and three blocks ahead, and a relay (to another decoy, from there three blocks more)
    add(_hop_case("hop", 200, [(15, 1, "record start"), (60, 3, "inside"), (110, None, ("decoy", 118)), (118, 3, "record start")]))
    add(_hop_case("long-hop", 1100, [(8, 110, "record start")], seed=7))
    add(_hop_case("long-hop-qual", 1100, [(8, 70, "inside")], where="qual", seed=8))
    # the file's last record: the second, and the third, fake ends where the stream ends
    add(build("stream-end-2", 60, [Decoy(59, n_fakes=2, tail=0, tail_cut=None, gap=9, expect="rejoin")], seed=9))
    add(build("stream-end-3", 60, [Decoy(59, n_fakes=3, tail=0, tail_cut=None, gap=130, expect="rejoin")], seed=10))
    # reference ids the header does not have: fools the guess only when it is not told the count
    # (their blocks run on to real records, so that a guess that is not fooled finds the plain entry)
    add(build("refs", 90, [Decoy(30, tid=N_REF, gap=21, tail_cut=None, expect="bad record"),
                           Decoy(60, tid=N_REF, land="host end", gap=77, tail_cut=None, expect="rejoin")], seed=11))
    # two fooled blocks in a row (the first hands on a bad exit), and a fooled block followed by blocks of a few bytes
    add(build("neighbours", 120, [Decoy(30, tail_cut=None, expect="bad record"), Decoy(31, land="host end", expect="rejoin"),
                                  Decoy(80, land="host end", tail=300, tail_cut=20, tiny=(3, 5, 1, 7, 4, 2, 9, 3), expect="rejoin")], seed=12))
    # where the fix kernel's wave and workgroup change: fooled blocks 63, 64 and 255, 256 (small blocks)
    add(build("wave-edge", 330, [Decoy(60, tail_cut=None, pin=63, expect="bad record"), Decoy(61, land="host end", pin=64, expect="rejoin"),
                                 Decoy(240, land="host end", tail_cut=None, pin=255, expect="rejoin"), Decoy(241, pin=256, expect="bad record")],
              piece=150, seed=13))
    return out


FILE_CASES = ("rejoin", "garbage", "truncated", "hop", "stream-end-2", "stream-end-3", "refs", "neighbours")     # B:C hosts only, at most 40 blocks
BROKEN_OF = ("garbage", "hop", "long-hop")


def broken(case):
    """[(what, raw, length)]: the last real record given block_size 31, and the stream cut 3 bytes short; the decoys stay intact"""
    bad = bytearray(case.raw)
    struct.pack_into("<I", bad, case.starts[-1], 31)
    return [("block_size 31", bytes(bad), len(bad)), ("cut short", case.raw, len(case.raw) - 3)]


def aimed(case, n_ref):
    """the blocks the case means to fool when the guess is told n_ref references"""
    return [d.block for d in case.decoys if d.fools(n_ref)]


# ---- the densest blocks ----
def dense_stream(n_blocks=3):
    """records of 36 bytes (block_size 32, no name) over blocks of 65 536 bytes behind a short first block: the first dense block's
    entry is its 5th byte, so it holds 1 821 record starts and the last lies 65 520 bytes behind the entry: (raw, first, ends, recs)"""
    hdr = rm.header(TEXT, REFS)
    first = len(hdr)
    rnd = random.Random(21)
    front_end = first + 36 * 9 - 4                       # the front block ends 4 bytes short of a record's end
    total = (front_end + 65536 * n_blocks - first) // 36 + 1
    recs, parts = [], []
    for i in range(total):
        flag, tid = rnd.choice(REAL_FLAGS), rnd.randrange(-1, N_REF)
        mtid = tid if rnd.random() < 0.8 else rnd.randrange(-1, N_REF)
        tlen = rnd.choice([0, 1, -1, 170, -170, 5000, 5001, -(1 << 31), (1 << 31) - 1, rnd.randrange(-6000, 6000)])
        parts.append(struct.pack("<IiiBBHHHiiii", 32, tid, i, 0, 60, 4680, 0, flag, 0, mtid, i + 5, tlen))
        recs.append(dict(flag=flag, refID=tid, next_refID=mtid, tlen=tlen))
    raw = hdr + b"".join(parts)
    ends = [front_end + 65536 * k for k in range(n_blocks + 1)]
    if ends[-1] >= len(raw):
        ends.pop()
    ends.append(len(raw))
    return raw, first, ends, recs


def dense_file_records(n_blocks=4):
    """records of 38 bytes (name "a", no CIGAR, no bases) for `n_blocks` blocks of 65 536 bytes: 1 725 record starts in a block"""
    rnd = random.Random(22)
    out = []
    for i in range((65536 * n_blocks) // 38):
        tid = rnd.randrange(N_REF)
        body = struct.pack("<iiBBHHHiiii", tid, rnd.randrange(3500), 2, rnd.randrange(61), 4680, 0, rnd.choice(REAL_FLAGS), 0, tid, rnd.randrange(3500),
                           rnd.choice([0, 150, -150, 7, 4999, 5001])) + b"a\0"
        out.append(struct.pack("<i", len(body)) + body)
    return out


# ---- the fields the file tests' models ask for ----
def read_dicts(raw):
    """every record as the dict tests/test_gpu_bam_reads.py's model reads: name, flag, codes, qual"""
    out = []
    for rec in rm.records(raw):
        l_name, n_cigar, flag, l_seq = rec[12], struct.unpack_from("<H", rec, 16)[0], struct.unpack_from("<H", rec, 18)[0], struct.unpack_from("<i", rec, 20)[0]
        at = 36 + l_name + 4 * n_cigar
        packed = rec[at:at + (l_seq + 1) // 2]
        codes = [(packed[k >> 1] >> (0 if k & 1 else 4)) & 15 for k in range(l_seq)]
        out.append(dict(name=rec[36:36 + l_name - 1], flag=flag, codes=codes, qual=list(rec[at + (l_seq + 1) // 2:at + (l_seq + 1) // 2 + l_seq])))
    return out
