"""Two plain-Python statements of `sam mark duplicates` (src/sam_mark_duplicates.rs) over raw BAM bytes, on tests/bam_rewrite_model.py's
reader and writer, and a generator of position-sorted inputs the command serves.

literal() follows the reference's loop line by line: the FIFO deque, find_clusters + flush_reads every 1000 records, at a change of tid
and at the end, and the partial output and exit code when a record stops the loop.
grouped() is the statement the device path rests on: a group is (run of equal tid in file order, start_pos, strand); per group, in file
order, the first unassigned mapped read is a seed, every later unassigned read of the group that is compatible WITH THE SEED joins it,
all get 0x400 and the member with the largest l_seq (the earliest on a tie) has it cleared."""
import random
import struct

from tests import bam_rewrite_model as rm
from tests.bam_rewrite_model import EOF_BLOCK, Stop, aux_a, aux_b, aux_h, aux_i, aux_z, members, out_header, records, write  # noqa: F401

MSG_SECONDARY = b"ERROR: BAM file contains secondary or supplementary reads. These are not currently supported.\n"
MSG_UNSORTED = b"ERROR: Input BAM file is not coordinate sorted.\n"
INT32_MIN = -(1 << 31)
U32_MAX = 0xFFFFFFFF


# ---- one record's fields ----
def core(rec):
    """tid, pos, l_read_name, n_cigar, flag, l_seq, tlen"""
    tid, pos = struct.unpack_from("<ii", rec, 4)
    n_cigar, flag, l_seq = struct.unpack_from("<HHi", rec, 16)
    (tlen,) = struct.unpack_from("<i", rec, 32)
    return tid, pos, rec[12], n_cigar, flag, l_seq, tlen


def find_rx(aux):
    """the value of the first RX field when its type is Z or H, else None (bam_aux_get: the walk stops, not finding it, where the aux
    data stop parsing)"""
    o, n = 0, len(aux)
    while o + 3 <= n:
        tag, ty = aux[o:o + 2], aux[o + 2:o + 3]
        v = o + 3
        if ty in b"AcC":
            e = v + 1
        elif ty in b"sS":
            e = v + 2
        elif ty in b"iIf":
            e = v + 4
        elif ty in b"ZH":
            z = aux.find(b"\0", v)
            if z < 0:
                return None
            e = z + 1
        elif ty == b"B":
            if v + 5 > n:
                return None
            es = {b"c": 1, b"C": 1, b"s": 2, b"S": 2, b"i": 4, b"I": 4, b"f": 4}.get(aux[v:v + 1])
            if not es:
                return None
            e = v + 5 + struct.unpack_from("<I", aux, v + 1)[0] * es
        else:
            return None
        if e > n:
            return None
        if tag == b"RX":
            return aux[v:e - 1] if ty in b"ZH" else None
        o = e
    return None


def end_pos(rec):
    """cigar().end_pos(): pos plus the lengths of M D N = X; Stop(101) where cigar() panics (an operation code above 8)"""
    tid, pos, lo, nc, flag, l_seq, tlen = core(rec)
    e = pos
    for k in range(nc):
        (op,) = struct.unpack_from("<I", rec, 36 + lo + 4 * k)
        if op & 15 > 8:
            raise Stop(101)
        if op & 15 in (0, 2, 3, 7, 8):
            e += op >> 4
    return e


def signature(rec, ignore_umi):
    """:72-91 — (start_pos, strand, fraglen, umi, mapped)"""
    tid, pos, lo, nc, flag, l_seq, tlen = core(rec)
    unmapped, reverse = bool(flag & 4), bool(flag & 16)
    start = 0 if unmapped else (end_pos(rec) & U32_MAX) if reverse else pos & U32_MAX
    umi, fraglen = b"", 0
    if not unmapped:
        if not ignore_umi:
            umi = find_rx(rec[36 + lo + 4 * nc + (l_seq + 1) // 2 + l_seq:]) or b""
        if not umi:
            fraglen = min(abs(tlen), 65535)
    return start, not reverse, fraglen, umi, not unmapped


def umi_matches(a, b):
    """:169-179"""
    if not a or not b:
        return True
    if len(a) != len(b):
        return False
    return sum(1 for x, y in zip(a, b) if not (x == y or x == 78 or y == 78)) <= 1


def with_flag(rec, flag):
    return rec[:18] + struct.pack("<H", flag) + rec[20:]


def summary(dups, total):
    pct = "NaN" if total == 0 else "%.1f" % (dups / total * 100.0)
    return ("%d / %d (%s%%) reads were marked as duplicates.\n" % (dups, total, pct)).encode()


# ---- the reference's loop ----
class _Read:
    __slots__ = ("start_pos", "strand", "ready", "fraglen", "umi", "rec", "flag", "pos", "l_seq")


def _find_clusters(reads, curr_pos):
    n = len(reads)
    for k in range(n):
        rk = reads[k]
        if rk.ready:
            continue
        if rk.start_pos >= curr_pos:
            continue
        best, best_score = rk, rk.l_seq
        rk.flag |= 0x400
        rk.ready = True
        for j in range(k + 1, n):
            rj = reads[j]
            if rj.ready:
                continue
            if rj.pos > rk.start_pos:
                break
            if rj.start_pos != rk.start_pos:
                continue
            if rj.strand != rk.strand:
                continue
            if rj.fraglen > 0 and rk.fraglen > 0 and rj.fraglen != rk.fraglen:
                continue
            if not umi_matches(rj.umi, rk.umi):
                continue
            rj.flag |= 0x400
            rj.ready = True
            if rj.l_seq > best_score:
                best_score, best = rj.l_seq, rj
        best.flag &= ~0x400


def _flush_reads(out, reads):
    i = dups = 0
    while i < len(reads) and reads[i].ready:
        if reads[i].flag & 0x400:
            dups += 1
        out.append(with_flag(reads[i].rec, reads[i].flag))
        i += 1
    del reads[:i]
    return dups


def literal(raw, ignore_umi=False):
    """(inflated output, exit code, stderr): src/sam_mark_duplicates.rs:46-114.  A stopping record leaves what flush_reads wrote before it."""
    out = [out_header(raw)]
    total = dups = 0
    prev_pos, prev_chr = 0, -1
    reads = []
    for rec in records(raw):
        tid, pos, lo, nc, flag, l_seq, tlen = core(rec)
        if flag & 0x900:
            return b"".join(out), 255, MSG_SECONDARY
        left_pos = pos & U32_MAX
        if tid != prev_chr:
            _find_clusters(reads, U32_MAX)
            dups += _flush_reads(out, reads)
            assert not reads
            prev_chr = tid
        elif left_pos < prev_pos:
            return b"".join(out), 255, MSG_UNSORTED
        prev_pos = left_pos
        try:
            start, strand, fraglen, umi, mapped = signature(rec, ignore_umi)
        except Stop as s:
            return b"".join(out), s.code, b"panicked"
        r = _Read()
        r.start_pos, r.strand, r.ready, r.fraglen, r.umi, r.rec, r.flag, r.pos, r.l_seq = start, strand, not mapped, fraglen, umi, rec, flag, left_pos, l_seq
        reads.append(r)
        total += 1
        if total % 1000 == 0:
            dups += _flush_reads(out, reads)
            _find_clusters(reads, left_pos)
    _find_clusters(reads, U32_MAX)
    dups += _flush_reads(out, reads)
    assert not reads
    return b"".join(out), 0, summary(dups, total)


# ---- the sort-and-greedy statement ----
def served(raw):
    """is the file one the grouped statement covers: no stopping record, and 0 <= pos, end_pos <= INT32_MAX for every mapped read"""
    prev = None
    for rec in records(raw):
        tid, pos, lo, nc, flag, l_seq, tlen = core(rec)
        if flag & 0x900:
            return False
        if prev is not None and prev[0] == tid and (pos & U32_MAX) < (prev[1] & U32_MAX):
            return False
        prev = (tid, pos)
        if not flag & 4:
            if pos < 0:
                return False
            if flag & 16:
                try:
                    if end_pos(rec) > 0x7FFFFFFF:
                        return False
                except Stop:
                    return False
    return True


def grouped_flags(raw, ignore_umi=False):
    """every record's output flag by the grouped statement (the file must be served())"""
    recs = list(records(raw))
    flags = [core(r)[4] for r in recs]
    groups, run, prev_tid = {}, -1, None
    for k, rec in enumerate(recs):
        tid = core(rec)[0]
        if k == 0 or tid != prev_tid:
            run += 1
        prev_tid = tid
        start, strand, fraglen, umi, mapped = signature(rec, ignore_umi)
        if mapped:
            groups.setdefault((run, start, strand), []).append((k, fraglen, umi, core(rec)[5]))
    for mem in groups.values():                                       # (file order inside a group: k ascends)
        todo = mem
        while todo:
            _, sf, su, _ = todo[0]
            join = [m for m in todo if not (m[1] > 0 and sf > 0 and m[1] != sf) and umi_matches(m[2], su)]
            assert join[0] is todo[0]
            best = max(join, key=lambda m: (m[3], -m[0]))
            for m in join:
                flags[m[0]] = flags[m[0]] | 0x400 if m is not best else flags[m[0]] & ~0x400
            taken = {m[0] for m in join}
            todo = [m for m in todo if m[0] not in taken]
    return recs, flags


def grouped(raw, ignore_umi=False):
    """(inflated output, 0, stderr) as literal() gives it for a served file"""
    recs, flags = grouped_flags(raw, ignore_umi)
    out = [out_header(raw)] + [with_flag(r, f) for r, f in zip(recs, flags)]
    return b"".join(out), 0, summary(sum(1 for f in flags if f & 0x400), len(recs))


# ---- inputs ----
M, I, D, N, S, H, P, EQ, X = range(9)


def rec(name, tid, pos, flag=0, cigar=((M, 20),), l_seq=None, tlen=0, aux=b"", mtid=None, mpos=0, mapq=60):
    """one record's bytes (block_size included); l_seq defaults to what the CIGAR's M I S = X operations consume"""
    if l_seq is None:
        l_seq = sum(ln for op, ln in cigar if op in (M, I, S, EQ, X))
    nm = name + b"\0"
    body = struct.pack("<iiBBHHHiiii", tid, pos, len(nm), mapq, 4680, len(cigar), flag, l_seq, tid if mtid is None else mtid, mpos, tlen)
    body += nm + b"".join(struct.pack("<I", (ln << 4) | op) for op, ln in cigar)
    body += bytes([0x12, 0x48, 0x84, 0x21][k & 3] for k in range((l_seq + 1) // 2)) + bytes(20 + (k * 7) % 21 for k in range(l_seq)) + aux
    return struct.pack("<i", len(body)) + body


def ref_len(cigar):
    return sum(ln for op, ln in cigar if op in (M, D, N, EQ, X))


# CIGARs with every operation: (operations, l_seq they consume) — end_pos differs from pos + l_seq
CIGARS = [((M, 20),), ((S, 3), (M, 17)), ((M, 10), (I, 2), (M, 8)), ((M, 10), (D, 5), (M, 10)), ((M, 8), (N, 300), (M, 12)),
          ((H, 4), (M, 20), (H, 2)), ((M, 10), (P, 1), (I, 1), (M, 9)), ((EQ, 12), (X, 1), (EQ, 7)), ((S, 2), (EQ, 10), (D, 1), (X, 2), (M, 6), (S, 5)),
          ((M, 30),), ((M, 50),), ((S, 10), (M, 40))]
TLENS = [0, 100, -100, 250, -250, 70000, -70001, 65535, 65536, INT32_MIN, 0x7FFFFFFF]
BASES = b"ACGT"


def _umi(rnd, n):
    return bytes(rnd.choice(BASES) for _ in range(n))


def _mutate(rnd, u, k):
    """u with k positions changed to another base"""
    u = bytearray(u)
    for p in rnd.sample(range(len(u)), k):
        u[p] = rnd.choice([b for b in BASES if b != u[p]])
    return bytes(u)


def _aux_kinds(rnd, fam):
    """the aux data of one read of a group whose UMI family is `fam`"""
    kind = rnd.randrange(16)
    pre = [b"", aux_i(b"NM", 1), aux_b(b"ZB", [1, 2, 3]) + aux_a(b"XA", b"Q"), aux_z(b"MD", b"20")][rnd.randrange(4)]
    if kind < 5:
        return pre + aux_z(b"RX", fam)
    if kind < 8:
        return pre + aux_z(b"RX", _mutate(rnd, fam, 1))
    if kind == 8:
        return pre + aux_z(b"RX", _mutate(rnd, fam, 2))
    if kind == 9:
        u = bytearray(_mutate(rnd, fam, rnd.randrange(0, 3)))
        u[rnd.randrange(len(u))] = 78                                   # an N
        return pre + aux_z(b"RX", bytes(u))
    if kind == 10:
        return pre + aux_z(b"RX", fam[:-1])                             # another length
    if kind == 11:
        return pre + aux_z(b"RX", b"")                                  # empty: the fragment length counts
    if kind == 12:
        return pre + aux_h(b"RX", fam)                                  # type H
    if kind == 13:
        return pre + aux_i(b"RX", 7) + aux_z(b"RX", fam)               # the first RX has type i: no UMI
    if kind == 14:
        return pre + aux_z(b"RX", fam) + aux_z(b"RX", _umi(rnd, len(fam)))   # only the first counts
    return pre                                                          # no RX


def sorted_records(seed=1, n=3000, big=1100, umi_share=0.7):
    """about n position-sorted records the command serves: several tid runs with a return to an earlier tid and an unmapped tail; forward
    and reverse reads (CIGARS) that share a start_pos; groups of 1, 2, 63-65 and `big` members; every UMI and tlen kind; l_seq ties and
    a later, longer member; unmapped reads at their mate's position, some with 0x400; mapped reads arriving with 0x400"""
    rnd = random.Random(seed)
    out = []
    sizes = [1] * 12 + [2] * 6 + [3, 4, 5, 7, 12, 30] + [63, 64, 65]
    runs = [0, 1, 0, 2, 1]                                              # tids in file order: 0 and 1 come back
    per_run = max(1, n // len(runs))
    gid = 0
    big_left = 1 if big else 0
    for tid in runs:
        frags, count = [], 0
        start = rnd.randrange(400, 600)
        while count < per_run:
            start += rnd.choice([0, 0, 1, 1, 2, 5, 40])
            m = rnd.choice(sizes)
            if big_left and count > per_run // 3:
                m, big_left = big, 0
            gid += 1
            fam = _umi(rnd, rnd.choice([6, 8, 8, 9, 12, 13]))
            use_umi = rnd.random() < umi_share
            strands = [rnd.random() < 0.5] * m if rnd.random() < 0.6 else [rnd.random() < 0.5 for _ in range(m)]
            for i in range(m):
                cg = rnd.choice(CIGARS)
                reverse = strands[i]
                pos = start - ref_len(cg) if reverse else start
                if pos < 0:
                    reverse, pos = False, start
                flag = (16 if reverse else 0) | rnd.choice([0, 1 | 0x40, 1 | 0x80, 0x400, 1 | 0x20 | 0x80 | 0x400, 0x200])
                aux = _aux_kinds(rnd, fam) if use_umi else [b"", aux_i(b"NM", 2), aux_i(b"RX", 3)][rnd.randrange(3)]
                frags.append((pos, rnd.random(), rec(b"g%d.%d" % (gid, i), tid, pos, flag, cg, tlen=rnd.choice(TLENS if rnd.random() < 0.5 else TLENS[:3]), aux=aux)))
            count += m
            if rnd.random() < 0.08:                                     # an unmapped read at its mate's position
                frags.append((start, rnd.random(), rec(b"u%d" % gid, tid, start, 4 | 1 | rnd.choice([0, 0x400, 16]), (), l_seq=20, aux=aux_z(b"RX", fam))))
                count += 1
        frags.sort(key=lambda f: (f[0], f[1]))                          # by pos; the order inside one pos is shuffled
        out += [f[2] for f in frags]
    for i in range(rnd.randrange(3, 40)):                               # the unmapped tail
        out.append(rec(b"tail%d" % i, -1, -1, 4 | rnd.choice([0, 1, 0x400]), (), l_seq=20, mtid=-1, mpos=-1, aux=rnd.choice([b"", aux_z(b"RX", b"ACGT")])))
    return out


def chain_records():
    """A~B, B~C, A!~C (one mismatch each, two between A and C) at one start_pos, in every file order, forward and reverse; the greedy
    takes the seed's neighbours only"""
    import itertools
    umis = {"A": b"AAAAAAAA", "B": b"AAAAAAAC", "C": b"AAAAAAGC"}
    out, pos = [], 1000
    for order in itertools.permutations("ABC"):
        for reverse in (False, True):
            for k, who in enumerate(order):
                cg = ((M, 20 + k),)
                out.append(rec(b"chain%s.%s" % ("".join(order).encode(), who.encode()), 0, pos - ref_len(cg) if reverse else pos, 16 if reverse else 0, cg,
                               aux=aux_z(b"RX", umis[who])))
            pos += 100
    out.sort(key=lambda r: core(r)[1])                                  # (stable: the order inside one pos stays)
    return out
