"""A plain-Python statement of `sam subsample` (src/sam_subsample.rs:16-62) over raw BAM bytes, on tests/bam_rewrite_model.py's
reader and writer: the f32 parse of the fraction, the generator (draw d of seed s is splitmix64's d-th output from state s), the loop
with its map, the two stderr lines, and a generator of records the command serves."""
import functools
import random
import re

import numpy as np

from tests import bam_rewrite_model as rm
from tests.bam_rewrite_model import EOF_BLOCK, Stop, members, out_header, records, write  # noqa: F401  (what the tests use)

MASK = (1 << 64) - 1
FRACTION_ERROR = b"ERROR: Subsampling fraction must be between 0 - 1.\n"
UNPAIRED_ERROR = b"ERROR: Only paired end sequencing data supported for now.\n"
SEED_ERROR = b"ERROR: --seed must be an integer between 0 and 18446744073709551615.\n"

# str::parse::<f32>(): a sign, then inf / infinity / nan in any case or a decimal number with at least one digit and an optional exponent
_F32 = re.compile(r"[+-]?(?:(?:inf|infinity|nan)|(?:[0-9]+\.?[0-9]*|\.[0-9]+)(?:[eE][+-]?[0-9]+)?)\Z", re.I)


def parse_fraction(text):
    """the fraction as the command takes it (a numpy.float32), or None: it does not parse, is NaN or lies outside [0, 1]"""
    if not _F32.match(text) or "\n" in text:
        return None
    with np.errstate(over="ignore"):
        f = np.float32(text)                                            # (the nearest f32, as Rust's parse)
    return f if 0.0 <= f <= 1.0 else None


def threshold(fraction):
    """T = floor(fraction * 2^24), the f32 widened exactly"""
    return int(float(np.float32(fraction)) * (1 << 24))


def draw_m(seed, d):
    """the 24 bits of draw number d (1, 2, 3 ..) under `seed`"""
    z = (seed + d * 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    z ^= z >> 31
    return z >> 40


def keep(seed, d, fraction):
    return draw_m(seed, d) <= threshold(fraction)


def flag_of(rec):
    return rec[18] | (rec[19] << 8)


def qname(rec):
    return rec[36:36 + rec[12] - 1]


def decisions(recs, seed, fraction):
    """per record: True kept, False dropped, None passed over (0x800); raises Stop(255) with .done = the decisions so far at a counted
    record without 0x1"""
    T = threshold(fraction)
    keep_mate, out, d = {}, [], 0
    for rec in recs:
        f = flag_of(rec)
        if f & 0x800:
            out.append(None)
            continue
        if not f & 1:
            s = Stop(255)
            s.done = out
            raise s
        name = qname(rec)
        if name in keep_mate:
            k = keep_mate.pop(name)
        else:
            d += 1
            k = draw_m(seed, d) <= T
            keep_mate[name] = k
        out.append(k)
    return out


def summary(kept, total):
    pct = "NaN" if total == 0 else "%.1f" % (kept / total * 100.0)
    return ("Total reads: %d\nKept reads: %d (%s%% of all reads)\n" % (total, kept, pct)).encode()


def model(raw, seed, fraction):
    """(inflated stdout, stderr, exit code, records kept, records counted); at an unpaired record the output so far, its message and 255"""
    recs = list(records(raw))
    try:
        dec, code = decisions(recs, seed, fraction), 0
    except Stop as s:
        dec, code = s.done, s.code
    out = out_header(raw) + b"".join(r for r, k in zip(recs, dec) if k)
    kept, total = sum(1 for k in dec if k), sum(1 for k in dec if k is not None)
    return out, (UNPAIRED_ERROR if code else summary(kept, total)), code, kept, total


# ---- inputs ----
def served_names(n, seed=1):
    """(name, extra flag bits) of n records: names on 1 to 5 records, mates adjacent and thousands of records apart, 0x100 records,
    0x800 records between mates, names of 1 and 254 bytes, names equal up to their last byte, x/1 and x/2 (two keys here)"""
    rnd = random.Random(seed)
    out, far = [], []
    k = 0
    while len(out) < n:
        k += 1
        kind = k % 12
        key = b"r%d:" % k + rm._word(rnd, rnd.randrange(0, 20))
        if kind == 0:                                                   # once
            out.append((key, 0))
        elif kind == 1:                                                 # mates adjacent
            out += [(key, 0x40), (key, 0x80)]
        elif kind == 2:                                                 # x/1 and x/2: two names, two draws
            out += [(key + b"/1", 0x40), (key + b"/2", 0x80)]
        elif kind == 3:                                                 # three times: the third draws anew
            out += [(key, 0x40), (key, 0x80), (key, 0x100)]
        elif kind == 4:                                                 # four times, the later two far away
            out += [(key, 0x40), (key, 0x80)]
            far += [(key, 0x40 | 0x100), (key, 0x80 | 0x100)]
        elif kind == 5:                                                 # five times, spread
            out.append((key, 0x40))
            far += [(key, 0x80), (key, 0x100), (key, 0x100), (key, 0)]
        elif kind == 6:                                                 # a supplementary record between two mates, and one far away
            out += [(key, 0x40), (key, 0x800 | 0x40), (key, 0x80)]
            far.append((key, 0x800))
        elif kind == 7:                                                 # a mate thousands of records later
            out.append((key, 0x40))
            far.append((key, 0x80))
        elif kind == 8:                                                 # 254 bytes, equal up to the last byte
            long = (key + rm._word(rnd, 254))[:253]
            out += [(long + b"a", 0x40), (long + b"b", 0x40), (long + b"a", 0x80)]
            far.append((long + b"b", 0x80))
        elif kind == 9:                                                 # one byte: few names, many records each
            out.append((bytes([rnd.choice(b"ABCDEFGHIJKLMNOPQRSTUVWXYZ")]), 0))
        elif kind == 10:                                                # a name that is a prefix of another
            out += [(key, 0x40), (key + b"x", 0x40), (key + b"x", 0x80), (key, 0x80)]
        else:                                                           # a supplementary record of a name nothing else carries
            out.append((key, 0x800))
        if len(far) > 3000:                                             # the far mates arrive in another order
            rnd.shuffle(far)
            out += far[:1500]
            del far[:1500]
    return out[:n]


@functools.lru_cache(maxsize=None)
def served_records(n=25000, seed=1):
    """records every one of which the command serves (each has 0x1 or 0x800): served_names, l_seq odd and even and 0, two records over
    64 KiB, aux data of several kinds"""
    rnd = random.Random(seed)
    aux = [b"", rm.aux_i(b"NM", 3), rm.aux_z(b"RX", b"ACGT") + rm.aux_a(b"XA", b"Q"), rm.aux_b(b"ZB", [1, 2, 3])]
    recs = []
    for i, (name, bits) in enumerate(served_names(n, seed)):
        l_seq = rnd.choice([0, 1, 7, 36, 100, 151, 151, 250])
        if i in (5, n * 2 // 3):
            l_seq = 50001 if i == 5 else 50000                          # over 64 KiB: crosses input blocks
        recs.append(rm.record(name, l_seq, flag=1 | bits | rnd.choice([0, 0x10, 0x20]), tid=rnd.randrange(-1, 3), aux=aux[i % len(aux)], seed=i))
    return tuple(recs)
