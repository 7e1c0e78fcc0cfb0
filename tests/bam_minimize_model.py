"""A plain-Python statement of `sam minimize` (src/sam_minimize.rs:46-82) over raw BAM bytes, on tests/bam_rewrite_model.py's writer,
and a generator of records the command serves."""
import functools
import random
import struct

from tests import bam_rewrite_model as rm
from tests.bam_rewrite_model import EOF_BLOCK, Stop, members, out_header, records, write  # noqa: F401  (what the tests use)

# the valid switch combinations: (read_ids, base_qualities, tags)
COMBOS = {"read-ids": (True, False, False), "tags": (False, False, True), "read-ids+tags": (True, False, True),
          "tags+base-qualities": (False, True, True), "all": (True, True, True)}


def args(combo, fill=None):
    """the command line's switches"""
    ids, bq, tags = COMBOS[combo]
    return (["--read-ids"] if ids else []) + (["--base-qualities"] if bq else []) + (["--tags"] if tags else []) \
        + ([] if fill is None else ["--baseq-fill=%d" % fill])


class Ids:
    """the reference's map: a key that is in it takes the stored id and leaves the map; any other takes the next id and enters it"""

    def __init__(self):
        self.highest, self.map = 0, {}

    def take(self, name):
        slash = name.find(b"/")
        key = name if slash < 0 else name[:slash]
        if key in self.map:
            return self.map.pop(key)
        self.highest += 1
        self.map[key] = self.highest
        return self.highest


def minimize(rec, ids, read_ids, base_qualities, tags, fill=255):
    """the record as the command writes it; raises Stop(101) where rust-htslib's cigar() panics"""
    lo, nc, S = rec[12], struct.unpack_from("<H", rec, 16)[0], struct.unpack_from("<i", rec, 20)[0]
    name = rec[36:36 + lo - 1]
    if read_ids:
        name = b"%d" % ids.take(name)
    cigar = rec[36 + lo:36 + lo + 4 * nc]
    if any((cigar[4 * k] & 15) > 8 for k in range(nc)):
        raise Stop(101)
    if read_ids and not base_qualities and not tags:                    # set_qname: everything behind the name stays
        rest = rec[36 + lo:]
    else:                                                               # set: CIGAR, the bases re-encoded, the qualities, no aux data
        o = 36 + lo + 4 * nc
        seq = bytearray(rec[o:o + (S + 1) // 2])
        if S & 1:
            seq[-1] &= 0xF0
        qual = bytes([fill]) * S if base_qualities else rec[o + (S + 1) // 2:o + (S + 1) // 2 + S]
        rest = cigar + bytes(seq) + qual
    body = rec[4:12] + bytes([len(name) + 1]) + rec[13:36] + name + b"\0" + rest
    return struct.pack("<i", len(body)) + body


def model(raw, combo, fill=255):
    """(inflated output, None) or (inflated output up to the stopping record, exit code)"""
    read_ids, base_qualities, tags = COMBOS[combo]
    out, ids = [out_header(raw)], Ids()
    for rec in records(raw):
        try:
            out.append(minimize(rec, ids, read_ids, base_qualities, tags, fill))
        except Stop as s:
            return b"".join(out), s.code
    return b"".join(out), None


# ---- inputs ----
def record(name, l_seq=10, aux=b"", seed=0, pad=None, qual=None, cigar_op=None, flag=0, tid=0):
    """bam_rewrite_model.record with a chosen pad nibble (odd l_seq), chosen qualities and a chosen code for the first CIGAR operation"""
    rec = bytearray(rm.record(name, l_seq, flag=flag, tid=tid, aux=aux, seed=seed))
    lo, nc = rec[12], struct.unpack_from("<H", rec, 16)[0]
    o = 36 + lo + 4 * nc
    if pad is not None and l_seq & 1:
        rec[o + l_seq // 2] = (rec[o + l_seq // 2] & 0xF0) | pad
    if qual is not None:
        rec[o + (l_seq + 1) // 2:o + (l_seq + 1) // 2 + l_seq] = bytes([qual]) * l_seq
    if cigar_op is not None and nc:
        rec[36 + lo] = (rec[36 + lo] & 0xF0) | cigar_op
    return bytes(rec)


AUX = [b"", rm.aux_i(b"NM", 3), rm.aux_z(b"RX", b"ACGT") + rm.aux_a(b"XA", b"Q"), rm.aux_b(b"ZB", [1, 2, 3]) + rm.aux_h(b"XH", b"0A1B"),
       rm.aux_z(b"MD", b"100") + rm.aux_i(b"AS", -7) + rm.aux_z(b"XX", b"")]


def served_names(n, seed=1):
    """n names: keys that occur 1 to 5 times, mates adjacent and thousands of records apart, x/1 and x/2, names equal up to the '/' and
    different behind it, a '/' at index 0, lengths 1 to 254, and (n = 25 000) enough distinct keys for ids of 1 to 5 digits"""
    rnd = random.Random(seed)
    names, far = [], []
    k = 0
    while len(names) < n:
        k += 1
        kind = k % 11
        key = b"r%d:" % k + rm._word(rnd, rnd.randrange(0, 20))
        if kind == 0:                                                   # once
            names.append(key)
        elif kind == 1:                                                 # mates adjacent, the same name
            names += [key, key]
        elif kind == 2:                                                 # x/1 and x/2
            names += [key + b"/1", key + b"/2"]
        elif kind == 3:                                                 # equal up to the '/', different behind it; three times
            names += [key + b"/1 lane:" + rm._word(rnd, 4), key + b"/2/extra", key + b"/"]
        elif kind == 4:                                                 # four times, the later two far away
            names += [key, key + b"/2"]
            far += [key + b"/1", key]
        elif kind == 5:                                                 # five times, spread
            names += [key]
            far += [key, key + b"/a", key + b"/b", key]
        elif kind == 6:                                                 # a '/' at index 0: the empty key, many times over the file
            names.append(b"/" + rm._word(rnd, rnd.randrange(0, 9)))
        elif kind == 7:                                                 # a mate thousands of records later
            names.append(key)
            far.append(key + b"/2")
        elif kind == 8:                                                 # long names: up to 254 bytes, the key up to 254 or cut by a '/'
            long = (key + rm._word(rnd, 254))[:rnd.choice([254, 253, 200, 128])]
            names += [long, long[:100] + b"/" + long[101:]]
        elif kind == 9:                                                 # one byte
            names.append(bytes([rnd.choice(b"ABCDEFGHIJKLMNOPQRSTUVWXYZ")]))
        else:                                                           # a key that is a prefix of another key
            names += [key, key + b"x", key + b"/1"]
        if len(far) > 3000:                                             # the far mates arrive in another order
            rnd.shuffle(far)
            names += far[:1500]
            del far[:1500]
    names = names[:n]
    return names


@functools.lru_cache(maxsize=None)
def served_records(n=25000, seed=1):
    """records every one of which the command serves: served_names, l_seq odd and even and 0, two records over 64 KiB, pad nibbles that
    are not 0, aux data of several types and none, qualities that already are 0xFF"""
    rnd = random.Random(seed)
    recs = []
    for i, name in enumerate(served_names(n, seed)):
        l_seq = rnd.choice([0, 1, 7, 36, 100, 151, 151, 250])
        if i in (5, n * 2 // 3):
            l_seq = 50001 if i == 5 else 50000                          # over 64 KiB: crosses input blocks
        recs.append(record(name, l_seq, aux=AUX[i % len(AUX)], seed=i, pad=rnd.choice([None, 0, 5, 15]), qual=0xFF if i % 9 == 0 else None,
                           flag=rnd.choice([0, 1 | 0x40, 1 | 0x80, 0x10, 0x100]), tid=rnd.randrange(-1, 3)))
    return tuple(recs)
