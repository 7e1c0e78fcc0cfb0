"""A plain-Python statement of `sam trim qnames`, `sam tags from qname` and `sam qname from tags` (src/sam_trim_qnames.rs:20-30,
src/sam_tags_from_qname.rs:33-52, src/sam_qname_from_tags.rs:32-41) over raw BAM bytes, and a BAM writer with aux fields, a free
header text and @SQ lines (tests/cli_util.write_bam has neither)."""
import random
import struct
import zlib

from tests import bam_spec

OPS = {"trim qnames": 1, "qname from tags": 2, "tags from qname": 3}
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


class Stop(Exception):
    """the reference ends at this record: code 101 (a panic) or 255 (error!)"""

    def __init__(self, code):
        super().__init__(code)
        self.code = code


# ---- aux fields (SAMv1 §4.2.4) ----
def aux_z(tag, val):
    return tag + b"Z" + val + b"\0"


def aux_h(tag, val):
    return tag + b"H" + val + b"\0"


def aux_a(tag, ch):
    return tag + b"A" + ch


def aux_i(tag, v):
    return tag + b"i" + struct.pack("<i", v)


def aux_b(tag, vals):
    return tag + b"BS" + struct.pack("<I", len(vals)) + b"".join(struct.pack("<H", v) for v in vals)


# ---- writer ----
def record(name, l_seq=10, flag=0, tid=0, pos=100, aux=b"", n_cigar=None, seed=0):
    """one record's bytes (block_size included); the bases and qualities are pseudo-random"""
    rnd = random.Random(seed)
    cigar = [(0, l_seq)] if l_seq and n_cigar is None else [(4, 1)] * (n_cigar or 0)
    nm = name + b"\0"
    body = struct.pack("<iiBBHHHiiii", tid, pos, len(nm), rnd.randrange(61), 4680 + rnd.randrange(50), len(cigar), flag, l_seq, tid, pos + 50, 150)
    body += nm + b"".join(struct.pack("<I", (ln << 4) | op) for op, ln in cigar)
    body += bytes(rnd.getrandbits(8) for _ in range((l_seq + 1) // 2)) + bytes(rnd.randrange(42) for _ in range(l_seq)) + aux
    return struct.pack("<i", len(body)) + body


def header(text, refs):
    raw = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(refs))
    for name, ln in refs:
        nb = name + b"\0"
        raw += struct.pack("<i", len(nb)) + nb + struct.pack("<i", ln)
    return raw


def bgzf(raw, piece=0xFF00, level=6, cuts=None):
    """cuts: the stream offsets at which the blocks end (ascending, the last one len(raw)), instead of blocks of `piece` bytes"""
    out = []
    bounds = zip([0] + list(cuts[:-1]), cuts) if cuts is not None else ((o, o + piece) for o in range(0, len(raw), piece))
    assert cuts is None or int(cuts[-1]) == len(raw)
    for lo, hi in bounds:
        data = raw[int(lo):int(hi)]
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        comp = c.compress(data) + c.flush()
        out.append(struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, len(comp) + 25) + comp
                   + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data)))
    return b"".join(out) + EOF_BLOCK


REFS = [(b"chr1", 248956422), (b"chr2", 242193529), (b"chrM", 16569)]
# @SQ lines that match the reference list, NUL padding and extra trailing newlines
TEXT = b"@HD\tVN:1.6\tSO:unsorted\n" + b"".join(b"@SQ\tSN:%s\tLN:%d\n" % r for r in REFS) + b"@PG\tID:x\n\n\n" + b"\0" * 7


def write(path, recs, text=TEXT, refs=REFS, piece=0xFF00, level=6, cuts=None):
    """piece: the inflated bytes of a BGZF block (cuts: where the blocks end instead); level: zlib's (1 writes a large file cheaply, 0 stores)"""
    raw = header(text, refs) + b"".join(recs)
    with open(path, "wb") as f:
        f.write(bgzf(raw, piece, level, cuts))
    return raw


# ---- the model ----
def out_header(raw):
    """Header::from_template + Writer: the text up to its first NUL, trailing '\\n's stripped, one appended if any is left"""
    (l_text,) = struct.unpack_from("<i", raw, 4)
    text = raw[8:8 + l_text].split(b"\0")[0].rstrip(b"\n")
    if text:
        text += b"\n"
    return b"BAM\1" + struct.pack("<i", len(text)) + text + raw[8 + l_text:header_end(raw)]


def header_end(raw):
    (l_text,) = struct.unpack_from("<i", raw, 4)
    o = 8 + l_text
    (n_ref,) = struct.unpack_from("<i", raw, o)
    o += 4
    for _ in range(n_ref):
        (ln,) = struct.unpack_from("<i", raw, o)
        o += 4 + ln + 4
    return o


def records(raw):
    o = header_end(raw)
    while o < len(raw):
        (bs,) = struct.unpack_from("<i", raw, o)
        yield raw[o:o + 4 + bs]
        o += 4 + bs


def first_rx(aux):
    """bam_aux_get(b"RX"): (type, value up to the NUL) of the first RX field, or None"""
    o = 0
    while o + 3 <= len(aux):
        tag, ty = aux[o:o + 2], aux[o + 2:o + 3]
        v = o + 3
        if ty in b"AcC":
            e = v + 1
        elif ty in b"sS":
            e = v + 2
        elif ty in b"iIf":
            e = v + 4
        elif ty in b"ZH":
            e = aux.index(b"\0", v) + 1
        elif ty == b"B":
            (cnt,) = struct.unpack_from("<I", aux, v + 1)
            e = v + 5 + cnt * {b"c": 1, b"C": 1, b"s": 2, b"S": 2, b"i": 4, b"I": 4, b"f": 4}[aux[v:v + 1]]
        else:
            raise ValueError("bad aux type")
        if tag == b"RX":
            return ty, aux[v:e - 1] if ty in b"ZH" else aux[v:e]
        o = e
    return None


def rewrite(rec, op):
    """the record as the command writes it; raises Stop where the reference ends"""
    lo, nc, S = rec[12], struct.unpack_from("<H", rec, 16)[0], struct.unpack_from("<i", rec, 20)[0]
    name, tail = rec[36:36 + lo - 1], rec[36 + lo:]
    app = b""
    if op == "trim qnames":
        t = name.find(b" ")
        if t < 0:
            return rec
        if t < 2:
            raise Stop(101)
        if name[t - 2:t] in (b"/1", b"/2"):
            t -= 2
        new = name[:t]
    elif op == "tags from qname":
        parts = name.split(b" ")
        if len(parts) == 1:
            return rec
        new = parts[0]
        for p in parts[1:]:
            if p.startswith(b"UMI:"):
                app += b"RXZ" + p[4:] + b"\0"
            elif len(p) >= 3 and p[2:3] == b":":
                app += p[:2] + b"Z" + p[3:] + b"\0"
            else:
                try:
                    p.decode()
                except UnicodeDecodeError:
                    raise Stop(101)
                raise Stop(255)
    else:
        rx = first_rx(rec[36 + lo + 4 * nc + (S + 1) // 2 + S:])
        if rx is None or rx[0] not in (b"Z", b"H"):
            return rec
        new = name + b" RX:" + rx[1]
        if len(new) > 254:
            raise Stop(101)
    body = rec[4:12] + bytes([len(new) + 1]) + rec[13:36] + new + b"\0" + tail + app
    return struct.pack("<i", len(body)) + body


def model(raw, op):
    """(inflated output, None) or (inflated output up to the stopping record, exit code)"""
    out = [out_header(raw)]
    for rec in records(raw):
        try:
            out.append(rewrite(rec, op))
        except Stop as s:
            return b"".join(out), s.code
    return b"".join(out), None


def members(data):
    """[(inflated bytes, stored?)] of every BGZF member, checked by bam_spec.bgzf_blocks (BSIZE, CRC32, ISIZE)"""
    raws = list(bam_spec.bgzf_blocks(data))
    kinds, at = [], 0
    while at < len(data):
        (xlen,) = struct.unpack_from("<H", data, at + 10)
        (bsize,) = struct.unpack_from("<H", data, at + 16)
        kinds.append((data[at + 12 + xlen] >> 1) & 3 == 0)
        at += bsize + 1
    return list(zip(raws, kinds))


# ---- inputs ----
def _word(rnd, n, alphabet=b"ACGTNacgt0123456789_:-."):
    return bytes(rnd.choice(alphabet) for _ in range(n))


def served_records(op, n=2500, seed=1):
    """records every one of which the command serves (no stop): names of 1 to 254 bytes, 0 bases up to records over 64 KiB"""
    rnd = random.Random(seed)
    recs = []
    for i in range(n):
        l_seq = rnd.choice([0, 1, 7, 36, 100, 151, 151, 250])
        if i in (5, 1700):
            l_seq = 50000                                       # over 64 KiB: crosses input blocks
        aux = b""
        if op == "trim qnames":
            kind = i % 6
            base = _word(rnd, rnd.randrange(2, 60))
            name = [base, base + b"/1 " + _word(rnd, 5), base + b"/2 " + _word(rnd, 3), base + b"/3 x",
                    _word(rnd, 2) + b" " + _word(rnd, rnd.randrange(0, 8)), _word(rnd, rnd.randrange(1, 255))][kind]
            name = name[:254]
            if b" " in name and name.index(b" ") < 2:
                name = b"ab" + name[2:]
        elif op == "tags from qname":
            parts = [_word(rnd, rnd.randrange(0, 30))]
            for _ in range(rnd.randrange(0, 4)):
                parts.append(rnd.choice([b"UMI:" + _word(rnd, rnd.randrange(0, 12), b"ACGT"), b"UMI:", b"BC:" + _word(rnd, 8, b"ACGT"),
                                         b"XY:", b"a1:" + _word(rnd, 3)]))
            name = b" ".join(parts)
            if len(name) > 254:
                name = parts[0][:254]
            aux = aux_i(b"NM", i) if i % 3 else b""
        else:
            name = _word(rnd, rnd.randrange(1, 200)) if i % 50 else _word(rnd, 250)      # (+ " RX:": 254 bytes)
            room = max(0, 254 - len(name) - 4)
            v = _word(rnd, min(room, rnd.randrange(0, 24)), b"ACGT")
            aux = [b"", aux_z(b"RX", v), aux_h(b"RX", b"0A1B"[:min(4, room)]), aux_a(b"RX", b"Q"), aux_i(b"RX", 7),
                   aux_i(b"NM", 1) + aux_z(b"RX", v) + aux_z(b"RX", b"second"), aux_b(b"ZB", [1, 2, 3]) + aux_z(b"RX", v),
                   aux_z(b"XX", b"nothing")][i % 8]
        recs.append(record(name, l_seq, flag=rnd.choice([0, 1 | 0x40, 1 | 0x80, 0x10, 0x100]), tid=rnd.randrange(-1, 3), aux=aux, seed=i))
    return recs


# records the reference stops at (where the device declines): (op, name, aux)
STOPS = [
    ("trim qnames", b" lead", b""),
    ("trim qnames", b"a rest", b""),
    ("tags from qname", b"read BAD", b""),
    ("tags from qname", b"read UMI:AC ", b""),
    ("tags from qname", b"read  UMI:AC", b""),
    ("tags from qname", b"read \xff\xfe", b""),
    ("qname from tags", b"n" * 240, aux_z(b"RX", b"ACGTACGTACGT")),
]
