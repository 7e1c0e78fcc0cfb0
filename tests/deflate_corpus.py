"""DEFLATE members that zlib's encoder never writes, made with tests/deflate_writer.py, for both inflaters (the device's
bgzf_inflate_kernel and host::inflate_raw): corpus_valid(out_offset) and corpus_invalid(), seeded and deterministic.

A Case is (name, payload, out, valid, report): `payload` the member's bytes, `out` the intended output (for an invalid member:
bytes of the length the block descriptor announces; its CRC-32 is the trailer's), `valid` what the case claims zlib says of
it — tests/test_deflate_writer.py holds every claim against zlib itself.  The geometry cases depend on the address of the
member's first output byte modulo 512 (the device decoder's ring unit): corpus_valid gets it.

The random part: RANDOM_MEMBERS = 1500 members of 1-4 blocks (tokens drawn over five data models, code lengths by each helper,
header recipe and block cuts drawn).  It is sized by what it costs the suite rather than by a full minute: it generates in about
12 s on one core (the named and geometry parts in under 1 s), and every test module that uses it pays that once."""
import functools
import random
import zlib
from collections import namedtuple

from tests.deflate_writer import (DIST_BASE, FIXED_LIT, Bits, Dynamic, Fixed, Stored, Sym, apply_tokens, deep_lengths, expected_output,
                                  flat_lengths, greedy_tokens, length_symbol, limited_lengths, make_dynamic, rle_greedy, single_lengths, write_member)

Case = namedtuple("Case", "name payload out valid report")
RANDOM_MEMBERS = 1500
UNIT = 512
# the first output addresses (modulo the unit) the device test places the corpus at: the unit's edges, the 16-byte store's, a few drawn
DEVICE_OFFSETS = (0, 1, 15, 16, 496, 511, 77, 259, 338)

# zlib accepts these and both decoders report them, by design: a literal/length alphabet that is incomplete with a single code
BY_DESIGN = ("by design: lone 1-bit end-of-block code, empty member",
             "by design: lone 1-bit end-of-block code, behind a fixed block of data",
             "by design: lone 1-bit end-of-block code, behind a stored block of data")

# every structured invalid stream that must be in corpus_invalid(), by name (names may carry a suffix behind these)
INVALID_NAMES = (
    "over-subscribed literal/length code", "over-subscribed distance code", "over-subscribed code-length code",
    "incomplete literal/length code", "incomplete distance code", "incomplete code-length code",
    "repeat symbol 16 first", "repeat overruns HLIT + HDIST", "no end-of-block code", "HLIT 287", "HLIT 288", "HDIST 31", "HDIST 32",
    "BTYPE 3", "unassigned half of a one-code distance alphabet", "distance op + 1", "match one byte past out_len",
    "literal one byte past out_len", "LEN/NLEN mismatch", "stored bytes cut by in_len", "fixed block cut 1 byte short",
    "fixed block cut 2 bytes short", "fixed block cut 3 bytes short", "empty input, out_len 0", "empty input, out_len 5",
    "symbol 286 in a fixed block", "symbol 287 in a fixed block", "distance code 30 in a fixed block", "distance code 31 in a fixed block",
    "HCLEN 4", "match with no distance code")


def zlib_verdict(payload, out_len, crc):
    """what zlib makes of the member: (accepted, bytes or None) — the end of the stream reached (bytes behind it are no error: the
    block's own length field bounds the member), the length the descriptor announces, the trailer's CRC"""
    try:
        dz = zlib.decompressobj(wbits=-15)
        got = dz.decompress(bytes(payload)) + dz.flush()
    except zlib.error:
        return False, None
    return bool(dz.eof and len(got) == out_len and (zlib.crc32(got) & 0xFFFFFFFF) == crc), got


def _case(name, blocks, off=0, valid=True, out_len=None, cut=0, tail=b""):
    payload, rep = write_member(blocks, off)
    if cut:
        payload = payload[:-cut]
    payload += tail
    try:
        out = expected_output(blocks)
    except ValueError:
        out = bytes(rep.out_len)
    if out_len is not None:
        out = (out + bytes(out_len))[:out_len]
    return Case(name, payload, out, valid, rep)


def _lits(rng, n, lo=0, hi=256):
    return [rng.randrange(lo, hi) for _ in range(n)]


class _Layout:
    """tokens placed by hand: literals up to a chosen output ADDRESS modulo the unit, then matches where the case wants them"""

    def __init__(self, rng, off):
        self.rng, self.off, self.tokens, self.pos = rng, off, [], 0

    def lit(self, n):
        self.tokens += _lits(self.rng, n)
        self.pos += n

    def to_mod(self, m):
        self.lit((m - (self.off + self.pos)) % UNIT)

    def match(self, length, dist):
        assert dist <= self.pos
        self.tokens.append((length, dist))
        self.pos += length


# ---- the named valid members that do not depend on the output address ------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _named_valid():
    rng = random.Random(20240607)
    out = []

    # -- codes longer than the decoders' table index bits (device: 10 literal/length, 8 distance; host: 11 and 8)
    skew = [min(39, int(rng.expovariate(0.7))) for _ in range(6000)]
    out.append(_case("deep literal codes", [make_dynamic(skew, lit="deep")]))
    toks = []
    pos = 0
    for i in range(900):
        if i % 3 == 0 or pos < 40:
            toks.append(rng.randrange(8)); pos += 1
        else:
            ln = rng.choice([3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 17, 23, 35, 67, 131, 258])
            toks.append((ln, rng.randrange(1, min(pos, 200) + 1))); pos += ln
    lens_used = sorted({t[0] for t in toks if not isinstance(t, int)})
    order = list(range(8)) + [256] + list(dict.fromkeys(length_symbol(l)[0] for l in lens_used))
    out.append(_case("deep length codes", [make_dynamic(toks, lit="deep", lit_order=order)]))
    toks = _lits(rng, 2100)
    pos = 2100
    for i in range(700):
        d = rng.choice(DIST_BASE[:22]) + (rng.randrange(3) if i % 2 else 0)
        toks.append((rng.randrange(3, 12), min(d, pos))); pos += toks[-1][0]
        if i % 4 == 0:
            toks.append(rng.randrange(256)); pos += 1
    out.append(_case("deep distance codes", [make_dynamic(toks, dist="deep")]))
    # 15-bit length codes with 5 extra bits and 15-bit distance codes with 13: 48 bits a token, eight in a row, twice
    far = rng.randbytes(33000)
    lit_order = list(range(65, 76)) + [256, 281, 282, 283, 284]
    dist_order = list(range(14)) + [28, 29]
    toks = _lits(rng, 20, 65, 76)
    for rep_ in range(2):
        for i in range(8):
            toks.append((rng.choice([195 + rng.randrange(32), 227 + rng.randrange(31)]), rng.choice([16385 + rng.randrange(8192), 24577 + rng.randrange(8192)])))
        toks += _lits(rng, 5, 65, 76) + [(rng.randrange(131, 195), rng.choice(DIST_BASE[:14]))]
    out.append(_case("48-bit tokens in a row behind a stored block",
                     [Stored(far), Dynamic(toks, deep_lengths(286, lit_order), deep_lengths(30, dist_order))]))

    # -- legal encodings zlib never emits
    out.append(_case("length 258 as symbol 284 + extra 31, fixed", [Fixed([65, Sym(284, 31, 0, 0), 66, Sym(284, 31, 1, 0)])]))
    t284 = _lits(rng, 300, 97, 123) + [Sym(284, 31, dist_s, 0) for dist_s in (0, 3, 2, 0, 1)] + [(258, 5), 120]
    out.append(_case("length 258 as symbol 284 + extra 31, dynamic", [make_dynamic(t284)]))
    out.append(_case("HLIT 257, HDIST 1, HCLEN 5 (the fewest a block with an end-of-block code can have)",
                     [Dynamic(_lits(rng, 500, 1, 256), [0] + [8] * 256, [0], rle="none")]))
    text = [rng.choice(b"ACGTN\n@+IIIIHHG#") for _ in range(3000)]
    text_toks = greedy_tokens(bytes(text))
    out.append(_case("code lengths without run symbols", [make_dynamic(text_toks, rle="none")]))
    out.append(_case("code lengths without run symbols, HLIT 286, HDIST 30, HCLEN 19", [make_dynamic(text_toks, rle="none", hlit=286, hdist=30, hclen=19)]))
    # a repeat (16) that begins in the literal/length lengths and ends in the distance lengths: 128 codes of 8 bits and 16 of 5; 5 5 4 3 2 1
    lit_l = [8] * 127 + [0] * 129 + [8] + [0] * 13 + [5] * 16
    dist_l = [5, 5, 4, 3, 2, 1]
    seq = lit_l + dist_l
    rle = rle_greedy(seq[:280]) + [(5, None), (16, 3), (5, None), (4, None), (3, None), (2, None), (1, None)]
    toks = _lits(rng, 200, 0, 127) + [(258, 1), (23, 2), (30, 3), (40, 4), (100, 5), (200, 7)]
    out.append(_case("repeat 16 crosses from the literal/length into the distance lengths", [Dynamic(toks, lit_l, dist_l, hlit=286, rle=rle)]))
    # a run of zeros (18) across the boundary
    toks = _lits(rng, 300, 0, 100) + [(10, 285), (17, 300)]
    lf = limited_lengths([1] * 100 + [0] * 156 + [1] + [0] * 7 + [1, 0, 0, 0, 1] + [0] * 17, 15)
    out.append(_case("zero run 18 crosses from the literal/length into the distance lengths",
                     [Dynamic(toks, lf, [0] * 15 + [1, 1], hlit=286)]))
    out.append(_case("a code-length code other than zlib's: all 19 symbols, flat", [make_dynamic(text_toks, cl_lens=flat_lengths(19, range(19)))]))
    out.append(_case("a code-length code other than zlib's: flat, no run symbols used", [make_dynamic(text_toks, rle="none", cl_lens=flat_lengths(19, range(19)))]))
    two = flat_lengths(286, [0, 256])
    out.append(_case("empty fixed block in the middle", [Fixed(_lits(rng, 40)), Fixed([]), Fixed(_lits(rng, 40))]))
    out.append(_case("empty dynamic block in the middle", [Fixed(_lits(rng, 40)), Dynamic([], two, [0]), make_dynamic(_lits(rng, 40))]))
    out.append(_case("empty blocks of every type, six in a row, then data", [Fixed([]), Dynamic([], two, [0]), Stored(b""), Fixed([]), Stored(b""), Dynamic([], two, [0]),
                                                                             Fixed(_lits(rng, 9))]))
    out.append(_case("lone end-of-block, stored", [Stored(b"")]))
    out.append(_case("lone end-of-block, fixed", [Fixed([])]))
    out.append(_case("lone end-of-block, dynamic", [Dynamic([], two, [0])]))
    out.append(_case("stored LEN 0 in the middle", [Fixed(_lits(rng, 33)), Stored(b""), Fixed(_lits(rng, 33))]))
    big = rng.randbytes(65535)
    out.append(_case("stored LEN 65535 in the middle", [Fixed([]), Stored(big), Fixed([77])]))
    out.append(_case("stored LEN 65535 first, a literal behind it", [Stored(big), make_dynamic([200])]))
    st = rng.randbytes(3000)
    toks = [(258, 3000), (100, 2999), 65, (3, 1), (50, 1600), (258, 3000 + 258 + 100)]
    out.append(_case("matches reach back across a block boundary into a stored block", [Stored(st), Fixed(toks)]))
    out.append(_case("matches reach back across two block boundaries", [Stored(st), Fixed(_lits(rng, 10)), make_dynamic([(258, 3010), (30, 3000), 7, (9, 3200)])]))

    # -- positions
    out.append(_case("distance == op: the member's first byte, at op 1", [Fixed([65, (258, 1), (3, 259)])]))
    out.append(_case("distance == op at op 700", [Fixed(_lits(rng, 700) + [(100, 700), (3, 800)])]))
    base = _lits(rng, 1000)
    body = list(base)
    p = 1000
    while p < 32768 - 258:
        body.append((258, 1000)); p += 258
    body += _lits(rng, 32768 - p)
    p = 32768
    body += [(258, 32768), (3, 32768), 9, (17, 32768)]
    p += 258 + 3 + 1 + 17
    while p < 40000:
        body.append((100, 777)); p += 100
    body += [(200, 32768), (4, 32767)]
    out.append(_case("distance 32768 at op 32768 and behind", [make_dynamic(body)]))
    out.append(_case("distance 32768 at op 32768 and behind, fixed", [Fixed(body)]))
    out.append(_case("match ends exactly at out_len", [Fixed(_lits(rng, 50) + [(3, 50)])]))
    out.append(_case("match of 258 ends exactly at out_len", [make_dynamic(_lits(rng, 600) + [(258, 600)])]))

    # -- 1 to 5 blocks of the three types; stored blocks at every bit phase, stored LEN 0 ... 9 with a Huffman block behind
    for k in range(1, 6):
        kinds = [("stored", "fixed", "dynamic")[(k + i) % 3] for i in range(k)]
        blocks, hist = [], bytearray()
        for kind in kinds:
            data = bytes(rng.choice(b"ACGT") for _ in range(rng.randrange(1, 900)))
            if kind == "stored":
                blocks.append(Stored(data)); hist += data
            else:
                t = greedy_tokens(data, bytes(hist))
                blocks.append(Fixed(t) if kind == "fixed" else make_dynamic(t, lit="flat", dist="flat"))
                hist += data
        out.append(_case(f"{k} blocks: {' '.join(kinds)}", blocks))
    for phase in range(8):
        for n in range(10):
            # a fixed block of j nine-bit literals ends at bit 3 + 9 j + 7: the stored header behind it begins at every phase
            j = (phase - 2) % 8
            data = rng.randbytes(n)
            behind = Fixed(_lits(rng, 5) + ([(3, 2)] if n else [])) if (n + phase) % 2 else make_dynamic(_lits(rng, 5, 0, 9) + [(4, 3)])
            c = _case(f"stored LEN {n} at bit phase {phase}, a Huffman block behind", [Fixed([200] * j), Stored(data), behind])
            assert c.report.starts[1] == phase
            out.append(c)
    out.append(_case("trailing bytes behind the final block", [Fixed(_lits(rng, 100))], tail=b"\x5a\xa5\xff\x00\x01"))
    out.append(_case("trailing bytes behind a final stored block", [Stored(b"hello")], tail=bytes(7)))

    # -- the host decoder's shapes: it leaves its unchecked loop 8 bytes before the input's end and 269 before the output's
    long_lit = [rng.choice(b"ACGT") for _ in range(9000)]
    out.append(_case("long member that ends in literals", [make_dynamic(greedy_tokens(bytes(long_lit)) + _lits(rng, 300))]))
    out.append(_case("long member that ends in matches of 258 up to out_len", [make_dynamic(greedy_tokens(bytes(long_lit)) + [(258, 4000)] * 3)]))
    out.append(_case("long member whose last 269 bytes are one literal and matches of 67", [make_dynamic(greedy_tokens(bytes(long_lit)) + [5] + [(67, 1)] * 4)]))
    out.append(_case("long member in the fixed code that ends in a match at distance 1", [Fixed(greedy_tokens(bytes(long_lit)) + [(258, 1), (11, 1)])]))

    # -- zlib accepts, both decoders report (BY_DESIGN): a literal/length alphabet that is a lone 1-bit end-of-block code
    lone = single_lengths(257, 256)
    out.append(_case(BY_DESIGN[0], [Dynamic([], lone, [0])]))
    out.append(_case(BY_DESIGN[1], [Fixed(_lits(rng, 64), final=0), Dynamic([], lone, [0])]))
    out.append(_case(BY_DESIGN[2], [Stored(rng.randbytes(64)), Dynamic([], lone, [0])]))
    return tuple(out)


# ---- the geometry of the device decoder's ring and batch: built for the address of the first output byte -------------------------
@functools.lru_cache(maxsize=None)
def _geometry(off):
    rng = random.Random(77 + off)
    out = []

    def done(name, lay, dynamic=True):
        lay.lit(rng.randrange(0, 30))
        out.append(_case(f"{name} (first output address {off} mod {UNIT})", [make_dynamic(lay.tokens) if dynamic else Fixed(lay.tokens)], off))

    for dynamic in (True, False):
        lay = _Layout(rng, off); lay.lit(1100); lay.to_mod(UNIT - 20); lay.match(20, 300); lay.lit(3)
        lay.to_mod(UNIT - 258); lay.match(258, 1000); lay.to_mod(UNIT - 3); lay.match(3, 1)
        done("matches end exactly at a unit's end", lay, dynamic)
        lay = _Layout(rng, off); lay.lit(1100); lay.to_mod(UNIT - 19); lay.match(20, 300); lay.lit(3)
        lay.to_mod(UNIT - 257); lay.match(258, 1000); lay.to_mod(UNIT - 2); lay.match(3, 1)
        done("matches cross a unit's end by one byte", lay, dynamic)
        lay = _Layout(rng, off); lay.lit(40)
        for d in range(1, 9):
            lay.to_mod(UNIT - 10 * d); lay.match(100 + 19 * d, d); lay.lit(2)
        done("overlapping matches of distance 1-8 split by a unit's end", lay, dynamic)
    # more than 64 matches inside one unit: 150 of three bytes; then 100 with a literal between
    lay = _Layout(rng, off); lay.lit(700); lay.to_mod(0)
    for _ in range(150):
        lay.match(3, rng.randrange(1, 600))
    lay.to_mod(0)
    for _ in range(100):
        lay.match(rng.randrange(3, 5), rng.randrange(1, 1200)); lay.lit(1)
    done("more than 64 matches inside one unit", lay)
    # a batch of every kind of source: flushed long ago (up to 8 bytes: a lane each; more: eight lanes each), the ring, another pending token's output
    lay = _Layout(rng, off); lay.lit(1700)
    for rep_ in range(3):
        lay.to_mod(5 * rep_)
        lay.match(5, 1200); lay.match(40, 1000); lay.lit(10); lay.match(6, 8); lay.match(8, 1650 - rep_); lay.match(30, 35); lay.match(9, 1500)
        lay.match(70, 70 + 30 + 8); lay.match(3, 900); lay.match(258, 600); lay.match(4, 260)
    done("a batch mixes sources flushed long ago, in the ring and pending", lay)
    return tuple(out)


# ---- the random part ------------------------------------------------------------------------------------------------------------
def _draw_tokens(rng, model, n_out, pos):
    toks, made = [], 0
    while made < n_out:
        room = n_out - made
        at = pos + made
        r = rng.random()
        if model == "noise":
            lit, mlen, mdist = r < 0.9, (3, 12), 4000
        elif model == "dense":
            lit, mlen, mdist = r < 0.3, (3, 10), 64
        elif model == "far":
            lit, mlen, mdist = r < 0.3, (3, 258), 32768
        elif model == "runs":
            lit, mlen, mdist = r < 0.2, (3, 258), 8
        else:                                  # "text": short literals runs and medium matches
            lit, mlen, mdist = r < 0.55, (3, 40), 1500
        if lit or room < 3 or at == 0:
            toks.append(rng.randrange(4) if model == "dense" else (rng.choice(b"ACGTN!#IF\n") if model == "text" else rng.randrange(256)))
            made += 1
        else:
            ln = min(room, rng.randrange(mlen[0], mlen[1] + 1) if rng.random() < 0.9 else 258)
            toks.append((ln, rng.randrange(1, min(at, mdist) + 1) if rng.random() < 0.97 else min(at, mdist)))
            made += ln
    return toks


def _random_member(rng, i):
    model = ("noise", "dense", "far", "runs", "text")[i % 5]
    r = rng.random()
    n_out = rng.randrange(0, 300) if r < 0.25 else (rng.randrange(300, 8000) if r < 0.7 else (rng.randrange(8000, 65537) if r < 0.97 else 65536))
    nb = rng.randrange(1, 5)
    cuts = sorted(rng.randrange(0, n_out + 1) for _ in range(nb - 1)) + [n_out]
    blocks, hist, recipe, pos = [], bytearray(), [], 0
    for end in cuts:
        toks = _draw_tokens(rng, model, end - pos, pos)
        kind = rng.choice(("stored", "fixed", "dynamic", "dynamic", "dynamic"))
        before = len(hist)
        apply_tokens(toks, hist)
        if kind == "stored" and end - pos < 65536:
            blocks.append(Stored(bytes(hist[before:])))
        elif kind == "fixed" or kind == "stored":
            blocks.append(Fixed(toks)); kind = "fixed"
        else:
            lit, dist = rng.choice(("optimal", "deep", "flat")), rng.choice(("optimal", "deep", "flat"))
            header = dict(rle=rng.choice(("none", "greedy")))
            if rng.random() < 0.3:
                header["hlit"] = 286
            if rng.random() < 0.3:
                header["hdist"] = 30
            if rng.random() < 0.3:
                header["cl_lens"] = flat_lengths(19, range(19))
            elif rng.random() < 0.3:
                header["hclen"] = 19
            blocks.append(make_dynamic(toks, lit=lit, dist=dist, **header))
            kind = f"dynamic/{lit}/{dist}/{header['rle']}"
        recipe.append(kind)
        pos = end
    return _case(f"random {i}: {model}, {n_out} bytes, {' + '.join(recipe)}", blocks)


@functools.lru_cache(maxsize=None)
def _random_valid():
    rng = random.Random(4711)
    return tuple(_random_member(rng, i) for i in range(RANDOM_MEMBERS))


def corpus_valid(out_offset=0, random_part=True):
    """every member zlib accepts (the BY_DESIGN ones included: the decoders' tests except them by name)"""
    return list(_named_valid()) + list(_geometry(out_offset % UNIT)) + (list(_random_valid()) if random_part else [])


@functools.lru_cache(maxsize=None)
def _invalid():
    rng = random.Random(99)
    out = []

    def bad(name, blocks, **kw):
        out.append(_case(name, blocks, valid=False, **kw))

    lits = _lits(rng, 20, 0, 3)
    bad("over-subscribed literal/length code", [Dynamic(lits, [1, 1, 1] + [0] * 253 + [2], [0])])
    bad("over-subscribed distance code", [Dynamic(lits + [(3, 1)], flat_lengths(286, [0, 1, 2, 256, 257]), [1, 1, 1])])
    bad("over-subscribed code-length code", [Dynamic(lits, flat_lengths(286, [0, 1, 2, 256]), [0], rle="none", cl_lens=[1, 0, 1, 0, 0, 1] + [0] * 13, hclen=19)])
    bad("over-subscribed code-length code, lengths 1 2 2 2", [Dynamic([1, 2], [0, 2, 2] + [0] * 253 + [1], [0], rle="none", cl_lens=[2, 2, 2] + [0] * 15 + [1])])
    bad("incomplete literal/length code", [Dynamic(lits, [2, 2, 2] + [0] * 253 + [3], [0])])
    bad("incomplete literal/length code: a lone code of two bits", [Dynamic([], single_lengths(257, 256, 2), [0])])
    bad("incomplete distance code", [Dynamic(lits + [(3, 1)], flat_lengths(286, [0, 1, 2, 256, 257]), [2, 2])])
    bad("incomplete distance code: a lone code of two bits", [Dynamic(lits + [(3, 1)], flat_lengths(286, [0, 1, 2, 256, 257]), [2])])
    bad("incomplete code-length code", [Dynamic(lits, flat_lengths(286, [0, 1, 2, 256]), [0], rle="none", cl_lens=[2, 0, 2] + [0] * 16)])
    good_l, good_d = flat_lengths(286, [0, 1, 2, 3, 256, 257]), [1, 1]
    seq = (good_l + [0] * 257)[:258] + good_d
    bad("repeat symbol 16 first", [Dynamic([3, 3, 3], [0, 0, 0] + good_l[3:], good_d, rle=[(16, 0)] + [(l, None) for l in seq[3:]], cl_lens=flat_lengths(19, [0, 1, 2, 3, 16]))])
    bad("repeat overruns HLIT + HDIST", [Dynamic(lits, good_l, [0] * 10, rle=[(l, None) for l in seq[:258]] + [(18, 0)], cl_lens=flat_lengths(19, [0, 1, 2, 3, 18]))])
    bad("repeat overruns HLIT + HDIST by one, with 16", [Dynamic(lits, good_l, [3, 3, 3, 3], rle=[(l, None) for l in seq[:258]] + [(3, None), (16, 1)],
                                                              cl_lens=flat_lengths(19, [0, 1, 2, 3, 16]))])
    bad("no end-of-block code", [Dynamic([t % 2 for t in lits], [1, 1, 0], [0], hlit=257)], out_len=20)
    bad("HLIT 287", [Dynamic(lits, flat_lengths(288, [0, 1, 2, 256]), [0], hlit=287)])
    bad("HLIT 288", [Dynamic(lits, list(FIXED_LIT), [0], hlit=288)])
    bad("HDIST 31", [Dynamic(lits, flat_lengths(286, [0, 1, 2, 256]), [1, 1], hdist=31)])
    bad("HDIST 32", [Dynamic(lits, flat_lengths(286, [0, 1, 2, 256]), [5] * 32, hdist=32)])
    out.append(Case("BTYPE 3", b"\x07" + bytes(8), b"", False, None))
    bad("BTYPE 3 behind a fixed block", [Fixed([65, Sym(256, 0, None), Bits(0b111, 3)], eob=False, final=0)], out_len=1)
    one = single_lengths(30, 0)
    bad("unassigned half of a one-code distance alphabet", [Dynamic([65, 66, 67, Sym(257, 0, None), Bits(1, 1)], flat_lengths(286, [65, 66, 67, 256, 257]), one)], out_len=6)
    bad("distance op + 1: the first token", [Fixed([(3, 1)])], out_len=3)
    bad("distance op + 1: behind ten literals", [Fixed(_lits(rng, 10) + [Sym(259, 0, 6, 2)])], out_len=15)
    bad("distance op + 1: behind a stored block", [Stored(rng.randbytes(100)), Fixed([Sym(257, 0, 13, 4)])], out_len=103)
    bad("distance op + 1: in a later unit, dynamic", [make_dynamic(_lits(rng, 1500) + [Sym(264, 0, 20, 1501 - 1025), 1, 2])], out_len=1512)
    toks = _lits(rng, 30, 0, 4) + [(3, d) for d in (1, 2, 3, 5, 8, 13, 21, 30)] * 6
    n = 30 + 3 * 48
    bad("distance op + 1: behind dense short matches", [make_dynamic(toks + [Sym(257, 0, 14, n + 1 - 129), 3])], out_len=n + 4)
    bad("distance op + 1: 32768 at op 32767", [Stored(rng.randbytes(32767)), Fixed([Sym(257, 0, 29, 8191)])], out_len=32770)
    bad("distance op + 1: with long codes", [Stored(rng.randbytes(20000)), Dynamic(_lits(rng, 5, 65, 76) + [Sym(284, 3, 28, 20006 - 16385)],
                                                                                 deep_lengths(286, list(range(65, 76)) + [256, 281, 282, 283, 284]),
                                                                                 deep_lengths(30, list(range(14)) + [28, 29]))], out_len=20005 + 230)
    bad("match one byte past out_len", [Fixed(_lits(rng, 100) + [(10, 50)])], out_len=109)
    bad("match one byte past out_len, dynamic, behind matches", [make_dynamic(_lits(rng, 100, 0, 4) + [(3, 7)] * 40 + [(258, 1)])], out_len=100 + 120 + 257)
    bad("literal one byte past out_len", [Fixed(_lits(rng, 100))], out_len=99)
    bad("literal one byte past out_len, dynamic, behind matches", [make_dynamic(_lits(rng, 100, 0, 4) + [(3, 7)] * 40 + [3])], out_len=220)
    bad("stored byte one past out_len", [Fixed(_lits(rng, 10)), Stored(b"abcdef")], out_len=15)
    bad("the stream makes one byte less than out_len", [make_dynamic(_lits(rng, 100, 0, 4) + [(3, 7)] * 40)], out_len=221)
    bad("LEN/NLEN mismatch", [Stored(b"hello world", nlen=0x1234)])
    bad("LEN/NLEN mismatch in the middle", [Fixed([1, 2, 3]), Stored(b"hello world", nlen=11), Fixed([4])])
    bad("stored bytes cut by in_len", [Stored(rng.randbytes(100))], cut=10)
    bad("stored bytes cut by in_len, by one byte, behind a fixed block", [Fixed([1, 2, 3]), Stored(rng.randbytes(700))], cut=1)
    bad("stored header cut by in_len", [Fixed([1, 2, 3]), Stored(rng.randbytes(7))], cut=9)
    eight = _lits(rng, 40, 0, 144)                                 # literals of 8 bits: the end-of-block code's last two bits are alone in the last byte
    for k in (1, 2, 3):
        bad(f"fixed block cut {k} byte{'s' if k > 1 else ''} short", [Fixed(eight)], cut=k)
    out.append(Case("empty input, out_len 0", b"", b"", False, None))
    out.append(Case("empty input, out_len 5", b"", bytes(5), False, None))
    bad("symbol 286 in a fixed block", [Fixed([65, Sym(286, 0, None), 66])], out_len=2)
    bad("symbol 287 in a fixed block", [Fixed([65, Sym(287, 0, None), 66])], out_len=2)
    bad("distance code 30 in a fixed block", [Fixed([65, 66, 67, Sym(257, 0, 30, 0), 68])], out_len=7)
    bad("distance code 31 in a fixed block", [Fixed([65, 66, 67, Sym(257, 0, 31, 0), 68])], out_len=7)
    bad("HCLEN 4: no length but zero can be said", [Dynamic([], [0] * 257, [0], cl_lens=[1] + [0] * 17 + [1])], out_len=0)
    bad("match with no distance code", [Dynamic([65, 66, 67, Sym(257, 0, None)], flat_lengths(286, [65, 66, 67, 256, 257]), [0])], out_len=6)
    bad("a final block is missing: the last block says there is another", [Fixed(_lits(rng, 30), final=0)])
    # the random part's members with their last 1-3 bytes missing, or with an out_len one off
    for i, c in enumerate(_random_valid()[::7]):
        k = i % 5
        if k < 3:
            out.append(Case(f"{c.name}, cut {k + 1} short", c.payload[:-(k + 1)], c.out, False, c.report))
        elif k == 3:
            out.append(Case(f"{c.name}, out_len one more", c.payload, c.out + b"\0", False, c.report))
        elif len(c.out):
            out.append(Case(f"{c.name}, out_len one less", c.payload, c.out[:-1], False, c.report))
    return tuple(out)


def corpus_invalid():
    return list(_invalid())
