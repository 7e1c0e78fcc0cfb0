"""A plain, token-level DEFLATE reader (RFC 1951) for tests: tests/deflate_writer.py's inverse.  It inflates nothing; it says what a
raw DEFLATE payload SAYS — per block the header as written and the tokens in the writer's token form — so that a test can hold an
encoder to the very tokens and code lengths it is supposed to produce, where a round trip through zlib only sees the bytes.

  read_member(payload) -> [Block, ...]           up to and including the block with BFINAL = 1; bytes behind it are not looked at
  Block.final, .btype, .kind                     BFINAL, BTYPE, 'stored' / 'fixed' / 'dynamic'
  Block.hlit, .hdist, .hclen                     the header's counts (HLIT + 257, HDIST + 1, HCLEN + 4), dynamic blocks only
  Block.cl_lens                                  the 19 code-length lengths by symbol (those not written: 0)
  Block.lit_lens, .dist_lens                     the code lengths as written (hlit / hdist of them)
  Block.tokens                                   int for a literal (a stored block's bytes too), (length, distance) for a match
  Block.start_bit, .bits                         where the block's header begins in the payload, and the bits it takes
  Block.matches                                  (output position, length, distance) of every match, as the writer's Report

It raises Invalid on anything zlib's inflate refuses inside the stream: BTYPE 3, LEN / NLEN, HLIT above 286, HDIST above 30, a
repeat with nothing before it or beyond HLIT + HDIST, an over-subscribed code, an incomplete one (but a lone 1-bit code in the
literal/length or distance alphabet, which zlib lets pass), no end-of-block code, a bit pattern without a symbol, symbols 286 /
287, distance symbols 30 / 31, a distance beyond the output so far, and a payload that ends before its final block does."""
from tests.deflate_writer import CL_ORDER, DIST_BASE, DIST_EXTRA, FIXED_DIST, FIXED_LIT, LEN_BASE, LEN_EXTRA

PRIMARY = 9                                  # bits of the decoding tables' first level


class Invalid(ValueError):
    pass


class Block:
    __slots__ = ("final", "btype", "kind", "hlit", "hdist", "hclen", "cl_lens", "lit_lens", "dist_lens", "tokens", "start_bit", "bits", "matches")

    def __init__(self):
        self.hlit = self.hdist = self.hclen = None
        self.cl_lens = self.lit_lens = self.dist_lens = None
        self.tokens, self.matches = [], []


class _Bits:
    """least significant bit first, over an accumulator refilled eight bytes at a time"""

    def __init__(self, data):
        self.data, self.at, self.acc, self.n = bytes(data), 0, 0, 0

    def need(self, k):
        while self.n < k:
            chunk = self.data[self.at:self.at + 8]
            if not chunk:
                raise Invalid("the payload ends inside a block")
            self.acc |= int.from_bytes(chunk, "little") << self.n
            self.n += 8 * len(chunk)
            self.at += len(chunk)

    def take(self, k):
        if k == 0:
            return 0
        self.need(k)
        v = self.acc & ((1 << k) - 1)
        self.acc >>= k
        self.n -= k
        return v

    def peek_upto(self, k):
        """the next k bits, zeros behind the payload's end (a code may be shorter than k)"""
        if self.n < k:
            try:
                self.need(k)
            except Invalid:
                pass
        return self.acc & ((1 << k) - 1)

    def drop(self, k):
        if k > self.n:
            raise Invalid("the payload ends inside a block")
        self.acc >>= k
        self.n -= k

    @property
    def pos(self):
        return 8 * self.at - self.n

    def align(self):
        self.drop(self.n & 7)


def _rev(code, n):
    r = 0
    for _ in range(n):
        r = (r << 1) | (code & 1)
        code >>= 1
    return r


class _Code:
    """a canonical code's decoder, judged as zlib's inflate_table judges it.  kind: 'cl' (must be complete), 'lit' / 'dist' (complete,
    or a lone code of one bit, or — distances only as far as any token goes — nothing at all)"""

    def __init__(self, lens, kind):
        count = [0] * 16
        for l in lens:
            if l > 15:
                raise Invalid("a code length above 15")
            count[l] += 1
        count[0] = 0
        self.maxl = max((l for l in range(16) if count[l]), default=0)
        left = 1
        for l in range(1, 16):
            left = 2 * left - count[l]
            if left < 0:
                raise Invalid(f"over-subscribed {kind} code")
        if left > 0 and self.maxl and (kind == "cl" or self.maxl != 1):
            raise Invalid(f"incomplete {kind} code")
        if self.maxl == 0 and kind == "cl":
            raise Invalid("incomplete cl code")
        nxt, code = [0] * 17, 0
        for l in range(1, 16):
            code = (code + count[l - 1]) << 1
            nxt[l] = code
        self.p = min(self.maxl, PRIMARY)
        self.table = [None] * (1 << self.p)
        self.long = {}
        for s, l in enumerate(lens):
            if not l:
                continue
            r = _rev(nxt[l], l)
            nxt[l] += 1
            if l <= self.p:
                for i in range(r, 1 << self.p, 1 << l):
                    self.table[i] = (s, l)
            else:
                self.long[(l, r)] = s

    def read(self, b):
        if self.maxl == 0:
            raise Invalid("a symbol of an alphabet without codes")
        v = b.peek_upto(self.maxl)
        e = self.table[v & ((1 << self.p) - 1)]
        if e is not None:
            b.drop(e[1])
            return e[0]
        for l in range(self.p + 1, self.maxl + 1):
            s = self.long.get((l, v & ((1 << l) - 1)))
            if s is not None:
                b.drop(l)
                return s
        raise Invalid("a bit pattern that is no code")


_FIXED = None


def _fixed_codes():
    global _FIXED
    if _FIXED is None:
        _FIXED = (_Code(FIXED_LIT, "lit"), _Code(FIXED_DIST, "dist"))
    return _FIXED


def _tokens(b, blk, lit, dist, out_pos):
    toks, matches = blk.tokens, blk.matches
    while True:
        s = lit.read(b)
        if s < 256:
            toks.append(s)
            out_pos += 1
        elif s == 256:
            return out_pos
        else:
            if s > 285:
                raise Invalid(f"literal/length symbol {s}")
            length = LEN_BASE[s - 257] + b.take(LEN_EXTRA[s - 257])
            d = dist.read(b)
            if d > 29:
                raise Invalid(f"distance symbol {d}")
            distance = DIST_BASE[d] + b.take(DIST_EXTRA[d])
            if distance > out_pos:
                raise Invalid(f"distance {distance} at output position {out_pos}")
            toks.append((length, distance))
            matches.append((out_pos, length, distance))
            out_pos += length


def read_member(payload):
    b = _Bits(payload)
    blocks, out_pos = [], 0
    while True:
        blk = Block()
        blk.start_bit = b.pos
        blk.final = b.take(1)
        blk.btype = b.take(2)
        if blk.btype == 0:
            blk.kind = "stored"
            b.align()
            n, nlen = b.take(16), b.take(16)
            if n != (nlen ^ 0xFFFF):
                raise Invalid("LEN / NLEN")
            for _ in range(n):
                blk.tokens.append(b.take(8))
            out_pos += n
        elif blk.btype == 1:
            blk.kind = "fixed"
            lit, dist = _fixed_codes()
            out_pos = _tokens(b, blk, lit, dist, out_pos)
        elif blk.btype == 2:
            blk.kind = "dynamic"
            blk.hlit, blk.hdist, blk.hclen = b.take(5) + 257, b.take(5) + 1, b.take(4) + 4
            if blk.hlit > 286 or blk.hdist > 30:
                raise Invalid(f"HLIT {blk.hlit}, HDIST {blk.hdist}")
            blk.cl_lens = [0] * 19
            for i in range(blk.hclen):
                blk.cl_lens[CL_ORDER[i]] = b.take(3)
            cl = _Code(blk.cl_lens, "cl")
            seq, want = [], blk.hlit + blk.hdist
            while len(seq) < want:
                s = cl.read(b)
                if s < 16:
                    seq.append(s)
                    continue
                if s == 16:
                    if not seq:
                        raise Invalid("repeat symbol 16 first")
                    v, rep = seq[-1], 3 + b.take(2)
                else:
                    v, rep = 0, (3 + b.take(3)) if s == 17 else (11 + b.take(7))
                if len(seq) + rep > want:
                    raise Invalid("a repeat overruns HLIT + HDIST")
                seq += [v] * rep
            blk.lit_lens, blk.dist_lens = seq[:blk.hlit], seq[blk.hlit:]
            if not blk.lit_lens[256]:
                raise Invalid("no end-of-block code")
            out_pos = _tokens(b, blk, _Code(blk.lit_lens, "lit"), _Code(blk.dist_lens, "dist"), out_pos)
        else:
            raise Invalid("BTYPE 3")
        blk.bits = b.pos - blk.start_bit
        blocks.append(blk)
        if blk.final:
            return blocks


def member_bits(blocks):
    """the bits of the member, from the payload's first bit to the last bit of the final block"""
    return blocks[-1].start_bit + blocks[-1].bits
