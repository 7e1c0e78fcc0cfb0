"""A plain, bit-level DEFLATE writer (RFC 1951) for tests: it turns an explicit description of a member into bytes and decides
nothing by itself.  Every compressed byte the decoders' other tests see was written by zlib's encoder, which has habits
(run-length coded headers, its own code-length code, no empty blocks, length 258 always as symbol 285 ...); this writer has
none, so a test can say exactly which legal — or illegal — encoding a decoder is shown.

  member  = [block, ...]                       write_member(blocks, out_offset) -> (bytes, Report)
  block   = Stored(data, nlen=None) | Fixed(tokens) | Dynamic(tokens, lit_lens, dist_lens, hlit, hdist, hclen, cl_lens, rle)
  token   = int                                a literal byte
          | (length, distance)                 a match, by the usual symbols (258 -> symbol 285)
          | Sym(lit, extra, dist, dist_extra)  raw symbol numbers with raw extra-bit values: 284 + 31, 286, 287, distance 30 / 31
          | Bits(value, n)                     n raw bits, for what no symbol says

The code lengths of a dynamic block are written AS GIVEN — complete, incomplete or over-subscribed; canonical codes are
assigned as far as they exist (an over-subscribed set's codes wrap).  Helpers make lengths: length-limited Huffman
(limited_lengths), a chain as deep as 15 bits (deep_lengths), flat (flat_lengths), a single code (single_lengths).  The
Report says what was written, so that a test can assert that a case is what its name claims."""
from collections import namedtuple

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32
UNIT = 512                                   # the device decoder's ring unit: the geometry figures of a Report count in these

Sym = namedtuple("Sym", "lit extra dist dist_extra", defaults=(0, None, 0))
Bits = namedtuple("Bits", "value n")


class Stored:
    def __init__(self, data, nlen=None, final=None):
        self.data, self.nlen, self.final = bytes(data), nlen, final


class Fixed:
    def __init__(self, tokens, eob=True, final=None):
        self.tokens, self.eob, self.final = list(tokens), eob, final


class Dynamic:
    """lit_lens / dist_lens: the code lengths as given.  hlit / hdist: how many of them the header announces and carries (None: up
    to the last one that is not zero, at least 257 / 1; the arrays are padded with zeros or cut to fit; 287, 288 / 31, 32 are
    sayable and illegal).  cl_lens: the 19 lengths of the code-length code (None: length-limited Huffman over what the header
    uses).  hclen: how many of them are written (None: up to the last one that is not zero in the header's order, at least 4).
    rle: 'none' (every length its own symbol), 'greedy' (runs as long as they go, across the literal/distance boundary too) or
    an explicit list of (symbol, extra value)."""

    def __init__(self, tokens, lit_lens, dist_lens, hlit=None, hdist=None, hclen=None, cl_lens=None, rle="greedy", eob=True, final=None):
        self.tokens, self.lit_lens, self.dist_lens = list(tokens), list(lit_lens), list(dist_lens)
        self.hlit, self.hdist, self.hclen, self.cl_lens, self.rle, self.eob, self.final = hlit, hdist, hclen, cl_lens, rle, eob, final


class BitSink:
    """bits to bytes, least significant bit first; a small accumulator flushed to a bytearray (linear in the output)"""

    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def bits(self, value, n):
        self.acc |= (value & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, n):
        """a Huffman code: most significant bit first"""
        r = 0
        for _ in range(n):
            r = (r << 1) | (code & 1)
            code >>= 1
        self.bits(r, n)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def raw(self, data):
        assert self.n == 0
        self.out += data

    @property
    def bitpos(self):
        return 8 * len(self.out) + self.n

    def getvalue(self):
        return bytes(self.out) + (bytes([self.acc & 0xFF]) if self.n else b"")


def canonical_codes(lens):
    """RFC 1951 §3.2.2, without judging the lengths: an over-subscribed set's codes are cut to their length"""
    maxl = max(lens, default=0)
    count = [0] * (maxl + 2)
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * (maxl + 2), 0
    for l in range(1, maxl + 1):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    codes = [0] * len(lens)
    for s, l in enumerate(lens):
        if l:
            codes[s] = nxt[l] & ((1 << l) - 1)
            nxt[l] += 1
    return codes


def kraft(lens):
    """sum of 2^-len over the codes, in units of 2^-15: 32768 = complete, more = over-subscribed, less = incomplete"""
    return sum(1 << (15 - l) for l in lens if l)


def length_symbol(length):
    if length == 258:
        return 285, 0, 0
    for i in range(27, -1, -1):
        if length >= LEN_BASE[i]:
            return 257 + i, LEN_EXTRA[i], length - LEN_BASE[i]
    raise ValueError(length)


def dist_symbol(dist):
    for i in range(29, -1, -1):
        if dist >= DIST_BASE[i]:
            return i, DIST_EXTRA[i], dist - DIST_BASE[i]
    raise ValueError(dist)


def token_symbols(tok):
    """(lit symbol, extra bits, extra value, dist symbol or None, extra bits, extra value) of a literal, match or Sym"""
    if isinstance(tok, int):
        return tok, 0, 0, None, 0, 0
    if isinstance(tok, Sym):
        ls = tok.lit
        ln = LEN_EXTRA[ls - 257] if 257 <= ls <= 285 else 0
        if tok.dist is None:
            return ls, ln, tok.extra, None, 0, 0
        return ls, ln, tok.extra, tok.dist, DIST_EXTRA[tok.dist] if tok.dist < 30 else 0, tok.dist_extra
    length, dist = tok
    ls, ln, lv = length_symbol(length)
    ds, dn, dv = dist_symbol(dist)
    return ls, ln, lv, ds, dn, dv


def token_match(tok):
    """(length, distance) a decoder makes of the token, or None for a literal / anything else"""
    if isinstance(tok, (int, Bits)):
        return None
    ls, _, lv, ds, _, dv = token_symbols(tok)
    if ds is None or not 257 <= ls <= 285 or ds >= 30:
        return None
    return LEN_BASE[ls - 257] + lv, DIST_BASE[ds] + dv


# ---- helpers that make code lengths ---------------------------------------------------------------------------------------------
def limited_lengths(freqs, maxbits, at_least_two=True):
    """Huffman lengths of at most maxbits: the frequencies are flattened until the tree is shallow enough.  A lone symbol gets a
    partner (the first unused one) unless at_least_two is False, so that the code is complete."""
    import heapq
    n = len(freqs)
    used = [s for s in range(n) if freqs[s]]
    lens = [0] * n
    if not used:
        return lens
    if len(used) == 1:
        lens[used[0]] = 1
        if at_least_two:
            lens[next(s for s in range(n) if s != used[0])] = 1
        return lens
    f = {s: freqs[s] for s in used}
    while True:
        heap = [(w, s, (s,)) for s, w in f.items()]
        heapq.heapify(heap)
        depth = dict.fromkeys(used, 0)
        tie = n
        while len(heap) > 1:
            w1, _, m1 = heapq.heappop(heap)
            w2, _, m2 = heapq.heappop(heap)
            for s in m1 + m2:
                depth[s] += 1
            heapq.heappush(heap, (w1 + w2, tie, m1 + m2))
            tie += 1
        if max(depth.values()) <= maxbits:
            break
        f = {s: (w + 1) // 2 + 1 for s, w in f.items()}
    for s in used:
        lens[s] = depth[s]
    return lens


def flat_lengths(n, used):
    """a complete code whose used symbols all sit at depth k or k + 1"""
    lens = [0] * n
    used = list(used)
    m = len(used)
    if m <= 1:
        for s in used:
            lens[s] = 1
        return lens
    k = m.bit_length() - 1
    short = (1 << (k + 1)) - m                 # symbols at depth k; the other m - short at k + 1
    for i, s in enumerate(used):
        lens[s] = k if i < short else k + 1
    return lens


def deep_lengths(n, order, maxbits=15):
    """a complete code over the symbols of `order`: the first ones a chain at depths 1, 2, 3 ..., the rest a flat subtree under the
    chain's last node, placed so that the LAST symbols of `order` have codes of maxbits bits (1, 2, 3 ... 14, 15, 15 for 16 symbols)"""
    order = list(order)
    m = len(order)
    lens = [0] * n
    if m <= 2:
        for s in order:
            lens[s] = 1
        return lens
    chain = 0
    for c in range(min(m - 2, maxbits - 1), -1, -1):
        rest = m - c
        if c + (rest - 1).bit_length() <= maxbits:
            chain = c
            break
    rest = order[chain:]
    for i in range(chain):
        lens[order[i]] = i + 1
    sub = flat_lengths(n, rest)
    for s in rest:
        lens[s] = chain + sub[s]
    return lens


def single_lengths(n, sym, length=1):
    lens = [0] * n
    lens[sym] = length
    return lens


def used_symbols(tokens, eob=True):
    """(frequencies of the 286 literal/length symbols, of the 30 distance symbols) of a token list"""
    lf, df = [0] * 288, [0] * 32
    for t in tokens:
        if isinstance(t, Bits):
            continue
        ls, _, _, ds, _, _ = token_symbols(t)
        lf[ls] += 1
        if ds is not None:
            df[ds] += 1
    if eob:
        lf[256] += 1
    return lf, df


def make_dynamic(tokens, lit="optimal", dist="optimal", lit_order=None, dist_order=None, **header):
    """a Dynamic block whose code lengths come from the helper named: 'optimal', 'deep', 'flat'.  *_order: the symbols of a deep code,
    shallow to deep (default: by falling frequency, so that the rarest are deepest)"""
    lf, df = used_symbols(tokens)

    def lengths(kind, freqs, n, order):
        used = [s for s in range(len(freqs)) if freqs[s]]
        if kind == "optimal":
            return limited_lengths(freqs[:n], 15)
        if len(used) == 1 and n > 30:                              # a literal/length alphabet of one code is incomplete: give it a partner
            used.append(0 if used[0] else 1)
        if kind == "flat":
            return flat_lengths(n, used)
        if kind == "deep":
            return deep_lengths(n, order if order is not None else sorted(used, key=lambda s: -freqs[s]))
        raise ValueError(kind)
    return Dynamic(tokens, lengths(lit, lf, 286, lit_order), lengths(dist, df, 30, dist_order), **header)


# ---- tokenizers ----------------------------------------------------------------------------------------------------------------
def greedy_tokens(data, history=b"", max_chain=6, min_len=3):
    """greedy LZ77 over `data` (matches may reach into `history`, the member's earlier output): hash chains over three bytes"""
    buf = history + data
    base = len(history)
    table = {}
    for i in range(max(0, base - 32768), base - 2):
        table.setdefault(buf[i:i + 3], []).append(i)
    toks, i, n = [], base, len(buf)
    while i < n:
        best_len, best_dist = 0, 0
        key = buf[i:i + 3]
        if len(key) == 3:
            for j in reversed(table.get(key, [])[-max_chain:]):
                if i - j > 32768:
                    break
                l = 3
                lim = min(258, n - i)
                while l < lim and buf[j + l] == buf[i + l]:
                    l += 1
                if l > best_len:
                    best_len, best_dist = l, i - j
        step = 1
        if best_len >= min_len:
            toks.append((best_len, best_dist))
            step = best_len
        else:
            toks.append(buf[i])
        for k in range(i, min(i + step, n - 2)):
            table.setdefault(buf[k:k + 3], []).append(k)
        i += step
    return toks


def apply_tokens(tokens, out):
    """append to the bytearray `out` what a decoder makes of the tokens; raises ValueError on a token no decoder accepts"""
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
            continue
        m = token_match(t)
        if m is None:
            if isinstance(t, Sym) and t.lit < 256 and t.dist is None:
                out.append(t.lit)
                continue
            raise ValueError(f"no decoder accepts {t!r}")
        length, dist = m
        if dist > len(out):
            raise ValueError(f"distance {dist} at position {len(out)}")
        if dist >= length:
            out += out[len(out) - dist:len(out) - dist + length]
        else:
            for _ in range(length):
                out.append(out[-dist])
    return out


def expected_output(blocks):
    out = bytearray()
    for b in blocks:
        if isinstance(b, Stored):
            out += b.data
        else:
            apply_tokens(b.tokens, out)
    return bytes(out)


# ---- the report ----------------------------------------------------------------------------------------------------------------
class Report:
    """what write_member wrote.  kinds: 'stored' / 'fixed' / 'dynamic' per block; starts: the bit phase (0-7) at which each block's
    header begins; max_lit_code / max_len_code / max_dist_code: the longest code a TOKEN used in each role; widest_token: the most
    bits one token took (codes and extra bits); wide_run: the longest run of adjacent tokens of 48 bits each; matches: (position,
    length, distance) of every match; out_len: the bytes the tokens and stored blocks make; headers: per dynamic block a dict
    (hlit, hdist, hclen, rle symbols used, whether a run crosses the literal/distance boundary, the code-length code's lengths)."""

    def __init__(self, out_offset):
        self.out_offset = out_offset
        self.kinds, self.starts, self.headers = [], [], []
        self.max_lit_code = self.max_len_code = self.max_dist_code = self.widest_token = self.wide_run = 0
        self.matches, self.out_len = [], 0
        self.block_out = []                   # output position at which each block begins

    # geometry, in the device decoder's terms: the output ADDRESS (out_offset + position) in units of 512 bytes
    def matches_per_unit(self):
        per = {}
        for pos, _, _ in self.matches:
            u = (self.out_offset + pos) // UNIT
            per[u] = per.get(u, 0) + 1
        return per

    def match_ends_at_unit_end(self):
        return any((self.out_offset + p + l) % UNIT == 0 for p, l, _ in self.matches)

    def match_crosses_unit_by_one(self):
        return any((self.out_offset + p + l) % UNIT == 1 and l >= 2 for p, l, _ in self.matches)

    def overlapping_match_split_by_unit(self):
        """distances (1-8, smaller than the length) of the overlapping matches that begin in one unit and end in the next"""
        return sorted({d for p, l, d in self.matches if d < l and d <= 8 and (self.out_offset + p) // UNIT != (self.out_offset + p + l - 1) // UNIT})

    def source_ages(self):
        """per unit the kinds of its matches' sources: 'flushed_short' / 'flushed_long' (the whole source lies before the unit's first
        byte, so it left for memory when the unit began; at most 8 bytes / more), 'pending' (the source overlaps the output of an
        earlier match of the same unit), 'recent' (anything else: in the ring)"""
        ages, in_unit = {}, {}
        for p, l, d in self.matches:
            u = (self.out_offset + p) // UNIT
            unit_first = u * UNIT - self.out_offset
            s0, s1 = p - d, p - d + l
            if s1 <= unit_first:
                kind = "flushed_short" if l <= 8 else "flushed_long"
            elif any(s0 < q + m and q < s1 for q, m in in_unit.get(u, [])):
                kind = "pending"
            else:
                kind = "recent"
            ages.setdefault(u, set()).add(kind)
            in_unit.setdefault(u, []).append((p, l))
        return ages


def write_tokens(sink, tokens, lit_lens, dist_lens, rep, eob=True):
    lit_codes, dist_codes = canonical_codes(lit_lens), canonical_codes(dist_lens)
    run = 0
    for t in tokens:
        if isinstance(t, Bits):
            sink.bits(t.value, t.n)
            run = 0
            continue
        ls, ln, lv, ds, dn, dv = token_symbols(t)
        if ls >= len(lit_lens) or not lit_lens[ls]:
            raise ValueError(f"literal/length symbol {ls} has no code")
        width = lit_lens[ls] + ln
        sink.code(lit_codes[ls], lit_lens[ls])
        if ln:
            sink.bits(lv, ln)
        if ds is None:
            if ls < 256:
                rep.max_lit_code = max(rep.max_lit_code, lit_lens[ls])
                rep.out_len += 1
        else:
            if ds >= len(dist_lens) or not dist_lens[ds]:
                raise ValueError(f"distance symbol {ds} has no code")
            sink.code(dist_codes[ds], dist_lens[ds])
            if dn:
                sink.bits(dv, dn)
            width += dist_lens[ds] + dn
            rep.max_len_code = max(rep.max_len_code, lit_lens[ls])
            rep.max_dist_code = max(rep.max_dist_code, dist_lens[ds])
            m = token_match(t)
            if m is not None:
                rep.matches.append((rep.out_len, m[0], m[1]))
                rep.out_len += m[0]
        rep.widest_token = max(rep.widest_token, width)
        run = run + 1 if width >= 48 else 0
        rep.wide_run = max(rep.wide_run, run)
    if eob and len(lit_lens) > 256 and lit_lens[256]:
        sink.code(lit_codes[256], lit_lens[256])


def rle_greedy(seq):
    out, i, n = [], 0, len(seq)
    while i < n:
        v = seq[i]
        j = i
        while j < n and seq[j] == v:
            j += 1
        run = j - i
        if v == 0 and run >= 3:
            take = min(run, 138)
            out.append((18, take - 11) if take >= 11 else (17, take - 3))
            i += take
        elif v != 0 and run >= 4:
            out.append((v, None))
            take = min(run - 1, 6)
            out.append((16, take - 3))
            i += 1 + take
        else:
            out.append((v, None))
            i += 1
    return out


def rle_spans(rle):
    """(start, end) in the length sequence of every run symbol of an rle list"""
    spans, n = [], 0
    for sym, extra in rle:
        if sym < 16:
            n += 1
            continue
        rep = (3 + extra) if sym in (16, 17) else (11 + extra)
        spans.append((n, n + rep))
        n += rep
    return spans


def write_member(blocks, out_offset=0):
    """-> (the member's bytes, Report).  out_offset: the address of the member's first output byte, for the Report's geometry."""
    sink, rep = BitSink(), Report(out_offset)
    for bi, b in enumerate(blocks):
        final = b.final if b.final is not None else int(bi == len(blocks) - 1)
        rep.starts.append(sink.bitpos & 7)
        rep.block_out.append(rep.out_len)
        sink.bits(final, 1)
        if isinstance(b, Stored):
            rep.kinds.append("stored")
            sink.bits(0, 2)
            sink.align()
            n = len(b.data)
            sink.bits(n & 0xFFFF, 16)
            sink.bits((n ^ 0xFFFF) & 0xFFFF if b.nlen is None else b.nlen, 16)
            sink.raw(b.data)
            rep.out_len += n
        elif isinstance(b, Fixed):
            rep.kinds.append("fixed")
            sink.bits(1, 2)
            write_tokens(sink, b.tokens, FIXED_LIT, FIXED_DIST, rep, b.eob)
        else:
            rep.kinds.append("dynamic")
            sink.bits(2, 2)
            hlit = b.hlit if b.hlit is not None else max(257, max((s + 1 for s, l in enumerate(b.lit_lens) if l), default=0))
            hdist = b.hdist if b.hdist is not None else max(1, max((s + 1 for s, l in enumerate(b.dist_lens) if l), default=0))
            lit_lens = (b.lit_lens + [0] * hlit)[:hlit]
            dist_lens = (b.dist_lens + [0] * hdist)[:hdist]
            seq = lit_lens + dist_lens
            rle = b.rle if isinstance(b.rle, list) else (rle_greedy(seq) if b.rle == "greedy" else [(l, None) for l in seq])
            if b.cl_lens is None:
                f = [0] * 19
                for s, _ in rle:
                    f[s] += 1
                cl_lens = limited_lengths(f, 7)
            else:
                cl_lens = list(b.cl_lens)
            hclen = b.hclen if b.hclen is not None else max(4, max((i + 1 for i, s in enumerate(CL_ORDER) if cl_lens[s]), default=0))
            sink.bits(hlit - 257, 5)
            sink.bits(hdist - 1, 5)
            sink.bits(hclen - 4, 4)
            for i in range(hclen):
                sink.bits(cl_lens[CL_ORDER[i]], 3)
            cl_codes = canonical_codes(cl_lens)
            for s, extra in rle:
                if not cl_lens[s]:
                    raise ValueError(f"code-length symbol {s} has no code")
                sink.code(cl_codes[s], cl_lens[s])
                if s >= 16:
                    sink.bits(extra, {16: 2, 17: 3, 18: 7}[s])
            rep.headers.append(dict(hlit=hlit, hdist=hdist, hclen=hclen, cl_lens=cl_lens, rle_symbols=sorted({s for s, _ in rle if s >= 16}),
                                    run_crosses_boundary=any(a < hlit < e for a, e in rle_spans(rle)),
                                    kraft=(kraft(lit_lens), kraft(dist_lens), kraft(cl_lens))))
            write_tokens(sink, b.tokens, lit_lens, dist_lens, rep, b.eob)
    return sink.getvalue(), rep
