"""bgzf_deflate_kernel's rules (seqkit_amd/csrc/sk_deflate.hip), restated in plain Python, and a crafted corpus that reaches what the
kernel has a path for.  The line numbers are sk_deflate.hip's.

Candidates          phase A's hash table (lines 243-269).  Positions go 64 at a time, a lane each.  A position p with p + 4 <= n (line
                    247) hashes its four little-endian bytes, (v * 2654435761 mod 2^32) >> 20 (line 250), and looks its candidate up
                    BEFORE the chunk's own positions go in (line 251 reads, the fence of line 268, line 269 writes).  Several lanes of
                    a chunk may write one slot, and which lane's write stays is the hardware's choice, so the statement is a set:
                    C(p) = every position with p's hash in the latest earlier chunk that holds any.
outcome()           lines 252-266: a candidate c is a match when p - c <= 32768 (line 255) and the four bytes are equal (line 255); its
                    length is the common prefix capped at min(258, n - p) (lines 257-263); anything else is the literal.
verify_tokens()     the greedy walk of lines 271-278 over somebody's tokens: every token must be the outcome of a member of C(p).
reference_tokens()  the same walk, the highest position of C(p) chosen.
code_lengths()      def_huffman (lines 106-185): ranks, the two-queue merge, depths, the retry with halved frequencies.
render()            phase C (lines 341-389) through tests/deflate_writer.py: BFINAL 1, dynamic, HLIT 286, HDIST 30, HCLEN 19, the fixed
                    code-length lengths of kPreLen (line 61), no run symbols.
corpus()            the crafted blocks, seeded; each carries a claim that check_claim() holds it to."""
import functools
from collections import namedtuple

import numpy as np

from tests import deflate_writer as dw

MAX_IN = 0xff00                              # kDefMaxIn (line 43)
HASH_BITS = 12                               # kDefHashBits (line 42)
MAX_DIST = 32768                             # line 255
PRE_LEN = [4, 5, 5, 5, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 5, 5, 5]      # kPreLen (line 61)
N_LL, N_D = 286, 30                          # kNLL, kND (line 44)


# ---- phase A ----------------------------------------------------------------------------------------------------------------------
def words_and_hashes(data):
    """(v, h) of every position p with p + 4 <= n: the four bytes little-endian (def_load4, lines 74-81) and their hash (line 250)"""
    a = np.frombuffer(bytes(data), dtype=np.uint8).astype(np.uint64)
    m = max(0, len(a) - 3)
    v = a[:m] | (a[1:m + 1] << np.uint64(8)) | (a[2:m + 2] << np.uint64(16)) | (a[3:m + 3] << np.uint64(24))
    h = ((v * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - HASH_BITS)
    return v, h.astype(np.int64)


class Candidates:
    """C(p) for every position of one block: of(p) -> the positions, ascending ([] for none, and for the last three positions)"""

    def __init__(self, data):
        self.n = len(data)
        self.v, h = words_and_hashes(data)
        m = len(h)
        if m == 0:
            self.order, self.lo, self.hi, self.vl = np.zeros(0, dtype=np.int64), [], [], []
            return
        pos = np.arange(m, dtype=np.int64)
        key = h * 1024 + (pos >> 6)                                  # (hash, chunk): a block has at most 1020 chunks
        order = np.argsort(key, kind="stable")                       # positions by hash, then chunk, then position
        skey = key[order]
        first = np.ones(m, dtype=bool)
        first[1:] = skey[1:] != skey[:-1]
        gstart = np.flatnonzero(first)                               # where each (hash, chunk) group begins in `order`
        gid = np.cumsum(first) - 1
        ghash = skey[gstart] >> 10
        # the group before p's own, when it has the same hash, is the latest earlier chunk that holds p's hash
        has = np.zeros(len(gstart), dtype=bool)
        has[1:] = ghash[1:] == ghash[:-1]
        lo = np.where(has, np.concatenate(([0], gstart[:-1])), 0)
        hi = np.where(has, gstart, 0)
        g_of = np.empty(m, dtype=np.int64)
        g_of[order] = gid
        self.order = order
        self.lo, self.hi = lo[g_of].tolist(), hi[g_of].tolist()      # C(p) = order[lo[p] : hi[p]]
        self.vl = self.v.tolist()

    def of(self, p):
        if p + 4 > self.n:
            return []
        return self.order[self.lo[p]:self.hi[p]].tolist()

    def highest(self, p):
        if p + 4 > self.n or self.hi[p] == self.lo[p]:
            return -1
        return int(self.order[self.hi[p] - 1])


def common_prefix(data, c, p, cap):
    a, b = data[c:c + cap], data[p:p + cap]
    if a == b:
        return cap
    l = 0
    while a[l] == b[l]:
        l += 1
    return l


def outcome(data, cands, c, p):
    """what the kernel makes of candidate c at position p: (length, distance) or the literal"""
    if p - c <= MAX_DIST and cands.vl[c] == cands.vl[p]:
        return (common_prefix(data, c, p, min(258, len(data) - p)), p - c)
    return data[p]


Seen = namedtuple("Seen", "lengths distances ambiguous highest_always tokens")


def verify_tokens(data, tokens):
    """walks `tokens` over `data` as lines 271-278 walk the chunk's lengths; raises AssertionError on a token the kernel's rules do
    not allow.  Returns Seen: the lengths and distances met, at how many token positions more than one outcome was legal, and whether
    the choice was the highest position's every time."""
    data = bytes(data)
    cands = Candidates(data)
    p, n = 0, len(data)
    lengths, distances, ambiguous, highest_always = set(), set(), 0, True
    for i, t in enumerate(tokens):
        assert p < n, f"token {i} begins behind the block's {n} bytes"
        cs = cands.of(p)
        if not cs:
            legal = [data[p]]
        elif len(cs) == 1:
            legal = [outcome(data, cands, cs[0], p)]
        else:
            legal = [outcome(data, cands, c, p) for c in cs]
        t = t if isinstance(t, int) else tuple(t)
        assert t in legal, f"token {i} at position {p}: {t!r} is not among the outcomes {sorted(set(map(repr, legal)))} of candidates {cs[-4:]}"
        if len(set(legal)) > 1:
            ambiguous += 1
            if t != legal[-1]:
                highest_always = False
        if isinstance(t, int):
            p += 1
        else:
            lengths.add(t[0])
            distances.add(t[1])
            p += t[0]
    assert p == n, f"the tokens cover {p} bytes of {n}"
    return Seen(lengths, distances, ambiguous, highest_always, len(tokens))


def reference_tokens(data):
    data = bytes(data)
    cands = Candidates(data)
    toks, p, n = [], 0, len(data)
    while p < n:
        c = cands.highest(p)
        t = outcome(data, cands, c, p) if c >= 0 else data[p]
        toks.append(t)
        p += 1 if isinstance(t, int) else t[0]
    return toks


# ---- phase B ----------------------------------------------------------------------------------------------------------------------
def code_lengths(freq, n):
    """def_huffman (lines 106-185) over freq[0 .. n): (lengths, the shift at which the code came out no deeper than 15)"""
    freq = list(freq[:n])
    used = [s for s in range(n) if freq[s]]
    lens = [0] * n
    if not used:                                                     # lines 120-124
        lens[0] = 1
        return lens, 0
    if len(used) == 1:                                               # lines 125-129
        lens[used[0]] = 1
        return lens, 0
    shift = 0
    while True:                                                      # line 112
        order = sorted(used, key=lambda s: (max(1, freq[s] >> shift), s))         # lines 130-143
        k = len(order)
        w = [max(1, freq[s] >> shift) for s in order] + [0] * (k - 1)
        parent = [0] * (2 * k - 1)
        li, ii, made = 0, k, k                                       # lines 147-165
        while made < 2 * k - 1:
            pick = []
            for _ in range(2):
                leaf_ok, int_ok = li < k, ii < made
                take_leaf = leaf_ok
                if leaf_ok and int_ok:
                    take_leaf = w[li] <= w[ii]
                if take_leaf:
                    pick.append(li)
                    li += 1
                else:
                    pick.append(ii)
                    ii += 1
            w[made] = w[pick[0]] + w[pick[1]]
            parent[pick[0]] = parent[pick[1]] = made
            made += 1
        depth = [0] * (2 * k - 1)                                    # lines 167-172
        for i in range(2 * k - 3, -1, -1):
            depth[i] = depth[parent[i]] + 1
        if max(depth[:k]) > 15:                                      # lines 174-181
            shift += 1
            continue
        for r, s in enumerate(order):                                # line 182
            lens[s] = depth[r]
        return lens, shift


def histograms(tokens):
    """the two histograms of lines 288-300, the end-of-block symbol counted"""
    lf, df = dw.used_symbols(tokens)
    return lf[:N_LL], df[:N_D]


def model_lengths(tokens):
    """(literal/length lengths, distance lengths, the two shifts) the kernel gives these tokens"""
    lf, df = histograms(tokens)
    ll, s1 = code_lengths(lf, N_LL)
    dl, s2 = code_lengths(df, N_D)
    return ll, dl, (s1, s2)


# ---- phase C ----------------------------------------------------------------------------------------------------------------------
def render(tokens, lit_lens, dist_lens):
    payload, _ = dw.write_member([dw.Dynamic(tokens, lit_lens, dist_lens, hlit=286, hdist=30, hclen=19, cl_lens=PRE_LEN, rle="none", final=1)])
    return payload


def model_payload(data):
    toks = reference_tokens(data)
    ll, dl, _ = model_lengths(toks)
    return render(toks, ll, dl)


# ---- the corpus -------------------------------------------------------------------------------------------------------------------
# claim: a dict, checked by check_claim() against a token list (the model's on the CPU, the device's on the GPU):
#   at: (position, (length, distance))   that token begins at that position (C(position) has one member, so the device has no choice)
#   literal_at: position                 a literal begins there
#   match: (min length, min distance)    some match is at least that long and that far
#   shift: (alphabet, minimum)           def_huffman's retry ran for alphabet 0 (literal/length) or 1 (distance)
#   depth: (alphabet, minimum)           the deepest code of that alphabet
#   one_dist_symbol / no_match           the distance alphabet is one used symbol / unused
#   skip: chunks                         some match covers that many whole chunks behind its own
#   overlap: distance                    some match of that distance is longer than its distance
#   shrinks / stored                     the payload is below / at least the input's bytes + 5 (the caller's rule for a stored member)
Case = namedtuple("Case", "name data claim")

DISTANCES = sorted({d for b, e in zip(dw.DIST_BASE, dw.DIST_EXTRA) for d in (b, b + (1 << e) - 1)})      # both ends of every symbol's range
LENGTHS = list(range(4, 259))


def _nonzero(rng, n):
    return rng.integers(1, 256, n, dtype=np.uint8).tobytes()


def _length_block(rng, L):
    """P (L nonzero bytes), zeros to the next chunk boundary and 64 more, P again, a byte that differs from the zero behind the first
    P, three more.  The zeros share one hash slot, so P's stays; the zeros' own matches end where P comes back."""
    q = (L // 64 + 1) * 64 + 64
    P = _nonzero(rng, L)
    return P + bytes(q - L) + P + _nonzero(rng, 4), q


def _distance_block(rng, d):
    """d <= 64: random bytes up to position 64 - d, from there on a period of d bytes, so that the token at 64 is (., d) and the only
    earlier occurrence is at 64 - d.  d > 64: P (8 bytes), zeros, P again at d, four bytes that differ."""
    if d <= 64:
        per = _nonzero(rng, d)
        ext = (per * (40 // d + 2))[:d + 40 - (d % 7)]
        return _nonzero(rng, 64 - d) + ext + _nonzero(rng, 4), 64
    P = _nonzero(rng, 8)
    return P + bytes(d - 8) + P + _nonzero(rng, 4), d


def _seeded(build, seed, tries=40):
    """the first seed from `seed` on whose block holds its claim under the model (a slot that was hit: the next seed)"""
    for k in range(tries):
        data, claim = build(np.random.default_rng(seed + 1000 * k))
        if check_claim(Case("", data, claim), reference_tokens(data), raise_=False):
            return data, claim
    raise AssertionError("no seed holds the claim")


def _retry_block(rng):
    """13056 groups [s, n0, 16 + n1, 32 + n2, 48 + n3]: s from 20 symbols with Fibonacci counts (an unbounded Huffman code of them and
    the 64 evenly used nibble bytes is deeper than 15 bits), the nibbles of (i * 40503) & 0xffff keep the matcher nearly quiet"""
    fib = [1, 1]
    while len(fib) < 20:
        fib.append(fib[-1] + fib[-2])
    s = np.concatenate([np.full(f, 64 + i, dtype=np.uint8) for i, f in enumerate(fib)])
    rng.shuffle(s)
    s = s[:13056]
    i = (np.arange(13056, dtype=np.uint32) * 40503) & 0xffff
    g = np.stack([s, (i & 15), 16 + ((i >> 4) & 15), 32 + ((i >> 8) & 15), 48 + ((i >> 12) & 15)], axis=1).astype(np.uint8)
    return g.tobytes()


def _deep_distance_block(rng, n_symbols):
    """4-byte copies at nine lanes of every chunk, from sources the hash table still holds alone, at distances whose symbols
    (12 .. 12 + n_symbols - 1, the farthest the rarest) have Fibonacci counts: the distance code is a chain"""
    n = MAX_IN
    data = bytearray(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
    fib = [1, 1]
    while len(fib) < n_symbols:
        fib.append(fib[-1] + fib[-2])
    plan = [12 + n_symbols - 1 - i for i, f in enumerate(fib) for _ in range(f)]
    plan = [plan[int(j)] for j in rng.permutation(len(plan))]
    table = {}                                                       # hash -> the positions of the latest chunk that holds it
    mult = 2654435761

    def h_at(p):
        return ((int.from_bytes(data[p:p + 4], "little") * mult) & 0xFFFFFFFF) >> (32 - HASH_BITS)

    for start in range(0, n - 64, 64):
        if start >= 128:
            for lane in range(8, 52, 5):
                if not plan:
                    break
                p = start + lane
                for k in range(min(len(plan), 12)):                  # the first of the next few planned symbols that can be placed here
                    sym = plan[k]
                    lo, hi = dw.DIST_BASE[sym], dw.DIST_BASE[sym] + (1 << dw.DIST_EXTRA[sym]) - 1
                    src = -1
                    for d in rng.integers(lo, hi + 1, 24).tolist():
                        c = p - d
                        if c >= 0 and c + 8 <= start and table.get(h_at(c)) == [c] and data[c + 4] != data[p + 4]:
                            keep = data[p:p + 4]
                            data[p:p + 4] = data[c:c + 4]
                            # the three positions before p must stay literals (a copy of a copy may have a twin one byte earlier)
                            if not any(data[x:x + 4] == data[q:q + 4] for q in (p - 3, p - 2, p - 1) for x in table.get(h_at(q), ())):
                                src = c
                                break
                            data[p:p + 4] = keep
                    if src >= 0:
                        plan.pop(k)
                        break
        chunk = {}
        for p in range(start, min(start + 64, n - 3)):
            chunk.setdefault(h_at(p), []).append(p)
        table.update(chunk)
    return bytes(data), len(plan)


def _mixture(rng, n):
    """a drawn mixture of text, few-letter noise, runs and copies from drawn distances"""
    words = [rng.integers(97, 123, int(rng.integers(2, 11)), dtype=np.uint8).tobytes() for _ in range(60)]
    out = bytearray()
    while len(out) < n:
        kind = int(rng.integers(0, 5))
        k = int(rng.integers(1, 3000))
        if kind == 0:
            out += b" ".join(words[int(j)] for j in rng.integers(0, 60, k // 6 + 1))
        elif kind == 1:
            out += rng.integers(0, int(rng.integers(2, 7)), k, dtype=np.uint8).tobytes()
        elif kind == 2:
            out += bytes(rng.integers(0, 256, k // 20 + 1, dtype=np.uint8).repeat(int(rng.integers(2, 40))))
        elif kind == 3 and out:
            d = int(rng.integers(1, min(len(out), MAX_DIST + 600) + 1))
            for _ in range(int(rng.integers(1, 6))):
                m = int(rng.integers(4, 400))
                out += out[len(out) - d:len(out) - d + m] if d >= m else (out[len(out) - d:] * (m // d + 1))[:m]
                out += rng.integers(0, 256, int(rng.integers(1, 5)), dtype=np.uint8).tobytes()
        else:
            out += rng.integers(0, 256, k // 4 + 1, dtype=np.uint8).tobytes()
    return bytes(out[:n])


RANDOM_BLOCKS = 200


@functools.lru_cache(maxsize=None)
def crafted():
    """the crafted cases (every one small enough, or compressible enough, to be looked at token by token)"""
    out = []
    # every match length
    for L in LENGTHS:
        def build(rng, L=L):
            data, q = _length_block(rng, L)
            return data, {"at": (q, (L, q))}
        out.append(Case(f"length {L}", *_seeded(build, 7000 + L)))
    # every distance symbol at both ends of its extra-bit range; below the length: an overlapping match
    for d in DISTANCES:
        def build(rng, d=d):
            data, q = _distance_block(rng, d)
            claim = {"at": (q, (len(data) - 4 - q, d))}
            if d <= 4:
                claim["overlap"] = d
            return data, claim
        out.append(Case(f"distance {d}", *_seeded(build, 9000 + d)))

    def build(rng):
        data, q = _distance_block(rng, MAX_DIST + 1)
        return data, {"literal_at": q}
    out.append(Case("distance 32769: the candidate is refused", *_seeded(build, 9999)))
    # codes that need the retry, deep codes
    out.append(retry_case())
    data, left = _deep_distance_block(np.random.default_rng(37), 15)
    assert left == 0
    out.append(Case("a deep distance code: 15 symbols, Fibonacci counts", data, {"depth": (1, 13)}))
    data, left = _deep_distance_block(np.random.default_rng(39), 16)
    assert left == 0
    out.append(Case("the deepest distance code there is: 16 symbols, Fibonacci counts", data, {"depth": (1, 15)}))
    data, left = _deep_distance_block(np.random.default_rng(41), 17)
    assert left == 0
    out.append(Case("a distance code that needs the retry: 17 symbols, Fibonacci counts", data, {"shift": (1, 1)}))
    # lone codes
    rng = np.random.default_rng(43)
    r64 = _nonzero(rng, 64)
    out.append(Case("one match: a lone distance code", r64 + r64[:8] + _nonzero(rng, 5), {"one_dist_symbol": True}))
    out.append(Case("no match: the unused 1-bit code on distance symbol 0", _nonzero(rng, 100), {"no_match": True}))
    out.append(Case("empty block: the lone end-of-block code", b"", {"no_match": True}))
    # block ends
    for n in list(range(1, 9)) + list(range(61, 69)):
        out.append(Case(f"{n} random bytes", _nonzero(rng, n), {"no_match": True}))
        out.append(Case(f"{n} equal bytes", b"A" * n, {"match": (4, 1)} if n == 68 else {"no_match": True}))
    r64 = _nonzero(rng, 64)
    out.append(Case("a match at p = n - 4 that ends on the last byte", r64 + r64[:4], {"at": (64, (4, 64))}))
    for k in (1, 2, 3):
        out.append(Case(f"{k} bytes behind the chunk: no position can match", r64 + r64[:k], {"no_match": True}))
    r100 = _nonzero(rng, 100)
    out.append(Case("a match that would run past the block's end (maxl = n - p)", r100 + bytes(28) + r100[:37], {"at": (128, (37, 128))}))
    out.append(Case("zeros, 64 + 100: the match is cut at the end", bytes(164), {"match": (100, 1)}))
    out.append(Case("zeros, 64 + 258 + 3: 258 and more available", bytes(64 + 258 + 3), {"match": (258, 1), "skip": 3}))
    r400 = _nonzero(rng, 400)
    out.append(Case("a match skips one whole chunk", r400[:256] + r400[:130] + _nonzero(rng, 9), {"at": (256, (130, 256)), "skip": 1}))
    out.append(Case("a match skips two whole chunks", r400[:256] + r400[:200] + _nonzero(rng, 9), {"at": (256, (200, 256)), "skip": 2}))
    out.append(Case("a match of 258 of 300 available, then the rest", r400[:320] + r400[:300] + _nonzero(rng, 9), {"at": (320, (258, 320)), "skip": 3}))
    out += [far_match_case(), Case("far matches, a two-letter filler between", _far_block((b"ab" * 16100)), {"match": (250, 30000), "shrinks": True})]
    # the largest payloads: nothing to match and nothing to gain, a full block (the caller stores it; the slot must still hold it)
    out.append(Case("random bytes, a full block: the payload is larger than the input", np.random.default_rng(61).integers(0, 256, MAX_IN, dtype=np.uint8).tobytes(), {"stored": True}))
    flat = np.random.default_rng(67).permutation(np.arange(MAX_IN, dtype=np.uint32) % 255).astype(np.uint8)
    out.append(Case("255 byte values equally often, a full block: codes of 7 and 8 bits next to the end-of-block's", flat.tobytes(), {"stored": True}))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def random_part():
    rng = np.random.default_rng(20250607)
    out = []
    for i in range(RANDOM_BLOCKS):
        n = int(rng.integers(0, MAX_IN + 1)) if i % 8 else int(rng.choice([0, 1, 63, 64, 65, MAX_IN, MAX_IN - 1, 4096]))
        out.append(Case(f"random {i}: {n} bytes", _mixture(rng, n), {}))
    return tuple(out)


def corpus():
    return list(crafted()) + list(random_part())


def _far_block(filler):
    """a 500-byte phrase that comes back after 30000 and again after 32000 bytes of a filler that leaves its hash slots alone"""
    ph = _nonzero(np.random.default_rng(47), 500)
    return ph + filler[:30000] + ph + filler[:32000] + ph


@functools.lru_cache(maxsize=None)
def far_match_case():
    return Case("far matches, zeros between", _far_block(bytes(32000)), {"match": (250, 30000), "shrinks": True})


@functools.lru_cache(maxsize=None)
def retry_case():
    return Case("a literal/length code that needs the retry", _retry_block(np.random.default_rng(31)), {"shift": (0, 1), "shrinks": True})


def check_claim(case, tokens, raise_=True):
    """holds `case` to its claim under `tokens` (whoever made them)"""
    claim, data = case.claim, case.data
    starts, p = {}, 0
    for t in tokens:
        starts[p] = t
        p += 1 if isinstance(t, int) else t[0]
    matches = [(q, t) for q, t in starts.items() if not isinstance(t, int)]
    ok = p == len(data)
    for key, want in claim.items():
        if key == "at":
            q, t = want
            ok &= starts.get(q) == t and Candidates(data).of(q) == [q - t[1]]
        elif key == "literal_at":
            ok &= isinstance(starts.get(want), int)
        elif key == "match":
            ok &= any(t[0] >= want[0] and t[1] >= want[1] for _, t in matches)
        elif key in ("shift", "depth"):
            ll, dl, shifts = model_lengths(tokens)
            got = shifts[want[0]] if key == "shift" else max((ll, dl)[want[0]])
            ok &= got >= want[1]
        elif key == "one_dist_symbol":
            ok &= sum(1 for f in histograms(tokens)[1] if f) == 1
        elif key == "no_match":
            ok &= not matches
        elif key == "skip":
            ok &= any((q + t[0]) // 64 - q // 64 - 1 >= want for q, t in matches)
        elif key == "overlap":
            ok &= any(t[1] == want and t[0] > want for _, t in matches)
        elif key in ("shrinks", "stored"):
            ll, dl, _ = model_lengths(tokens)
            ok &= (len(render(tokens, ll, dl)) < len(data) + 5) == (key == "shrinks")
        else:
            raise KeyError(key)
        if raise_:
            assert ok, f"{case.name}: the claim {key} = {want!r} does not hold"
    return bool(ok)
