"""The device deflater's test code held to its own claims, on any CPU: the token-level reader (tests/deflate_reader.py) against zlib's
streams and against the writer's corpus, the restated kernel rules (tests/deflate_device_model.py) against zlib's inflate and against
the writer's length-limited Huffman, every claim of the crafted corpus under the model, and the verifier against token lists it
must refuse.  tests/test_gpu_deflate_crafted.py rests on all of it."""
import random
import zlib

import numpy as np
import pytest

from tests import deflate_corpus as dc
from tests import deflate_device_model as dm
from tests import deflate_reader as dr
from tests import deflate_writer as dw


def raw(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_every=None):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    if flush_every is None:
        return c.compress(data) + c.flush()
    out = b""
    for o in range(0, len(data), flush_every):
        out += c.compress(data[o:o + flush_every]) + c.flush(zlib.Z_FULL_FLUSH)
    return out + c.flush()


def all_tokens(blocks):
    return [t for b in blocks for t in b.tokens]


TEXT = b"".join(b"@SIM:1:%d 1:N:0 BC:ACGTACGT+TTGCAAGG the quick brown fox %d\n" % (i, i * i) for i in range(900))


def test_reader_reads_zlibs_own_streams():
    rng = np.random.default_rng(3)
    noise = rng.integers(0, 5, 40000, dtype=np.uint8).tobytes()
    inputs = [b"", b"A", TEXT, noise, bytes(70000), rng.integers(0, 256, 3000, dtype=np.uint8).tobytes() * 9]
    kinds = set()
    for data in inputs:
        for kw in (dict(level=1), dict(level=6), dict(level=9), dict(strategy=zlib.Z_FIXED), dict(strategy=zlib.Z_HUFFMAN_ONLY), dict(flush_every=7001), dict(level=0)):
            payload = raw(data, **kw)
            blocks = dr.read_member(payload)
            assert bytes(dw.apply_tokens(all_tokens(blocks), bytearray())) == data == zlib.decompress(payload, wbits=-15)
            assert -(-dr.member_bits(blocks) // 8) == len(payload) and blocks[-1].final and not any(b.final for b in blocks[:-1])
            if kw.get("strategy") == zlib.Z_HUFFMAN_ONLY:
                assert not any(b.matches for b in blocks)
            if kw.get("strategy") == zlib.Z_FIXED:
                assert {b.kind for b in blocks} <= {"fixed", "stored"}
            if "flush_every" in kw and len(data) > 7001:
                assert len(blocks) >= 2 * (len(data) // 7001)
            kinds |= {b.kind for b in blocks}
    assert kinds == {"stored", "fixed", "dynamic"}


def test_reader_gives_back_what_the_writer_was_given():
    """over the writer's valid corpus: the block kinds, the header counts and the code-length lengths the writer reports, every match
    where the writer put it, and the literals between them (the tokens make the member's intended bytes)"""
    seen = 0
    for c in dc.corpus_valid(0):
        blocks = dr.read_member(c.payload)
        assert [b.kind for b in blocks] == c.report.kinds, c.name
        assert [m for b in blocks for m in b.matches] == c.report.matches, c.name
        assert bytes(dw.apply_tokens(all_tokens(blocks), bytearray())) == c.out, c.name
        dyn = [b for b in blocks if b.kind == "dynamic"]
        assert [(b.hlit, b.hdist, b.hclen, b.cl_lens) for b in dyn] == [(h["hlit"], h["hdist"], h["hclen"], (h["cl_lens"] + [0] * 19)[:19]) for h in c.report.headers], c.name
        assert [b.start_bit & 7 for b in blocks] == c.report.starts, c.name
        seen += 1
    assert seen > dc.RANDOM_MEMBERS


def test_reader_refuses_what_is_invalid_inside_the_stream():
    """a member of corpus_invalid() is invalid INSIDE the stream when zlib, given the payload alone, raises or does not reach the end
    (the others only disagree with the length or the CRC their descriptor announces): the reader raises for exactly those"""
    inside = outside = 0
    for c in dc.corpus_invalid():
        try:
            dz = zlib.decompressobj(wbits=-15)
            dz.decompress(bytes(c.payload))
            bad = not dz.eof
        except zlib.error:
            bad = True
        if bad:
            inside += 1
            with pytest.raises(dr.Invalid):
                dr.read_member(c.payload)
        else:
            outside += 1
            dr.read_member(c.payload)
    assert inside >= 40 and outside >= 5


def test_code_lengths_against_the_writers_length_limited_huffman():
    def cost(freq, lens):
        return sum(f * l for f, l in zip(freq, lens))

    rng = random.Random(11)
    # without ties (distinct powers-of-two-free weights would still tie in sums: draw until the merge meets none) and no deeper than 15
    done = 0
    while done < 60:
        n = rng.choice([2, 3, 5, 30, 100, 286])
        freq = [0] * n
        for s in rng.sample(range(n), rng.randrange(2, n + 1)):
            freq[s] = rng.randrange(1, 1 << 20) * 2 + rng.randrange(2)
        lens, shift = dm.code_lengths(freq, n)
        want = dw.limited_lengths(freq, 15)
        if shift or max(want) > 15:
            continue
        done += 1
        assert dw.kraft(lens) == 32768 and all((l > 0) == (f > 0) for l, f in zip(lens, freq))
        assert cost(freq, lens) == cost(freq, want)                  # both are Huffman codes: the total cost is the optimum
    # with ties: small counts, many equal
    for _ in range(200):
        n = rng.choice([2, 4, 30, 286])
        freq = [rng.choice([0, 1, 1, 2, 3, 5]) for _ in range(n)]
        if sum(1 for f in freq if f) < 2:
            continue
        lens, shift = dm.code_lengths(freq, n)
        assert shift == 0 and dw.kraft(lens) == 32768 and cost(freq, lens) == cost(freq, dw.limited_lengths(freq, 15))
    # the edges: nothing used, one symbol used (lines 120-129)
    assert dm.code_lengths([0] * 30, 30) == ([1] + [0] * 29, 0)
    assert dm.code_lengths([0, 0, 7, 0], 4) == ([0, 0, 1, 0], 0)
    # Fibonacci weights: the chain is as deep as the alphabet, and the retry halves until it fits
    fib = [1, 1]
    while len(fib) < 24:
        fib.append(fib[-1] + fib[-2])
    assert max(dm.code_lengths(fib[:16], 16)[0]) == 15 and dm.code_lengths(fib[:16], 16)[1] == 0
    for k in (17, 20, 24):
        lens, shift = dm.code_lengths(fib[:k], k)
        assert shift >= 1 and max(lens) <= 15 and dw.kraft(lens) == 32768 and all(lens)


def test_render_of_the_reference_tokens_inflates_and_every_claim_holds():
    """every corpus block: the model's tokens pass the model's own verifier, its rendering is a stream zlib inflates to the block, the
    reader reads the rendering back as the tokens and lengths that went in, and the case's claim holds"""
    lengths, distances, deepest, biggest = set(), set(), [0, 0], 0
    for c in dm.corpus():
        toks = dm.reference_tokens(c.data)
        ll, dl, shifts = dm.model_lengths(toks)
        payload = dm.render(toks, ll, dl)
        assert zlib.decompress(payload, wbits=-15) == c.data, c.name
        if c.claim or len(c.data) < 3000:
            (b,) = dr.read_member(payload)
            assert (b.final, b.btype, b.hlit, b.hdist, b.hclen, b.cl_lens) == (1, 2, 286, 30, 19, dm.PRE_LEN), c.name
            assert b.tokens == toks and b.lit_lens == ll and b.dist_lens == dl and -(-b.bits // 8) == len(payload), c.name
            seen = dm.verify_tokens(c.data, toks)
            assert seen.highest_always
            lengths |= seen.lengths
            distances |= seen.distances
        dm.check_claim(c, toks)
        deepest = [max(deepest[0], max(ll)), max(deepest[1], max(dl))]
        biggest = max(biggest, len(payload))
    assert lengths >= set(dm.LENGTHS) and 3 not in lengths and max(lengths) == 258
    assert distances >= set(dm.DISTANCES) and max(distances) == 32768
    assert deepest[1] == 15 and deepest[0] >= 14
    assert biggest <= 81920
    # the two cases test_gpu_deflate.py's corpus() takes: both shrink, so the framed path carries the device's payload
    for c in (dm.far_match_case(), dm.retry_case()):
        assert len(dm.model_payload(c.data)) < len(c.data) + 5 and len(c.data) <= dm.MAX_IN
    # the names say what the corpus must hold
    names = [c.name for c in dm.crafted()]
    assert len(set(names)) == len(names) and len(dm.random_part()) == dm.RANDOM_BLOCKS
    assert {len(c.data) for c in dm.crafted()} >= set(range(0, 9)) | set(range(61, 69))
    assert {len(c.data) for c in dm.random_part()} >= {0, dm.MAX_IN}


def test_verifier_refuses_other_parses():
    text = TEXT[:20000]
    good = dm.reference_tokens(text)
    dm.verify_tokens(text, good)
    # zlib's level-1 tokens: a legal parse of the text, not this parse
    theirs = all_tokens(dr.read_member(raw(text, level=1)))
    assert bytes(dw.apply_tokens(theirs, bytearray())) == text
    with pytest.raises(AssertionError):
        dm.verify_tokens(text, theirs)
    # a match shortened by one (the byte it leaves follows as a literal)
    i = next(i for i, t in enumerate(good) if not isinstance(t, int) and t[0] > 4)
    p = sum(1 if isinstance(t, int) else t[0] for t in good[:i])
    short = good[:i] + [(good[i][0] - 1, good[i][1]), text[p + good[i][0] - 1]]
    with pytest.raises(AssertionError):
        dm.verify_tokens(text, short)
    # a match from an older occurrence than the table can hold: A, A with its last byte changed, A — the third's slot holds the second
    rng = np.random.default_rng(5)
    a = rng.integers(1, 255, 64, dtype=np.uint8).tobytes()
    data = a + a[:63] + bytes([a[63] + 1]) + a + b"\x00\x01\x02\x03"
    toks = dm.reference_tokens(data)
    assert toks[64:] == [(63, 64), a[63] + 1, (63, 64), a[63], 0, 1, 2, 3]
    dm.verify_tokens(data, toks)
    older = toks[:66] + [(64, 128)] + toks[68:]
    assert bytes(dw.apply_tokens(older, bytearray())) == data
    with pytest.raises(AssertionError):
        dm.verify_tokens(data, older)
    # a distance of 32769
    far = next(c for c in dm.crafted() if c.name.startswith("distance 32769"))
    toks = dm.reference_tokens(far.data)
    q = far.claim["literal_at"]
    i = next(i for i in range(len(toks)) if sum(1 if isinstance(t, int) else t[0] for t in toks[:i]) == q)
    assert toks[i:i + 8] == list(far.data[q:q + 8])
    with pytest.raises(AssertionError):
        dm.verify_tokens(far.data, toks[:i] + [(8, 32769)] + toks[i + 8:])
    # a literal where every candidate matches
    near = next(c for c in dm.crafted() if c.name == "distance 96")
    toks = dm.reference_tokens(near.data)
    i = next(i for i, t in enumerate(toks) if t == near.claim["at"][1])
    with pytest.raises(AssertionError):
        dm.verify_tokens(near.data, toks[:i] + list(near.data[96:104]) + toks[i + 1:])
    # tokens that stop short of the block, or run past it
    with pytest.raises(AssertionError):
        dm.verify_tokens(text, good[:-1])
    with pytest.raises(AssertionError):
        dm.verify_tokens(text, good + [65])
