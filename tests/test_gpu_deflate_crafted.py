"""bgzf_deflate_kernel held to a token-level model on crafted inputs (tests/deflate_device_model.py; tests/test_deflate_device_model.py
holds the model, the reader and the corpus to their claims on any CPU).  A round trip through zlib cannot see a stale hash-table
entry (the kernel compares four bytes before it takes a match), a histogram left over from the wave's previous block (a valid but
worse code) or a matcher that finds nothing; a test that knows which tokens and which code lengths the kernel is supposed to
produce sees all three.  For every block of the device half (sk_bgzf_deflate_dev), at every alignment of its input:
  1  the payload is one final dynamic block in the kernel's dialect (HLIT 286, HDIST 30, HCLEN 19, the fixed code-length lengths),
     it ends in the byte result[2 i] names, zlib inflates it to the input — whether or not the block shrinks;
  2  its tokens are a walk the kernel's rules allow (verify_tokens: every token the outcome of a candidate the table can hold);
  3  its code lengths are def_huffman's for the histogram of its own tokens;
  4  its bytes are the rendering of those tokens with those lengths;
  5  its CRC-32 is zlib's;
  6  nothing behind the payload's last dword in its slot, and nothing between the slots, was written;
  7  the four alignments of a block give the same payload.
Wall time on an MI355X: 40 s; Python's bit-level reading is nearly all of it."""
import subprocess
import sys
import time
import zlib

import numpy as np
import pytest

from tests import deflate_device_model as dm
from tests import deflate_reader as dr
from tests.test_gpu_inflate import Dev
from tests.test_gpu_inflate_crafted import bgzf_members

pytestmark = pytest.mark.gpu

SLOT = 81920                                 # SK_DEFLATE_SLOT
GAP = 64                                     # the canary between slots
MAX_IN = 0xff00


def compute_units():
    """the CU count of GPU 0, by torch's device properties — asked in a child process: this one's HIP runtime is the library's"""
    r = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return int(r.stdout.split()[-1])


def deflate_on_device(ctx, datas, aligns, mod=4, canary=True):
    """one launch of sk_bgzf_deflate_dev over datas[i] laid at in_off = aligns[i] (mod `mod`), gaps of 0xA5 between them, the buffer
    readable 8 bytes behind the end, slots of SLOT + GAP bytes pre-filled with 0xEE.  Returns (payloads, ntok, crc) and asserts check 6."""
    n = len(datas)
    buf = bytearray()
    blocks = np.zeros(n, dtype=ctx.DEFLATE_BLOCK_DTYPE)
    for i, d in enumerate(datas):
        buf += bytes([0xA5]) * ((aligns[i] - len(buf)) % mod)
        assert len(d) <= MAX_IN
        blocks[i] = (len(buf), len(d), 0)
        buf += d
    buf += bytes([0xA5]) * 8
    stride = SLOT + GAP
    dev = Dev(ctx)
    try:
        d_in = dev.put(np.frombuffer(bytes(buf), dtype=np.uint8))
        d_blk = dev.put(blocks.view(np.uint8))
        d_slots = dev.put(np.full(n * stride, 0xEE, dtype=np.uint8)) if canary else dev.empty(n * stride)
        d_tok = dev.empty(n * MAX_IN * 4)
        d_res = dev.put(np.full(2 * n, 0xFFFFFFFF, dtype=np.uint32).view(np.uint8))
        d_crc = dev.put(np.zeros(n, dtype=np.uint32).view(np.uint8))
        assert d_in % 16 == 0
        ctx.bgzf_deflate_dev(d_in, d_blk, n, d_slots, stride, d_tok, d_res, d_crc)
        ctx.sync()
        res = dev.get(d_res, 2 * n, np.uint32)
        crc = dev.get(d_crc, n, np.uint32)
        slots = dev.get(d_slots, n * stride).reshape(n, stride)
    finally:
        dev.close()
    nbytes = res[0::2].astype(np.int64)
    assert (nbytes <= SLOT).all(), f"a payload of {int(nbytes.max())} bytes: beyond the slot"
    if canary:
        written = (nbytes + 3) // 4 * 4                                # whole dwords leave for the slot
        untouched = np.arange(stride)[None, :] >= written[:, None]
        bad = np.flatnonzero(((slots != 0xEE) & untouched).any(axis=1))
        assert not len(bad), f"bytes behind the payload's last dword were written in slots {bad[:10].tolist()}"
    payloads = [slots[i, :int(nbytes[i])].tobytes() for i in range(n)]
    return payloads, res[1::2].tolist(), crc.tolist()


def hold_block(name, data, payload, ntok, crc):
    """checks 1-5; returns (tokens, Seen, literal/length lengths, distance lengths, shifts)"""
    (b,) = dr.read_member(payload)                                     # 1
    assert (b.final, b.btype, b.hlit - 257, b.hdist - 1, b.hclen - 4, b.cl_lens) == (1, 2, 29, 29, 15, dm.PRE_LEN), name
    assert -(-b.bits // 8) == len(payload), (name, b.bits, len(payload))
    assert zlib.decompress(payload, wbits=-15) == data, name
    assert len(b.tokens) == ntok, name
    seen = dm.verify_tokens(data, b.tokens)                            # 2
    ll, dl, shifts = dm.model_lengths(b.tokens)                        # 3
    assert b.lit_lens == ll, (name, "literal/length code lengths", shifts)
    assert b.dist_lens == dl, (name, "distance code lengths", shifts)
    assert payload == dm.render(b.tokens, ll, dl), name                # 4
    assert crc == (zlib.crc32(data) & 0xFFFFFFFF), name                # 5
    return b.tokens, seen, ll, dl, shifts


@pytest.fixture(scope="module")
def device_corpus(ctx):
    """the corpus through the device half, once: every crafted block at in_off = 0, 1, 2, 3 (mod 4), every random block at one of them"""
    crafted, rnd = dm.crafted(), dm.random_part()
    datas, aligns, which = [], [], []
    for j, c in enumerate(crafted):
        for a in range(4):
            datas.append(c.data); aligns.append(a); which.append((j, a))
    for k, c in enumerate(rnd):
        datas.append(c.data); aligns.append(k % 4); which.append((len(crafted) + k, k % 4))
    t0 = time.time()
    payloads, ntok, crc = deflate_on_device(ctx, datas, aligns)
    print(f"launch: {len(datas)} blocks, {sum(map(len, datas))} bytes in, {time.time() - t0:.1f} s with the copies", flush=True)
    return list(crafted) + list(rnd), datas, which, payloads, ntok, crc


def test_every_crafted_block_is_the_models_block(device_corpus):
    cases, datas, which, payloads, ntok, crc = device_corpus
    t0 = time.time()
    lengths, distances, ambiguous, highest_always, positions = set(), set(), 0, True, 0
    deepest, biggest, first = [0, 0], ("", 0), {}
    for i, (j, a) in enumerate(which):
        c = cases[j]
        if j in first:                                                 # 7 (and 5, 6 for every alignment)
            assert payloads[i] == payloads[first[j]], f"{c.name}: the payload at in_off = {a} (mod 4) differs from the one at 0"
            assert ntok[i] == ntok[first[j]] and crc[i] == crc[first[j]], c.name
            continue
        first[j] = i
        toks, seen, ll, dl, shifts = hold_block(c.name, c.data, payloads[i], ntok[i], crc[i])
        dm.check_claim(c, toks)                                        # the case is what its name says, by the device's own tokens
        lengths |= seen.lengths
        distances |= seen.distances
        ambiguous += seen.ambiguous
        positions += seen.tokens
        highest_always &= seen.highest_always
        deepest = [max(deepest[0], max(ll)), max(deepest[1], max(dl))]
        if len(payloads[i]) > biggest[1]:
            biggest = (c.name, len(payloads[i]))
        if c.name == dm.retry_case().name:
            assert shifts[0] >= 1 and max(ll) <= 15, shifts
        if c.name.startswith("a distance code that needs the retry"):
            assert shifts[1] >= 1 and max(dl) <= 15, shifts
    print(f"{len(first)} blocks read token by token in {time.time() - t0:.1f} s: {positions} tokens, {ambiguous} of them at positions with more than one "
          f"legal outcome, the highest position always won: {highest_always}; deepest codes {deepest[0]} (literal/length) and {deepest[1]} (distance) bits; "
          f"largest payload {biggest[1]} bytes ({biggest[0]})", flush=True)
    assert lengths >= set(dm.LENGTHS), sorted(set(dm.LENGTHS) - lengths)
    assert distances >= set(dm.DISTANCES), sorted(set(dm.DISTANCES) - distances)
    assert 32768 in distances and max(distances) <= 32768 and 3 not in lengths and min(lengths) == 4 and max(lengths) == 258
    assert deepest[1] == 15 and deepest[0] >= 14
    assert biggest[1] + 4 <= SLOT                                      # (no case comes within a dword of the slot's end)


def test_crc_at_every_alignment_and_length(ctx):
    """bgzf_crc_out_kernel's head (up to the 16-byte boundary), body (a piece a lane) and tails: in_off mod 16 in 0 .. 15 crossed with
    lengths 0 .. 40, 1023 .. 1025 and 0xff00, in one launch"""
    rng = np.random.default_rng(53)
    lens = list(range(41)) + [1023, 1024, 1025, MAX_IN]
    datas, aligns = [], []
    for a in range(16):
        for n in lens:
            datas.append(rng.integers(0, 256, n, dtype=np.uint8).tobytes()); aligns.append(a)
    payloads, _, crc = deflate_on_device(ctx, datas, aligns, mod=16)
    for d, a, got, p in zip(datas, aligns, crc, payloads):
        assert got == (zlib.crc32(d) & 0xFFFFFFFF), (len(d), a)
        assert zlib.decompress(p, wbits=-15) == d, (len(d), a)


def test_waves_that_take_several_blocks(ctx):
    """more blocks than the launch has waves, so that every wave compresses two blocks in a row and a few a third (the loop of
    `bi += gridDim.x * kDefWaves`, with head, freq and stage made new per block).  launch_bgzf_deflate caps the grid at
    n_cu * per_cu * 4 workgroups of kDefWaves = 4 waves, per_cu = 160 KiB / (4 * sizeof(DefLds)) = 2: n_cu * 32 blocks in flight; this
    test computes it the same way.  The block a wave takes second follows one that leaves the table and the histograms full: the
    first round's blocks begin with zeros (their last all-zero window at position 8) and are rich in matches, the later rounds'
    begin with a run of zeros that has no candidate in its first chunk — a table left over gives it one — and use few symbols."""
    n_cu = compute_units()
    cap = n_cu * 2 * 4 * 4
    n = 2 * cap + 5
    rng = np.random.default_rng(59)
    words = [rng.integers(97, 123, int(rng.integers(2, 9)), dtype=np.uint8).tobytes() for _ in range(40)]
    datas = []
    for i in range(n):
        m = int(rng.integers(200, 601))
        if i < cap:
            kind = i % 4
            if kind == 0:
                body = b" ".join(words[int(j)] for j in rng.integers(0, 40, m // 4))
            elif kind == 1:
                body = rng.integers(1, 5, m, dtype=np.uint8).tobytes()
            elif kind == 2:
                body = rng.integers(1, 256, int(rng.integers(3, 90)), dtype=np.uint8).tobytes() * (m // 3)
            else:
                body = bytes(rng.integers(1, 256, m // 9 + 1, dtype=np.uint8).repeat(9))
            datas.append((bytes(12) + body)[:m])
        else:
            kind = i % 3
            if kind == 0:
                datas.append((bytes(150) + rng.integers(1, 256, m, dtype=np.uint8).tobytes())[:m])
            elif kind == 1:
                datas.append((bytes(40) + rng.integers(1, 256, m, dtype=np.uint8).tobytes())[:m])
            else:
                datas.append((bytes(70) + b" ".join(words[int(j)] for j in rng.integers(0, 40, m // 4)))[:m])
    aligns = [i % 4 for i in range(n)]
    t0 = time.time()
    payloads, ntok, crc = deflate_on_device(ctx, datas, aligns, canary=False)
    print(f"launch: {n} blocks on {n_cu} CUs ({cap} in flight), {time.time() - t0:.1f} s with the copies", flush=True)
    t0 = time.time()
    matches = 0
    for i in range(n):
        toks, *_ = hold_block(f"block {i}", datas[i], payloads[i], ntok[i], crc[i])
        matches += sum(1 for t in toks if not isinstance(t, int))
    print(f"{n} blocks read token by token in {time.time() - t0:.1f} s, {matches} matches", flush=True)
    assert matches > n


def test_framed_entry_point_agrees_with_the_device_half(ctx, device_corpus):
    """sk_bgzf_deflate over every corpus block: a member is stored exactly when the raw payload is >= len + 5 bytes, otherwise its
    payload is the device half's, byte for byte; no member is longer than len + 31"""
    cases, datas, which, payloads, _, crc = device_corpus
    raw = {}
    for i, (j, a) in enumerate(which):
        raw.setdefault(j, (payloads[i], crc[i]))
    src = bytearray()
    blocks = np.zeros(len(cases), dtype=ctx.DEFLATE_BLOCK_DTYPE)
    for j, c in enumerate(cases):
        blocks[j] = (len(src), len(c.data), 0)
        src += c.data
    n_in = len(src)
    arr = np.frombuffer(bytes(src) + bytes(8), dtype=np.uint8)
    out = np.empty(len(cases) * 65536 + 64, dtype=np.uint8)
    off = np.zeros(len(cases) + 1, dtype=np.uint64)
    ctx._check(ctx._lib.sk_bgzf_deflate(ctx._h, arr.ctypes.data, n_in, blocks.ctypes.data, len(cases), out.ctypes.data, out.nbytes, off.ctypes.data), "sk_bgzf_deflate")
    stored = 0
    for j, c in enumerate(cases):
        member = out[int(off[j]):int(off[j + 1])].tobytes()
        ((payload, mcrc, isize),) = list(bgzf_members(member))
        dev_payload, dev_crc = raw[j]
        assert isize == len(c.data) and mcrc == dev_crc == (zlib.crc32(c.data) & 0xFFFFFFFF), c.name
        assert len(member) <= len(c.data) + 31, c.name
        if len(dev_payload) >= len(c.data) + 5:
            stored += 1
            n = len(c.data)
            assert payload == bytes([1, n & 0xff, n >> 8, ~n & 0xff, (~n >> 8) & 0xff]) + c.data, c.name
        else:
            assert payload == dev_payload, c.name
    print(f"{len(cases)} members, {stored} of them stored", flush=True)
    assert 0 < stored < len(cases)
