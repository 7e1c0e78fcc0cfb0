"""The `_dev` entry points on buffers the caller owns (include/seqkit_hip.h, "Conventions" and each call's comment).

The host entry points stage rows into the ctx's workspace, which is 256-byte aligned and rounded up: a store behind the last row
lands in slack that belongs to the library, and no comparison of values sees it.  Here every buffer of a call is a device
allocation of its own (tests/dev_guard.py): exactly the size the header states, at the smallest alignment the entry point accepts,
between guard bytes.  After sk_sync the outputs equal the oracle where the header specifies them, every guard byte is what it was,
and every input is unchanged.  The shapes are the smallest at which each kernel's tail path is taken."""
import numpy as np
import pytest

from seqkit_amd import capi, synth
from seqkit_amd.capi import SeqkitHipError
from tests.dev_guard import Guarded, default_trail

pytestmark = pytest.mark.gpu

A16 = dict(align=16, skew=16)            # 16-byte aligned and no better: the byte matrices, bc, assign, the blocked buffers, BAM columns
A8 = dict(align=8, skew=8)               # first_idx / last_idx, u64 vectors
A4 = dict(align=4, skew=4)               # lowest_diff, the sequence() matrices
A2 = dict(align=2, skew=2)               # u16 columns: len, lowest_k, flag
A1 = dict(align=1, skew=1)


def rows(n, stride, seed):
    """Bases with some N; qualities read-like in one half of the rows and arbitrary bytes in the other (both sides of 20 and of 223)."""
    rng = np.random.default_rng(seed)
    seq = synth.BASES[rng.integers(0, 4, size=(n, stride), dtype=np.uint8)]
    seq[rng.random((n, stride)) < 0.01] = ord("N")
    qual = rng.integers(33, 75, size=(n, stride), dtype=np.uint8)
    wild = rng.random(n) < 0.5
    qual[wild] = rng.integers(0, 256, size=(int(wild.sum()), stride), dtype=np.uint8)
    return np.ascontiguousarray(seq), np.ascontiguousarray(qual)


def ragged(n, stride, seed):
    """len[n] in 0 .. stride with `stride`, 0 and 1 forced in as far as n allows."""
    ln = np.random.default_rng(seed).integers(0, stride + 1, size=n).astype(np.uint16)
    ln[0] = stride
    if n > 1:
        ln[n - 1] = 0
    if n > 2:
        ln[1] = 1
    return ln


def valid_mask(n, stride, ln):
    return np.ones((n, stride), dtype=bool) if ln is None else (np.arange(stride)[None, :] < ln[:, None].astype(np.int64))


def sheet_of(shape):
    """"16 x 8" / "96 x 8+8" -> (table, halves)"""
    S = int(shape.split(" x ")[0])
    dual = "+" in shape
    L = int(shape.split(" x ")[1].split("+")[0])
    return synth.make_sheet(S, L, dual=dual, seed=S + 2), (2 if dual else 1)


def observe(table, halves, n, seed):
    return np.ascontiguousarray(synth.observe_barcodes(table, max(n, 4), seed=seed, halves=halves)[0][:n])


def preset_counts(S):
    return np.arange(7, 7 + S + 3, dtype=np.uint64) * 1_000_003


def demux_outputs(g, n, detail, counts=None):
    """assign (+ the three detail columns) (+ a caller's counters), each of exactly its size at its smallest alignment"""
    kw = dict(assign=g.put(4 * n, **A16))
    if detail:
        kw.update(lowest_diff=g.put(n, **A4), first_idx=g.put(2 * n, **A8), last_idx=g.put(2 * n, **A8))
    if counts is not None:
        kw["counts"] = g.put(counts, **A8)
    return kw


def check_demux_outputs(g, kw, e, n, matched=False, counts=None):
    assign = g.payload(kw["assign"], np.int32)
    assert np.array_equal(assign, e[0])
    if "lowest_diff" in kw:
        m = (e[0] != -1) if matched else np.ones(n, dtype=bool)       # SK_DETAIL_MATCHED: the detail of unmatched rows is unspecified
        assert np.array_equal(g.payload(kw["lowest_diff"], np.uint8)[m], e[1][m])
        assert np.array_equal(g.payload(kw["first_idx"], np.int16)[m], e[2][m])
        assert np.array_equal(g.payload(kw["last_idx"], np.int16)[m], e[3][m])
    if counts is not None:
        assert np.array_equal(g.payload(kw["counts"], np.uint64), counts + e[4].astype(np.uint64))


# ---- sk_mask_by_quality_dev: always mask_flat_kernel — whole 16 KiB spans, whole 16-byte chunks, a byte tail ----------------------------
@pytest.mark.parametrize("n,stride", [(1, 1), (15, 1), (16, 1), (17, 1), (4095, 1), (16383, 1), (16384, 1), (16385, 1), (16399, 1), (16400, 1),
                                      (32768 + 5, 1), (3, 17), (65, 151), (63, 150)])
def test_mask_by_quality_dev(ctx, oracle, n, stride):
    seq, qual = rows(n, stride, seed=n + stride)
    for m in (20, 223):                                               # two packed-compare modes
        exp = oracle.mask_batch(seq, qual, None, m)
        for in_place in (False, True):                                # out_seq == seq is allowed (include/seqkit_hip.h, M1)
            with Guarded(ctx) as g:
                d_seq, d_qual = g.put(seq, **A16), g.put(qual, **A16)
                d_out = d_seq if in_place else g.put(n * stride, trail=default_trail(stride), **A16)
                ctx.mask_by_quality_dev(d_seq, d_qual, stride, n, m, d_out)
                ctx.sync()
                assert np.array_equal(g.payload(d_out).reshape(n, stride), exp), (m, in_place)
                g.assert_all(outputs=[d_out], inputs=[d_qual] if in_place else [d_qual, d_seq])


# ---- sk_trim_by_quality_dev: the trim-only tile pass; above kMaxTileStride = 960 trim_rows_global_kernel ----------------------------------
@pytest.mark.parametrize("stride", [1, 3, 150, 151, 960, 961, 2100])
def test_trim_by_quality_dev(ctx, oracle, stride):
    for n in {961: (70,), 2100: (65,)}.get(stride, (1, 63, 64, 65, 129, 257)):
        _, qual = rows(n, stride, seed=3 * n + stride)
        for ln in (None, ragged(n, stride, seed=n)):
            with Guarded(ctx) as g:
                d_qual = g.put(qual, **A16)
                d_len = 0 if ln is None else g.put(ln, **A2)
                d_k = g.put(2 * n, **A2)                              # lowest_k: exactly 2 n bytes
                ctx.trim_by_quality_dev(d_qual, d_len, stride, n, 20, d_k)
                ctx.sync()
                assert np.array_equal(g.payload(d_k, np.uint16), oracle.trim_batch(qual, ln, 20)), (n, ln is None)
                g.assert_all(outputs=[d_k], inputs=[d_qual] + ([d_len] if d_len else []))


# ---- sk_fused_pass_dev ---------------------------------------------------------------------------------------------------------------------
def fused_case(ctx, oracle, mates, m, do_mask=True, do_trim=True, in_place=False, table=None, bc=None, detail=False, matched=False, what=None):
    """One sk_fused_pass_dev call on guarded buffers: mates = [(seq, qual, len or None)]; with bc, a caller's preset counters too."""
    n, stride = mates[0][1].shape if mates else (bc.shape[0], 0)
    with Guarded(ctx) as g:
        ins, outs, dm = [], [], []
        for seq, qual, ln in mates:
            d = {"qual": g.put(qual, **A16)}
            ins.append(d["qual"])
            if ln is not None:
                d["len"] = g.put(ln, **A2)
                ins.append(d["len"])
            if do_mask:
                d["seq"] = g.put(seq, **A16)
                if in_place:
                    d["out_seq"] = d["seq"]
                else:
                    ins.append(d["seq"])
                    d["out_seq"] = g.put(n * stride, trail=default_trail(stride), **A16)
                outs.append(d["out_seq"])
            if do_trim:
                d["lowest_k"] = g.put(2 * n, **A2)
                outs.append(d["lowest_k"])
            dm.append(d)
        kw, counts = {}, None
        if bc is not None:
            counts = preset_counts(table.shape[0])
            kw = demux_outputs(g, n, detail, counts)
            outs += list(kw.values())
            kw.update(bc=g.put(bc, **A16), bc_stride=bc.shape[1])
            ins.append(kw["bc"])
        ctx.fused_pass_dev(n, stride, m, dm, **kw)
        ctx.sync()
        for d, (seq, qual, ln) in zip(dm, mates):
            if do_trim:
                assert np.array_equal(g.payload(d["lowest_k"], np.uint16), oracle.trim_batch(qual, ln, m)), what
            if do_mask:
                v = valid_mask(n, stride, ln)                         # bytes past a row's length are unspecified on output
                assert np.array_equal(g.payload(d["out_seq"]).reshape(n, stride)[v], oracle.mask_batch(seq, qual, ln, m)[v]), what
        if bc is not None:
            check_demux_outputs(g, kw, oracle.demux_batch(table, bc, 1), n, matched, counts)
        g.assert_all(outputs=outs, inputs=ins)


FUSED_N = [1, 63, 64, 65, 257]
FUSED_STRIDE = [17, 150, 151, 250, 961]        # n * stride % 4 in {1, 2, 3}: mask_tail_kernel; 961: the kernels behind the tile pass


@pytest.mark.parametrize("stride", FUSED_STRIDE)
@pytest.mark.parametrize("n", FUSED_N)
def test_fused_pass_dev_mask_and_trim(ctx, oracle, n, stride):
    mates = [rows(n, stride, seed=n * 7 + stride + k) for k in range(2)]
    ln = ragged(n, stride, seed=n + stride)
    full = [(s, q, None) for s, q in mates]
    rag = [(s, q, ln) for s, q in mates]
    for what, ms, kw in (("single, mask + trim", full[:1], {}),
                         ("paired, mask + trim, ragged", rag, {}),
                         ("single, mask alone, in place", full[:1], dict(do_trim=False, in_place=True)),
                         ("paired, mask alone, ragged", rag, dict(do_trim=False)),
                         ("single, trim alone, ragged", rag[:1], dict(do_mask=False)),
                         ("paired, trim alone", full, dict(do_mask=False)),
                         ("paired, mask in place + trim", full, dict(in_place=True))):
        fused_case(ctx, oracle, ms, 20, what=what, **kw)


@pytest.mark.parametrize("detail", [False, True])
@pytest.mark.parametrize("phase", ["96 x 8+8: the tile pass's matcher", "200 x 8+8: the generic matcher", "16 x 8: the table, SK_DETAIL_MATCHED"])
def test_fused_pass_dev_with_a_barcode_phase(ctx, oracle, phase, detail):
    """96 samples ride in the tile pass (bit-sliced matcher, bc_stride 17); 200 are a launch of their own beside it; the 16 x 8 sheet
    under SK_DETAIL_MATCHED is looked up in the table wherever the barcode phase is a launch of its own (stride 961)."""
    table, halves = sheet_of(phase.split(":")[0])
    matched = "MATCHED" in phase
    ctx.set_barcodes(table, 1)
    if matched:
        ctx.set_detail_mode(capi.SK_DETAIL_MATCHED)
    try:
        if matched:
            assert ctx.barcode_table_info()["kind"] != capi.SK_TABLE_NONE
        for n in FUSED_N:
            bc = observe(table, halves, n, seed=n)
            for stride in FUSED_STRIDE:
                mates = [rows(n, stride, seed=n + stride + k) + (None,) for k in range(1 + n % 2)]
                if stride == 151:
                    ln = ragged(n, stride, seed=n)
                    mates = [(s, q, ln) for s, q, _ in mates]
                fused_case(ctx, oracle, mates, 20, table=table, bc=bc, detail=detail, matched=matched, what=(n, stride))
    finally:
        ctx.set_detail_mode(capi.SK_DETAIL_FULL)


# ---- sk_demux_assign_dev by the S x L matchers (SK_DETAIL_FULL with the detail columns: no table) -----------------------------------------
@pytest.mark.parametrize("shape", ["16 x 8", "96 x 8+8", "200 x 8+8"])
def test_demux_assign_dev_by_the_matchers(ctx, oracle, shape):
    table, halves = sheet_of(shape)
    ctx.set_barcodes(table, 1)
    ctx.set_detail_mode(capi.SK_DETAIL_FULL)
    for n in (1, 63, 64, 65, 255, 256, 257, 1025):
        bc = observe(table, halves, n, seed=n + 1)
        for own_counts in (False, True):
            counts = preset_counts(table.shape[0]) if own_counts else None
            ctx.counts_reset()
            with Guarded(ctx) as g:
                kw = demux_outputs(g, n, True, counts)
                d_bc = g.put(bc, **A16)
                ctx.demux_assign_dev(d_bc, bc.shape[1], n, **kw)
                ctx.sync()
                e = oracle.demux_batch(table, bc, 1)
                check_demux_outputs(g, kw, e, n, False, counts)
                assert np.array_equal(ctx.counts(), np.zeros_like(e[4]) if own_counts else e[4])
                g.assert_all(outputs=kw.values(), inputs=[d_bc])


# ---- the many-batch forms: every output column of every batch from ONE allocation, 64 pattern bytes between neighbours ---------------------
MANY_SIZES = [1, 64, 257, 1000, 3]


@pytest.mark.parametrize("gather_form", [False, True])
@pytest.mark.parametrize("shape", ["16 x 8", "96 x 8+8", "384 x 8+8", "130 x 12"])
def test_demux_assign_many_dev(ctx, oracle, shape, gather_form, monkeypatch):
    """A batch that ran over into its neighbour's column would be overwritten again by that batch, or not: the gaps tell."""
    if gather_form:
        monkeypatch.setenv("SK_LUT_MANY_GATHER", "1")
    table, halves = sheet_of(shape)
    S = table.shape[0]
    bcs = [observe(table, halves, n, seed=100 + i) for i, n in enumerate(MANY_SIZES)]
    es = [oracle.demux_batch(table, bc, 1) for bc in bcs]
    ctx.set_barcodes(table, 1)
    try:
        for detail in (False, True):
            ctx.set_detail_mode(capi.SK_DETAIL_MATCHED if detail else capi.SK_DETAIL_FULL)
            ctx.counts_reset()
            with Guarded(ctx) as g:
                d_bcs = g.carve(bcs, **A16)
                widths = [(4, A16), (1, A4), (2, A8), (2, A8)] if detail else [(4, A16)]
                items = [(n * w, a) for n in MANY_SIZES for w, a in widths]
                cols = g.carve([nb for nb, _ in items], align=[a["align"] for _, a in items], skew=[a["skew"] for _, a in items])
                per = len(widths)
                batches = [(d_bcs[i], n, *cols[i * per:(i + 1) * per]) for i, n in enumerate(MANY_SIZES)]
                ctx.demux_assign_many_dev(batches, bcs[0].shape[1])
                ctx.sync()
                for i, (n, e) in enumerate(zip(MANY_SIZES, es)):
                    kw = dict(zip(("assign", "lowest_diff", "first_idx", "last_idx"), cols[i * per:(i + 1) * per]))
                    check_demux_outputs(g, kw, e, n, matched=True)
                assert np.array_equal(ctx.counts(), sum(e[4].astype(np.uint64) for e in es))
                g.assert_guards(cols[0], "the batches' output columns")
                g.assert_unchanged(d_bcs[0], "the batches' barcodes")
    finally:
        ctx.set_detail_mode(capi.SK_DETAIL_FULL)


@pytest.mark.parametrize("two_streams", ["1", "0"])
def test_trim_by_quality_many_dev(ctx, oracle, two_streams, monkeypatch):
    monkeypatch.setenv("SK_MANY_TWO_STREAMS", two_streams)
    for stride in (150, 151):
        quals = [rows(n, stride, seed=30 + i)[1] for i, n in enumerate(MANY_SIZES)]
        lens = [ragged(n, stride, seed=i) if i % 2 else None for i, n in enumerate(MANY_SIZES)]
        with Guarded(ctx) as g:
            d_q = g.carve(quals, **A16)
            d_l = dict(zip([i for i, ln in enumerate(lens) if ln is not None], g.carve([ln for ln in lens if ln is not None], **A2)))
            d_k = g.carve([2 * n for n in MANY_SIZES], **A2)
            ctx.trim_by_quality_many_dev([(d_q[i], d_l.get(i, 0), n, d_k[i]) for i, n in enumerate(MANY_SIZES)], stride, 20)
            ctx.sync()
            for i in range(len(MANY_SIZES)):
                assert np.array_equal(g.payload(d_k[i], np.uint16), oracle.trim_batch(quals[i], lens[i], 20)), i
            g.assert_guards(d_k[0], "the batches' lowest_k")
            g.assert_unchanged(d_q[0], "the batches' qualities")
            g.assert_unchanged(next(iter(d_l.values())), "the batches' lengths")


@pytest.mark.parametrize("two_streams", ["1", "0"])
@pytest.mark.parametrize("with_bc", [False, True])
def test_fused_pass_many_dev(ctx, oracle, with_bc, two_streams, monkeypatch):
    """mask + trim of one mate per batch (on the ctx's two streams in turn when no batch has a barcode phase), with and without the 96
    dual-index sheet's barcode phase and its detail columns; out_seq, lowest_k, assign and detail of all batches in one allocation."""
    monkeypatch.setenv("SK_MANY_TWO_STREAMS", two_streams)
    stride = 151
    table, halves = sheet_of("96 x 8+8")
    ctx.set_barcodes(table, 1)
    ctx.set_detail_mode(capi.SK_DETAIL_FULL)
    ctx.counts_reset()
    data = [rows(n, stride, seed=60 + i) for i, n in enumerate(MANY_SIZES)]
    lens = [ragged(n, stride, seed=i) if i % 2 else None for i, n in enumerate(MANY_SIZES)]
    bcs = [observe(table, halves, n, seed=70 + i) for i, n in enumerate(MANY_SIZES)]
    with Guarded(ctx) as g:
        d_seq, d_qual = g.carve([s for s, _ in data], **A16), g.carve([q for _, q in data], **A16)
        d_len = dict(zip([i for i, ln in enumerate(lens) if ln is not None], g.carve([ln for ln in lens if ln is not None], **A2)))
        d_bc = g.carve(bcs, **A16) if with_bc else None
        widths = [(stride, A16), (2, A2)] + ([(4, A16), (1, A4), (2, A8), (2, A8)] if with_bc else [])
        items = [(n * w, a) for n in MANY_SIZES for w, a in widths]
        cols = g.carve([nb for nb, _ in items], align=[a["align"] for _, a in items], skew=[a["skew"] for _, a in items],
                       trail=default_trail(stride))
        per = len(widths)
        batches = []
        for i, n in enumerate(MANY_SIZES):
            c = cols[i * per:(i + 1) * per]
            b = dict(n=n, stride=stride, min_baseq=20, mates=[dict(seq=d_seq[i], qual=d_qual[i], len=d_len.get(i, 0), out_seq=c[0], lowest_k=c[1])])
            if with_bc:
                b.update(bc=d_bc[i], bc_stride=bcs[i].shape[1], assign=c[2], lowest_diff=c[3], first_idx=c[4], last_idx=c[5])
            batches.append(b)
        ctx.fused_pass_many_dev(batches)
        ctx.sync()
        total = np.zeros(table.shape[0] + 3, dtype=np.uint64)
        for i, n in enumerate(MANY_SIZES):
            c = cols[i * per:(i + 1) * per]
            seq, qual = data[i]
            v = valid_mask(n, stride, lens[i])
            assert np.array_equal(g.payload(c[0]).reshape(n, stride)[v], oracle.mask_batch(seq, qual, lens[i], 20)[v]), i
            assert np.array_equal(g.payload(c[1], np.uint16), oracle.trim_batch(qual, lens[i], 20)), i
            if with_bc:
                e = oracle.demux_batch(table, bcs[i], 1)
                check_demux_outputs(g, dict(zip(("assign", "lowest_diff", "first_idx", "last_idx"), c[2:])), e, n)
                total += e[4].astype(np.uint64)
        assert np.array_equal(ctx.counts(), total)
        g.assert_guards(cols[0], "the batches' output columns")
        for p in [d_seq[0], d_qual[0], next(iter(d_len.values()))] + ([d_bc[0]] if with_bc else []):
            g.assert_unchanged(p)


# ---- sk_fused_pass_blocked_dev: out is exactly ((n + 63) / 64) * out_block bytes ------------------------------------------------------------
@pytest.mark.parametrize("layout", ["paired, mask + trim + barcodes + detail", "single, trim only", "paired, ragged, mask + trim + barcodes"])
@pytest.mark.parametrize("n", [1, 64, 65, 777])
def test_fused_pass_blocked_dev(ctx, oracle, n, layout):
    stride = 151 if "ragged" in layout else 150
    paired, with_bc, detail, do_mask = layout.startswith("paired"), "barcodes" in layout, "detail" in layout, "mask" in layout
    ln = ragged(n, stride, seed=n) if "ragged" in layout else None
    mates = [rows(n, stride, seed=n + k) + (ln,) for k in range(2 if paired else 1)]
    table, halves = sheet_of("96 x 8+8")
    bc = observe(table, halves, n, seed=n) if with_bc else None
    ctx.set_barcodes(table, 1)
    ctx.set_detail_mode(capi.SK_DETAIL_FULL)
    flags = (capi.SK_BLK_MASK if do_mask else 0) | capi.SK_BLK_TRIM | (capi.SK_BLK_LEN if ln is not None else 0) | (capi.SK_BLK_DETAIL if detail else 0)
    lay = capi.blocked_layout(len(mates), stride, bc.shape[1] if with_bc else 0, flags)
    hin = lay.pack(mates, bc)
    assert hin.nbytes == lay.in_bytes(n)
    counts = preset_counts(table.shape[0]) if with_bc else None
    with Guarded(ctx) as g:
        d_in = g.put(hin, trail=default_trail(stride), **A16)
        d_out = g.put(lay.out_bytes(n), trail=default_trail(stride), **A16)
        d_counts = g.put(counts, **A8) if with_bc else 0
        ctx.fused_pass_blocked_dev(lay, d_in, d_out, n, 20, d_counts)
        ctx.sync()
        r = lay.unpack(g.payload(d_out), n)                           # (the padding rows of the last tile are unspecified: not unpacked)
        for i, (seq, qual, _) in enumerate(mates):
            assert np.array_equal(r["lowest_k"][i], oracle.trim_batch(qual, ln, 20)), i
            if do_mask:
                v = valid_mask(n, stride, ln)
                assert np.array_equal(r["out_seq"][i][v], oracle.mask_batch(seq, qual, ln, 20)[v]), i
        if with_bc:
            e = oracle.demux_batch(table, bc, 1)
            assert np.array_equal(r["assign"], e[0])
            if detail:
                assert np.array_equal(r["lowest_diff"], e[1]) and np.array_equal(r["first_idx"], e[2]) and np.array_equal(r["last_idx"], e[3])
            assert np.array_equal(g.payload(d_counts, np.uint64), counts + e[4].astype(np.uint64))
        g.assert_all(outputs=[d_out] + ([d_counts] if with_bc else []), inputs=[d_in])


# ---- sk_bam_sequence_dev ---------------------------------------------------------------------------------------------------------------------
def bam_rows(n, stride, seq4_stride, seed):
    """Packed 4-bit codes (some ambiguity codes), raw phred bytes, flags of both strands."""
    rng = np.random.default_rng(seed)
    codes = np.array([1, 2, 4, 8], dtype=np.uint8)[rng.integers(0, 4, size=(n, seq4_stride * 2))]
    amb = rng.random((n, seq4_stride * 2)) < 0.1
    codes[amb] = rng.integers(0, 16, size=int(amb.sum()), dtype=np.uint8)
    seq4 = np.ascontiguousarray(((codes[:, 0::2] << 4) | codes[:, 1::2]).astype(np.uint8))
    qual = rng.integers(0, 61, size=(n, stride), dtype=np.uint8)
    flag = np.tile(np.array([0, 16, 83, 99, 147, 163, 4, 1040], dtype=np.uint16), n // 8 + 1)[:n].copy()
    return seq4, qual, flag


@pytest.mark.parametrize("way", ["16-byte aligned matrices", "out at 4 bytes", "SK_SEQ_TILE=0, all three at 4 bytes"])
@pytest.mark.parametrize("stride", [4, 8, 12, 100, 148, 152, 160, 164])     # 12, 148: a last unit of four bytes; 164: beyond the LDS-tile kernel
def test_bam_sequence_dev(ctx, oracle, stride, way, monkeypatch):
    """bam_sequence_tile_kernel where it applies, bam_sequence8_kernel by the pointers' alignment and by SK_SEQ_TILE=0; on a pitch that
    is an odd multiple of 4 the 8-byte kernel's last unit of a row must store its first dword only."""
    if way.startswith("SK_SEQ_TILE"):
        monkeypatch.setenv("SK_SEQ_TILE", "0")
    a_in = A4 if way.startswith("SK_SEQ_TILE") else A16
    a_out = A16 if way.startswith("16") else A4
    for seq4_stride in ((stride // 2 + 3) // 4 * 4, (stride // 2 + 3) // 4 * 4 + 8):
        for n in (1, 63, 64, 65, 130):
            seq4, qual, flag = bam_rows(n, stride, seq4_stride, seed=n + stride)
            for ln in (None, ragged(n, stride, seed=n + 1)):
                with Guarded(ctx) as g:
                    d_seq4, d_qual = g.put(seq4, **a_in), g.put(qual, **a_in)
                    d_flag = g.put(flag, **A2)
                    d_len = 0 if ln is None else g.put(ln, **A2)
                    d_out = g.put(n * stride, trail=default_trail(stride), **a_out)
                    ctx.bam_sequence_dev(d_seq4, seq4_stride, d_qual, stride, d_len, d_flag, n, 10, d_out)
                    ctx.sync()
                    v = valid_mask(n, stride, ln)                     # bytes of out past a row's length are unspecified
                    got = g.payload(d_out).reshape(n, stride)
                    assert np.array_equal(got[v], oracle.bam_sequence_batch(seq4, qual, ln, flag, 10)[v]), (seq4_stride, n, ln is None)
                    g.assert_all(outputs=[d_out], inputs=[d_seq4, d_qual, d_flag] + ([d_len] if d_len else []))


# ---- the BAM column calls ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 7, 8, 9, 63, 64, 65, 255, 257, 100003])
def test_bam_fragments_dev(ctx, oracle, n):
    flag, tid, mtid, tlen = synth.make_bam_cores(n, seed=n)
    with Guarded(ctx) as g:
        cols = [g.put(c, **A16) for c in (flag, tid, mtid, tlen)]
        d_bits = g.put((n + 7) // 8, **A1)                            # keep_bits: exactly (n + 7) / 8 bytes
        d_kept = g.put(np.array([5], dtype=np.uint64), **A8)          # *kept is ADDED to
        ctx.bam_fragments_dev(*cols, n, 0, 5000, d_bits, d_kept)
        ctx.sync()
        exp = oracle.fragments_keep(flag, tid, mtid, tlen, 0, 5000)
        assert np.array_equal(np.unpackbits(g.payload(d_bits), bitorder="little")[:n], exp)
        assert int(g.payload(d_kept, np.uint64)[0]) == 5 + int(exp.sum())
        g.assert_all(outputs=[d_bits, d_kept], inputs=cols)


@pytest.mark.parametrize("skew", [16, 4])                             # 16-byte aligned columns: the vectorised kernel; at 4: the scalar one
@pytest.mark.parametrize("n", [1, 1000, 300001])
def test_bam_flag_tlen_dev(ctx, oracle, n, skew):
    flag, tid, mtid, tlen = synth.make_bam_cores(n, seed=5)
    for max_frag in (0, 100, 5000):
        preset = np.arange(3, 3 + 3 + 1 + max_frag + 1, dtype=np.uint64)
        with Guarded(ctx) as g:
            cols = [g.put(c, align=c.itemsize, skew=skew) for c in (flag, tid, mtid, tlen)]
            d_out = g.put(preset, **A8)                               # exactly 8 * (3 + 1 + max_frag + 1) bytes, ADDED to
            ctx.bam_flag_tlen_dev(*cols, n, max_frag, d_out)
            ctx.sync()
            ec, eh, et = oracle.bam_flag_tlen(flag, tid, mtid, tlen, max_frag)
            got = g.payload(d_out, np.uint64) - preset
            assert np.array_equal(got[:3], ec) and int(got[3]) == et and np.array_equal(got[4:], eh), max_frag
            g.assert_all(outputs=[d_out], inputs=cols)


def test_bam_walk_dev(ctx):
    """entry and exit_scratch of exactly 8 n bytes, nrec_scratch of exactly 4 (n + 1); the stream readable 8 bytes beyond its end."""
    import struct

    from tests.test_gpu_inflate import bam_stream, cut_blocks
    rng = np.random.default_rng(4)
    raw, first, recs = bam_stream(rng, 1800)
    ends = cut_blocks(raw, first, rng, "anywhere")
    n = len(ends)
    assert 25 <= n <= 80, n
    starts, o = [], first
    while o < len(raw):
        starts.append(o)
        o += 4 + struct.unpack_from("<I", raw, o)[0]
    starts = np.array(starts + [len(raw)], dtype=np.uint64)
    begins = np.concatenate([[0], ends[:-1]]).astype(np.uint64)
    want_entry = starts[np.searchsorted(starts, np.maximum(begins, first))]
    with Guarded(ctx) as g:
        d_stream = g.put(np.frombuffer(raw, dtype=np.uint8), **A16)
        d_ends = g.put(ends, **A8)
        d_entry, d_exit, d_nrec = g.put(8 * n, **A8), g.put(8 * n, **A8), g.put(4 * (n + 1), **A4)
        verified, n_records, _ = ctx.bam_walk_dev(d_stream, len(raw), d_ends, n, first, d_entry, d_exit, d_nrec, max_rounds=1000, n_ref=3)
        ctx.sync()
        assert verified and n_records == len(recs)
        assert np.array_equal(g.payload(d_entry, np.uint64), want_entry)
        g.assert_all(outputs=[d_entry, d_exit, d_nrec], inputs=[d_stream, d_ends])


@pytest.mark.parametrize("n,L,stride", [(1, 8, 8), (255, 17, 17), (70000, 17, 24)])
def test_census_add_dev(ctx, oracle, n, L, stride):
    """The call writes ctx memory only: the caller's bc and assign columns must come back as they went in."""
    rng = np.random.default_rng(n + L)
    alpha = np.frombuffer(b"ACGTNacgtn+", dtype=np.uint8)
    bc = np.zeros((n, stride), dtype=np.uint8)
    bc[:, :L] = alpha[rng.integers(0, 4, size=(n, L))]
    hot = rng.random(n) < 0.6
    bc[hot, :L] = alpha[rng.integers(0, len(alpha), size=(7, L))][rng.integers(0, 7, size=int(hot.sum()))]
    assign = rng.choice(np.array([-1, -1, -2, 0, 5], dtype=np.int32), size=n)
    for use_assign in (False, True):
        ctx.census_reset()
        with Guarded(ctx) as g:
            d_bc = g.put(bc, **A16)
            d_assign = g.put(assign, **A4) if use_assign else 0
            ctx.census_add_dev(d_bc, stride, L, n, d_assign, row_base=11)
            ctx.sync()
            got, total = ctx.census_entries()
            want = oracle.census(bc, L=L, assign=assign if use_assign else None, row_base=11)
            assert total == len(want) and got == want
            g.assert_all(inputs=[d_bc] + ([d_assign] if use_assign else []))


def test_on_target_add_dev_leaves_its_columns_alone(ctx):
    from tests import bam_on_target_model as om
    from tests.test_gpu_on_target import DTYPES, columns, set_regions
    recs = om.crafted_records()
    recs += om.drawn_records(max(0, 1025 - len(recs)), seed=7)
    cols = columns(recs)
    for skew in (16, 4):                                              # the wide loads and the narrow ones
        set_regions(ctx, om.CRAFTED_BED)
        with Guarded(ctx) as g:
            ptrs = [g.put(cols[name], align=cols[name].itemsize, skew=skew) for name in DTYPES]
            ctx.on_target_add_dev(*ptrs, len(recs))
            ctx.sync()
            assert [int(x) for x in ctx.on_target_get()] == om.sweep(recs, om.CRAFTED_BED) + [0]
            g.assert_all(inputs=ptrs)


def test_count_add_dev_leaves_its_columns_alone(ctx, oracle):
    from tests.test_gpu_parity import count_inputs, grouped_regions
    n, n_chr = 20_001, 5
    cols, rchr, rstart, rend = count_inputs(n, n_chr, 300, seed=9)
    want, code, _ = oracle.count_batch(**cols, n_chr=n_chr, rchr=rchr, rstart=rstart, rend=rend, single_end=True)
    assert code == 0
    chr_off, gs, ge, gi = grouped_regions(rchr, rstart, rend, n_chr)
    ctx.count_set_regions(chr_off, gs, ge, gi, n_regions=300)
    with Guarded(ctx) as g:
        ptrs = [g.put(cols[k], **A16) for k in ("flag", "mapq", "tid", "mtid", "pos", "mpos", "tlen", "end_pos")]
        ctx.count_add_dev(*ptrs, n, single_end=True)
        ctx.sync()
        assert np.array_equal(ctx.count_get()[gi], want[gi])
        g.assert_all(inputs=ptrs)


# ---- rejections: a pointer short of an alignment rule by the smallest step ------------------------------------------------------------------
def test_misaligned_device_pointers_are_refused_before_any_launch(ctx, oracle):
    """Every alignment rule the entry points enforce (include/seqkit_hip.h: 16 bytes for the byte matrices, bc, assign, the blocked
    buffers and the fragment columns; 4 for lowest_diff; 8 for first_idx / last_idx; 4 for the sequence() matrices): SK_ERR_INVALID,
    every buffer of the call as it was — payload and guards — and the ctx serves the next valid call."""
    n, stride = 65, 152
    seq, qual = rows(n, stride, seed=1)
    table, halves = sheet_of("96 x 8+8")
    bc = observe(table, halves, n, seed=2)
    ctx.set_barcodes(table, 1)
    ctx.set_detail_mode(capi.SK_DETAIL_FULL)
    ctx.counts_reset()
    flag, tid, mtid, tlen = synth.make_bam_cores(n, seed=3)
    seq4, bq, bflag = bam_rows(n, stride, 76, seed=4)
    lay = capi.blocked_layout(1, stride, 0, capi.SK_BLK_MASK | capi.SK_BLK_TRIM)
    hin = lay.pack([(seq, qual, None)])
    short = {16: dict(align=8, skew=8), 8: dict(align=4, skew=4), 4: dict(align=2, skew=2)}      # the rule -> the pointer just short of it
    with Guarded(ctx) as g:
        everything = []

        def buf(x, rule=None, good=A16):
            p = g.put(x, **(short[rule] if rule else good))
            assert rule is None or (p % rule != 0 and p % (rule // 2) == 0)
            everything.append(p)
            return p

        def refused(fn, *a, **kw):
            with pytest.raises(SeqkitHipError, match=r"failed \(-1\)"):
                fn(*a, **kw)

        ok = dict(seq=buf(seq), qual=buf(qual), out=buf(n * stride), k=buf(2 * n, good=A2), bc=buf(bc), assign=buf(4 * n), low=buf(n, good=A4),
                  first=buf(2 * n, good=A8), last=buf(2 * n, good=A8))
        bad = dict(seq=buf(seq, 16), qual=buf(qual, 16), out=buf(n * stride, 16), bc=buf(bc, 16), assign=buf(4 * n, 16), low=buf(n, 4),
                   first=buf(2 * n, 8), last=buf(2 * n, 8))

        def pick(which):
            return {k: (bad[k] if k == which else ok[k]) for k in ok}

        for which in ("seq", "qual", "out"):
            p = pick(which)
            refused(ctx.mask_by_quality_dev, p["seq"], p["qual"], stride, n, 20, p["out"])
        refused(ctx.trim_by_quality_dev, bad["qual"], 0, stride, n, 20, ok["k"])
        refused(ctx.trim_by_quality_many_dev, [(ok["qual"], 0, n, ok["k"]), (bad["qual"], 0, n, ok["k"])], stride, 20)
        for which in ("seq", "qual", "out", "bc", "assign", "low", "first", "last"):
            p = pick(which)
            args = dict(n=n, stride=stride, min_baseq=20, mates=[dict(seq=p["seq"], qual=p["qual"], out_seq=p["out"], lowest_k=p["k"])],
                        bc=p["bc"], bc_stride=bc.shape[1], assign=p["assign"], lowest_diff=p["low"], first_idx=p["first"], last_idx=p["last"])
            refused(ctx.fused_pass_dev, **args)
            good_args = dict(args, mates=[dict(seq=ok["seq"], qual=ok["qual"], out_seq=ok["out"], lowest_k=ok["k"])], bc=ok["bc"], assign=ok["assign"],
                             lowest_diff=ok["low"], first_idx=ok["first"], last_idx=ok["last"])
            refused(ctx.fused_pass_many_dev, [good_args, args])          # every batch is checked before the first is launched
            if which in ("bc", "assign", "low", "first", "last"):
                refused(ctx.demux_assign_dev, p["bc"], bc.shape[1], n, p["assign"], p["low"], p["first"], p["last"])
                refused(ctx.demux_assign_many_dev, [(ok["bc"], n, ok["assign"], ok["low"], ok["first"], ok["last"]),
                                                    (p["bc"], n, p["assign"], p["low"], p["first"], p["last"])], bc.shape[1])
        d_in, d_out = buf(hin), buf(lay.out_bytes(n))
        refused(ctx.fused_pass_blocked_dev, lay, buf(hin, 16), d_out, n, 20)
        refused(ctx.fused_pass_blocked_dev, lay, d_in, buf(lay.out_bytes(n), 16), n, 20)
        cols = [buf(c) for c in (flag, tid, mtid, tlen)]
        d_bits, d_kept = buf((n + 7) // 8, good=A1), buf(np.array([5], dtype=np.uint64), good=A8)
        for k, c in enumerate((flag, tid, mtid, tlen)):
            refused(ctx.bam_fragments_dev, *[buf(c, 16) if j == k else q for j, q in enumerate(cols)], n, 0, 5000, d_bits, d_kept)
        s_ok = dict(seq4=buf(seq4, good=A4), qual=buf(bq, good=A4), out=buf(n * stride, good=A4))
        d_bflag = buf(bflag, good=A2)
        for which, x in (("seq4", seq4), ("qual", bq), ("out", n * stride)):
            p = dict(s_ok, **{which: buf(x, 4)})
            refused(ctx.bam_sequence_dev, p["seq4"], 76, p["qual"], stride, 0, d_bflag, n, 10, p["out"])
        ctx.census_reset()
        refused(ctx.census_add_dev, bad["bc"], bc.shape[1], bc.shape[1], n)
        ctx.sync()
        for p in everything:
            g.assert_unchanged(p, "a buffer of a refused call")
        assert ctx.counts().sum() == 0 and ctx.census_stats()["counted"] == 0
        # the ctx serves the next valid call
        ctx.fused_pass_dev(n, stride, 20, [dict(seq=ok["seq"], qual=ok["qual"], out_seq=ok["out"], lowest_k=ok["k"])], bc=ok["bc"], bc_stride=bc.shape[1],
                           assign=ok["assign"], lowest_diff=ok["low"], first_idx=ok["first"], last_idx=ok["last"])
        ctx.sync()
        assert np.array_equal(g.payload(ok["out"]).reshape(n, stride), oracle.mask_batch(seq, qual, None, 20))
        assert np.array_equal(g.payload(ok["k"], np.uint16), oracle.trim_batch(qual, None, 20))
        e = oracle.demux_batch(table, bc, 1)
        check_demux_outputs(g, dict(assign=ok["assign"], lowest_diff=ok["low"], first_idx=ok["first"], last_idx=ok["last"]), e, n)
        assert np.array_equal(ctx.counts(), e[4])
        for p in (ok["out"], ok["k"], ok["assign"], ok["low"], ok["first"], ok["last"]):
            g.assert_guards(p)
