"""GPU: sk_bam_file_rewrite / sk_bam_file_rewrite_next — `sam trim qnames`, `sam tags from qname` and `sam qname from tags` rewritten and
BGZF-compressed on the device from the inflated BAM file — against the plain-Python model of tests/bam_rewrite_model.py."""
import pytest

from tests import bam_rewrite_model as m
from tests.bam_out_util import checked_windows

pytestmark = pytest.mark.gpu


def collect(ctx, path, op, level, window_bytes):
    return checked_windows(ctx, ctx.bam_file_rewrite(str(path), op, level, window_bytes), m)[:3]


def ctx_windows(ctx, path, op, level, window_bytes):
    assert ctx.bam_file_rewrite(str(path), op, level, window_bytes)[0]
    return list(ctx.bam_file_rewrite_windows())


@pytest.mark.parametrize("op", list(m.OPS))
@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("window", [0, 64 << 10])
def test_rewrite_matches_model(ctx, tmp_path, op, level, window):
    path = tmp_path / "in.bam"
    raw = m.write(path, m.served_records(op))
    exp, code = m.model(raw, op)
    assert code is None
    handled, out, mem = collect(ctx, path, op, level, window)
    assert handled
    assert out == exp
    if level == 0:
        assert all(stored for _, stored in mem[:-1])
    else:
        assert not all(stored for _, stored in mem[:-1])                               # (the device deflated what shrinks)
    if window:                                                                        # (many windows: records change length across their edges)
        assert len(ctx_windows(ctx, path, op, level, window)) > 10


def test_rewrite_no_records_and_empty_text(ctx, tmp_path):
    path = tmp_path / "empty.bam"
    raw = m.write(path, [], text=b"\n\n\0\0")
    for op in m.OPS:
        handled, out, _ = collect(ctx, path, op, 1, 0)
        assert handled and out == m.model(raw, op)[0]
        assert out[4:8] == b"\0\0\0\0"


def test_rewrite_small_input_blocks(ctx, tmp_path):
    """records that straddle several input blocks of 12 KiB, and a window of 256 bytes (one or two records each)"""
    path = tmp_path / "small.bam"
    raw = m.write(path, m.served_records("tags from qname", 300, seed=7), piece=0x3000)
    assert ctx.bam_file_rewrite(str(path), "tags from qname", 1, 256)[0], ctx.bam_file_rewrite(str(path), "tags from qname", 1, 256)[3]
    handled, out, _ = collect(ctx, path, "tags from qname", 1, 256)
    assert handled and out == m.model(raw, "tags from qname")[0]


@pytest.mark.parametrize("case", range(len(m.STOPS)))
def test_rewrite_declines_where_the_reference_stops(ctx, tmp_path, case):
    op, name, aux = m.STOPS[case]
    path = tmp_path / "stop.bam"
    raw = m.write(path, [m.record(b"ok1", 20), m.record(name, 20, aux=aux), m.record(b"ok2", 20)])
    assert m.model(raw, op)[1] is not None
    handled, _, _, info = ctx.bam_file_rewrite(str(path), op, 1, 0)
    assert not handled and info[5] <= -30


def test_rewrite_declines_unparsed_aux(ctx, tmp_path):
    path = tmp_path / "aux.bam"
    m.write(path, [m.record(b"r1", 20, aux=m.aux_z(b"RX", b"AC") + b"XXQ\1")])
    handled, _, _, _ = ctx.bam_file_rewrite(str(path), "qname from tags", 1, 0)
    assert not handled
    handled, _, _, _ = ctx.bam_file_rewrite(str(path), "trim qnames", 1, 0)         # (only qname from tags reads the aux data)
    assert handled
    assert len(list(ctx.bam_file_rewrite_windows())) == 2


def test_rewrite_next_after_another_file_call_is_invalid(ctx, tmp_path):
    from seqkit_amd.capi import SeqkitHipError
    path = tmp_path / "in.bam"
    m.write(path, m.served_records("trim qnames", 50))
    assert ctx.bam_file_rewrite(str(path), "trim qnames", 1, 0)[0]
    assert ctx.bam_file_reads(str(path), "fastq")[0]
    with pytest.raises(SeqkitHipError):
        next(ctx.bam_file_rewrite_windows())
