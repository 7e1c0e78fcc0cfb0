"""GPU: `sam recalculate tlen` on the device path (sk_bam_file_recalc_tlen), the host reader (SEQKIT_HOST_INFLATE=1) and stdin: the same
inflated stdout and the same stderr, equal to tests/bam_recalc_tlen_model.py, and the reference's statuses."""
import re

import pytest

from tests import bam_out_util as bu
from tests import bam_recalc_tlen_model as m
from tests.bam_out_util import sam  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

WORDS = ("recalculate", "tlen")


@pytest.fixture(scope="module")
def bam(tmp_path_factory):
    path = tmp_path_factory.mktemp("recalc_tlen") / "in.bam"
    return path, m.write(path, m.served_records(3000, seed=1))


def three(sam, path, extra=(), **kw):
    """bam_out_util.three (device path, host reader, stdin: status, inflated stdout and stderr checked equal; the trace names the path) with
    stderr kept byte for byte: (status, inflated stdout, stderr without the trace's lines, runs)"""
    code, out, _, runs = bu.three(sam, m, WORDS, path, extra=extra, **kw)
    who = b"sam recalculate tlen: "
    err = b"".join(ln + b"\n" for ln in runs[0][2].split(b"\n")[:-1] if not ln.startswith(who) and not ln.startswith(b"sk_bam"))
    return code, out, err, runs


@pytest.mark.parametrize("extra,max_len", [((), 5000), (("--max-len=1",), 1), (("--max-len", "1"), 1), (("--max-len=1099511627776",), 1 << 40),
                                           (("--uncompressed", "--max-len", "5000"), 5000)])
def test_three_paths_match_model(sam, bam, extra, max_len):
    path, raw = bam
    code, out, err, runs = three(sam, path, extra)
    assert (out, err, code) == m.literal(raw, max_len) and code == 0
    written = len(m.grouped_parts(raw, max_len)[1])
    assert b"sam recalculate tlen: device path, %d records" % written in runs[0][2]      # the device served the file
    if "--uncompressed" in extra:
        assert all(stored for _, stored in m.members(runs[0][1])[:-1])


def test_small_windows_on_the_device_path(sam, bam):
    path, raw = bam
    code, out, err, runs = three(sam, path, env={"SK_BAMFILE_WINDOW": "4096"})
    assert (out, err, code) == m.literal(raw, 5000)


def test_more_discarded_records_than_one_chunk_of_names(sam, tmp_path):
    """5 000 lone candidates: the discard lines come in file order from two chunks, and nothing but the header is written"""
    path = tmp_path / "lone.bam"
    raw = m.write(path, [m.cand(b"l%d" % i, 0, 100 + i, 150 + i, i & 1, i & 2) for i in range(5000)])
    code, out, err, runs = three(sam, path)
    assert (out, err, code) == m.literal(raw, 5000) and out == m.out_header(raw) and err.count(b"\n") == 5000
    assert b"sam recalculate tlen: device path, 0 records" in runs[0][2]


def test_hash_collision_falls_back_to_the_host_reader(sam, bam):
    """SK_TLEN_KEY_BITS=4 makes the names' hashes collide: the device declines and the host reader serves the file"""
    path, raw = bam
    code, out, err, runs = three(sam, path, expect_path="host reader", env={"SK_TLEN_KEY_BITS": "4"})
    assert (out, err, code) == m.literal(raw, 5000)
    # (the bits are ORed: records of different names linked under the collision may add 2 or 32 to the 64)
    found = re.search(rb"sk_bam_file_recalc_tlen: declined \(bits 0x([0-9a-f]+)\)", runs[0][2])
    assert found and int(found.group(1), 16) & 0x40


@pytest.mark.parametrize("what,bits", [("secondary", 0x1), ("assert", 0x2), ("utf8", 0x10), ("cigar", 0x20)])
def test_a_stopping_record_ends_the_command_after_the_flushed_records(sam, tmp_path, what, bits):
    recs, at, status, msg = m.stop_files()[what]
    path = tmp_path / "in.bam"
    raw = m.write(path, recs)
    code, out, err, runs = three(sam, path, expect_path="host reader")
    assert (out, err, code) == m.literal(raw, 5000) and (err, code) == (msg, status)
    assert b"sk_bam_file_recalc_tlen: declined (bits 0x%x)" % bits in runs[0][2]
