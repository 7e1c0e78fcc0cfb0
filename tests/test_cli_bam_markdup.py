"""GPU: `sam mark duplicates` on the device path (sk_bam_file_markdup), the host reader (SEQKIT_HOST_INFLATE=1) and stdin: the same
inflated stdout, equal to literal() of tests/bam_markdup_model.py, the same stderr, and the reference's statuses."""
import pytest

from tests import bam_markdup_model as m
from tests import bam_out_util as bu
from tests.bam_out_util import sam  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bam(tmp_path_factory):
    path = tmp_path_factory.mktemp("markdup") / "in.bam"
    return path, m.write(path, m.sorted_records(11, 25000, big=1100))


def three(sam, path, extra, expect_path="device path"):
    return bu.three(sam, m, ["mark", "duplicates"], path, extra, expect_path)


@pytest.mark.parametrize("ignore_umi", [False, True])
@pytest.mark.parametrize("uncompressed", [False, True])
def test_three_paths_match_literal(sam, bam, ignore_umi, uncompressed):
    path, raw = bam
    code, out, err, runs = three(sam, path, (["--uncompressed"] if uncompressed else []) + (["--ignore-umi"] if ignore_umi else []))
    exp, stop, msg = m.literal(raw, ignore_umi)
    assert stop == 0 and code == 0 and out == exp and err == msg
    if uncompressed:
        for _, o, _ in runs:
            assert all(stored for _, stored in m.members(o)[:-1])


def test_no_records(sam, tmp_path):
    path = tmp_path / "empty.bam"
    raw = m.write(path, [])
    code, out, err, _ = three(sam, path, [])
    assert (out, code, err) == m.literal(raw) and b"NaN%" in err


@pytest.mark.parametrize("what", ["secondary", "unsorted", "cigar"])
def test_declined_file_falls_back_to_the_host_reader(sam, tmp_path, what):
    base = m.sorted_records(5, 2300, big=0)
    at = 1500
    tid, pos = m.core(base[at - 1])[:2]
    bad = {"secondary": m.rec(b"sec", tid, pos, 0x100), "unsorted": m.rec(b"back", tid, pos - 1), "cigar": m.rec(b"op9", tid, pos, 16, ((9, 20),), l_seq=20)}[what]
    path = tmp_path / "in.bam"
    raw = m.write(path, base[:at] + [bad] + base[at:])
    exp, stop, msg = m.literal(raw)
    code, out, err, runs = three(sam, path, [], expect_path="host reader")
    assert code == stop and out == exp and 0 < len(list(m.records(out))) <= at
    assert (b"panicked" in err) if what == "cigar" else err == msg
    assert b"sk_bam_file_markdup: declined (bits %s)" % {"secondary": b"0x1", "unsorted": b"0x2", "cigar": b"0x20"}[what] in runs[0][2]


def test_served_file_with_unparsable_aux_falls_back_and_matches(sam, tmp_path):
    """aux data that stop parsing: the device declines, the host reader reads them as the reference does (no UMI)"""
    base = m.sorted_records(5, 2300, big=0)
    tid, pos = m.core(base[99])[:2]
    path = tmp_path / "in.bam"
    raw = m.write(path, base[:100] + [m.rec(b"aux", tid, pos, aux=b"XX?\1")] + base[100:])
    code, out, err, runs = three(sam, path, [], expect_path="host reader")
    assert (out, code, err) == m.literal(raw)
    assert b"declined (bits 0x10)" in runs[0][2]
