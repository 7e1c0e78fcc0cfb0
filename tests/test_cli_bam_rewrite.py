"""GPU: `sam trim qnames`, `sam tags from qname` and `sam qname from tags` on the device path (sk_bam_file_rewrite), the host reader
(SEQKIT_HOST_INFLATE=1) and stdin: the same inflated stdout, equal to tests/bam_rewrite_model.py, and the reference's statuses."""
import pytest

from tests import bam_rewrite_model as m
from tests import bam_out_util as bu
from tests import cli_util as cu
from tests.bam_out_util import sam  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu


def three(sam, words, path, extra=(), expect_path="device path"):
    return bu.three(sam, m, words, path, extra, expect_path)


@pytest.mark.parametrize("op,uncompressed", [("trim qnames", False), ("tags from qname", False), ("tags from qname", True),
                                              ("qname from tags", False), ("qname from tags", True)])
def test_three_paths_match_model(sam, tmp_path, op, uncompressed):
    path = tmp_path / "in.bam"
    raw = m.write(path, m.served_records(op, 1500, seed=3))
    code, out, err, runs = three(sam, op.split(), path, ["--uncompressed"] if uncompressed else [])
    assert code == 0 and out == m.model(raw, op)[0] and err == b""
    if uncompressed:
        for _, o, _ in runs:
            assert all(stored for _, stored in m.members(o)[:-1])


def test_trim_has_no_uncompressed(sam, tmp_path):
    path = tmp_path / "in.bam"
    m.write(path, m.served_records("trim qnames", 10))
    code, out, err = cu.run(sam, ["trim", "qnames", "--uncompressed", str(path)])
    assert code == 255 and err.startswith(b"ERROR: Invalid arguments.\n") and b"sam trim qnames [options] <bam_file>" in err


def test_unsupported_tag(sam, tmp_path):
    path = tmp_path / "in.bam"
    m.write(path, [m.record(b"r1 UMI:AC", 10), m.record(b"r2 BAD", 10), m.record(b"r3", 10)])
    code, _, err, _ = three(sam, ["tags", "from", "qname"], path, expect_path="host reader")
    assert code == 255 and err.strip() == b"ERROR: Tag 'BAD' is not supported."


@pytest.mark.parametrize("name", [b" x", b"a x"])
def test_trim_space_at_0_or_1(sam, tmp_path, name):
    path = tmp_path / "in.bam"
    recs = [m.record(b"first/1 a", 10), m.record(b"second", 10), m.record(name, 10), m.record(b"never", 10)]
    raw = m.write(path, recs)
    exp, c = m.model(raw, "trim qnames")
    assert c == 101
    code, out, _, runs = three(sam, ["trim", "qnames"], path, expect_path="host reader")
    assert code == 101 and out == exp
    for _, o, _ in runs:
        assert o.endswith(m.EOF_BLOCK)


def test_qname_too_long(sam, tmp_path):
    path = tmp_path / "in.bam"
    raw = m.write(path, [m.record(b"ok", 10, aux=m.aux_z(b"RX", b"AC")), m.record(b"n" * 245, 10, aux=m.aux_z(b"RX", b"ACGTACGT"))])
    exp, c = m.model(raw, "qname from tags")
    assert c == 101
    code, out, _, _ = three(sam, ["qname", "from", "tags"], path, expect_path="host reader")
    assert code == 101 and out == exp


def test_header_normalized(sam, tmp_path):
    path = tmp_path / "in.bam"
    raw = m.write(path, [m.record(b"ab/1 c", 10)], text=b"@HD\tVN:1.6\n@CO\tx\n\n\n\0junk\0\0")
    code, out, _, _ = three(sam, ["trim", "qnames"], path)
    assert code == 0 and out == m.model(raw, "trim qnames")[0]
    assert out[8:8 + 17] == b"@HD\tVN:1.6\n@CO\tx\n" and out[4] == 17


def test_round_trip_umi(sam, tmp_path):
    path = tmp_path / "in.bam"
    names = [b"read%d UMI:%s" % (i, b"ACGT"[i % 4:] * 3) for i in range(200)] + [b"plain", b"empty UMI:"]
    m.write(path, [m.record(n, 30, seed=i) for i, n in enumerate(names)])
    code, tagged, err = cu.run(sam, ["tags", "from", "qname", str(path)])
    assert code == 0, err
    mid = tmp_path / "tagged.bam"
    mid.write_bytes(tagged)
    code, back, err = cu.run(sam, ["qname", "from", "tags", str(mid)])
    assert code == 0, err
    raw = bu.inflated(m, back)
    got = [r[36:36 + r[12] - 1] for r in m.records(raw)]
    want = [n.replace(b" UMI:", b" RX:") for n in names]
    assert got == want
    for r in m.records(raw):                                               # the RX field stays
        if r[36:36 + r[12] - 1] != b"plain":
            assert b"RXZ" in r[36 + r[12]:]
