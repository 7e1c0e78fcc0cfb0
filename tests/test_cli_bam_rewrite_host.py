"""CPU: the host reader of `sam tags from qname` and `sam qname from tags` with --uncompressed (stored members: no device needed),
from a file and from stdin, against tests/bam_rewrite_model.py."""
import pytest

from tests import bam_rewrite_model as m
from tests import cli_util as cu


@pytest.fixture(scope="module")
def sam(hip_lib):
    from seqkit_amd import build
    build.build_hosts()
    return cu.SAM


HOST = {"SEQKIT_HOST_INFLATE": "1"}


@pytest.mark.parametrize("op", ["tags from qname", "qname from tags"])
@pytest.mark.parametrize("stdin", [False, True])
def test_host_uncompressed_matches_model(sam, tmp_path, op, stdin):
    path = tmp_path / "in.bam"
    raw = m.write(path, m.served_records(op, 400, seed=11))
    args = op.split() + ["--uncompressed", "-" if stdin else str(path)]
    code, out, err = cu.run(sam, args, stdin=open(path, "rb").read() if stdin else None, env=HOST)
    assert code == 0, err
    mem = m.members(out)
    assert all(stored for _, stored in mem[:-1]) and out.endswith(m.EOF_BLOCK)
    assert b"".join(x for x, _ in mem) == m.model(raw, op)[0]


def test_host_unsupported_tag(sam, tmp_path):
    path = tmp_path / "in.bam"
    m.write(path, [m.record(b"r1 UMI:AC", 10), m.record(b"r2 zz", 10)])
    code, _, err = cu.run(sam, ["tags", "from", "qname", "--uncompressed", str(path)], env=HOST)
    assert code == 255 and err == b"ERROR: Tag 'zz' is not supported.\n"


def test_host_qname_too_long_keeps_earlier_records(sam, tmp_path):
    path = tmp_path / "in.bam"
    raw = m.write(path, [m.record(b"ok", 10, aux=m.aux_z(b"RX", b"AC")), m.record(b"n" * 250, 10, aux=m.aux_z(b"RX", b"A"))])
    exp, c = m.model(raw, "qname from tags")
    code, out, _ = cu.run(sam, ["qname", "from", "tags", "--uncompressed", str(path)], env=HOST)
    assert c == code == 101
    assert out.endswith(m.EOF_BLOCK) and b"".join(x for x, _ in m.members(out)) == exp


@pytest.mark.parametrize("words,usage", [(["trim", "qnames"], b"sam trim qnames [options] <bam_file>"),
                                         (["tags", "from", "qname"], b"--uncompressed     Output in uncompressed BAM format"),
                                         (["qname", "from", "tags"], b"appends them to the QNAME.")])
def test_invalid_arguments(sam, words, usage):
    code, out, err = cu.run(sam, words)
    assert code == 255 and out == b"" and err.startswith(b"ERROR: Invalid arguments.\n") and usage in err
