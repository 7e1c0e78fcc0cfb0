"""CPU: the host reader of `sam minimize` with --uncompressed (stored members: no device needed), from a file and from stdin, against
tests/bam_minimize_model.py; the command's error messages and usage."""
import pytest

from tests import bam_minimize_model as m
from tests import cli_util as cu


@pytest.fixture(scope="module")
def sam(hip_lib):
    from seqkit_amd import build
    build.build_hosts()
    return cu.SAM


HOST = {"SEQKIT_HOST_INFLATE": "1"}


@pytest.fixture(scope="module")
def bam(tmp_path_factory):
    path = tmp_path_factory.mktemp("minimize") / "in.bam"
    return path, m.write(path, m.served_records())


@pytest.mark.parametrize("combo,fill", [(c, None) for c in m.COMBOS] + [("tags+base-qualities", 0), ("all", 30), ("all", 255)])
@pytest.mark.parametrize("stdin", [False, True])
def test_host_uncompressed_matches_model(sam, bam, combo, fill, stdin):
    path, raw = bam
    argv = ["minimize", "--uncompressed"] + m.args(combo, fill) + ["-" if stdin else str(path)]
    code, out, err = cu.run(sam, argv, stdin=open(path, "rb").read() if stdin else None, env=HOST)
    assert code == 0, err
    mem = m.members(out)
    assert all(stored for _, stored in mem[:-1]) and out.endswith(m.EOF_BLOCK)
    exp, stop = m.model(raw, combo, 255 if fill is None else fill)
    assert stop is None and b"".join(x for x, _ in mem) == exp


def test_host_cigar_op_9_keeps_earlier_records(sam, tmp_path):
    path = tmp_path / "in.bam"
    raw = m.write(path, [m.record(b"a/1", 11, pad=3), m.record(b"a/2", 10), m.record(b"b", 10, cigar_op=9), m.record(b"c", 10)])
    for combo in m.COMBOS:
        exp, c = m.model(raw, combo)
        code, out, err = cu.run(sam, ["minimize", "--uncompressed"] + m.args(combo) + [str(path)], env=HOST)
        assert c == code == 101 and b"panicked" in err
        assert out.endswith(m.EOF_BLOCK) and b"".join(x for x, _ in m.members(out)) == exp


@pytest.mark.parametrize("argv,msg", [
    ([], b"One of --read-ids, --base-qualities, or --tags must be given."),
    (["--uncompressed"], b"One of --read-ids, --base-qualities, or --tags must be given."),
    (["--base-qualities"], b"Running 'sam minimize' with --base-qualities but without the --tags flag is not yet supported."),
    (["--base-qualities", "--read-ids"], b"Running 'sam minimize' with --base-qualities but without the --tags flag is not yet supported."),
    (["--tags", "--baseq-fill=256"], b"--baseq-fill must be an integer between 0 and 255."),
    (["--tags", "--baseq-fill=-1"], b"--baseq-fill must be an integer between 0 and 255."),
    (["--tags", "--baseq-fill=x"], b"--baseq-fill must be an integer between 0 and 255."),
    (["--baseq-fill=256"], b"--baseq-fill must be an integer between 0 and 255."),          # the fill is checked first
    (["--base-qualities", "--baseq-fill="], b"--baseq-fill must be an integer between 0 and 255."),
])
def test_error_messages(sam, tmp_path, argv, msg):
    path = tmp_path / "in.bam"
    m.write(path, [m.record(b"a", 10)])
    code, out, err = cu.run(sam, ["minimize"] + argv + [str(path)], env=HOST)
    assert code == 255 and out == b"" and err == b"ERROR: " + msg + b"\n"


USAGE = b"""
Usage:
  sam minimize [options] <bam_file>

Options:
  --uncompressed    Output in uncompressed BAM format
  --read-ids        Minimize read identifiers (i.e. QNAME fields)
  --base-qualities  Remove per-base qualities
  --tags            Remove all aux fields (tags)
  --baseq-fill=N    Base quality value to fill in as placeholder [default: 255]

Changes read IDs into simple numeric identifiers, removes per-base qualities,
and removes all auxiliary fields (tags).
"""


@pytest.mark.parametrize("argv", [[], ["--tags"], ["--tags", "a.bam", "b.bam"], ["--nonsense", "a.bam"], ["--tags=1", "a.bam"]])
def test_usage(sam, argv):
    code, out, err = cu.run(sam, ["minimize"] + argv)
    assert code == 255 and out == b"" and err == b"ERROR: Invalid arguments.\n" + USAGE + b"\n"
