"""CPU: the host reader of `sam recalculate tlen` (SEQKIT_HOST_INFLATE=1; its members deflated by zlib on the host, SEQKIT_GPU_DEFLATE=0:
no device needed), from a file and from stdin, against tests/bam_recalc_tlen_model.py: inflated stdout, stderr bytes and status; every
record the reference's loop stops at; the --max-len errors and the usage."""
import pytest

from tests import bam_recalc_tlen_model as m
from tests import cli_util as cu


@pytest.fixture(scope="module")
def sam(hip_lib):
    from seqkit_amd import build
    build.build_hosts()
    return cu.SAM


HOST = {"SEQKIT_HOST_INFLATE": "1", "SEQKIT_GPU_DEFLATE": "0"}
CMD = ["recalculate", "tlen"]


@pytest.fixture(scope="module")
def bam(tmp_path_factory):
    path = tmp_path_factory.mktemp("recalc_tlen") / "in.bam"
    return path, m.write(path, m.served_records(3000, seed=1))


def run(sam, argv, stdin=None):
    code, out, err = cu.run(sam, CMD + argv, stdin=stdin, env=HOST)
    mem = m.members(out) if out else []
    if out:
        assert out.endswith(m.EOF_BLOCK) and all(0 < len(x) <= 0xFF00 for x, _ in mem[:-1])
    return code, b"".join(x for x, _ in mem), err, mem


@pytest.mark.parametrize("max_len", [1, 5000, 1 << 40])
def test_host_matches_model(sam, bam, max_len):
    path, raw = bam
    exp = m.literal(raw, max_len)
    assert exp[2] == 0 and exp[1].count(b"\n") > 100
    for form in (["--max-len=%d" % max_len], ["--max-len", "%d" % max_len]):
        code, out, err, mem = run(sam, form + [str(path)])
        assert (out, err, code) == exp
        assert not all(stored for _, stored in mem[:-1])
    code, out, err, mem = run(sam, ["--uncompressed", "--max-len=%d" % max_len, str(path)])
    assert (out, err, code) == exp and all(stored for _, stored in mem[:-1])


def test_host_default_max_len_is_5000(sam, bam):
    path, raw = bam
    code, out, err, _ = run(sam, [str(path)])
    assert (out, err, code) == m.literal(raw, 5000) != m.literal(raw, 5001)


def test_host_file_and_stdin_agree(sam, bam):
    """both ways into the host loop: the same inflated output and stderr, the model's"""
    path, raw = bam
    data = open(path, "rb").read()
    from_file = run(sam, ["--max-len=300", str(path)])[:3]
    for argv in (["--max-len=300", "-"], ["-", "--max-len", "300"]):
        assert run(sam, argv, stdin=data)[:3] == from_file
    assert (from_file[1], from_file[2], from_file[0]) == m.literal(raw, 300)


@pytest.mark.parametrize("what", sorted(m.stop_files()))
def test_host_stops(sam, tmp_path, what):
    """message, status, and on stdout the records already flushed from the FIFO, closed by the EOF block"""
    recs, at, status, msg = m.stop_files()[what]
    path = tmp_path / "in.bam"
    raw = m.write(path, recs)
    exp = m.literal(raw, 5000)
    assert exp[1:] == (msg, status)
    for stdin, argv in ((None, [str(path)]), (open(path, "rb").read(), ["-"])):
        code, out, err, _ = run(sam, argv, stdin=stdin)
        assert (out, err, code) == exp
    assert (len(list(m.records(exp[0]))) == 0) == (what == "first record")


def test_host_no_records(sam, tmp_path):
    path = tmp_path / "empty.bam"
    raw = m.write(path, [], text=b"\n\n\0\0")
    code, out, err, _ = run(sam, [str(path)])
    assert (code, err) == (0, b"") and out == m.out_header(raw)


@pytest.mark.parametrize("text", ["0", "-5", "abc", "", "1e3", " 5", "9223372036854775808", "0x10", "+"])
def test_bad_max_len(sam, text):
    assert m.parse_max_len(text) <= 0
    code, out, err = cu.run(sam, CMD + ["--max-len=" + text, "/nonexistent/x.bam"], env=HOST)      # (refused before the file is opened)
    assert code == 255 and out == b"" and err == m.MSG_MAX_LEN


def test_max_len_with_a_sign_and_at_the_top_of_i64(sam, bam):
    path, raw = bam
    for text in ("+5000", "9223372036854775807"):
        code, out, err, _ = run(sam, ["--max-len=" + text, str(path)])
        assert (out, err, code) == m.literal(raw, m.parse_max_len(text))


USAGE = b"""
Usage:
  sam recalculate tlen [options] <bam_file>

Options:
  --uncompressed    Output in uncompressed BAM format
  --max-len=N       Maximum fragment length [default: 5000]

Recalculates SAM record TLEN (template length) field based on the distance
between the 5' ends of paired mates. This ensures that the TLEN represents the\x20
actual DNA fragment length.
"""


@pytest.mark.parametrize("argv", [[], ["a.bam", "extra"], ["--nonsense", "a.bam"], ["--max-len"], ["-x", "a.bam"], ["--uncompressed=1", "a.bam"]])
def test_usage(sam, argv):
    code, out, err = cu.run(sam, CMD + argv, env=HOST)
    assert code == 255 and out == b"" and err == b"ERROR: Invalid arguments.\n" + USAGE + b"\n"


def test_top_level_usage_is_unchanged(sam):
    code, out, err = cu.run(sam, ["recalculate"], env=HOST)
    assert code == 0 and out == b"" and err.startswith(b"\nUsage:\n  sam merge <bam_files>...\n") and b"recalculate" not in err
