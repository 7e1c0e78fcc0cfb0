"""CPU: the host reader of `sam coverage histogram` (SEQKIT_HOST_INFLATE=1, and "-" on stdin: no device needed) against the literal
statement of tests/bam_coverage_model.py: stdout bytes, stderr and status in the three modes, every REGION form, the BED oddities, and
the command's failures."""
import pytest

from tests import bam_coverage_model as m
from tests import cli_util as cu

HOST = {"SEQKIT_HOST_INFLATE": "1"}
TEXT = b"@HD\tVN:1.6\n"
BED = (b"#comment\ntrack name=x\nbrowser position\n\n   \nref1\t10\t200\nref1 150 400\nref1\t400\t450\nref3\t0\t99999\nnope\t1\t2\nref5  400\t500  extra\n"
       b"ref7\t50\t50\nref9\t3000\t9000\nodd:1-5\t3\t9\r\n")


@pytest.fixture(scope="module")
def sam(hip_lib):
    from seqkit_amd import build
    build.build_hosts()
    return cu.SAM


@pytest.fixture(scope="module")
def bam(tmp_path_factory):
    d = tmp_path_factory.mktemp("coverage")
    refs = m.refs_for() + [(b"odd:1-5", 500)]
    recs = m.sorted_records(3000, refs, skip_refs=(4,)) + [m.rec(b"colon", 11, 3, 0, ((m.M, 4),))]
    return d, d / "in.bam", m.write(d / "in.bam", recs, text=TEXT, refs=refs, piece=0x3000)


def run(sam, argv, stdin=None):
    return cu.run(sam, ["coverage", "histogram"] + argv, stdin=stdin, env=HOST)


def expect(raw, mode):
    hist, dropped, n_pos, _ = m.literal(raw, mode)
    assert sum(hist) + dropped == n_pos == m.target_size(raw, mode)
    return m.stdout_of(hist)


def test_everywhere_from_a_file_and_from_stdin(sam, bam):
    _, path, raw = bam
    exp = expect(raw, ("everywhere",))
    assert exp.count(b"\n") == 10001 and exp.startswith(b"0\t") and exp.endswith(b"\n10000\t0\n")
    assert run(sam, [str(path)]) == (0, exp, b"")
    assert run(sam, ["-"], stdin=open(path, "rb").read()) == (0, exp, b"")
    assert run(sam, ["--region=everywhere", "--regions", "everywhere", str(path)]) == (0, exp, b"")


@pytest.mark.parametrize("region", ["ref2", "ref2:100", "ref2:100-1,000", "ref2:0-50", "ref2:1,0-99999", "odd:1-5", "odd:1-5:2-7", "ref4", "ref4:7-7", "ref2:9-3"])
def test_region_forms(sam, bam, region):
    _, path, raw = bam
    exp = expect(raw, ("region", region.encode()))
    assert run(sam, ["--region=" + region, str(path)]) == (0, exp, b"")
    assert run(sam, ["-", "--region", region], stdin=open(path, "rb").read()) == (0, exp, b"")


@pytest.mark.parametrize("region", ["nope", "ref2:", "ref2:x", "ref2:5-", "ref2:-5", "ref2:1-2-3", "ref2 ", "odd"])
def test_unknown_region_gives_zeros_and_status_0(sam, bam, region):
    _, path, raw = bam
    code, out, err = run(sam, ["--region", region, str(path)])
    assert code == 0 and out == m.stdout_of([0] * m.BINS) == expect(raw, ("region", region.encode()))
    assert err.count(b"\n") == 1 and region.encode() in err and b"nknown region" in err


def test_bed(sam, bam):
    d, path, raw = bam
    (d / "r.bed").write_bytes(BED)
    exp = expect(raw, ("bed", BED))
    assert exp != expect(raw, ("everywhere",)) and exp != m.stdout_of([0] * m.BINS)
    assert run(sam, ["--regions=" + str(d / "r.bed"), str(path)]) == (0, exp, b"")
    assert run(sam, ["--regions", str(d / "r.bed"), "-"], stdin=open(path, "rb").read()) == (0, exp, b"")
    # a reference with counted records none of which overlaps an interval is not reported: ref4 has none at all, ref8's lie elsewhere
    refs = m.refs_of(raw)
    far = b"ref8\t%d\t%d\nref4\t0\t10\n" % (refs[8][1] + 200, refs[8][1] + 300)
    (d / "far.bed").write_bytes(far)
    assert run(sam, ["--regions", str(d / "far.bed"), str(path)]) == (0, m.stdout_of([0] * m.BINS), b"") and m.target_size(raw, ("bed", far)) == 0


@pytest.mark.parametrize("line", [b"ref1\t10\n", b"ref1\tx\t20\n", b"ref1\t10\t2e3\n", b"ref1 -1 5\n"])
def test_bad_bed_line(sam, bam, line):
    d, path, raw = bam
    (d / "bad.bed").write_bytes(b"ref1\t1\t2\n" + line + b"ref2\t1\t2\n")
    code, out, err = run(sam, ["--regions", str(d / "bad.bed"), str(path)])
    assert (code, out) == (255, b"") and err.startswith(m.MSG_BED + line)


def test_both_options_and_usage(sam, bam):
    d, path, raw = bam
    (d / "r.bed").write_bytes(BED)
    assert run(sam, ["--region=ref1", "--regions=" + str(d / "r.bed"), str(path)]) == (255, b"", m.MSG_BOTH)
    code, out, err = run(sam, [])
    assert (code, out) == (255, b"") and b"sam coverage histogram [options] <bam_file>" in err and b"--regions=BED" in err
    code, out, err = run(sam, [str(path), "extra"])
    assert code == 255 and b"Usage:" in err


def test_unreadable_bam(sam, bam, tmp_path):
    d, path, raw = bam
    data = open(path, "rb").read()
    cut = tmp_path / "cut.bam"
    cut.write_bytes(data[:len(data) // 2])
    code, out, err = run(sam, [str(cut)])
    assert code == 255 and out == b"" and err.startswith(b"ERROR: ")
    code, out, err = run(sam, [str(tmp_path / "missing.bam")])
    assert code == 255 and err == b"ERROR: Cannot open BAM file '%s'\n" % str(tmp_path / "missing.bam").encode()
