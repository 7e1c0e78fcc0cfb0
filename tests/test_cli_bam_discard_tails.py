"""GPU: `sam discard tail artifacts` on the device path (sk_bam_file_discard_tails), the host reader (SEQKIT_HOST_INFLATE=1) and stdin:
the same inflated stdout and the same stderr (the seconds masked), equal to tests/bam_discard_tails_model.py, and the reference's
statuses; every file the device declines ends on the host reader with the model's status and output."""
import pytest

from tests import bam_discard_tails_model as m
from tests import bam_out_util as bu
from tests.bam_out_util import sam  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

WHO = b"sam discard tail artifacts: "


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("tails_cli")
    fasta, genome = m.write_genome(d)
    path = d / "in.bam"
    return fasta, genome, path, m.write(path, list(m.served_records()), text=m.TEXT, refs=m.REFS)


def three(sam, fasta, path, opts=(), expect_path="device path", env=None):
    """device path, host reader, stdin: (code, inflated stdout, stderr without the trace's lines and with the seconds masked) of the
    three, checked equal, and the runs; the trace names the path.  (bam_out_util.three compares stderr as it is; here the seconds
    line is masked first.)"""
    argv = ["discard", "tail", "artifacts"] + list(opts) + [str(fasta)]
    runs = []
    for e, args, stdin in (({"SK_BAMFILE_TRACE": "1"}, argv + [str(path)], None),
                           ({"SK_BAMFILE_TRACE": "1", "SEQKIT_HOST_INFLATE": "1"}, argv + [str(path)], None),
                           ({"SK_BAMFILE_TRACE": "1"}, argv + ["-"], open(path, "rb").read())):
        runs.append(bu.cu.run(sam, args, stdin=stdin, env=dict(e, **(env or {}))))
    traces = [[ln for ln in err.split(b"\n") if ln.startswith(WHO)] for _, _, err in runs]
    assert traces[0] and traces[0][0].startswith(WHO + expect_path.encode()), traces[0]
    assert traces[1] == [WHO + b"host reader"] and traces[2] == traces[1]
    assert runs[0][0] == runs[1][0] == runs[2][0]
    for _, out, _ in runs:
        assert out.endswith(m.EOF_BLOCK)
    outs = [bu.inflated(m, out) for _, out, _ in runs]
    assert outs[0] == outs[1] == outs[2]
    strip = [m.mask_seconds(b"".join(ln for ln in err.splitlines(True) if not ln.startswith(WHO) and not ln.startswith(b"sk_bam"))) for _, _, err in runs]
    assert strip[0] == strip[1] == strip[2]
    return runs[0][0], outs[0], strip[0], runs


@pytest.mark.parametrize("T,opt", [(20, "--threshold=0.15"), (1, "--threshold=0"), (33, "--threshold=1"), (64, "--mismatches=3"), (300, "--threshold=0.15")])
def test_three_paths_match_model(sam, files, T, opt):
    fasta, genome, path, raw = files
    key, val = opt.split("=")
    exp = m.model(raw, genome, T, float(val)) if key == "--threshold" else m.model(raw, genome, T, 0.15, mismatches=int(val))
    code, out, err, runs = three(sam, fasta, path, ["--tail-length=%d" % T, opt])
    assert (code, out, err) == (exp[2], exp[0], exp[1]) and code == 0
    assert WHO + b"device path, %d records" % (exp[3][0] - exp[3][1]) in runs[0][2]


def test_defaults_and_small_windows_on_the_device_path(sam, files):
    fasta, genome, path, raw = files
    exp = m.model(raw, genome)
    assert three(sam, fasta, path)[:3] == (0, exp[0], exp[1])
    assert three(sam, fasta, path, env={"SK_BAMFILE_WINDOW": "4096"})[:3] == (0, exp[0], exp[1])


@pytest.mark.parametrize("label", sorted(m.stop_cases()))
def test_declined_files_end_on_the_host_reader(sam, files, tmp_path, label):
    fasta, genome, _, _ = files
    before, stop, status, line = m.stop_cases()[label]
    path = tmp_path / "stop.bam"
    raw = m.write(path, before + [stop] + before, text=m.TEXT, refs=m.REFS)
    exp = m.model(raw, genome)
    code, out, err, runs = three(sam, fasta, path, expect_path="host reader")
    assert (code, out, err) == (exp[2], exp[0], exp[1]) and code == status and err.endswith(line)
    assert b"sk_bam_file_discard_tails: declined (bits 0x" in runs[0][2]


def test_an_op_no_tail_reaches_is_declined_and_served_by_the_host(sam, files, tmp_path):
    fasta, genome, _, _ = files
    recs = list(m.served_records(40, seed=9))
    recs[20] = m.record(b"spliced", 0, 100, [(0, 30), (3, 500), (0, 30)], [1] * 60, 0)
    path = tmp_path / "n.bam"
    raw = m.write(path, recs, text=m.TEXT, refs=m.REFS)
    exp = m.model(raw, genome, 20, 1.0)
    code, out, err, runs = three(sam, fasta, path, ["--threshold=1"], expect_path="host reader")
    assert (code, out, err) == (0, exp[0], exp[1]) and b"sk_bam_file_discard_tails: declined (bits 0x1)" in runs[0][2]
    assert recs[20] in out


def test_debug_stays_on_the_host(sam, files, tmp_path):
    fasta, genome, _, _ = files
    path = tmp_path / "some.bam"
    raw = m.write(path, list(m.served_records(300, seed=3)), text=m.TEXT, refs=m.REFS)
    name = str(tmp_path / "some_tail_discards_debug.bam").encode()
    exp = m.model(raw, genome, debug_filename=name)
    code, out, err = bu.cu.run(sam, ["discard", "tail", "artifacts", "--debug", str(fasta), str(path)], env={"SK_BAMFILE_TRACE": "1"})
    assert code == 0 and bu.inflated(m, out) == exp[0] and WHO + b"host reader\n" in err          # (never offered to the device)
    assert m.mask_seconds(b"".join(ln for ln in err.splitlines(True) if not ln.startswith(b"sk_bam") and not ln.startswith(WHO))) == exp[1]
    assert bu.inflated(m, open(name.decode(), "rb").read()) == m.rm.out_header(raw) + b"".join(exp[5])
