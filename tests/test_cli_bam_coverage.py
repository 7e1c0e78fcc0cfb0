"""GPU: `sam coverage histogram` on the device path (sk_bam_file_coverage), through the host reader (SEQKIT_HOST_INFLATE=1) and from
stdin: identical stdout, equal to the literal statement of tests/bam_coverage_model.py, in the three modes; an unknown region; a file
the device declines."""
import pytest

from tests import bam_coverage_model as m
from tests import cli_util as cu
from tests.bam_out_util import sam  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

WHO = b"sam coverage histogram: "
TEXT = b"@HD\tVN:1.6\n"
BED = b"#comment\ntrack x\nref1\t10\t200\nref1 150 400\nref3\t0\t99999\nnope\t1\t2\nref5  400\t500\nref9\t3000\t9000\nodd:1-5\t3\t9\n"


@pytest.fixture(scope="module")
def bam(tmp_path_factory):
    d = tmp_path_factory.mktemp("coverage")
    refs = m.refs_for() + [(b"odd:1-5", 500)]
    recs = m.sorted_records(25000, refs, skip_refs=(4,)) + [m.rec(b"colon", 11, 3, 0, ((m.M, 4),))]
    (d / "r.bed").write_bytes(BED)
    return d, d / "in.bam", m.write(d / "in.bam", recs, text=TEXT, refs=refs)


def three(sam, path, opts, expect_path="device path"):  # noqa: F811
    """device path, host reader, stdin: the same status and stdout, and the same stderr but for the trace; the trace names the path"""
    argv = ["coverage", "histogram"] + opts
    runs = []
    for e, args, stdin in (({"SK_BAMFILE_TRACE": "1"}, argv + [str(path)], None),
                           ({"SK_BAMFILE_TRACE": "1", "SEQKIT_HOST_INFLATE": "1"}, argv + [str(path)], None),
                           ({"SK_BAMFILE_TRACE": "1"}, argv + ["-"], open(path, "rb").read())):
        runs.append(cu.run(sam, args, stdin=stdin, env=e))
    traces = [[ln for ln in err.split(b"\n") if ln.startswith(WHO)] for _, _, err in runs]
    assert traces[0] and traces[0][0].startswith(WHO + expect_path.encode()), runs[0][2]
    assert traces[1] == [WHO + b"host reader"] and traces[2] == traces[1]
    assert runs[0][:2] == runs[1][:2] == runs[2][:2]
    strip = [b"".join(ln + b"\n" for ln in err.split(b"\n")[:-1] if not ln.startswith(WHO) and not ln.startswith(b"sk_bam")) for _, _, err in runs]
    assert strip[0] == strip[1] == strip[2]
    return runs[0][0], runs[0][1], strip[0], runs


@pytest.mark.parametrize("opts,mode", [([], ("everywhere",)), (["--region=ref6:100-1,000"], ("region", b"ref6:100-1,000")),
                                       (["--region", "odd:1-5"], ("region", b"odd:1-5")), (["--regions=r.bed"], ("bed", BED))],
                         ids=["everywhere", "region", "colon", "bed"])
def test_three_paths_match_model(sam, bam, opts, mode):  # noqa: F811
    d, path, raw = bam
    opts = [o.replace("r.bed", str(d / "r.bed")) for o in opts]
    hist, dropped, n_pos, n_counted = m.literal(raw, mode)
    assert sum(hist) + dropped == n_pos == m.target_size(raw, mode) > 0
    code, out, err, runs = three(sam, path, opts)
    assert (code, out, err) == (0, m.stdout_of(hist), b"")
    assert WHO + b"device path, %d records" % n_counted in runs[0][2]


def test_unknown_region(sam, bam):  # noqa: F811
    d, path, raw = bam
    code, out, err, _ = three(sam, path, ["--region=odd:1"])
    assert code == 0 and out == m.stdout_of([0] * m.BINS) and err.count(b"\n") == 1 and b"odd:1" in err


def test_declined_file_goes_to_the_host_reader(sam, tmp_path):  # noqa: F811
    """a record whose variable part is shorter than its fields: the device declines (bit 8) and the host reader says what it always says"""
    refs = m.refs_for(seed=3)
    recs = m.sorted_records(300, refs, seed=3)
    bad = bytearray(m.rec(b"bad", 0, 5, 0, ((m.M, 20),)))
    bad[16:18] = (4000).to_bytes(2, "little")                                # n_cigar_op beyond the record
    m.write(tmp_path / "bad.bam", recs[:200] + [bytes(bad)] + recs[200:], text=TEXT, refs=refs)
    code, out, err, runs = three(sam, tmp_path / "bad.bam", [], expect_path="host reader")
    assert (code, out, err) == (255, b"", b"ERROR: Invalid BAM record.\n")
    assert b"sk_bam_file_coverage: declined (bits 0x8)" in runs[0][2]


def test_events_in_the_compressed_files_buffer(sam, tmp_path):  # noqa: F811
    """records whose aux data do not compress: the file is larger than the events' working memory, which then lies in the device
    buffer of the compressed file (the other files of these tests compress too well and take memory of their own)"""
    import random
    rnd = random.Random(8)
    refs = m.refs_for(seed=8)
    printable = bytes(33 + b % 94 for b in range(256))
    recs = [m.rec(b"r%d" % k, k % len(refs), 3 * k % 280, 0, rnd.choice(m.CIGARS), aux=b"XXZ" + rnd.randbytes(1500).translate(printable) + b"\0")
            for k in range(3000)]
    raw = m.write(tmp_path / "aux.bam", recs, text=TEXT, refs=refs)
    code, out, err = cu.run(sam, ["coverage", "histogram", str(tmp_path / "aux.bam")], env={"SK_BAMFILE_TRACE": "1"})
    assert b"bytes of scratch in the compressed file's buffer" in err and WHO + b"device path, 3000 records" in err
    assert (code, out) == (0, m.stdout_of(m.literal(raw)[0]))
