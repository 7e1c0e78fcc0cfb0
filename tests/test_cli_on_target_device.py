"""GPU: `sam statistics --on-target=BED FILE` served from the file by the device (sk_bam_file_columns, sk_on_target_add_dev) against
the same command on the host reader (SEQKIT_HOST_INFLATE=1) and the reference's sweep as tests/bam_on_target_model.py states it (the
oracle command line rejects the option): same stdout, stderr and exit code.  The trace line says which path served the file; what
the device path declines falls back to the host reader and still matches."""
import pytest

from tests import bam_on_target_model as om
from tests import cli_util as cu
from tests.test_cli_gpu import make_bam, sorted_bam
from tests.test_gpu_on_target import model_records

pytestmark = pytest.mark.gpu

REFS = [("chr1", 1_000_000), ("chr2", 900_000), ("chrM", 16_000)]
NAMES = [name for name, _ in REFS]
ANNOUNCE = b"Reading target regions into memory...\n"
# comments, blank lines, a chromosome the BAM has but no record uses (chrM is used: chrU below is not), and the crafted shapes: one start
# many times, a long early region over later short ones, inverted and zero-length lines, touching neighbours, out of order
BED = (b"# targets\n\nchr1\t1000\t200000\nchr1\t500000\t600000\textra\tcolumns\n   \nchr1\t150000\t150010\nchr1\t150020\t150030\n"
       b"chr2\t400000\t450000\nchr2\t0\t300000\nchr2\t300000\t300100\nchr2\t300100\t300100\nchr2\t700\t650\n#chrM\t0\t16000\n"
       b"chrM\t500\t600\nchrM\t500\t520\nchrM\t500\t900\nchrM\t500\t500\n")


@pytest.fixture(scope="module")
def sam(hip_lib):
    from seqkit_amd import build
    build.build_hosts()
    return cu.SAM


def three(sam, args, tmp_path, want=None, stdin=None, path="device", n_records=None):
    """The device path, the host reader and the traced run: the same exit code, stdout and stderr between the first two, stdout as the
    model says (want), and one trace line that says which path served the file.  Returns the first run."""
    d = tmp_path / "run"
    d.mkdir(exist_ok=True)
    args = ["statistics"] + args
    dev = cu.run(sam, args, cwd=d, stdin=stdin)
    host = cu.run(sam, args, cwd=d, stdin=stdin, env={"SEQKIT_HOST_INFLATE": "1"})
    assert dev[0] == host[0], (dev[0], host[0], dev[2][-300:], host[2][-300:])
    assert dev[1] == host[1]
    assert dev[2] == host[2]
    if want is not None:
        assert dev[1] == want
    traced = cu.run(sam, args, cwd=d, stdin=stdin, env={"SK_BAMFILE_TRACE": "1"})
    assert traced[0] == dev[0] and traced[1] == dev[1]
    lines = [ln for ln in traced[2].split(b"\n") if ln.startswith(b"sam statistics: ")]
    if path is None:                                                        # the command ended before either path was taken
        assert lines == []
    else:
        assert len(lines) == 1, traced[2][-500:]
        if path == "device":
            assert lines[0] == b"sam statistics: device path, %d records" % n_records, lines
        else:
            assert lines[0] == b"sam statistics: host reader", lines
    for run in (dev, host, traced):
        assert run[2].count(ANNOUNCE) == (1 if any(a.startswith("--on-target") for a in args) else 0), run[2][-500:]
    return dev


@pytest.mark.parametrize("maker", [make_bam, sorted_bam], ids=["unsorted", "sorted"])
def test_device_path(sam, tmp_path, maker):
    bam, bed = tmp_path / "t.bam", tmp_path / "t.bed"
    refs = REFS + [("chrU", 1000)]
    raw = maker(str(bam), 30000, seed=31)
    cu.write_bam(str(bam), refs, raw)                                       # the same records under a header with one more reference
    recs = model_records(raw)
    bed.write_bytes(BED + b"chrU\t0\t10\n")
    counters = om.sweep(recs, om.parse_bed(BED, [n for n, _ in refs]))
    assert 0 < counters[4] < counters[3]
    dev = three(sam, [f"--on-target={bed}", str(bam)], tmp_path, want=om.report(counters), n_records=len(recs))
    assert dev[0] == 0 and dev[2] == ANNOUNCE


def test_edge_values_and_small_files(sam, tmp_path):
    bam, bed = tmp_path / "e.bam", tmp_path / "e.bed"
    # the model's crafted regions and records as a file: references r0 .. r4
    refs = [(f"r{k}", 1 << 30) for k in range(len(om.CRAFTED_BED))]
    bed.write_bytes(b"".join(b"r%d\t%d\t%d\n" % (tid, s - 1, e) for tid, rs in enumerate(om.CRAFTED_BED) for s, e in rs))
    # (a CIGAR cannot end before pos nor span 2^28: those unpaired records stay with tests/test_gpu_on_target.py; a paired record's end is not read)
    recs = [r[:6] + (r[3],) if r[0] & 1 else r for r in om.crafted_records() if r[0] & 1 or 0 <= r[6] - r[3] < 1 << 28] * 3
    cu.write_bam(str(bam), refs, [dict(zip(om.REC_FIELDS[:6], r[:6]), cigar=[(0, r[6] - r[3])], seq_len=0) for r in recs])
    assert any(r[3] == om.I32_MAX and r[5] == 5000 for r in recs) and any(r[5] == om.I32_MIN for r in recs) and any(r[3] == -1 for r in recs)
    counters = om.sweep(recs, om.CRAFTED_BED)
    assert 0 < counters[4] < counters[3]
    three(sam, ["--on-target", str(bed), str(bam)], tmp_path, want=om.report(counters), n_records=len(recs))
    # a comment-only BED: every fragment is off target
    bed.write_bytes(b"# nothing\n\n#r1\t0\t10\n")
    dev = three(sam, [f"--on-target={bed}", str(bam)], tmp_path, want=om.report(counters[:4] + [0]), n_records=len(recs))
    assert dev[1].endswith(b"On-target: 0.0%\n")
    # no records
    cu.write_bam(str(bam), refs, [])
    dev = three(sam, [f"--on-target={bed}", str(bam)], tmp_path, want=om.report([0, 0, 0, 0, 0]), n_records=0)
    assert dev[1].endswith(b"On-target: NaN%\n")


def test_fallbacks_truncated_and_stdin(sam, tmp_path):
    bam, bed = tmp_path / "f.bam", tmp_path / "f.bed"
    bed.write_bytes(BED)
    regions = om.parse_bed(BED, NAMES)
    # a truncated file: the records before the cut, then the reference's message
    make_bam(str(bam), 3000, seed=19, truncate=30000)
    dev = three(sam, [f"--on-target={bed}", str(bam)], tmp_path, path="host")
    assert dev[0] == 255 and dev[1] == b"" and dev[2].startswith(ANNOUNCE + b"ERROR: ")
    # stdin
    recs = model_records(sorted_bam(str(bam), 3000, seed=6))
    dev = three(sam, [f"--on-target={bed}", "-"], tmp_path, want=om.report(om.sweep(recs, regions)), stdin=bam.read_bytes(), path="host")
    assert dev[0] == 0


def test_fallbacks_bad_tid(sam, tmp_path):
    bam, bed = tmp_path / "f.bam", tmp_path / "f.bed"
    bed.write_bytes(BED)
    regions = om.parse_bed(BED, NAMES)
    # a mapped record whose tid has no reference: the reference panics there
    raw = make_bam(str(bam), 3000, seed=8)
    j = next(k for k, r in enumerate(model_records(raw)) if k > 100 and om.fragment(r)[3] is not None)
    raw[j]["tid"] = raw[j]["mtid"] = -1
    cu.write_bam(str(bam), REFS, raw)
    dev = three(sam, [f"--on-target={bed}", str(bam)], tmp_path, want=b"", path="host")
    assert dev[0] == 101 and dev[2].startswith(ANNOUNCE)
    with pytest.raises(om.BadTid):
        om.sweep(model_records(raw), regions)
    raw[j]["tid"] = raw[j]["mtid"] = len(REFS)
    cu.write_bam(str(bam), REFS, raw)
    assert three(sam, [f"--on-target={bed}", str(bam)], tmp_path, want=b"", path="host")[0] == 101
    # such a tid on a record the filters drop: the device path serves the file
    raw[j]["tid"] = raw[j]["mtid"] = -1
    raw[j]["flag"] |= 0x4
    cu.write_bam(str(bam), REFS, raw)
    three(sam, [f"--on-target={bed}", str(bam)], tmp_path, want=om.report(om.sweep(model_records(raw), regions)), n_records=len(raw))


def test_fallbacks_no_references_and_bed_overflow(sam, tmp_path):
    bam, bed = tmp_path / "f.bam", tmp_path / "f.bed"
    raw = make_bam(str(bam), 3000, seed=8)
    # a header without references and a comment-only BED: no On-target line
    for r in raw:
        r["flag"] |= 0x4
    cu.write_bam(str(bam), [], raw)
    bed.write_bytes(b"# nothing\n")
    dev = three(sam, [f"--on-target={bed}", str(bam)], tmp_path, want=om.report(om.sweep(model_records(raw), []), on_target=False), path="host")
    assert dev[0] == 0 and dev[1].count(b"\n") == 3
    # a BED start whose + 1 does not fit 64 bits
    make_bam(str(bam), 3000, seed=9)
    bed.write_bytes(b"chr1\t9223372036854775807\t9223372036854775807\n")
    three(sam, [f"--on-target={bed}", str(bam)], tmp_path, path="host")


def test_bed_errors(sam, tmp_path):
    bam, bed = tmp_path / "b.bam", tmp_path / "b.bed"
    make_bam(str(bam), 2000, seed=5)
    for text, code, msg in ((b"chr1\t5\t100\nchr9\t5\t100\n", 255, b"ERROR: Chromosome chr9 is listed in target region BED file, but is not found in BAM file.\n"),
                            (b"chr1\t5\t100\nchr1\t5\n", 255, b"ERROR: Invalid line in BED file %s:\nchr1\t5\n\n" % str(bed).encode()),      # (the line keeps its newline)
                            (b"chr1\tfive\t100\n", 101, None), (b"chr1\t5\t9223372036854775808\n", 101, None)):
        bed.write_bytes(text)
        dev = three(sam, [f"--on-target={bed}", str(bam)], tmp_path, want=b"", path=None)
        assert dev[0] == code and dev[2].startswith(ANNOUNCE)
        if msg is not None:
            assert dev[2] == ANNOUNCE + msg
    dev = three(sam, [f"--on-target={tmp_path / 'missing.bed'}", str(bam)], tmp_path, want=b"", path=None)
    assert dev[0] != 0
    # a BAM that cannot be opened is reported before the BED is read
    dev = cu.run(sam, ["statistics", f"--on-target={bed}", "missing.bam"], cwd=tmp_path)
    assert dev[0] == 255 and dev[1] == b"" and dev[2] == b"ERROR: Cannot open BAM file 'missing.bam'\n"


def test_without_the_option(sam, tmp_path):
    bam = tmp_path / "n.bam"
    recs = model_records(make_bam(str(bam), 3000, seed=12))
    want = om.report(om.sweep(recs, [[], [], []]), on_target=False)
    d = tmp_path / "run"
    d.mkdir()
    dev = cu.run(sam, ["statistics", str(bam)], cwd=d)
    host = cu.run(sam, ["statistics", str(bam)], cwd=d, env={"SEQKIT_HOST_INFLATE": "1"})
    traced = cu.run(sam, ["statistics", str(bam)], cwd=d, env={"SK_BAMFILE_TRACE": "1"})
    assert dev == host == (0, want, b"") and traced[:2] == (0, want)
    lines = [ln for ln in traced[2].split(b"\n") if ln.startswith(b"sam statistics: ")]
    assert len(lines) == 1 and lines[0].startswith(b"sam statistics: waited ") and b" ms for the device contexts, sk_bam_file_reduce " in lines[0]
    assert b"device path" not in traced[2] and b"host reader" not in traced[2]
