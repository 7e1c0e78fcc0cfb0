"""GPU: `sam to [interleaved] raw|fasta|fastq` served from the file by the device (sk_bam_file_reads) against the same commands on the
host reader (SEQKIT_HOST_INFLATE=1) and the oracle command line: same stdout, stderr, exit code and decompressed .gz files.  The trace
line says which path served the file; the files the device path declines end on the host reader and still match."""
import pytest

from tests import cli_util as cu
from tests.test_cli_gpu import reads_bam

pytestmark = pytest.mark.gpu

BASE = dict(tid=0, mtid=0, pos=1, mpos=1, tlen=0)


@pytest.fixture(scope="module")
def bins(hip_lib, oracle):
    from seqkit_amd import build
    build.build_hosts()
    return {"sam": (cu.SAM, oracle.SAM_BIN)}


def three(bins, args, tmp_path, path="device", env=None, same_stderr=True, oracle=True):
    """the device path (with its trace line), the host reader and the oracle: the same output and files; returns the device run.
    oracle=False: where this build's host reader stops on purpose (reads over 65 532 bases), the device path matches the host reader."""
    runs = []
    for k, (binary, extra) in enumerate(((bins["sam"][0], {}), (bins["sam"][0], {"SEQKIT_HOST_INFLATE": "1"}),
                                         (bins["sam"][1] if oracle else bins["sam"][0], {} if oracle else {"SEQKIT_HOST_INFLATE": "1"}),
                                         (bins["sam"][0], {"SK_BAMFILE_TRACE": "1"}))):
        d = tmp_path / f"run{k}"
        d.mkdir(exist_ok=True)
        r = cu.run(binary, args, cwd=d, env=dict(env or {}, **extra))
        runs.append((r, cu.gunzip_dir(d)))
    (dev, fd), (host, fh), (orc, fo), (traced, ft) = runs
    assert dev[0] == host[0] == orc[0] == traced[0], (dev[0], host[0], orc[0], dev[2][-300:], orc[2][-300:])
    assert dev[1] == host[1] == orc[1] == traced[1]
    assert fd == fh == fo == ft
    if same_stderr:
        assert dev[2] == host[2] == orc[2]
    else:
        assert dev[2] == host[2]
    lines = [ln for ln in traced[2].split(b"\n") if ln.startswith(b"sam to: ")]
    assert len(lines) == 1, traced[2][-500:]
    if path == "device":
        assert lines[0].startswith(b"sam to: device path, "), lines
    else:
        assert lines[0] == b"sam to: host reader", lines
    return dev, fd, lines[0]


def all_modes(bins, bam, tmp_path, path="device", env=None, same_stderr=True):
    for fmt in ("raw", "fasta", "fastq"):
        three(bins, ["to", fmt, str(bam), "out"], tmp_path, path, env, same_stderr)
        three(bins, ["to", "interleaved", fmt, str(bam)], tmp_path, path, env, same_stderr)


@pytest.mark.parametrize("sort", ["name", "shuffled"])
def test_sam_to_device_path(bins, tmp_path, sort):
    bam = tmp_path / "r.bam"
    recs = reads_bam(str(bam), 3000, seed=61, sort=sort)
    dev, files, line = three(bins, ["to", "fastq", str(bam), "out"], tmp_path)
    assert line == b"sam to: device path, %d records" % len(recs)
    assert files["out_1.fq.gz"].count(b"\n") == files["out_2.fq.gz"].count(b"\n") > 4000 and len(files["out.fq.gz"]) > 100
    all_modes(bins, bam, tmp_path)


def test_sam_to_windows_cross_pairs(bins, tmp_path):
    bam = tmp_path / "w.bam"
    reads_bam(str(bam), 3000, seed=62, sort="shuffled")
    all_modes(bins, bam, tmp_path, env={"SK_BAMFILE_WINDOW": "8192"})      # dozens of windows: mates and leftovers cross them


def test_sam_to_pending_semantics(bins, tmp_path):
    bam = tmp_path / "p.bam"
    r = lambda name, flag, codes: dict(BASE, flag=flag, name=name, codes=codes, qual=[30] * len(codes))
    recs = [
        r("dup", 1 | 64, [1]), r("dup", 1 | 64, [2]),                       # same mate flag twice: the second replaces the first
        r("three", 1 | 64, [1]), r("three", 1 | 128, [2]), r("three", 1 | 128, [4]),    # a name seen three times
        r("re", 1 | 64, [1]), r("x1", 1 | 64, [8]), r("re", 1 | 128, [2]), r("re", 1 | 64, [4]),   # removed, then inserted again: a new order
        r("neither", 1, [1, 2]), r("neither", 1 | 16, [4]),                 # paired, flagged neither first nor last: dropped
        r("single", 0, [1, 1]), r("single2", 16, [2, 8]),                   # unpaired: out_single, or nowhere when interleaved
        r("dup", 1 | 128, [8]), r("o2", 1 | 128, [1, 2, 4]), r("x2", 1 | 64, [2]),
    ]
    cu.write_bam(str(bam), [("chr1", 1000)], recs)
    all_modes(bins, bam, tmp_path)
    all_modes(bins, bam, tmp_path, env={"SK_BAMFILE_WINDOW": "256"})
    _, files, _ = three(bins, ["to", "raw", str(bam), "o"], tmp_path)
    assert files["o_1.seq.gz"] == b"A\nA\nC\n" and files["o_2.seq.gz"] == b"C\nC\nT\n"
    assert files["o.seq.gz"] == b"AA\nAG\nT\nG\nC\nG\nACG\n"             # reads_1 leftovers in insertion order, then reads_2


def test_sam_to_declined_files_end_on_the_host_reader(bins, tmp_path):
    bam = tmp_path / "d.bam"
    ok = [dict(BASE, flag=1 | 64, name="ok", codes=[1], qual=[30]), dict(BASE, flag=1 | 128, name="ok", codes=[2], qual=[30])]
    cu.write_bam(str(bam), [("chr1", 1000)], ok + [dict(BASE, flag=0, name=b"bad\xff", codes=[1], qual=[30])])
    for fmt in ("raw", "fasta", "fastq"):                                          # the panic: exit 101 after what the records before wrote
        dev, _, _ = three(bins, ["to", "interleaved", fmt, str(bam)], tmp_path, path="host", same_stderr=False)
        assert dev[0] == 101
        three(bins, ["to", fmt, str(bam), "o"], tmp_path, path="host", same_stderr=False, oracle=False)
    cu.write_bam(str(bam), [("chr1", 1000)], ok + [dict(BASE, flag=0, name="hi", codes=[1, 2, 4], qual=[95, 30, 30])])
    three(bins, ["to", "fastq", str(bam), "o"], tmp_path, path="host", same_stderr=False)
    three(bins, ["to", "interleaved", "fastq", str(bam)], tmp_path, path="host", same_stderr=False)
    for fmt in ("raw", "fasta"):                                                   # q = 95 declines fastq only
        three(bins, ["to", fmt, str(bam), "o"], tmp_path)
        three(bins, ["to", "interleaved", fmt, str(bam)], tmp_path)
    cu.write_bam(str(bam), [("chr1", 1000)], ok + [dict(BASE, flag=0, name="long", codes=[1] * 65533, qual=[30] * 65533)])
    for args in (["to", "interleaved", "raw", str(bam)], ["to", "fastq", str(bam), "o"]):
        dev, _, _ = three(bins, args, tmp_path, path="host", oracle=False)
        assert dev[0] != 0
    # stdin keeps the host reader
    reads_bam(str(bam), 200, seed=5)
    d = tmp_path / "stdin"
    d.mkdir()
    a = cu.run(bins["sam"][0], ["to", "interleaved", "fastq", "-"], cwd=d, stdin=bam.read_bytes(), env={"SK_BAMFILE_TRACE": "1"})
    o = cu.run(bins["sam"][1], ["to", "interleaved", "fastq", "-"], cwd=d, stdin=bam.read_bytes())
    assert a[0] == o[0] and a[1] == o[1] and b"sam to: host reader" in a[2]
