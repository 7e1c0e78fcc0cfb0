"""GPU: `sam fragments` and `sam count` served from the file by the device (sk_bam_file_columns and the kernels behind it) against
the same commands on the host reader (SEQKIT_HOST_INFLATE=1) and the oracle command line: same stdout, stderr and exit code.  The
trace line says which path served the file; irregular files fall back to the host reader and still match."""
import numpy as np
import pytest

from tests import cli_util as cu
from tests.test_cli_gpu import make_bam, sorted_bam

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bins(hip_lib, oracle):
    from seqkit_amd import build
    build.build_hosts()
    return {"sam": (cu.SAM, oracle.SAM_BIN)}


def three(bins, args, tmp_path, stdin=None, path="device"):
    """the device path (with its trace line), the host reader and the oracle: the same output; returns the device run and its trace"""
    d = tmp_path / "run"
    d.mkdir(exist_ok=True)
    dev = cu.run(bins["sam"][0], args, cwd=d, stdin=stdin)
    host = cu.run(bins["sam"][0], args, cwd=d, stdin=stdin, env={"SEQKIT_HOST_INFLATE": "1"})
    orc = cu.run(bins["sam"][1], args, cwd=d, stdin=stdin)
    assert dev[0] == host[0] == orc[0], (dev[0], host[0], orc[0], dev[2][-300:], orc[2][-300:])
    assert dev[1] == host[1] == orc[1]
    assert dev[2] == host[2] == orc[2]
    traced = cu.run(bins["sam"][0], args, cwd=d, stdin=stdin, env={"SK_BAMFILE_TRACE": "1"})
    assert traced[0] == dev[0] and traced[1] == dev[1]
    cmd = b"sam " + args[0].encode() + b": "
    lines = [ln for ln in traced[2].split(b"\n") if ln.startswith(cmd)]
    assert len(lines) == 1, traced[2][-500:]
    if path == "device":
        assert lines[0].startswith(cmd + b"device path, "), lines
    else:
        assert lines[0] == cmd + b"host reader", lines
    return dev, lines[0]


def test_fragments_device_path(bins, tmp_path):
    bam = tmp_path / "f.bam"
    recs = make_bam(str(bam), 30000, seed=15)
    dev, line = three(bins, ["fragments", str(bam)], tmp_path)
    assert line.endswith(b", %d records" % len(recs))
    assert dev[0] == 0 and dev[1].count(b"\n") > 100
    for extra in (["--min-size=150", "--max-size", "200"], ["--max-size=-1"], ["--min-size=0", "--max-size=0"], ["--max-size=3000000000"],
                  ["--min-size=-5", "--max-size=100"]):
        three(bins, ["fragments"] + extra + [str(bam)], tmp_path)


def test_fragments_edge_values(bins, tmp_path):
    bam = tmp_path / "e.bam"
    fwd = 0x1 | 0x20 | 0x40
    recs = [dict(tid=0, mtid=0, flag=fwd, tlen=-(1 << 31), pos=(1 << 31) - 1, mpos=0), dict(tid=1, mtid=1, flag=fwd, tlen=100, pos=-1, mpos=0),
            dict(tid=2, mtid=2, flag=fwd, tlen=5, pos=7, mpos=0)] * 50
    cu.write_bam(str(bam), [("chr1", 10), ("a" * 2000, 10), ("x\x01y", 10)], recs)
    dev, _ = three(bins, ["fragments", "--max-size=3000000000", str(bam)], tmp_path)
    assert dev[1].count(b"\n") == 150
    cu.write_bam(str(bam), [("chr1", 10)], [])
    three(bins, ["fragments", str(bam)], tmp_path)


def count_bed(tmp_path, n=400, seed=42):
    rng = np.random.default_rng(seed)
    lines = [b"# comment line\n"]
    for i in range(n):
        c = [b"chr1", b"chr2", b"chrM", b"chrUn"][int(rng.integers(0, 4))]
        st = int(rng.integers(0, 500_000))
        ln = int(rng.choice([0, 1, 100, 1000, 50000]))
        lines.append(c + b"\t%d\t%d\n" % (st, st + ln))
    bed = tmp_path / "r.bed"
    bed.write_bytes(b"".join(lines))
    return bed


def test_count_device_path(bins, tmp_path):
    bam = tmp_path / "s.bam"
    recs = sorted_bam(str(bam), 30000, seed=41)
    bed = count_bed(tmp_path)
    dev, line = three(bins, ["count", str(bam), str(bed)], tmp_path)
    assert line.endswith(b", %d records" % len(recs))
    assert sum(int(x) for x in dev[1].split()) > 1000
    for extra in (["--single-end"], ["--center"], ["--single-end", "--center"], ["--min-mapq=30"], ["--max-frag-len", "200"],
                  ["--single-end", "--center", "--min-mapq", "20", "--max-frag-len=50"], ["--max-frag-len=0"], ["--min-mapq=255"]):
        three(bins, ["count"] + extra + [str(bam), str(bed)], tmp_path)


def test_fallbacks(bins, tmp_path):
    bed = count_bed(tmp_path, n=50)
    bam = tmp_path / "u.bam"
    # an unsorted file (count): the host reader reports it
    recs = sorted_bam(str(bam), 5000, seed=3)
    passing = [i for i, r in enumerate(recs) if not (r["flag"] & (0x4 | 0x400 | 0x100 | 0x800))]
    assert recs[passing[-1]]["tid"] == recs[passing[-2]]["tid"]
    recs[passing[-1]]["pos"] = recs[passing[-2]]["pos"] - 1
    cu.write_bam(str(bam), [("chr1", 1_000_000), ("chr2", 900_000), ("chrM", 16_000)], recs)
    dev, _ = three(bins, ["count", str(bam), str(bed)], tmp_path, path="host")
    assert dev[0] == 255 and b"not coordinate sorted" in dev[2]
    # a passing record whose tid has no name (count), and a kept record whose tid has none (fragments)
    recs = sorted_bam(str(bam), 5000, seed=4)
    i = next(i for i, r in enumerate(recs) if r["flag"] == 99 and i > 2000)
    recs[i]["tid"] = recs[i]["mtid"] = 3
    recs[i]["tlen"] = 100
    for r in recs[i + 1:]:                                                  # (sorted behind it: only the tid is wrong)
        r["tid"] = 3
    cu.write_bam(str(bam), [("chr1", 1_000_000), ("chr2", 900_000), ("chrM", 16_000)], recs)
    dev, _ = three(bins, ["count", str(bam), str(bed)], tmp_path, path="host")
    assert dev[0] == 101
    recs = make_bam(str(bam), 3000, seed=8)
    j = next(k for k, r in enumerate(recs) if (r["flag"] & 0xF3D) == 0x21 and r["tid"] == r["mtid"] and abs(r["tlen"]) <= 5000 and k > 100)
    recs[j]["tid"] = recs[j]["mtid"] = 5
    cu.write_bam(str(bam), [("chr1", 1_000_000), ("chr2", 900_000), ("chrM", 16_000)], recs)
    dev, _ = three(bins, ["fragments", str(bam)], tmp_path, path="host")
    assert dev[0] == 101 and dev[1].count(b"\n") > 5
    # a truncated file
    make_bam(str(bam), 3000, seed=19, truncate=30000)
    three(bins, ["fragments", str(bam)], tmp_path, path="host")
    sorted_bam(str(bam), 3000, seed=19, truncate=30000)
    three(bins, ["count", str(bam), str(bed)], tmp_path, path="host")


def test_fallback_stdin_and_bad_utf8(bins, tmp_path):
    bed = count_bed(tmp_path, n=50)
    bam = tmp_path / "s.bam"
    sorted_bam(str(bam), 3000, seed=6)
    three(bins, ["count", "-", str(bed)], tmp_path, stdin=bam.read_bytes(), path="host")
    make_bam(str(bam), 3000, seed=6)
    three(bins, ["fragments", "-"], tmp_path, stdin=bam.read_bytes(), path="host")
    # a reference name that is not UTF-8: write the header by hand
    from tests import bam_spec
    sorted_bam(str(bam), 3000, seed=7)
    raw = bytearray(b"".join(bam_spec.bgzf_blocks(bam.read_bytes())))
    k = raw.index(b"chrM\0")
    raw[k:k + 4] = b"ch\xffM"
    with open(bam, "wb") as f:
        for i in range(0, len(raw), 60000):
            f.write(cu.bgzf_block(bytes(raw[i:i + 60000])))
        f.write(cu.bgzf_block(b""))
    dev, _ = three(bins, ["count", str(bam), str(bed)], tmp_path, path="host")
    assert dev[0] == 101
    # (fragments writes names verbatim: the device path serves that file)
    three(bins, ["fragments", str(bam)], tmp_path)
