"""GPU: `sam to [interleaved] raw|fasta|fastq` over its paths — the default, the mates paired on the device (SEQKIT_DEVICE_PAIRING=1,
sk_bam_file_pairs), paired on the host over the device's texts (SEQKIT_HOST_PAIRING=1, sk_bam_file_reads) and the record-at-a-time
reader (SEQKIT_HOST_INFLATE=1): the same decompressed outputs, stderr and status, and the outputs tests/bam_pair_model.py states."""
import pytest

from tests import cli_util as cu
from tests.test_gpu_bam_pairs import FORMATS, expected, mixed_records, ordered, rec, F1, F2

pytestmark = pytest.mark.gpu

EXT = {"raw": "seq", "fasta": "fa", "fastq": "fq"}
PATHS = (("default", {}), ("device pairing", {"SEQKIT_DEVICE_PAIRING": "1"}), ("host pairing", {"SEQKIT_HOST_PAIRING": "1"}),
         ("host reader", {"SEQKIT_HOST_INFLATE": "1"}))
DEVICE_SERVES = ("any", "device", "host", None)                         # who pairs the mates on each path (the default: either)


@pytest.fixture(scope="module")
def sam(hip_lib):
    from seqkit_amd import build
    build.build_hosts()
    return cu.SAM


def run_paths(sam, args, tmp_path, env=None, pairing=DEVICE_SERVES):
    """(status, stdout, stderr without the trace lines, files) of the four paths, checked equal; the trace says which path paired the
    mates"""
    runs = []
    for k, ((_, extra), how) in enumerate(zip(PATHS, pairing)):
        d = tmp_path / ("path%d" % k)
        d.mkdir(exist_ok=True)
        for f in d.iterdir():
            f.unlink()
        code, out, err = cu.run(sam, args, cwd=d, env=dict(env or {}, SK_BAMFILE_TRACE="1", **extra))
        lines = err.split(b"\n")
        said = [ln for ln in lines if ln.startswith(b"sam to pairing: ")]
        if how == "any":
            assert said in ([b"sam to pairing: device"], [b"sam to pairing: host"]), err[-400:]
        else:
            assert said == ([b"sam to pairing: " + how.encode()] if how else []), err[-400:]
        assert (b"sam to: host reader" in lines) == (how is None)
        quiet = b"\n".join(ln for ln in lines if not ln.startswith(b"sam to") and not ln.startswith(b"sk_bam"))
        runs.append((code, out, quiet, cu.gunzip_dir(d)))
    assert runs[0] == runs[1] == runs[2] == runs[3], [(r[0], r[2][-200:]) for r in runs]
    return runs[0]


def check_all_modes(sam, bam, recs, tmp_path, env=None, pairing=DEVICE_SERVES, formats=FORMATS):
    for fmt in formats:
        code, out, err, files = run_paths(sam, ["to", fmt, str(bam), "o"], tmp_path, env, pairing)
        exp = expected(recs, fmt, False)
        assert code == 0 and out == b"" and err == b""
        assert files == {"o_1.%s.gz" % EXT[fmt]: exp[0], "o_2.%s.gz" % EXT[fmt]: exp[1], "o.%s.gz" % EXT[fmt]: exp[2]}
        code, out, err, files = run_paths(sam, ["to", "interleaved", fmt, str(bam)], tmp_path, env, pairing)
        assert code == 0 and out == expected(recs, fmt, True)[0] and files == {}


@pytest.mark.parametrize("order", ["name", "position", "shuffled"])
def test_sam_to_paths(sam, tmp_path, order):
    recs = ordered(mixed_records(700, seed=21), order)
    bam = tmp_path / "m.bam"
    cu.write_bam(str(bam), [("chr1", 100000)], recs)
    check_all_modes(sam, bam, recs, tmp_path, formats=FORMATS if order == "shuffled" else ("fastq",))


def test_sam_to_paths_small_windows(sam, tmp_path):
    recs = ordered(mixed_records(400, seed=22), "shuffled")
    bam = tmp_path / "w.bam"
    cu.write_bam(str(bam), [("chr1", 100000)], recs)
    check_all_modes(sam, bam, recs, tmp_path, env={"SK_BAMFILE_WINDOW": "4096"}, formats=("fasta",))


def test_sam_to_one_name_on_every_record(sam, tmp_path):
    recs = [rec("same", (F1, F1, F2)[k % 3], 2 + k % 5, k) for k in range(3000)]
    bam = tmp_path / "s.bam"
    cu.write_bam(str(bam), [("chr1", 100000)], recs)
    check_all_modes(sam, bam, recs, tmp_path, formats=("raw",))


def test_sam_to_key_collision_falls_back_to_the_host_pairing(sam, tmp_path):
    """with the key cut to 4 bits the device pairing declines before it writes anything; the command pairs on the host and succeeds
    with the same outputs"""
    recs = ordered(mixed_records(300, seed=23), "shuffled")
    bam = tmp_path / "c.bam"
    cu.write_bam(str(bam), [("chr1", 100000)], recs)
    check_all_modes(sam, bam, recs, tmp_path, env={"SK_PAIR_KEY_BITS": "4"}, pairing=("host", "host", "host", None), formats=("fastq",))
