"""GPU: `sam to raw|fasta|fastq <bam> <prefix>` with the mates paired on the device (SEQKIT_DEVICE_PAIRING=1): the three .gz files are
deflated and framed there too (sk_bam_file_pairs_gz) and written as they come.  Each file, read raw, is BGZF members of at most 64 KiB
that end with the one EOF block and inflate to what tests/bam_pair_model.py states; SEQKIT_GPU_DEFLATE=0 and a declined pairing write
the same streams through the writers' pool."""
import pytest

from tests import cli_util as cu
from tests.bam_out_util import zlib_members
from tests.test_gpu_bam_pairs import FORMATS, expected, mixed_records, ordered

pytestmark = pytest.mark.gpu

EXT = {"raw": "seq", "fasta": "fa", "fastq": "fq"}
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
PAIRING, DEFLATE = b"sam to pairing: ", b"sam to deflate: device"


@pytest.fixture(scope="module")
def sam(hip_lib):
    from seqkit_amd import build
    build.build_hosts()
    return cu.SAM


@pytest.fixture(scope="module")
def mixed(tmp_path_factory):
    recs = ordered(mixed_records(700, seed=31), "shuffled")
    bam = tmp_path_factory.mktemp("cli_pairs_gz") / "m.bam"
    cu.write_bam(str(bam), [("chr1", 100000)], recs)
    return bam, recs


def run_to(sam, args, d, env):
    """(status, stdout, the trace's `sam to` lines, {file: inflated bytes}); every file is checked raw"""
    d.mkdir(exist_ok=True)
    for f in d.iterdir():
        f.unlink()
    code, out, err = cu.run(sam, ["to"] + args, cwd=d, env=dict(env, SK_BAMFILE_TRACE="1"))
    said = [ln for ln in err.split(b"\n") if ln.startswith(b"sam to")]
    files = {}
    for f in sorted(d.iterdir()):
        if f.name.endswith(".gz"):
            raw = f.read_bytes()
            mem = zlib_members(raw)                                            # (every member at most 64 KiB, CRC and ISIZE right)
            assert raw.endswith(EOF_BLOCK) and raw.count(EOF_BLOCK) == 1 and mem[-1] == b"" and all(mem[:-1])
            files[f.name] = b"".join(mem)
    return code, out, said, files


def names(fmt, exp):
    return {"o_1.%s.gz" % EXT[fmt]: exp[0], "o_2.%s.gz" % EXT[fmt]: exp[1], "o.%s.gz" % EXT[fmt]: exp[2]}


@pytest.fixture(scope="module")
def want(mixed):
    """{format: the three files the model states}: what every path below must write, so the paths' files are identical"""
    return {fmt: names(fmt, expected(mixed[1], fmt, False)) for fmt in FORMATS}


DEV = {"SEQKIT_DEVICE_PAIRING": "1"}
WINDOWS = ({}, {"SK_BAMFILE_WINDOW": "4096"})


@pytest.mark.parametrize("window", [0, 1])
@pytest.mark.parametrize("fmt", FORMATS)
def test_sam_to_files_deflated_on_the_device(sam, mixed, want, tmp_path, fmt, window):
    code, out, said, files = run_to(sam, [fmt, str(mixed[0]), "o"], tmp_path / "dev", dict(DEV, **WINDOWS[window]))
    assert code == 0 and out == b"" and files == want[fmt]
    assert PAIRING + b"device" in said and DEFLATE in said


@pytest.mark.parametrize("window", [0, 1])
@pytest.mark.parametrize("fmt", FORMATS)
def test_sam_to_files_through_the_pool_on_request(sam, mixed, want, tmp_path, fmt, window):
    """SEQKIT_GPU_DEFLATE=0: the texts come back as they are and go through the writers' pool: no line, the same streams"""
    code, out, said, files = run_to(sam, [fmt, str(mixed[0]), "o"], tmp_path / "pool", dict(DEV, SEQKIT_GPU_DEFLATE="0", **WINDOWS[window]))
    assert code == 0 and out == b"" and files == want[fmt]
    assert PAIRING + b"device" in said and DEFLATE not in said


@pytest.mark.parametrize("fmt", FORMATS)
def test_sam_to_files_when_the_pairing_declines(sam, mixed, want, tmp_path, fmt):
    """two names under one key: the host pairs, the pool deflates, nothing was written before"""
    code, out, said, files = run_to(sam, [fmt, str(mixed[0]), "o"], tmp_path / "host", dict(DEV, SK_PAIR_KEY_BITS="4"))
    assert code == 0 and out == b"" and files == want[fmt]
    assert PAIRING + b"host" in said and PAIRING + b"device" not in said and DEFLATE not in said


def test_sam_to_files_without_records(sam, tmp_path):
    bam = tmp_path / "empty.bam"
    cu.write_bam(str(bam), [("chr1", 100000)], [])
    code, out, said, files = run_to(sam, ["fastq", str(bam), "o"], tmp_path / "e", {"SEQKIT_DEVICE_PAIRING": "1"})
    assert code == 0 and out == b"" and files == names("fastq", (b"", b"", b""))
    for f in (tmp_path / "e").iterdir():
        assert f.read_bytes() == EOF_BLOCK


def test_sam_to_interleaved_is_never_deflated_on_the_device(sam, mixed, tmp_path):
    bam, recs = mixed
    code, out, said, files = run_to(sam, ["interleaved", "fastq", str(bam)], tmp_path / "i", {"SEQKIT_DEVICE_PAIRING": "1"})
    assert code == 0 and out == expected(recs, "fastq", True)[0] and files == {}
    assert PAIRING + b"device" in said and DEFLATE not in said
