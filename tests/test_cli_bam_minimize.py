"""GPU: `sam minimize` on the device path (sk_bam_file_minimize), the host reader (SEQKIT_HOST_INFLATE=1) and stdin: the same inflated
stdout, equal to tests/bam_minimize_model.py, and the reference's statuses."""
import pytest

from tests import bam_minimize_model as m
from tests import bam_out_util as bu
from tests.bam_out_util import sam  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bam(tmp_path_factory):
    path = tmp_path_factory.mktemp("minimize") / "in.bam"
    return path, m.write(path, m.served_records())


def three(sam, path, extra, expect_path="device path", env=None):
    return bu.three(sam, m, ["minimize"], path, extra, expect_path, env)


@pytest.mark.parametrize("combo,fill", [(c, None) for c in m.COMBOS] + [("tags+base-qualities", 0), ("all", 30)])
@pytest.mark.parametrize("uncompressed", [False, True])
def test_three_paths_match_model(sam, bam, combo, fill, uncompressed):
    path, raw = bam
    code, out, err, runs = three(sam, path, (["--uncompressed"] if uncompressed else []) + m.args(combo, fill))
    exp, stop = m.model(raw, combo, 255 if fill is None else fill)
    assert stop is None and code == 0 and out == exp and err == b""
    if uncompressed:
        for _, o, _ in runs:
            assert all(stored for _, stored in m.members(o)[:-1])


def test_hash_collision_falls_back_to_the_host_reader(sam, bam):
    """SK_MINIMIZE_KEY_BITS=8 makes the 25 000 names' hashes collide: the device declines and the host reader serves the file"""
    path, raw = bam
    code, out, err, runs = three(sam, path, ["--read-ids"], expect_path="host reader", env={"SK_MINIMIZE_KEY_BITS": "8"})
    assert code == 0 and out == m.model(raw, "read-ids")[0]
    assert b"sk_bam_file_minimize: declined (bits 0x40)" in runs[0][2]


@pytest.mark.parametrize("combo", list(m.COMBOS))
def test_cigar_op_9_panics_after_the_earlier_records(sam, tmp_path, combo):
    path = tmp_path / "in.bam"
    recs = list(m.served_records(200, seed=4))
    recs[120] = m.record(b"stop", 21, cigar_op=9)
    raw = m.write(path, recs)
    exp, c = m.model(raw, combo)
    assert c == 101
    code, out, err, runs = three(sam, path, m.args(combo), expect_path="host reader")
    assert code == 101 and out == exp and b"panicked" in err
    assert len(list(m.records(out))) == 120
