"""GPU: `sam subsample` on the device path (sk_bam_file_subsample), the host reader (SEQKIT_HOST_INFLATE=1) and stdin: the same inflated
stdout and the same stderr, equal to tests/bam_subsample_model.py, and the reference's statuses."""
import pytest

from tests import bam_subsample_model as m
from tests import bam_out_util as bu
from tests.bam_out_util import sam  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bam(tmp_path_factory):
    path = tmp_path_factory.mktemp("subsample") / "in.bam"
    return path, m.write(path, m.served_records())


WHO = b"sam subsample: "


def three(sam, path, seed, text, expect_path="device path", env=None):
    """device path, host reader, stdin: (code, inflated stdout, stderr without the trace's lines) of the three, checked equal, and the
    runs; the trace names the path.  (bam_out_util.three puts the file last; here the fraction follows it, and stderr is compared.)"""
    argv = ["subsample", "--seed=%d" % seed]
    runs = []
    for e, args, stdin in (({"SK_BAMFILE_TRACE": "1"}, argv + [str(path), text], None),
                           ({"SK_BAMFILE_TRACE": "1", "SEQKIT_HOST_INFLATE": "1"}, argv + [str(path), text], None),
                           ({"SK_BAMFILE_TRACE": "1"}, argv + ["-", text], open(path, "rb").read())):
        runs.append(bu.cu.run(sam, args, stdin=stdin, env=dict(e, **(env or {}))))
    traces = [[ln for ln in err.split(b"\n") if ln.startswith(WHO)] for _, _, err in runs]
    assert traces[0] and traces[0][0].startswith(WHO + expect_path.encode()), traces[0]
    assert traces[1] == [WHO + b"host reader"] and traces[2] == traces[1]
    assert runs[0][0] == runs[1][0] == runs[2][0]
    for _, out, _ in runs:
        assert out.endswith(m.EOF_BLOCK)
    outs = [bu.inflated(m, out) for _, out, _ in runs]
    assert outs[0] == outs[1] == outs[2]
    strip = [b"".join(ln + b"\n" for ln in err.split(b"\n")[:-1] if not ln.startswith(WHO) and not ln.startswith(b"sk_bam")) for _, _, err in runs]
    assert strip[0] == strip[1] == strip[2]
    return runs[0][0], outs[0], strip[0], runs


@pytest.mark.parametrize("text,seed", [("0.5", 0), ("0.5", 12345), ("0.25", (1 << 64) - 1), ("1", 1), ("0", 1)])
def test_three_paths_match_model(sam, bam, text, seed):
    path, raw = bam
    code, out, err, runs = three(sam, path, seed, text)
    exp_out, exp_err, exp_code, kept, _ = m.model(raw, seed, m.parse_fraction(text))
    assert (code, out, err) == (exp_code, exp_out, exp_err) and code == 0
    assert b"sam subsample: device path, %d records" % kept in runs[0][2]


def test_small_windows_on_the_device_path(sam, bam):
    path, raw = bam
    code, out, err, runs = three(sam, path, 3, "0.5", env={"SK_BAMFILE_WINDOW": "4096"})
    assert (code, out, err) == (0,) + m.model(raw, 3, m.parse_fraction("0.5"))[:2]


def test_hash_collision_falls_back_to_the_host_reader(sam, bam):
    """SK_SUBSAMPLE_KEY_BITS=8 makes the names' hashes collide: the device declines and the host reader serves the file"""
    path, raw = bam
    code, out, err, runs = three(sam, path, 4, "0.5", expect_path="host reader", env={"SK_SUBSAMPLE_KEY_BITS": "8"})
    assert (code, out, err) == (0,) + m.model(raw, 4, m.parse_fraction("0.5"))[:2]
    assert b"sk_bam_file_subsample: declined (bits 0x40)" in runs[0][2]


def test_unpaired_record_ends_the_command_after_the_earlier_records(sam, tmp_path):
    path = tmp_path / "in.bam"
    recs = list(m.served_records(200, seed=4))
    recs[120] = m.rm.record(b"single", 21, flag=0x10)
    raw = m.write(path, recs)
    exp_out, exp_err, exp_code, kept, _ = m.model(raw, 2, m.parse_fraction("0.5"))
    code, out, err, runs = three(sam, path, 2, "0.5", expect_path="host reader")
    assert exp_code == code == 255 and out == exp_out and err == exp_err
    assert len(list(m.records(out))) == kept
    assert b"sk_bam_file_subsample: declined (bits 0x1)" in runs[0][2]
