"""GPU: `sam merge` on the device path (sk_bam_file_merge), the host reader (SEQKIT_HOST_INFLATE=1) and with "-" for one input: the same
inflated stdout, stderr and status, equal to tests/bam_merge_model.py; every decline of the device ends in the host reader."""
import struct

import pytest

from tests import bam_merge_model as m
from tests import bam_out_util as bu
from tests.bam_out_util import sam  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

WHO = b"sam merge: "


def write_all(d, files, **kw):
    paths = [d / ("in%d.bam" % (i + 1)) for i in range(len(files))]
    return [str(p) for p in paths], [m.write(p, recs, **kw) for p, recs in zip(paths, files)]


def three(sam, paths, extra=(), expect_path="device path", env=None, stdin_at=1):
    """device path, host reader, "-" for input stdin_at: (code, inflated stdout, stderr without the trace's lines) of the three, checked
    equal, and the runs; the trace names the path.  (bam_out_util.three takes one path.)"""
    argv = ["merge"] + list(extra)
    dashed = [p if i != stdin_at else "-" for i, p in enumerate(paths)]
    runs = []
    for e, args, stdin in (({"SK_BAMFILE_TRACE": "1"}, argv + paths, None),
                           ({"SK_BAMFILE_TRACE": "1", "SEQKIT_HOST_INFLATE": "1"}, argv + paths, None),
                           ({"SK_BAMFILE_TRACE": "1"}, argv + dashed, open(paths[stdin_at], "rb").read())):
        runs.append(bu.cu.run(sam, args, stdin=stdin, env=dict(e, **(env or {}))))
    traces = [[ln for ln in err.split(b"\n") if ln.startswith(WHO)] for _, _, err in runs]
    assert traces[0] and traces[0][0].startswith(WHO + expect_path.encode()), traces[0]
    assert traces[1] == [WHO + b"host reader"] and traces[2] == traces[1]
    assert runs[0][0] == runs[1][0] == runs[2][0]
    outs = [bu.inflated(m, out) if out else b"" for _, out, _ in runs]
    assert outs[0] == outs[1] == outs[2]
    for _, out, _ in runs:
        assert out == b"" or out.endswith(m.EOF_BLOCK)
    strip = [b"".join(ln + b"\n" for ln in err.split(b"\n")[:-1] if not ln.startswith(WHO) and not ln.startswith(b"sk_bam")) for _, _, err in runs]
    assert strip[0] == strip[1] and strip[2] == strip[0].replace(paths[stdin_at].encode(), b"-")
    return runs[0][0], outs[0], strip[0], runs


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("merge_cli")
    return write_all(d, m.served_inputs(12, [2500, 1200, 0, 300, 1, 200, 150, 100, 80, 60, 40, 20], seed=6), piece=0x3000)


@pytest.mark.parametrize("extra", [(), ("--suffix",), ("--uncompressed", "--suffix")])
@pytest.mark.parametrize("k", [2, 12])
def test_three_paths_match_model(sam, inputs, k, extra):
    paths, raws = inputs
    code, out, err, runs = three(sam, paths[:k], extra, stdin_at=k - 1)
    assert (out, err, code) == m.model(raws[:k], "--suffix" in extra) and code == 0
    assert b"sam merge: device path, %d records" % sum(len(list(m.records(r))) for r in raws[:k]) in runs[0][2]
    if "--uncompressed" in extra:
        assert all(stored for _, stored in m.members(runs[0][1])[:-1])


def test_small_windows_on_the_device_path(sam, inputs):
    paths, raws = inputs
    code, out, err, _ = three(sam, paths[:3], ("--suffix",), env={"SK_BAMFILE_WINDOW": "4096"})
    assert (out, err, code) == m.model(raws[:3], True)


def test_declines_end_in_the_host_reader(sam, inputs, tmp_path):
    paths, raws = inputs
    files = [list(m.records(r)) for r in raws[:2]]
    # an unsorted input: the loop of the model all the same
    bad = files[1][600:] + files[1][:600]
    p = tmp_path / "unsorted.bam"
    raw = m.write(p, bad)
    code, out, err, runs = three(sam, [paths[0], str(p)], expect_path="host reader")
    assert (out, err, code) == m.model([raws[0], raw], False) and b"sk_bam_file_merge: declined (bits 0x2)" in runs[0][2]
    # a name too long with its suffix: 101 behind the earlier records; without --suffix the device serves it
    long = list(files[1])
    long[50] = m.rm.record(b"n" * 253, 10, tid=m.key(long[50])[0], pos=m.key(long[50])[1])
    p = tmp_path / "long.bam"
    raw = m.write(p, long)
    code, out, err, runs = three(sam, [paths[0], str(p)], ("--suffix",), expect_path="host reader")
    exp = m.model([raws[0], raw], True)
    assert (out, err, code) == exp and code == 101 and len(out) > len(m.out_header(raws[0])) and b"sk_bam_file_merge: declined (bits 0x1)" in runs[0][2]
    code, out, err, _ = three(sam, [paths[0], str(p)])
    assert (out, err, code) == m.model([raws[0], raw], False) and code == 0
    # other reference names: the SQ error, nothing on stdout
    p = tmp_path / "names.bam"
    raw = m.write(p, files[1], refs=m.rm.REFS[:2] + [(b"chrX", 16569)])
    argv = [paths[0], paths[3], str(p)]
    code, out, err, runs = three(sam, argv, expect_path="host reader", stdin_at=1)
    assert (out, err, code) == (b"", m.sq_error(argv[0], argv[2]), 255) and b"sk_bam_file_merge: declined (bits 0x4)" in runs[0][2]
    # an invalid record: the reader's message behind the records before it
    inv = list(files[1])
    b = bytearray(inv[300])
    struct.pack_into("<i", b, 20, 4000)
    inv[300] = bytes(b)
    p = tmp_path / "invalid.bam"
    m.write(p, inv)
    code, out, err, runs = three(sam, [paths[0], str(p)], expect_path="host reader")
    assert code == 255 and err == b"ERROR: Invalid BAM record.\n" and b"sk_bam_file_merge: declined (bits 0x8)" in runs[0][2]
    assert out.startswith(m.out_header(raws[0])) and len(list(m.records(out))) >= 300
