"""CPU: the host reader of `sam concatenate` (SEQKIT_HOST_INFLATE=1; its members deflated by zlib on the host, SEQKIT_GPU_DEFLATE=0: no
device needed) against tests/bam_concatenate_model.py: inflated stdout, stderr bytes and status; the command's error messages and usage."""
import pytest

from tests import bam_concatenate_model as m
from tests import cli_util as cu


@pytest.fixture(scope="module")
def sam(hip_lib):
    from seqkit_amd import build
    build.build_hosts()
    return cu.SAM


HOST = {"SEQKIT_HOST_INFLATE": "1", "SEQKIT_GPU_DEFLATE": "0"}


def run(sam, argv, stdin=None):
    code, out, err = cu.run(sam, ["concatenate"] + argv, stdin=stdin, env=HOST)
    mem = m.members(out) if out else []
    if out:
        assert out.endswith(m.EOF_BLOCK) and out.count(m.EOF_BLOCK) == 1                      # the EOF block, exactly once
        assert mem[-1][0] == b"" and all(0 < len(x) <= 0xFF00 for x, _ in mem[:-1])
    return code, b"".join(x for x, _ in mem), err, mem


SIZES = [700, 500, 0, 300, 1, 200, 150, 100, 80, 60, 40, 20]


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """12 files of 0 to 700 unsorted records, their reference lists different"""
    d = tmp_path_factory.mktemp("concat")
    return m.write_all(d, m.served_inputs(12, SIZES, seed=6))


@pytest.mark.parametrize("k", [2, 3, 12])
def test_host_matches_model(sam, inputs, k):
    paths, raws = inputs
    exp = m.model(raws[:k], paths[:k])
    assert exp[1:] == (b"", 0)
    code, out, err, _ = run(sam, paths[:k])
    assert (out, err, code) == exp
    names = {r[36:36 + r[12] - 1].rsplit(b".", 1)[1] for r in m.records(out)}
    assert names == {b"%d" % (b + 1) for b in range(k) if SIZES[b]}
    if k == 12:
        assert {b"1", b"9", b"10", b"12"} <= names


def test_different_reference_lists_are_served_under_the_first_header(sam, inputs):
    paths, raws = inputs
    assert m.refs_of(1) != m.refs_of(0) and m.refs_of(3) != m.refs_of(0)
    for order in ([1, 0], [3, 1, 0]):
        code, out, err, _ = run(sam, [paths[i] for i in order])
        assert (out, err, code) == m.model([raws[i] for i in order])
        assert code == 0 and out.startswith(m.out_header(raws[order[0]]))


def test_uncompressed_in_any_argument_position(sam, inputs):
    paths, raws = inputs
    p = paths[:3]
    exp = m.model(raws[:3], p)
    for argv in (["--uncompressed"] + p, [p[0], "--uncompressed", p[1], p[2]], p + ["--uncompressed"]):
        code, out, err, mem = run(sam, argv)
        assert (out, err, code) == exp and all(stored for _, stored in mem[:-1])
    code, out, err, mem = run(sam, p)
    assert (out, err, code) == exp and not all(stored for _, stored in mem[:-1])


def test_stdin_in_first_middle_and_last_place(sam, inputs):
    paths, raws = inputs
    data = open(paths[1], "rb").read()
    for at in (0, 1, 2):
        order = [0, 3]
        order.insert(at, 1)
        argv = [paths[i] if i != 1 else "-" for i in order]
        code, out, err, _ = run(sam, argv, stdin=data)
        assert (out, err, code) == m.model([raws[i] for i in order], argv)


def test_inputs_without_records(sam, inputs):
    paths, raws = inputs
    assert len(list(m.records(raws[2]))) == 0
    for order in ([2, 0], [0, 2], [0, 2, 4], [2, 4, 2], [2, 2, 2]):
        code, out, err, _ = run(sam, [paths[i] for i in order])
        assert (out, err, code) == m.model([raws[i] for i in order])
    assert out == m.out_header(raws[2])                                                       # three of them alone: the header, the EOF block


def test_a_name_too_long_with_its_suffix(sam, tmp_path):
    one = m.served_inputs(1, 40, seed=2)[0]
    two = m.served_inputs(1, 30, seed=3)[0]
    two[11] = m.rm.record(b"n" * 253, 5)
    raw1, raw2 = m.write(tmp_path / "a.bam", one), m.write(tmp_path / "b.bam", two)
    code, out, err, _ = run(sam, [str(tmp_path / "a.bam"), str(tmp_path / "b.bam")])
    assert (out, err, code) == m.model([raw1, raw2]) and (err, code) == (m.PANIC, 101)
    assert len(list(m.records(out))) == 40 + 11
    code, out, err, _ = run(sam, [str(tmp_path / "b.bam"), str(tmp_path / "a.bam")])          # 253 bytes + ".1" as well
    assert (out, err, code) == m.model([raw2, raw1]) and code == 101 and len(list(m.records(out))) == 11


def test_a_missing_file_in_third_place(sam, inputs):
    paths, raws = inputs
    argv = [paths[0], paths[1], "/nonexistent/x.bam", paths[3]]
    code, out, err, _ = run(sam, argv)
    exp = m.model([raws[0], raws[1], None, raws[3]], argv)
    assert (out, err, code) == exp and (err, code) == (b"ERROR: Cannot open BAM file '/nonexistent/x.bam'\n", 255)
    assert len(list(m.records(out))) == SIZES[0] + SIZES[1]
    argv = ["/nonexistent/x.bam", paths[0]]                                                   # in first place: nothing is written
    assert cu.run(sam, ["concatenate"] + argv, env=HOST) == (255, b"", m.open_error(argv[0]))


def test_too_few_paths_and_usage(sam, inputs):
    paths, _ = inputs
    for argv in ([paths[0]], ["--uncompressed", paths[0]], ["/nonexistent/x.bam"]):
        assert cu.run(sam, ["concatenate"] + argv, env=HOST) == (255, b"", m.TWO_ERROR)
    for argv in ([], ["--uncompressed"], ["--nonsense", paths[0], paths[1]], ["-x", paths[0], paths[1]], ["--uncompressed=1", paths[0], paths[1]],
                 ["--suffix", paths[0], paths[1]]):
        assert cu.run(sam, ["concatenate"] + argv, env=HOST) == (255, b"", m.INVALID)


def test_the_top_level_usage_does_not_list_the_command(sam):
    code, out, err = cu.run(sam, [], env=HOST)
    assert out == b"" and b"sam merge <bam_files>..." in err and b"concatenate" not in err
