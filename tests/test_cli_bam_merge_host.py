"""CPU: the host reader of `sam merge` (SEQKIT_HOST_INFLATE=1; its members deflated by zlib on the host, SEQKIT_GPU_DEFLATE=0: no device
needed) against tests/bam_merge_model.py: inflated stdout, stderr bytes and status; the command's error messages and usage."""
import pytest

from tests import bam_merge_model as m
from tests import cli_util as cu


@pytest.fixture(scope="module")
def sam(hip_lib):
    from seqkit_amd import build
    build.build_hosts()
    return cu.SAM


HOST = {"SEQKIT_HOST_INFLATE": "1", "SEQKIT_GPU_DEFLATE": "0"}


def run(sam, argv, stdin=None):
    code, out, err = cu.run(sam, ["merge"] + argv, stdin=stdin, env=HOST)
    mem = m.members(out) if out else []
    if out:
        assert out.endswith(m.EOF_BLOCK) and all(0 < len(x) <= 0xFF00 for x, _ in mem[:-1])
    return code, b"".join(x for x, _ in mem), err, mem


def write_all(d, files, **kw):
    paths = [d / ("in%d.bam" % (i + 1)) for i in range(len(files))]
    return [str(p) for p in paths], [m.write(p, recs, **kw) for p, recs in zip(paths, files)]


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """12 files of 0 to 700 records, half of their keys shared, an unmapped tail in each"""
    d = tmp_path_factory.mktemp("merge")
    files = m.served_inputs(12, [700, 500, 0, 300, 1, 200, 150, 100, 80, 60, 40, 20], seed=6)
    return write_all(d, files)


@pytest.mark.parametrize("suffix", [False, True])
@pytest.mark.parametrize("k", [2, 3, 12])
def test_host_matches_model(sam, inputs, k, suffix):
    paths, raws = inputs
    exp = m.model(raws[:k], suffix, paths[:k])
    assert exp[2] == 0
    code, out, err, _ = run(sam, (["--suffix"] if suffix else []) + paths[:k])
    assert (out, err, code) == exp
    if suffix and k == 12:
        names = {r[36:36 + r[12] - 1].rsplit(b".", 1)[1] for r in m.records(out)}
        assert {b"1", b"10", b"11", b"12"} <= names


def test_uncompressed_and_option_placement(sam, inputs):
    paths, raws = inputs
    p = paths[:3]
    exp = m.model(raws[:3], True, p)
    for argv in (["--suffix", "--uncompressed"] + p, [p[0], "--uncompressed", p[1], "--suffix", p[2]], p + ["--uncompressed", "--suffix"]):
        code, out, err, mem = run(sam, argv)
        assert (out, err, code) == exp and all(stored for _, stored in mem[:-1])
    code, out, err, mem = run(sam, ["--suffix"] + p)
    assert (out, err, code) == exp and not all(stored for _, stored in mem[:-1])


def test_stdin_as_one_of_the_inputs(sam, inputs):
    paths, raws = inputs
    data = open(paths[1], "rb").read()
    for at in (0, 1, 2):
        order = [0, 3]
        order.insert(at, 1)
        argv = [paths[i] if i != 1 else "-" for i in order]
        code, out, err, _ = run(sam, ["--suffix"] + argv, stdin=data)
        assert (out, err, code) == m.model([raws[i] for i in order], True, argv)


def test_inputs_without_records(sam, inputs, tmp_path):
    paths, raws = inputs
    assert len(list(m.records(raws[2]))) == 0
    for order in ([2, 0], [0, 2], [2, 4, 2]):
        code, out, err, _ = run(sam, [paths[i] for i in order])
        assert (out, err, code) == m.model([raws[i] for i in order], False)
    code, out, err, _ = run(sam, [paths[2], paths[2], "--suffix"])
    assert (out, err, code) == (m.out_header(raws[2]), b"", 0)


def test_unmapped_tails_and_key_edges(sam, tmp_path):
    def rec(tid, pos, name):
        return m.placed(m.rm.record(name, 7), tid, pos)
    a = [rec(0, -1, b"a0"), rec(0, 0, b"a1"), rec(0, 2**31 - 1, b"a2"), rec(2, 5, b"a3"), rec(-1, -1, b"a4"), rec(-1, -1, b"a5")]
    b = [rec(0, 0, b"b0"), rec(1, -1, b"b1"), rec(2, 2**31 - 1, b"b2"), rec(-1, -1, b"b3"), rec(-1, -1, b"b4")]
    c = [rec(-1, -1, b"c0"), rec(-1, -1, b"c1")]
    paths, raws = write_all(tmp_path, [a, b, c])
    code, out, err, _ = run(sam, paths)
    assert (out, err, code) == m.model(raws, False)
    assert [r[36:38] for r in m.records(out)][-6:] == [b"a4", b"a5", b"b3", b"b4", b"c0", b"c1"]


def test_an_unsorted_input_is_still_the_loop(sam, tmp_path):
    files = m.served_inputs(3, 200, seed=8)
    files[1] = files[1][100:] + files[1][:100]
    files[2][10], files[2][150] = files[2][150], files[2][10]
    paths, raws = write_all(tmp_path, files)
    for suffix in (False, True):
        code, out, err, _ = run(sam, paths + (["--suffix"] if suffix else []))
        assert (out, err, code) == m.model(raws, suffix)
    assert list(m.records(out)) != m.sorted_by_key(list(m.records(out)))


def test_too_few_paths_and_usage(sam, inputs):
    paths, _ = inputs
    for argv in ([paths[0]], ["--suffix", paths[0]], ["/nonexistent/x.bam"]):
        assert cu.run(sam, ["merge"] + argv, env=HOST) == (255, b"", m.TWO_ERROR)
    usage = (b"\nUsage:\n  sam merge [options] <bam_files>...\n\nOptions:\n  --suffix          Add a suffix to read identifiers to avoid clashes\n"
             b"  --uncompressed    Output in uncompressed BAM format\n\nMerges two or more position-sorted BAM files together, ensuring that the\n"
             b"resulting output BAM file is also position-sorted.\n")
    for argv in ([], ["--suffix"], ["--nonsense", paths[0], paths[1]], ["-x", paths[0], paths[1]], ["--suffix=1", paths[0], paths[1]]):
        assert cu.run(sam, ["merge"] + argv, env=HOST) == (255, b"", b"ERROR: Invalid arguments.\n" + usage + b"\n")


def test_a_file_that_cannot_be_opened(sam, inputs):
    paths, _ = inputs
    code, out, err = cu.run(sam, ["merge", paths[0], "/nonexistent/x.bam"], env=HOST)
    assert (code, out, err) == (255, b"", b"ERROR: Cannot open BAM file '/nonexistent/x.bam'\n")


def test_reference_names(sam, tmp_path):
    recs = m.served_inputs(4, 30, seed=5)
    refs = m.rm.REFS
    paths, raws = [], []
    for i, (text, rf) in enumerate([(b"@HD\tVN:1.6\n\n", refs), (m.rm.TEXT, [(n, ln + 1) for n, ln in refs]), (m.rm.TEXT, refs[:2] + [(b"chrX", 16569)]),
                                    (m.rm.TEXT, refs[:2])]):
        p = tmp_path / ("h%d.bam" % i)
        raws.append(m.write(p, recs[i], text=text, refs=rf))
        paths.append(str(p))
    code, out, err, _ = run(sam, paths[:2])                                # equal names, other lengths and another text: merged under input 1's header
    assert (out, err, code) == m.model(raws[:2], False) and code == 0 and out.startswith(m.out_header(raws[0]))
    for order in ([0, 1, 2], [0, 3, 2], [2, 0], [3, 1, 0]):                # other names, another count: the first pair that differs
        argv = [paths[i] for i in order]
        code, out, err, _ = run(sam, argv)
        exp = m.model([raws[i] for i in order], False, argv)
        assert (out, err, code) == exp and exp[:1] == (b"",) and code == 255
    assert m.sq_error(paths[0], paths[2]) == m.model([raws[0], raws[1], raws[2]], False, [paths[0], paths[1], paths[2]])[1]


def test_a_name_too_long_with_its_suffix(sam, tmp_path):
    a = [m.rm.record(b"ok", 5, pos=1), m.rm.record(b"n" * 253, 5, pos=3), m.rm.record(b"late", 5, pos=9)]
    b = [m.rm.record(b"b", 5, pos=2), m.rm.record(b"c", 5, pos=4)]
    paths, raws = write_all(tmp_path, [a, b])
    code, out, err, _ = run(sam, ["--suffix"] + paths)
    assert (out, err, code) == m.model(raws, True) and code == 101
    assert [r[36:36 + r[12] - 1] for r in m.records(out)] == [b"ok.1", b"b.2"]
    code, out, err, _ = run(sam, paths)
    assert (out, err, code) == m.model(raws, False) and code == 0
    code, out, err, _ = run(sam, ["--suffix"] + paths[::-1])               # 253 bytes + ".2" as well
    assert (out, err, code) == m.model(raws[::-1], True) and code == 101
