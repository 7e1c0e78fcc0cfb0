"""GPU: `sam concatenate` with every input on the device path (sk_bam_file_concatenate), on the host reader (SEQKIT_HOST_INFLATE=1) and
with the two mixed — "-" for one input, an input the device declines —: the same inflated stdout, stderr and status, equal to
tests/bam_concatenate_model.py; the trace says which way each input went."""
import pytest

from tests import bam_concatenate_model as m
from tests import bam_out_util as bu
from tests.bam_out_util import sam  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

WHO = b"sam concatenate: "
SIZES = [2500, 1200, 0, 300, 1, 200, 150, 100, 80, 60, 40, 20]


def run(sam, argv, stdin=None, env=None):
    """(code, inflated stdout, stderr without the trace's lines, the trace's lines of this command, members)"""
    code, out, err = bu.cu.run(sam, ["concatenate"] + list(argv), stdin=stdin, env=dict({"SK_BAMFILE_TRACE": "1"}, **(env or {})))
    mem = m.members(out) if out else []
    if out:
        assert out.endswith(m.EOF_BLOCK) and out.count(m.EOF_BLOCK) == 1
        assert all(0 < len(x) <= 0xFF00 for x, _ in mem[:-1])
    lines = err.split(b"\n")[:-1]
    trace = [ln[len(WHO):] for ln in lines if ln.startswith(WHO)]
    rest = b"".join(ln + b"\n" for ln in lines if not ln.startswith(WHO) and not ln.startswith(b"sk_bam"))
    return code, b"".join(x for x, _ in mem), rest, trace, mem


def device_line(b, n):
    return b"input %d: device path, %d records" % (b, n)


def host_line(b):
    return b"input %d: host reader" % b


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("concat_cli")
    return m.write_all(d, m.served_inputs(12, SIZES, seed=6), piece=0x3000)


@pytest.mark.parametrize("extra", [(), ("--uncompressed",)])
@pytest.mark.parametrize("k", [2, 12])
def test_device_host_and_model(sam, inputs, k, extra):
    paths, raws = inputs
    exp = m.model(raws[:k], paths[:k])
    assert exp[1:] == (b"", 0)
    code, out, err, trace, mem = run(sam, list(extra) + paths[:k])
    assert (out, err, code) == exp
    assert trace == [device_line(b + 1, SIZES[b]) for b in range(k)]
    if extra:
        assert all(stored for _, stored in mem[:-1])
    else:
        assert not all(stored for _, stored in mem[:-1])
    code, out, err, trace, _ = run(sam, list(extra) + paths[:k], env={"SEQKIT_HOST_INFLATE": "1"})
    assert (out, err, code) == exp and trace == [host_line(b + 1) for b in range(k)]


def test_small_windows_on_the_device_path(sam, inputs):
    paths, raws = inputs
    code, out, err, trace, _ = run(sam, paths[:4], env={"SK_BAMFILE_WINDOW": "4096"})
    assert (out, err, code) == m.model(raws[:4], paths[:4]) and trace == [device_line(b + 1, SIZES[b]) for b in range(4)]


@pytest.mark.parametrize("at", [0, 1, 2])
def test_stdin_among_the_inputs(sam, inputs, at):
    """the host reader serves that input alone, and the next one is offered to the device again"""
    paths, raws = inputs
    order = [0, 3, 1]
    argv = [paths[i] if j != at else "-" for j, i in enumerate(order)]
    code, out, err, trace, _ = run(sam, argv, stdin=open(paths[order[at]], "rb").read())
    assert (out, err, code) == m.model([raws[i] for i in order], argv)
    assert trace == [host_line(j + 1) if j == at else device_line(j + 1, SIZES[i]) for j, i in enumerate(order)]


def test_a_declined_input_goes_to_the_host_reader_alone(sam, inputs, tmp_path):
    paths, raws = inputs
    long = list(m.records(raws[1]))
    long[50] = m.rm.record(b"n" * 253, 10)
    p = tmp_path / "long.bam"
    raw = m.write(p, long, refs=m.refs_of(1))
    argv = [paths[0], str(p), paths[3]]
    exp = m.model([raws[0], raw, raws[3]], argv)
    assert exp[1:] == (m.PANIC, 101)
    code, out, err, trace, _ = run(sam, argv)
    assert (out, err, code) == exp and len(list(m.records(out))) == SIZES[0] + 50
    assert trace == [device_line(1, SIZES[0]), host_line(2)]
    host = run(sam, argv, env={"SEQKIT_HOST_INFLATE": "1"})
    assert host[:3] == (code, out, err) and host[3] == [host_line(1), host_line(2)]
    # 252 bytes take ".2" but not ".10": the same file is served on the device in second place and declined in tenth
    long[50] = m.rm.record(b"n" * 252, 10)
    raw = m.write(p, long, refs=m.refs_of(1))
    code, out, err, trace, _ = run(sam, [paths[0], str(p), paths[3]])
    assert (out, err, code) == m.model([raws[0], raw, raws[3]]) and code == 0
    assert trace == [device_line(1, SIZES[0]), device_line(2, SIZES[1]), device_line(3, SIZES[3])]
    argv = [paths[4]] * 9 + [str(p), paths[5]]
    code, out, err, trace, _ = run(sam, argv)
    assert (out, err, code) == m.model([raws[4]] * 9 + [raw, raws[5]]) and code == 101
    assert trace == [device_line(b + 1, 1) for b in range(9)] + [host_line(10)]


def test_a_missing_file_behind_device_served_inputs(sam, inputs):
    paths, raws = inputs
    argv = [paths[0], paths[1], "/nonexistent/x.bam"]
    code, out, err, trace, _ = run(sam, argv)
    assert (out, err, code) == m.model([raws[0], raws[1], None], argv) and code == 255
    assert trace == [device_line(1, SIZES[0]), device_line(2, SIZES[1]), host_line(3)]
