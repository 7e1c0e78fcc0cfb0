"""CPU: the host reader of `sam discard tail artifacts` (SEQKIT_HOST_INFLATE=1; its members deflated by zlib on the host,
SEQKIT_GPU_DEFLATE=0: no device needed), from a file and from stdin, against tests/bam_discard_tails_model.py: inflated stdout, stderr
bytes (the seconds masked) and status; every stop of the reference with the records before it; the argument errors and the usage;
--test; --debug."""
import pytest

from tests import bam_discard_tails_model as m
from tests import cli_util as cu


@pytest.fixture(scope="module")
def sam(hip_lib):
    from seqkit_amd import build
    build.build_hosts()
    return cu.SAM


HOST = {"SEQKIT_HOST_INFLATE": "1", "SEQKIT_GPU_DEFLATE": "0"}
WORDS = ["discard", "tail", "artifacts"]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("tails")
    fasta, genome = m.write_genome(d)
    path = d / "in.bam"
    return d, fasta, genome, path, m.write(path, list(m.served_records()), text=m.TEXT, refs=m.REFS)


def run(sam, argv, stdin=None):
    code, out, err = cu.run(sam, WORDS + argv, stdin=stdin, env=HOST)
    mem = m.members(out) if out else []
    if out:
        assert out.endswith(m.EOF_BLOCK) and all(0 < len(x) <= 0xFF00 for x, _ in mem[:-1])
    return code, b"".join(x for x, _ in mem), m.mask_seconds(err)


GRID = [(T, opt) for T in (1, 20, 33, 64, 300) for opt in ("--threshold=0", "--threshold=0.15", "--threshold=1", "--mismatches=3")]


def model_of(raw, genome, T, opt):
    key, val = opt.split("=")
    return m.model(raw, genome, T, float(val)) if key == "--threshold" else m.model(raw, genome, T, 0.15, mismatches=int(val))


@pytest.mark.parametrize("T,opt", GRID)
def test_host_matches_model(sam, files, T, opt):
    _, fasta, genome, path, raw = files
    exp_out, exp_err, exp_code, counts, _, _ = model_of(raw, genome, T, opt)
    code, out, err = run(sam, ["--tail-length=%d" % T, opt, str(fasta), str(path)])
    assert (code, err) == (exp_code, exp_err) and out == exp_out
    if exp_code == 0:
        assert counts[0] == len(m.served_records()) and len(list(m.records(out))) == counts[0] - counts[1]
        if opt == "--threshold=0":                                              # every mapped read fails: only the unmapped ones are written
            assert counts[2] == 0 and all(r[18] & 4 for r in m.records(out))
    else:                                                                       # --mismatches=3 of one base: a ratio of 3
        assert (T, opt, exp_code, out) == (1, "--mismatches=3", 255, b"") and err.endswith(m.THRESHOLD_RANGE_ERROR)


def test_host_stdin_defaults_and_option_placement(sam, files):
    _, fasta, genome, path, raw = files
    exp_out, exp_err, _, _, _, _ = m.model(raw, genome)
    data = open(path, "rb").read()
    for argv in ([str(fasta), "-"], ["--tail-length", "20", str(fasta), "-"], [str(fasta), "-", "--threshold=0.15"]):
        code, out, err = run(sam, argv, stdin=data)
        assert (code, err) == (0, exp_err) and out == exp_out
    assert b"THRESHOLD:0.2\n" in exp_out and b"INFO: 3 mismatches in 20 read tail bases" in exp_err


@pytest.mark.parametrize("label", sorted(m.stop_cases()))
def test_host_stops_where_the_reference_does(sam, files, tmp_path, label):
    _, fasta, genome, _, _ = files
    before, stop, status, line = m.stop_cases()[label]
    path = tmp_path / "stop.bam"
    raw = m.write(path, before + [stop] + before, text=m.TEXT, refs=m.REFS)
    exp_out, exp_err, exp_code, counts, _, _ = m.model(raw, genome)
    assert exp_code == status and exp_err.endswith(line) and counts[0] == len(before) + 1
    for argv, stdin in (([str(fasta), str(path)], None), ([str(fasta), "-"], open(path, "rb").read())):
        code, out, err = run(sam, argv, stdin)
        assert (code, err) == (exp_code, exp_err) and out == exp_out
        assert len(list(m.records(out))) == counts[0] - 1 - counts[1]           # the records before it, less the failed ones


def test_an_op_the_tails_never_reach_is_served(sam, files, tmp_path):
    """one N in the middle of a read: neither walk reaches it, and the reference writes the record"""
    _, fasta, genome, _, _ = files
    recs = list(m.served_records(40, seed=9))
    recs[20] = m.record(b"spliced", 0, 100, [(0, 30), (3, 500), (0, 30)], [1] * 60, 0)
    path = tmp_path / "n.bam"
    raw = m.write(path, recs, text=m.TEXT, refs=m.REFS)
    exp_out, exp_err, exp_code, _, _, _ = m.model(raw, genome, 20, 1.0)
    code, out, err = run(sam, ["--threshold=1", str(fasta), str(path)])
    assert (code, err, exp_code) == (0, exp_err, 0) and out == exp_out


def test_host_chromosome_and_genome_errors(sam, files, tmp_path):
    d, fasta, genome, path, raw = files
    recs = list(m.served_records(30, seed=9))
    # a reference name the index lacks, met at a record: the records before it are written
    odd = tmp_path / "odd.bam"
    raw_odd = m.write(odd, recs + [m.record(b"x", 3, 5, [(0, 30)], [1] * 30, 0)] + recs, text=m.TEXT, refs=m.REFS + [(b"chrZ", 900)])
    exp = m.model(raw_odd, genome)
    assert exp[2] == 255 and exp[1].endswith(m.not_found_error(b"chrZ", fasta))
    code, out, err = run(sam, [str(fasta), str(odd)])
    assert (out, err, code) == exp[:3]
    # reference 0 itself: before the first record
    first = tmp_path / "first.bam"
    raw_first = m.write(first, recs, text=m.TEXT, refs=[(b"chrZ", 900)] + m.REFS)
    exp = m.model(raw_first, genome)
    assert exp[2] == 255 and exp[0] == m.out_header(raw_first, 20, 0.15)
    assert run(sam, [str(fasta), str(first)]) == (255, exp[0], exp[1])
    # an empty reference list
    none = tmp_path / "none.bam"
    raw_none = m.write(none, [m.record(b"u", -1, -1, [], [1, 2], 4)], text=b"", refs=[])
    exp = m.model(raw_none, genome)
    assert exp[2] == 101 and run(sam, [str(fasta), str(none)]) == (101, exp[0], exp[1])
    # a missing .fai, a missing FASTA file, an index that does not parse
    lone = tmp_path / "lone.fa"
    lone.write_bytes(m.genome_files()[0])
    for gpath, g in ((lone, m.Genome(m.genome_files()[0], None, lone)), (tmp_path / "absent.fa", m.Genome(None, None, tmp_path / "absent.fa"))):
        exp = m.model(raw, g)
        assert exp[2] == 255 and exp[1].endswith(m.open_error(gpath)) and exp[0] == m.out_header(raw, 20, 0.15)
        assert run(sam, [str(gpath), str(path)]) == (255, exp[0], exp[1])
    (tmp_path / "lone.fa.fai").write_bytes(b"chrA\t5000\t22\t60\n")
    assert run(sam, [str(lone), str(path)])[::2] == (255, exp[1].replace(str(tmp_path / "absent.fa").encode(), str(lone).encode()))


@pytest.mark.parametrize("argv,message", [
    (["--tail-length=x"], m.TAIL_LENGTH_ERROR), (["--tail-length=0"], m.TAIL_LENGTH_ERROR), (["--tail-length=-3"], m.TAIL_LENGTH_ERROR),
    (["--tail-length=1.5"], m.TAIL_LENGTH_ERROR), (["--threshold=abc"], m.THRESHOLD_PARSE_ERROR), (["--threshold="], m.THRESHOLD_PARSE_ERROR),
    (["--tail-length=0", "--threshold=abc"], m.THRESHOLD_PARSE_ERROR),             # (the parse of :54 comes before the check of :59)
    (["--mismatches=x"], m.MISMATCHES_ERROR), (["--mismatches=-1"], m.MISMATCHES_ERROR), (["--mismatches=4294967296"], m.MISMATCHES_ERROR),
    (["--threshold=1.01"], m.THRESHOLD_RANGE_ERROR), (["--threshold=-0.5"], m.THRESHOLD_RANGE_ERROR), (["--threshold=inf"], m.THRESHOLD_RANGE_ERROR),
    (["--mismatches=21"], b"INFO: Mismatch threshold ratio set to 1.05\n" + m.THRESHOLD_RANGE_ERROR)])
def test_argument_errors(sam, argv, message):
    code, out, err = cu.run(sam, WORDS + argv + ["/nonexistent/g.fa", "/nonexistent/x.bam"], env=HOST)      # (refused before a file is opened)
    assert (code, out, err) == (255, b"", message)


@pytest.mark.parametrize("argv", [[], ["g.fa"], ["g.fa", "a.bam", "extra"], ["--nonsense", "g.fa", "a.bam"], ["--tail-length", "g.fa"], ["-x", "g.fa", "a.bam"]])
def test_usage(sam, argv):
    code, out, err = cu.run(sam, WORDS + argv, env=HOST)
    assert code == 255 and out == b"" and err == m.INVALID


def test_top_level_usage_does_not_list_the_command(sam):
    code, out, err = cu.run(sam, ["discard"], env=HOST)
    assert code == 0 and out == b"" and b"discard" not in err and err.startswith(b"\nUsage:\n  sam merge <bam_files>...\n")


def test_self_test(sam):
    """the reference's self-test (:442-563) has 29 expectations and its performance gate: 30 lines, each in ansi_term's green"""
    code, out, err = cu.run(sam, WORDS + ["--test"], env=HOST)
    lines = err.split(b"\n")
    assert code == 0 and out == b"" and lines[-2:] == [b"INFO: All tests passed. [OK]", b""]
    assert len(lines) == 32 and all(ln.startswith(b"[\x1b[32mPASS\x1b[0m] ") for ln in lines[:30])
    assert lines[0] == b"[\x1b[32mPASS\x1b[0m] IDENTICAL LEFT: " and lines[28] == b"[\x1b[32mPASS\x1b[0m] INS-DEL RIGHT"
    assert lines[29].startswith(b"[\x1b[32mPASS\x1b[0m] PERFORMANCE (") and lines[29].endswith(b" seconds)") and b"FAIL" not in err


def test_debug_writes_the_discarded_reads(sam, files, tmp_path):
    _, fasta, genome, _, _ = files
    recs = list(m.served_records(400, seed=3))
    path = tmp_path / "some.bam"
    raw = m.write(path, recs, text=m.TEXT, refs=m.REFS)
    name = str(tmp_path / "some_tail_discards_debug.bam").encode()
    exp_out, exp_err, exp_code, counts, _, discarded = m.model(raw, genome, debug_filename=name)
    assert counts[1] == len(discarded) > 10
    code, out, err = run(sam, ["--debug", str(fasta), str(path)])
    assert (code, err) == (0, exp_err) and out == exp_out
    data = open(name.decode(), "rb").read()
    assert data.endswith(m.EOF_BLOCK)
    assert b"".join(x for x, _ in m.members(data)) == m.rm.out_header(raw) + b"".join(discarded)      # (its header carries no @CO line: :90)
    # a path without ".bam" would name the input itself
    other = tmp_path / "plain"
    other.write_bytes(open(path, "rb").read())
    code, out, err = run(sam, ["--debug", str(fasta), str(other)])
    assert code == 255 and err.endswith(b"ERROR: Cannot create file '%s'\n" % str(other).encode()) and other.read_bytes() == open(path, "rb").read()
