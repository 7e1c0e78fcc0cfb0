"""CPU: the host reader of `sam subsample` (SEQKIT_HOST_INFLATE=1; its members deflated by zlib on the host, SEQKIT_GPU_DEFLATE=0: no
device needed), from a file and from stdin, against tests/bam_subsample_model.py: inflated stdout, stderr bytes and status; the
command's error messages and usage; and, without --seed, what any seed must give."""
import re

import pytest

from tests import bam_subsample_model as m
from tests import cli_util as cu


@pytest.fixture(scope="module")
def sam(hip_lib):
    from seqkit_amd import build
    build.build_hosts()
    return cu.SAM


HOST = {"SEQKIT_HOST_INFLATE": "1", "SEQKIT_GPU_DEFLATE": "0"}


@pytest.fixture(scope="module")
def bam(tmp_path_factory):
    path = tmp_path_factory.mktemp("subsample") / "in.bam"
    return path, m.write(path, m.served_records(6000))


def run(sam, argv, stdin=None):
    code, out, err = cu.run(sam, ["subsample"] + argv, stdin=stdin, env=HOST)
    mem = m.members(out) if out else []
    if out:
        assert out.endswith(m.EOF_BLOCK) and all(0 < len(x) <= 0xFF00 for x, _ in mem[:-1])
    return code, b"".join(x for x, _ in mem), err


@pytest.mark.parametrize("text", ["0", "1", "0.5", ".5", "5e-1", "+0.25"])
@pytest.mark.parametrize("seed", [0, 1, 0xDEADBEEF, (1 << 64) - 1])
def test_host_matches_model(sam, bam, text, seed):
    path, raw = bam
    exp_out, exp_err, exp_code, kept, total = m.model(raw, seed, m.parse_fraction(text))
    code, out, err = run(sam, ["--seed=%d" % seed, str(path), text])
    assert (code, err) == (exp_code, exp_err) and out == exp_out
    if text == "1":
        assert kept == total and out == m.out_header(raw) + b"".join(r for r in m.records(raw) if not m.flag_of(r) & 0x800)
    if text == "0.5":
        assert 0.4 * total < kept < 0.6 * total


def test_host_stdin_and_option_placement(sam, bam):
    path, raw = bam
    exp_out, exp_err, _, _, _ = m.model(raw, 5, m.parse_fraction("0.5"))
    data = open(path, "rb").read()
    for argv in (["--seed=5", "-", "0.5"], ["-", "0.5", "--seed", "5"], ["-", "--seed=5", "0.5"]):
        code, out, err = run(sam, argv, stdin=data)
        assert (code, err) == (0, exp_err) and out == exp_out


def test_host_unpaired_record_keeps_the_earlier_records(sam, tmp_path):
    path = tmp_path / "in.bam"
    recs = list(m.served_records(200, seed=4))
    recs[120] = m.rm.record(b"single", 21, flag=0x10)
    raw = m.write(path, recs)
    for text in ("1", "0.5"):
        exp_out, exp_err, exp_code, kept, _ = m.model(raw, 3, m.parse_fraction(text))
        code, out, err = run(sam, ["--seed=3", str(path), text])
        assert exp_code == code == 255 and err == exp_err == m.UNPAIRED_ERROR and out == exp_out
        assert len(list(m.records(out))) == kept
    assert len(list(m.records(m.model(raw, 3, 1.0)[0]))) == sum(1 for r in recs[:120] if not m.flag_of(r) & 0x800)


def test_host_no_records(sam, tmp_path):
    path = tmp_path / "empty.bam"
    raw = m.write(path, [], text=b"\n\n\0\0")
    code, out, err = run(sam, ["--seed=1", str(path), "0.5"])
    assert code == 0 and out == m.out_header(raw) and err == b"Total reads: 0\nKept reads: 0 (NaN% of all reads)\n"


@pytest.mark.parametrize("text", ["abc", "-0.1", "1.5", "nan", " 0.5", "0x1p-1", "", "1e", "inf", "1_0"])
def test_bad_fraction(sam, text):
    assert m.parse_fraction(text) is None
    code, out, err = cu.run(sam, ["subsample", "/nonexistent/x.bam", text], env=HOST)     # (refused before the file is opened)
    assert code == 255 and out == b"" and err == m.FRACTION_ERROR


@pytest.mark.parametrize("seed", ["x", "-1", "18446744073709551616", "", "1.5", "0x10"])
def test_bad_seed(sam, bam, seed):
    code, out, err = cu.run(sam, ["subsample", "--seed=" + seed, str(bam[0]), "0.5"], env=HOST)
    assert code == 255 and out == b"" and err == m.SEED_ERROR


USAGE = b"""
Usage:
  sam subsample [options] <bam_file> <fraction>

Options:
  --seed=N    Seed of the random draws, for a reproducible result [default: from the OS]

If your BAM file has been duplicate-flagged, remember to re-run duplicate
flagging after subsampling, otherwise random subsampling can delete the only
non-duplicate-flagged DNA fragment in a duplicate cluster.
"""


@pytest.mark.parametrize("argv", [[], ["a.bam"], ["a.bam", "0.5", "extra"], ["--nonsense", "a.bam", "0.5"], ["--seed", "a.bam"], ["-x", "a.bam", "0.5"]])
def test_usage(sam, argv):
    code, out, err = cu.run(sam, ["subsample"] + argv, env=HOST)
    assert code == 255 and out == b"" and err == b"ERROR: Invalid arguments.\n" + USAGE + b"\n"


def test_without_a_seed_every_run_is_a_consistent_subsample(sam, bam):
    """two runs with seeds from the OS: each output is an in-order subset of the counted records, closed under the pairing, and the
    counts agree with stderr; which records were kept is not asserted"""
    path, raw = bam
    recs = list(m.records(raw))
    counted = [r for r in recs if not m.flag_of(r) & 0x800]
    for _ in range(2):
        code, out, err = run(sam, [str(path), "0.5"])
        assert code == 0
        assert out.startswith(m.out_header(raw))
        got = list(m.records(out))
        it = iter(counted)
        assert all(any(g == c for c in it) for g in got)                    # an in-order subset (records may repeat: matched greedily)
        # closed under the pairing: walk the counted records with the map, taking each record's fate from the output
        at, pending = 0, {}
        for r in counted:
            kept = at < len(got) and got[at] == r
            name = m.qname(r)
            if name in pending:
                assert pending.pop(name) == kept
            else:
                pending[name] = kept
            at += kept
        assert at == len(got)
        mt = re.fullmatch(rb"Total reads: (\d+)\nKept reads: (\d+) \(([0-9.]+)% of all reads\)\n", err)
        assert mt and int(mt.group(1)) == len(counted) and int(mt.group(2)) == len(got)
        assert mt.group(3) == b"%.1f" % (len(got) / len(counted) * 100.0)
