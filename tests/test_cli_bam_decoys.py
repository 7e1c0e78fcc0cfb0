"""GPU: `sam statistics` and `sam trim qnames` on two files of tests/bam_decoy.py that fool the record walk's guess, three ways: the
device path, the host reader (SEQKIT_HOST_INFLATE=1), and the device path allowed one round (SK_BAMFILE_MAX_ROUNDS=1), which must
decline and leave the file to the host reader.  The same inflated stdout, the same stderr apart from the trace lines, the same status."""
import pytest

from tests import bam_decoy as bd
from tests import bam_rewrite_model as rm
from tests import bam_spec
from tests import bam_out_util as bu
from tests import cli_util as cu
from tests.bam_out_util import sam  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

CASES = bd.cases()
WAYS = ({}, {"SEQKIT_HOST_INFLATE": "1"}, {"SK_BAMFILE_MAX_ROUNDS": "1"})


def three_ways(sam, words, path):
    """[(code, stdout, stderr without the trace lines, the trace lines)] of the three ways, checked equal"""
    who = ("sam " + " ".join(words) + ": ").encode()
    runs = []
    for env in WAYS:
        code, out, err = cu.run(sam, list(words) + [str(path)], env=dict(env, SK_BAMFILE_TRACE="1"))
        lines = err.split(b"\n")
        trace = [ln for ln in lines if ln.startswith(who) or ln.startswith(b"sk_bam")]
        runs.append((code, out, b"\n".join(ln for ln in lines if ln not in trace), trace))
    assert runs[0][0] == runs[1][0] == runs[2][0] == 0
    assert runs[0][2] == runs[1][2] == runs[2][2]
    return runs, who


@pytest.mark.parametrize("name", ["garbage", "long-hop"])
def test_statistics_three_ways(sam, tmp_path, name):
    c = CASES[name]
    path = tmp_path / "d.bam"
    path.write_bytes(rm.bgzf(c.raw, cuts=c.ends))
    runs, _ = three_ways(sam, ["statistics"], path)
    assert runs[0][1] == runs[1][1] == runs[2][1] == bam_spec.statistics_text(bam_spec.read_bam(str(path))[1])
    # (sk_bam_file_reduce's own trace line is there when it served the file)
    served = [any(ln.startswith(b"sk_bam_file_reduce: alloc") for ln in r[3]) for r in runs]
    assert not served[1] and not served[2]
    if name == "garbage":                                                  # (18 blocks: within the cap by the derived bound)
        assert served[0]


@pytest.mark.parametrize("name", ["garbage", "long-hop"])
def test_trim_qnames_three_ways(sam, tmp_path, name):
    c = CASES[name]
    path = tmp_path / "d.bam"
    path.write_bytes(rm.bgzf(c.raw, cuts=c.ends))
    runs, who = three_ways(sam, ["trim", "qnames"], path)
    outs = [bu.inflated(rm, r[1]) for r in runs]
    assert outs[0] == outs[1] == outs[2] == rm.model(c.raw, "trim qnames")[0]
    path_of = [[ln for ln in r[3] if ln.startswith(who)] for r in runs]
    assert path_of[1] == [who + b"host reader"] and path_of[2] == [who + b"host reader"]
    if name == "garbage":
        assert path_of[0] == [who + b"device path, %d records" % c.n_real]
    else:                                                                  # either way (the cap of 64 rounds), and not asserted which
        assert path_of[0] in ([who + b"device path, %d records" % c.n_real], [who + b"host reader"])
