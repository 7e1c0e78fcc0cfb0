"""GPU: sk_bam_file_discard_tails on contexts planned for one CU and for three (SK_PLAN_CUS, as tests/test_gpu_small_grid.py): the
capped grids of bam_tail_used_kernel and bam_tail_keep_kernel — 8 workgroups of 256 records a planned CU — turn their stride loops
three times and more, and the result is the model's and, byte for byte, the default grid's."""
import pytest

from tests import bam_discard_tails_model as m
from tests import test_gpu_bam_discard_tails as tg
from tests.test_gpu_small_grid import Recording, planned

pytestmark = pytest.mark.gpu


class Rec(Recording):
    """Recording, but the loads call leaves what the windows held alone"""

    def __getattr__(self, name):
        return getattr(self._c, name) if name.endswith("_loads") else super().__getattr__(name)


PER_CU = 8 * 256                             # launch_bam_tail_keep / launch_bam_tail_used: n_cu * 8 workgroups x 256 records


@pytest.fixture(scope="module")
def small(hip_lib):
    cs = {k: planned(str(k)) for k in (1, 3)}
    for k, c in cs.items():
        assert c.planned_cus() == k
    yield cs
    for c in cs.values():
        c.close()


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """one file per CU count, each three trips and a ragged fourth; its model computed once"""
    d = tmp_path_factory.mktemp("tails_small_grid")
    fasta, genome = m.write_genome(d)
    out = {}
    for cus in (1, 3):
        n = 3 * PER_CU * cus + 777
        path = d / ("in%d.bam" % cus)
        raw = m.write(path, list(m.served_records(n, seed=3)), text=m.TEXT, refs=m.REFS, piece=0x3000, level=1)
        out[cus] = (path, raw, m.model(raw, genome, 20, 0.15), n)
    return fasta, out


@pytest.mark.parametrize("cus", [1, 3])
def test_discard_tails_past_the_first_trip(ctx, small, inputs, cus):
    fasta, files = inputs
    path, raw, exp, n = files[cus]
    assert n + 1 >= 3 * PER_CU * cus and exp[3][0] == n + 1
    for window in (0, len(exp[0]) // 3 + 1):
        rec, ref = Rec(small[cus]), Rec(ctx)
        got = [tg.check(c, path, fasta, raw, exp, 20, m.f32(0.15), 1, window) for c in (rec, ref)]
        assert got[0] == got[1] and (rec.launches, rec.bytes) == (ref.launches, ref.bytes)
        assert len(rec.launches) >= (4 if window else 2)
