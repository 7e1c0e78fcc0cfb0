"""GPU: sk_bam_file_pairs_gz on contexts planned for one CU and for three (SK_PLAN_CUS, as tests/test_gpu_small_grid.py), where the
grids of the text, deflate and pack kernels are capped far lower than on the whole chip: every window's compressed bytes are the
default grid's, and the inflated streams the model's."""
import pytest

from tests import test_gpu_bam_pairs_gz as tg
from tests.test_gpu_small_grid import Recording, planned

pytestmark = pytest.mark.gpu

mixed, mixed_files = tg.mixed, tg.mixed_files                              # (the module's fixtures, made once here too)


@pytest.fixture(scope="module")
def small(hip_lib):
    cs = {k: planned(str(k)) for k in (1, 3)}
    for k, c in cs.items():
        assert c.planned_cus() == k
    yield cs
    for c in cs.values():
        c.close()


@pytest.fixture(scope="module")
def default_grid(ctx, mixed_files):
    """{window: (the default grid's windows, the inflated streams)} of the shuffled file in fastq at level 1: computed once"""
    path, _, exp = mixed_files["shuffled"]
    out = {}
    for window in (4096, 0):
        ref = Recording(ctx)
        ok, got, *_ = tg.collect_gz(ref, path, "fastq", 1, window)
        assert ok and got == exp["fastq"]
        out[window] = (ref.launches, ref.bytes)
    return out


@pytest.mark.parametrize("cus", [1, 3])
def test_pairs_gz_on_a_small_grid(small, mixed_files, default_grid, cus):
    path, _, exp = mixed_files["shuffled"]
    for window in (4096, 0):
        rec = Recording(small[cus])
        ok, got, *_ = tg.collect_gz(rec, path, "fastq", 1, window)
        assert ok and got == exp["fastq"]
        assert (rec.launches, rec.bytes) == default_grid[window]
        assert len(rec.launches) >= (60 if window else 3)
