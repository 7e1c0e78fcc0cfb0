"""CPU: the plain-Python model of `sam subsample` (tests/bam_subsample_model.py) against the command's rules, and the library's
sk_subsample_keep — host code that needs no device — against the model's generator."""
import math

import numpy as np
import pytest

from tests import bam_subsample_model as m

U64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def lib(hip_lib):
    from seqkit_amd import capi
    return capi.load_library(hip_lib)


def keep_c(lib, seed, d, fraction):
    from seqkit_amd import capi
    return capi.subsample_keep(seed, d, float(fraction), lib)


def test_the_first_three_draws_of_seed_0():
    assert [m.draw_m(0, d) for d in (1, 2, 3)] == [0xE220A8, 0x6E789E, 0x06C45D]


def test_threshold():
    assert m.threshold(0) == 0 and m.threshold(1) == 1 << 24 and m.threshold(0.5) == 1 << 23
    assert m.threshold(np.float32(2.0 ** -24)) == 1
    assert m.threshold(np.float32(0.1)) == int(float(np.float32(0.1)) * (1 << 24)) == 1677721


@pytest.mark.parametrize("text,value", [("0", 0.0), ("1", 1.0), ("0.5", 0.5), (".5", 0.5), ("5e-1", 0.5), ("+0.25", 0.25), ("1.", 1.0), ("1E0", 1.0),
                                        ("-0", 0.0), ("0.1", float(np.float32(0.1))), ("1e-60", 0.0)])
def test_fraction_parses(text, value):
    f = m.parse_fraction(text)
    assert f is not None and float(f) == value


@pytest.mark.parametrize("text", ["abc", "-0.1", "1.5", "nan", "NaN", " 0.5", "0.5 ", "0x1p-1", "1_0", "", ".", "e5", "1e", "inf", "-inf", "1e400", "0.5\n"])
def test_fraction_refused(text):
    assert m.parse_fraction(text) is None


def rec(name, flag):
    return m.rm.record(name, 10, flag=flag)


def test_mates_share_a_fate_and_a_third_occurrence_draws_anew():
    seed = 0                                                                # draws 1, 2, 3: m = 0xe220a8, 0x6e789e, 0x06c45d
    recs = [rec(b"a", 0x41), rec(b"b", 0x41), rec(b"a", 0x81), rec(b"a", 0x101), rec(b"b", 0x81)]
    # T = 2^23 = 0x800000: draw 1 drops a, draw 2 keeps b, a's third record makes draw 3 and is kept
    assert m.decisions(recs, seed, 0.5) == [False, True, False, True, True]
    assert m.decisions(recs, seed, 1.0) == [True] * 5
    assert m.decisions(recs, seed, 0.0) == [False] * 5


def test_a_supplementary_record_between_mates_does_not_break_the_pair():
    recs = [rec(b"a", 0x41), rec(b"a", 0x841), rec(b"a", 0x81), rec(b"b", 0x41)]
    assert m.decisions(recs, 0, 0.5) == [False, None, False, True]          # (b makes draw 2)
    raw = m.rm.header(m.rm.TEXT, m.rm.REFS) + b"".join(recs)
    out, err, code, kept, total = m.model(raw, 0, 0.5)
    assert (code, kept, total) == (0, 1, 3) and out == m.out_header(raw) + recs[3]
    assert err == b"Total reads: 3\nKept reads: 1 (33.3% of all reads)\n"


def test_names_with_slash_endings_are_distinct_keys():
    recs = [rec(b"x/1", 0x41), rec(b"x/2", 0x81)]
    assert m.decisions(recs, 0, 0.5) == [False, True]                        # two draws


def test_an_unpaired_record_stops_the_command():
    recs = [rec(b"a", 0x41), rec(b"b", 0x800), rec(b"c", 0), rec(b"a", 0x81)]
    raw = m.rm.header(m.rm.TEXT, m.rm.REFS) + b"".join(recs)
    out, err, code, kept, total = m.model(raw, 0, 1.0)
    assert code == 255 and err == m.UNPAIRED_ERROR and out == m.out_header(raw) + recs[0]


def test_summary_of_no_reads():
    assert m.summary(0, 0) == b"Total reads: 0\nKept reads: 0 (NaN% of all reads)\n"


def test_served_records_cover_the_cases():
    names = m.served_names(25000)
    count = {}
    for n, bits in names:
        if not bits & 0x800:
            count[n] = count.get(n, 0) + 1
    assert {1, 2, 3, 4, 5} <= set(count.values())
    assert any(len(n) == 1 for n in count) and any(len(n) == 254 for n in count)
    assert any(bits & 0x800 for _, bits in names) and any(bits & 0x100 for _, bits in names)
    assert any(n.endswith(b"/1") for n in count) and any(n.endswith(b"/2") for n in count)
    dec = m.decisions(m.served_records(), 7, 0.5)
    assert None in dec and True in dec and False in dec


# ---- sk_subsample_keep ----
SEEDS = [0, 1, 1 << 63, U64]
FRACTIONS = [np.float32(0), np.float32(2.0 ** -24), np.nextafter(np.float32(0.5), np.float32(0)), np.float32(0.5),
             np.nextafter(np.float32(0.5), np.float32(1)), np.float32(1)]


@pytest.mark.parametrize("seed", SEEDS)
def test_keep_equals_the_model_on_a_grid(lib, seed):
    draws = list(range(1, 4097)) + [1 << 32, U64]
    for f in FRACTIONS:
        T = m.threshold(f)
        got = [keep_c(lib, seed, d, f) for d in draws]
        assert got == [1 if m.draw_m(seed, d) <= T else 0 for d in draws], (seed, float(f))


def test_keep_at_the_ends(lib):
    for seed in SEEDS:
        assert all(keep_c(lib, seed, d, 1.0) == 1 for d in range(1, 2000))
    assert keep_c(lib, 0, 1, 0.0) == 0


@pytest.mark.parametrize("fraction", [-0.0001, 1.0001, math.nan, math.inf, -1.0])
def test_keep_refuses_a_fraction_outside_0_1(lib, fraction):
    assert keep_c(lib, 0, 1, fraction) == -1                                 # SK_ERR_INVALID


@pytest.mark.parametrize("fraction", [0.01, 0.25, 0.5, 0.9])
def test_share_kept_lies_within_5_sigma_of_the_binomial(fraction):
    """seeds 0 .. 63, 2^63, 2^64 - 1 and 0xDEADBEEF, draws 1 .. 65 536: the kept count against the binomial with p = (T + 1) / 2^24"""
    n = 65536
    T = m.threshold(np.float32(fraction))
    p = (T + 1) / (1 << 24)
    sd = math.sqrt(n * p * (1 - p))
    d = np.arange(1, n + 1, dtype=np.uint64)
    with np.errstate(over="ignore"):
        for seed in list(range(64)) + [1 << 63, U64, 0xDEADBEEF]:
            z = np.uint64(seed) + d * np.uint64(0x9E3779B97F4A7C15)
            z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
            z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
            z ^= z >> np.uint64(31)
            mm = z >> np.uint64(40)
            assert [int(x) for x in mm[:3]] == [m.draw_m(seed, k) for k in (1, 2, 3)]       # (the vector form is the model's)
            kept = int((mm <= np.uint64(T)).sum())
            assert abs(kept - n * p) <= 5 * sd, (seed, fraction, (kept - n * p) / sd)
