"""The census's claim log past its capacity (sk_census.hip: census_log_claim, census_clear_kernel).

Whoever claims a slot of the HBM table appends its index to one of 256 regions of a log; a reset clears the slots the log names, or,
when a region's counter went beyond its capacity (or there is no log: SK_CENSUS_LOG_CAP_LOG2=-1), the whole table.  A slot that a
reset misses shows in the NEXT census as a barcode that is not in its input.  So every case here runs reset -> add(set) -> compare
(tests/test_gpu_small_grid.py's census_case: the entries in first-seen order with counts and first rows, the statistics, the count
histogram and the min_count=3 listing, against oracle.census of that set alone) over sets that have no barcode in common, on
contexts whose log holds c = 2^v entries a region, v = 0, 4, 6 — the default is 2^16, which no test input fills.

No output says which branch of census_clear_kernel ran; the inputs make it certain (branch_after, asserted by every case).  Between
two zeroings of the counters (a reset, or a rehash into a grown table: census_reserve zeroes them and the rehash kernel claims every
key again) a key claims its slot once, so behind an add of K distinct keys the 256 counters sum to K:
  K <= c        no counter is above c: the next reset clears by the log, and every one of the K slots must be named in it;
  K > 256 c     some counter is above c: the next reset clears the whole table.
Between the two the claims' spread over the regions decides (they are blockIdx.x mod 256 of whichever kernel claims): the sweep holds
the property alone, and there a wave's claims straddle the capacity (`base + rank < log_cap` for some of its lanes).

The CPU half (no gpu mark) holds the generator: the sets are pairwise disjoint, have the K the cases state, and the oracle's entries
of one set name that set's barcodes alone."""
import numpy as np
import pytest

from tests.test_gpu_small_grid import census_case, planned

L, STRIDE = 10, 12
REGIONS = 256                                 # sk_census.hip: kLogRegions
SLOTS_LOG2 = 13
SWEEP = (1, 2, 17, 64, 255, 256, 257)
N_VALUES = 4 ** L


def branch_after(K, c):
    """which branch of census_clear_kernel the reset behind an add of K distinct keys takes with c log entries a region (0: no log);
    None: the spread of the claims decides"""
    if c == 0 or K > REGIONS * c:
        return "whole table"
    return "log" if K <= c else None


def sequence_sizes(c):
    """big (several growths from 2^13 slots where 2 K is beyond them), small, small', big', small'': K of each"""
    return [3 * REGIONS * c, c, max(1, c - 1), REGIONS * c + 1, c]


def plan(c):
    """[(K, the branch the reset BEHIND this set takes)] of a context with c entries a region: the sequence, the sweep, and one small
    set that looks at the reset behind the sweep's last.  Without a log (c == 0) the first three of c = 16's sequence."""
    if c == 0:
        return [(K, "whole table") for K in sequence_sizes(16)[:3]]
    ks = sequence_sizes(c) + [c * f for f in SWEEP] + [c]
    return [(K, branch_after(K, c)) for K in ks]


_VALUES = []


def values():
    """every 10-mer once, shuffled (as test_census_grows_between_launches draws them)"""
    if not _VALUES:
        _VALUES.append(np.random.default_rng(21).permutation(N_VALUES).astype(np.int64))
    return _VALUES[0]


def matrix(vals):
    bc = np.zeros((len(vals), STRIDE), dtype=np.uint8)
    bc[:, :L] = np.frombuffer(b"ACGT", dtype=np.uint8)[(vals[:, None] >> (2 * np.arange(L))) & 3]
    return bc


def key_sets(c):
    """[(the set's K values, its rows' values)] for plan(c): set i takes the next K of values(), so no two share a barcode.  A set's
    rows are each of its keys once and half as many again (and 40), of which half fall on at most eight hot keys — the shape of
    tests/test_gpu_parity.py's random_barcodes — in shuffled order: counts and first rows differ from key to key."""
    out, at = [], 0
    for i, (K, _) in enumerate(plan(c)):
        keys = values()[at:at + K]
        at += K
        rng = np.random.default_rng(1000 * c + i)
        extra = K // 2 + 40
        hot = keys[:min(K, 8)]
        more = np.where(rng.random(extra) < 0.5, hot[rng.integers(0, len(hot), extra)], keys[rng.integers(0, K, extra)])
        out.append((keys, rng.permutation(np.concatenate([keys, more]))))
    assert at <= N_VALUES
    return out


CAPS = {"0": 1, "4": 16, "6": 64, "-1": 0}


# ---- CPU: the generator and the conditions ----------------------------------------------------------------------------------------
def test_branch_after_by_hand():
    assert [branch_after(K, 1) for K in (1, 2, 256, 257)] == ["log", None, None, "whole table"]
    assert [branch_after(K, 64) for K in (63, 64, 65, 16384, 16385)] == ["log", "log", None, None, "whole table"]
    assert branch_after(1, 0) == "whole table"
    assert sequence_sizes(1) == [768, 1, 1, 257, 1] and sequence_sizes(64) == [49152, 64, 63, 16385, 64]
    for c in (1, 16, 64):
        p = plan(c)
        assert [b for _, b in p[:5]] == ["whole table", "log", "log", "whole table", "log"]
        assert [K for K, _ in p[5:]] == [c * f for f in SWEEP] + [c]
        assert p[5][1] == "log" and p[-2][1] == "whole table" and [b for _, b in p[6:-2]] == [None] * 5
    assert plan(0) == [(12288, "whole table"), (16, "whole table"), (15, "whole table")]
    assert 2 * sequence_sizes(16)[0] > 1 << SLOTS_LOG2 and 2 * sequence_sizes(64)[3] > 1 << SLOTS_LOG2     # these grow the first table


@pytest.mark.parametrize("v", list(CAPS))
def test_key_sets_are_disjoint_and_as_large_as_stated(oracle, v):
    c = CAPS[v]
    sets = key_sets(c)
    assert [len(keys) for keys, _ in sets] == [K for K, _ in plan(c)]
    every = np.concatenate([keys for keys, _ in sets])
    assert len(np.unique(every)) == len(every)                                        # pairwise disjoint
    repeated = 0
    for keys, rows in sets:
        uniq, counts = np.unique(rows, return_counts=True)
        assert np.array_equal(uniq, np.sort(keys)) and len(rows) == len(keys) + len(keys) // 2 + 40
        repeated += int(counts.max() >= 3)
        # the oracle's entries of the set by itself: its K barcodes in first-seen order, nothing of another set
        want = oracle.census(matrix(rows), L=L)
        first = {}
        for r, val in enumerate(rows.tolist()):
            first.setdefault(val, r)
        by_count = dict(zip(uniq.tolist(), counts.tolist()))
        order = sorted(first, key=first.get)
        assert [e[0] for e in want] == [bytes(m[:L]) for m in matrix(np.array(order, dtype=np.int64))]
        assert [(e[1], e[2]) for e in want] == [(by_count[val], first[val]) for val in order]
    assert repeated == len(sets)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wanted(oracle):
    """(the rows' matrix, oracle.census of it) of set i of key_sets(c), computed once for every path and context"""
    cache = {}

    def get(c, i):
        if (c, i) not in cache:
            if c not in cache:
                cache[c] = key_sets(c)
            bc = matrix(cache[c][i][1])
            cache[c, i] = (bc, oracle.census(bc, L=L))
        return cache[c, i]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["direct", "partition", "spilled_direct"])
@pytest.mark.parametrize("v,cus", [("0", "1"), ("4", "1"), ("6", "1"), ("-1", "1"), ("4", None)],
                         ids=["cap1", "cap16", "cap64", "no_log", "cap16_default_grid"])
def test_no_reset_leaves_a_slot_behind(hip_lib, wanted, monkeypatch, v, cus, path):
    """the three launch paths of tests/test_gpu_small_grid.py's test_census: the claiming kernel, and with it the regions, differ.
    Planned for one CU the launches are 2^13 rows at most, so the big sets grow the table several times and the log is written behind a rehash;
    the default grid (whose rehash kernel claims from all 256 regions) takes its launches whole."""
    monkeypatch.setenv("SK_CENSUS_SPILL", "0" if path == "direct" else "1")
    if path != "direct":
        monkeypatch.setenv("SK_CENSUS_SPILL_MAX_PCT", "100" if path == "partition" else "0")
    if cus:
        monkeypatch.setenv("SK_CENSUS_CHUNK_LOG2", "13")
        monkeypatch.setenv("SK_CENSUS_MIN_CHUNK_LOG2", "10")
    cap = CAPS[v]
    c = planned(cus, SK_CENSUS_SLOTS_LOG2=str(SLOTS_LOG2), SK_CENSUS_LOG_CAP_LOG2=v)
    try:
        assert c.census_stats()["slots"] == 1 << SLOTS_LOG2 and (c.planned_cus() == 1) == (cus == "1")
        steps = plan(cap)
        branches = []
        for i, (K, branch) in enumerate(steps):
            bc, want = wanted(cap, i)
            assert len(want) == K and branch == branch_after(K, cap)
            if cap and K <= cap:
                assert branch == "log"
            if K > REGIONS * cap:
                assert branch == "whole table"
            census_case(c, bc, L, want)                                               # (its reset is the one behind set i - 1)
            st = c.census_stats()
            assert st["slots"] >= max(2 * K, 1 << SLOTS_LOG2)
            branches.append(branch)
        if cap == 0:
            assert branches == ["whole table"] * 3
        else:
            assert branches[:5] == ["whole table", "log", "log", "whole table", "log"]      # each looked at by the set behind it
            assert branches[-2:] == ["whole table", "log"]
        if cap != 1:
            assert c.census_stats()["slots"] > 1 << SLOTS_LOG2                          # (a big set grew the table; no reset shrinks it)
    finally:
        c.close()
