"""GPU: sk_bam_fragments_bed_dev (the BED lines of `sam fragments`) against Python formatting of the same kept records, and
sk_count_order_check_dev (the order checks of `sam count`) against a record-at-a-time statement of the loop."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


class Dev:
    """host arrays on the device for one test; freed at the end"""

    def __init__(self, ctx):
        self.ctx, self.ptrs = ctx, []

    def put(self, a):
        a = np.ascontiguousarray(a)
        p = self.ctx.malloc_device(max(a.nbytes, 1) + 16)
        if a.nbytes:
            self.ctx.copy_h2d(p, a)
        self.ptrs.append(p)
        return p

    def close(self):
        self.ctx.sync()
        for p in self.ptrs:
            self.ctx.free_device(p)


@pytest.fixture
def dev(ctx):
    d = Dev(ctx)
    yield d
    d.close()


def bed_expect(keep, tid, pos, tlen, names):
    out, bad = [], -1
    for i in np.flatnonzero(keep):
        t = int(tid[i])
        if t < 0 or t >= len(names):
            bad = int(i)
            break
        p = int(pos[i])
        out.append(names[t] + b"\t%d\t%d\n" % (p, p + abs(int(tlen[i]))))
    return b"".join(out), bad


def run_bed(ctx, dev, keep, tid, pos, tlen, names):
    n = len(keep)
    bits = np.packbits(np.asarray(keep, dtype=np.uint8), bitorder="little") if n else np.zeros(0, np.uint8)
    return ctx.bam_fragments_bed_dev(dev.put(bits), dev.put(np.asarray(tid, np.int32)), dev.put(np.asarray(pos, np.int32)),
                                     dev.put(np.asarray(tlen, np.int32)), n, names)


@pytest.mark.parametrize("n", [0, 1, 7, 63, 65, 2047, 2049, 100_003])
@pytest.mark.parametrize("kept", ["none", "all", "some"])
def test_bed_lines(ctx, dev, n, kept):
    rng = np.random.default_rng(n + len(kept))
    names = [b"chr1", b"c", b"chrUn_KI270302v1", b"x" * 3000, b"with\x00nul", b"\xff\xfe"]
    keep = {"none": np.zeros(n, bool), "all": np.ones(n, bool), "some": rng.random(n) < 0.4}[kept]
    tid = rng.integers(0, len(names), n).astype(np.int32)
    tid[rng.random(n) < 0.9] = 0                                            # (the long name is rarer)
    pos = rng.integers(-1, 1 << 31, n).astype(np.int32)
    tlen = rng.integers(-(1 << 31), 1 << 31, n, dtype=np.int64).astype(np.int32)
    if n >= 3:
        pos[:3] = [-1, (1 << 31) - 1, 0]
        tlen[:3] = [0, -(1 << 31), (1 << 31) - 1]
    text, bad = run_bed(ctx, dev, keep, tid, pos, tlen, names)
    e_text, e_bad = bed_expect(keep, tid, pos, tlen, names)
    assert bad == e_bad == -1
    assert text == e_text


def test_bed_bad_tid_reported(ctx, dev):
    n = 5000
    rng = np.random.default_rng(3)
    keep = rng.random(n) < 0.5
    tid = rng.integers(0, 2, n).astype(np.int32)
    pos = np.arange(n, dtype=np.int32)
    tlen = np.full(n, 150, np.int32)
    names = [b"chr1", b"chr2"]
    for where, t in ((int(np.flatnonzero(keep)[0]), 2), (int(np.flatnonzero(keep)[700]), -1), (int(np.flatnonzero(keep)[-1]), 1 << 20)):
        tt = tid.copy()
        tt[where] = t
        tt[~keep & (np.arange(n) > where)] = 99                             # (records not kept do not count)
        text, bad = run_bed(ctx, dev, keep, tt, pos, tlen, names)
        e_text, e_bad = bed_expect(keep, tt, pos, tlen, names)
        assert bad == e_bad == where
        assert text == e_text
    # no references at all: the first kept record is bad
    text, bad = run_bed(ctx, dev, keep, tid, pos, tlen, [])
    assert bad == int(np.flatnonzero(keep)[0]) and text == b""


# ---- sam count's order checks ------------------------------------------------------------------------------------------
def order_expect(flag, mapq, tid, pos, min_mapq, n_ref):
    prev_chr, prev_pos = -1, 0                                              # src/sam_count.rs:40-41
    for i in range(len(flag)):
        f = int(flag[i])
        if f & 0x4 or f & 0x400 or f & 0x100 or f & 0x800 or int(mapq[i]) < min_mapq:
            continue
        t, p = int(tid[i]), int(pos[i])
        if t != prev_chr:
            prev_chr = t
            if t < 0 or t >= n_ref:
                return i, 101
        elif p < prev_pos:
            return i, 255
        prev_pos = p
    return -1, 0


def sorted_records(n, seed, n_ref=3):
    rng = np.random.default_rng(seed)
    flag = rng.choice(np.array([99, 147, 83, 163, 0, 16, 4, 1024, 256, 2048], np.uint16), n).astype(np.uint16)
    mapq = rng.integers(0, 61, n).astype(np.uint8)
    tid = np.sort(rng.integers(0, n_ref, n)).astype(np.int32)
    pos = np.zeros(n, np.int32)
    for t in range(n_ref):
        m = tid == t
        pos[m] = np.sort(rng.integers(0, 1 << 30, int(m.sum())))
    return flag, mapq, tid, pos


def run_order(ctx, dev, flag, mapq, tid, pos, min_mapq, n_ref):
    return ctx.count_order_check_dev(dev.put(flag), dev.put(mapq), dev.put(tid), dev.put(pos), len(flag), min_mapq, n_ref)


@pytest.mark.parametrize("n", [1, 255, 4096, 4097, 100_000])
def test_order_sorted(ctx, dev, n):
    flag, mapq, tid, pos = sorted_records(n, seed=n)
    assert run_order(ctx, dev, flag, mapq, tid, pos, 0, 3) == (-1, 0)
    assert run_order(ctx, dev, flag, mapq, tid, pos, 30, 3) == (-1, 0)


@pytest.mark.parametrize("n", [4096 * 3 + 5, 300_001])
def test_order_violations(ctx, dev, n):
    base = sorted_records(n, seed=7)
    flag0 = base[0].copy()
    flag0[:] = 99                                                           # every record passes
    cases = [0, 1, 15, 16, 255, 256, 4095, 4096, 4097, 8191, n // 2, n - 2, n - 1]
    for where in cases:
        for kind in ("back", "bad_tid", "neg_tid"):
            flag, mapq, tid, pos = flag0.copy(), np.full(n, 60, np.uint8), base[2].copy(), base[3].copy()
            if kind == "back":
                if where == 0:
                    pos[0] = -5                                             # against the initial state: tid -1 vs tid 0 is a change, so make tid -1
                    tid[0] = -1
                else:
                    tid[where] = tid[where - 1]
                    pos[where] = pos[where - 1] - 1
            elif kind == "bad_tid":
                tid[where:] = 3
            else:
                tid[where] = -1 if where == 0 or tid[where - 1] != -1 else 5
            e = order_expect(flag, mapq, tid, pos, 0, 3)
            assert run_order(ctx, dev, flag, mapq, tid, pos, 0, 3) == e, (where, kind)
            assert e[0] >= 0 or (kind == "neg_tid" and where == 0)


def test_order_initial_state(ctx, dev):
    # tid -1 as the first passing record is no change of tid: its pos is compared with 0
    for pos0, e in ((0, (-1, 0)), (5, (-1, 0)), (-1, (0, 255))):
        flag = np.array([99, 99], np.uint16)
        mapq = np.array([60, 60], np.uint8)
        tid = np.array([-1, 0], np.int32)
        pos = np.array([pos0, 10], np.int32)
        assert run_order(ctx, dev, flag, mapq, tid, pos, 0, 1) == order_expect(flag, mapq, tid, pos, 0, 1) == e
    # a tid -1 record later (after a change): a change to an out-of-range tid
    flag, mapq = np.full(3, 99, np.uint16), np.full(3, 60, np.uint8)
    tid, pos = np.array([0, -1, 0], np.int32), np.array([5, 6, 7], np.int32)
    assert run_order(ctx, dev, flag, mapq, tid, pos, 0, 1) == (1, 101)


def test_order_filter_excludes(ctx, dev):
    n = 50_000
    flag, mapq, tid, pos = sorted_records(n, seed=3)
    flag[:] = 99
    mapq[:] = 60
    rng = np.random.default_rng(4)
    out = rng.choice(n, 500, replace=False)
    f_out = rng.choice(np.array([4, 1024 + 99, 256 + 99, 2048 + 99, 0x4 | 0x400], np.uint16), 500)
    pos2, tid2 = pos.copy(), tid.copy()
    pos2[out] = 0                                                           # unsorted, but excluded
    tid2[out[:100]] = 77                                                    # a tid with no name, but excluded
    for mode in ("flag", "mapq"):
        fl, mq = flag.copy(), mapq.copy()
        if mode == "flag":
            fl[out] = f_out
        else:
            mq[out] = 19
        assert run_order(ctx, dev, fl, mq, tid2, pos2, 20, 3) == (-1, 0)
        assert run_order(ctx, dev, fl, mq, tid2, pos2, 0, 3) == order_expect(fl, mq, tid2, pos2, 0, 3)
    # no record passes at all
    assert run_order(ctx, dev, np.full(n, 4, np.uint16), mapq, tid2, pos2, 0, 3) == (-1, 0)


def test_order_random_against_the_loop(ctx, dev):
    rng = np.random.default_rng(99)
    for trial in range(12):
        n = int(rng.integers(1, 40_000))
        flag, mapq, tid, pos = sorted_records(n, seed=trial)
        k = int(rng.integers(0, 4))
        for _ in range(k):
            i = int(rng.integers(0, n))
            if rng.random() < 0.5:
                pos[i] = int(rng.integers(-2, 1 << 30))
            else:
                tid[i] = int(rng.integers(-1, 5))
        mq = int(rng.integers(0, 61))
        assert run_order(ctx, dev, flag, mapq, tid, pos, mq, 3) == order_expect(flag, mapq, tid, pos, mq, 3), trial
