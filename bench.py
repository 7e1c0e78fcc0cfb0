#!/usr/bin/env python3
"""bench.py — M reads/s of the fused per-read pass (add barcode + demultiplex + trim + mask by quality).

Workload (BASELINE.json configs[3], the one the metric is quoted on): 2x150 bp paired clusters, 96 dual-index
8+8 barcodes (`i7+i5`, 17 chars), <=1 mismatch, min_baseq 20.  configs[3] is 500 M clusters read-sharded over
8 GPUs; one GPU's shard (62.5 M clusters, 57.8 GB of device-resident buffers) is the per-GPU work at every N
(weak scaling), so N=8 is exactly configs[3].  A "step" = one pass of the hot path over the rank's whole shard +
the count reduce (RCCL all-reduce of u64[S+3] through the library's own communicator when N > 1).  A "read" is one
cluster, as the reference's own `total_reads` counter counts them (src/fasta_demultiplex.rs:169).

Launch: `python bench.py --gpus N` starts the N rank processes ITSELF (before torch or the GPU is touched) when it
is not already running under a launcher; under `python -m torch.distributed.run --nproc-per-node N bench.py --gpus N`
it is one of the ranks.  Either way: one process per GPU, rank 0 prints ONE JSON line on stdout.  Inputs are
resident in HBM before the timed region; the kernel duration for the roofline object comes from HIP events recorded
on the stream the kernel runs on.

A plain run does only what the headline needs: set up (shard, placement choice), warm up, time --steps steps, write
--dump-outputs DIR if given, print the line.  --full adds what is measured or checked beside it: the device identity,
the parity sample against the CPU oracle with cpu_baseline, and extra (the other configs' rates, BAM files).
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import socket
import subprocess
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

L_READ = 150
S_SAMPLES = 96
L_BC = 17
MIN_BASEQ = 20
# algorithmic bytes per cluster: read 2*(2*150) + 17, write 2*(150 + 2) + 4
BYTES_PER_PAIR = 2 * (2 * L_READ) + L_BC + 2 * (L_READ + 2) + 4      # 925
HBM_PEAK_GBS = 8000.0
DUMP_ROWS = 32768               # --dump-outputs: clusters sampled from rank 0's shard (their 2 x 150 output bytes as float32: 39 MB)
DUMP_SEED = 4242


def steps_arg(s):
    v = int(s)
    if v < 1:
        raise argparse.ArgumentTypeError("the number of timed steps must be at least 1")
    return v


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=steps_arg, default=20, help="timed steps (ms_per_step = their wall time / steps)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--full", action="store_true",
                    help="also measure and check what the headline does not need: the device identity from rocm-smi, the parity sample "
                         "against the CPU oracle with cpu_baseline (--cpu-sample, --cpu-threads, --no-all-cores, --faithful-reads) and "
                         "extra (rates of the other configs, BAM files; --no-extra).  A plain run sets up, warms up, times the steps, "
                         "writes --dump-outputs and prints the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last step computed as DIR/<name>.npy (float32 / float64): the counters, "
                         f"the outputs of {DUMP_ROWS} clusters drawn with a fixed seed, and whole-shard column sums and histograms")
    ap.add_argument("--pairs", type=int, default=62_500_000, help="clusters per GPU (default: configs[3] / 8)")
    ap.add_argument("--layout", choices=["soa", "blocked"], default=os.environ.get("SK_BENCH_LAYOUT", "soa"),
                    help="batch layout in HBM: row-major SoA matrices (with placement tuning the faster of the two) or tile-blocked "
                         "(one read range + one write range per 64-cluster tile)")
    ap.add_argument("--cpu-sample", type=int, default=4_000_000, help="with --full: clusters checked against and timed on the CPU oracle (0 = skip)")
    ap.add_argument("--cpu-threads", type=int, default=1,
                    help="threads for the CPU baseline (the reference's loops are single-threaded, so 1 is the faithful number; "
                         "more threads split the sample into slices)")
    ap.add_argument("--no-all-cores", action="store_true", help="skip cpu_baseline.all_cores (the restatement on every usable core)")
    ap.add_argument("--faithful-reads", type=int, default=1_000_000,
                    help="reads of cfg 2 / cfg 3 text run through the line-at-a-time oracle CLI for cpu_baseline.faithful (0 = skip)")
    ap.add_argument("--no-extra", action="store_true", help="with --full: skip extra.rates (device-resident rates of the other configs)")
    ap.add_argument("--gen-chunk", type=int, default=2_000_000)
    ap.add_argument("--placements", type=int, default=None,
                    help="candidate device buffers per big matrix (SoA) / per buffer (blocked): allocated at start-up, the pass is timed "
                         "while one matrix at a time is swapped for its other candidates (sk_fused_tune_placement_dev), the fastest combination "
                         "is kept and the rest freed — where a buffer's pages lie moves the same kernel by up to 12 %%; 1 = take what comes. "
                         "Default 3 on one GPU, 2 when --gpus N > 1 (every rank allocates its candidates at start-up: K x 56 GB each)")
    ap.add_argument("--test-worker", default=None, help=argparse.SUPPRESS)     # tests/test_bench_launcher.py: the script the launcher starts as a rank
    return ap.parse_args(argv)


# ---------------------------------------------------------------------------------------------------------------------
# N > 1 without a launcher: start the ranks here.  Nothing above or inside this function imports torch or touches the
# GPU, so no process that has initialised a GPU is ever re-executed; rank 0's stdout (the JSON line) is relayed.
# ---------------------------------------------------------------------------------------------------------------------
EXIT_PORT_TAKEN = 98                                            # a rank's exit code when the rendezvous port was taken: the launcher draws another


def launch_ranks(args) -> int:
    n = args.gpus
    worker = args.test_worker                                   # test-only flag, never read from the environment
    argv, skip = [], False
    for a in sys.argv[1:]:                                      # the ranks get the command line without the test flag
        if skip:
            skip = False
        elif a == "--test-worker":
            skip = True
        elif not a.startswith("--test-worker="):
            argv.append(a)
    cmd = ([sys.executable, worker] if worker else [sys.executable, os.path.abspath(__file__)]) + argv
    for attempt in range(3):
        # the port is free now; another process may take it before rank 0 listens — rank 0 then exits with EXIT_PORT_TAKEN
        # and all ranks are started again on a new port (fresh processes: nothing that touched a GPU is re-executed)
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
        s.close()
        rc, out0 = run_ranks(cmd, n, port)
        if rc != EXIT_PORT_TAKEN:
            break
        sys.stderr.write(f"[bench] port {port} was taken before rank 0 could listen; starting the ranks again\n")
    if rc != 0:
        return rc
    lines = [ln for ln in out0.decode(errors="replace").splitlines() if ln.strip()]
    if not lines:
        sys.stderr.write("[bench] rank 0 printed nothing\n")
        return 1
    sys.stdout.write(lines[-1] + "\n")
    sys.stdout.flush()
    return 0


def run_ranks(cmd, n, port):
    """Start the n ranks, relay rank 0's stdout, and keep every rank's stderr readable: each line goes to this process's stderr
    behind `[rank r]`, and when a rank fails its last lines are repeated under the verdict.  Returns (exit code, rank 0's stdout)."""
    import select
    import threading
    procs, tails, readers = [], [], []
    for r in range(n):
        env = dict(os.environ)
        # HSA_ENABLE_IPC_MODE_LEGACY: a DEFAULT, not an override — the pool's host driver only has dmabuf IPC, and without
        # the variable RCCL's (and torch's) cross-process buffer sharing fails with `hipIpcGetMemHandle: invalid argument`; the
        # image exports it already, a caller's own value is kept, and a bare environment (a scheduler's) still gets the working one
        env.update({"RANK": str(r), "LOCAL_RANK": str(r), "WORLD_SIZE": str(n), "LOCAL_WORLD_SIZE": str(n),
                    "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "HSA_ENABLE_IPC_MODE_LEGACY": env.get("HSA_ENABLE_IPC_MODE_LEGACY", "0")})
        p = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL, stderr=subprocess.PIPE)
        procs.append(p)
        tails.append([])

        def pump(r=r, p=p):
            for raw in iter(p.stderr.readline, b""):
                line = raw.decode(errors="replace").rstrip("\n")
                tails[r].append(line)
                del tails[r][:-30]
                sys.stderr.write(f"[rank {r}] {line}\n")
                sys.stderr.flush()
        th = threading.Thread(target=pump, daemon=True)
        th.start()
        readers.append(th)
    out0 = b""
    failed = None
    codes = {}
    deadline = time.time() + float(os.environ.get("SK_BENCH_LAUNCH_TIMEOUT", "3000"))
    pending = set(range(n))
    while pending:
        if 0 in pending:
            rd, _, _ = select.select([procs[0].stdout], [], [], 0.2)
            if rd:
                chunk = os.read(procs[0].stdout.fileno(), 1 << 16)
                out0 += chunk
        else:
            time.sleep(0.2)
        for r in list(pending):
            rc = procs[r].poll()
            if rc is None:
                continue
            if r == 0:
                out0 += procs[0].stdout.read() or b""
            pending.discard(r)
            codes[r] = rc
            if rc != 0 and failed is None:
                failed = (r, rc)
        if failed is not None or time.time() > deadline:
            # Only rank 0 binds the rendezvous port: when another process took it, the OTHER ranks can fail first (a refused
            # connection, exit code 1) — give rank 0 a moment to say so itself before the run is judged
            grace = time.time() + 5.0
            while failed is not None and 0 in pending and time.time() < grace:
                rc = procs[0].poll()
                if rc is not None:
                    pending.discard(0)
                    codes[0] = rc
                    break
                time.sleep(0.1)
            for r in pending:                                   # the exact children started above, nothing else
                procs[r].kill()
            for r in pending:
                procs[r].wait()
            if failed is None:
                failed = (-1, 124)
            break
    for th in readers:
        th.join(timeout=2.0)
    if failed is not None:
        if EXIT_PORT_TAKEN in codes.values():
            return EXIT_PORT_TAKEN, b""
        if failed[0] < 0:
            sys.stderr.write(f"[bench] no rank finished within SK_BENCH_LAUNCH_TIMEOUT; still running at the end: {sorted(pending)}\n")
        else:
            sys.stderr.write(f"[bench] rank {failed[0]} failed with exit code {failed[1]}\n")
            for line in tails[failed[0]][-12:]:
                sys.stderr.write(f"[bench]   rank {failed[0]} said: {line}\n")
        return (failed[1] if 0 < failed[1] < 256 else 1), b""
    return 0, out0


def gen_shard(torch, dev, n, table_np, seed, chunk, into=None, sink=None):
    """Synthetic shard on the device (SURVEY.md §8d cfg 4 distributions), generated chunk by chunk.
    `into` = (seq[2], qual[2], bc) preallocated uint8 tensors to fill instead of allocating; `sink(r0, seq[2], qual[2], bc)`
    takes each chunk (rows r0 ...) instead of any big matrices being kept (the blocked layout is packed chunk by chunk)."""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    u8 = torch.uint8
    bases = torch.tensor(list(b"ACGT"), dtype=u8, device=dev)
    alphabet = torch.tensor(list(b"ACGTN"), dtype=u8, device=dev)
    table = torch.tensor(table_np, dtype=u8, device=dev)
    mu = 36.0 - 16.0 * (torch.arange(L_READ, device=dev, dtype=torch.float32) / (L_READ - 1)) ** 2
    if sink is not None:
        seq = qual = bc = None
    elif into is not None:
        seq, qual, bc = into
    else:
        seq = [torch.empty((n, L_READ), dtype=u8, device=dev) for _ in range(2)]
        qual = [torch.empty((n, L_READ), dtype=u8, device=dev) for _ in range(2)]
        bc = torch.empty((n, L_BC), dtype=u8, device=dev)
    for r0 in range(0, n, chunk):
        m = min(chunk, n - r0)
        cs, cq = [], []
        for mi in range(2):
            idx = torch.randint(0, 4, (m, L_READ), generator=g, device=dev)
            s = bases[idx]
            s[torch.rand((m, L_READ), generator=g, device=dev) < 0.005] = ord("N")
            q = torch.randn((m, L_READ), generator=g, device=dev) * 6.0 + mu
            q = (q.round_().clamp_(2, 40) + 33).to(u8)
            if sink is not None:
                cs.append(s)
                cq.append(q)
            else:
                seq[mi][r0:r0 + m] = s
                qual[mi][r0:r0 + m] = q
            del idx, s, q
        b = observed_barcodes(torch, g, dev, m, table, bases, alphabet)
        if sink is not None:
            sink(r0, cs, cq, b)
        else:
            bc[r0:r0 + m] = b
    return seq, qual, bc


def observed_barcodes(torch, g, dev, m, table, bases, alphabet, p_exact=0.85, p_sub=0.10):
    """m observed dual-index barcodes drawn on the device (SURVEY.md §8d cfg 4): a sheet row, then per half p_exact as it is,
    p_sub one substitution (uniform position, uniform from ACGTN other than the letter there), the rest a uniform random 8-mer."""
    truth = torch.randint(0, table.shape[0], (m,), generator=g, device=dev)
    b = table[truth].clone()
    rows = torch.arange(m, device=dev)
    for lo in (0, 9):
        u = torch.rand((m,), generator=g, device=dev)
        sub = (u >= p_exact) & (u < p_exact + p_sub)
        pos = lo + torch.randint(0, 8, (m,), generator=g, device=dev)
        ai = torch.randint(0, 5, (m,), generator=g, device=dev)
        cur = b[rows, pos]
        ai = torch.where(alphabet[ai] == cur, (ai + 1) % 5, ai)
        b[rows[sub], pos[sub]] = alphabet[ai[sub]]
        rnd = u >= p_exact + p_sub
        nr = int(rnd.sum())
        if nr:
            b[rnd, lo:lo + 8] = bases[torch.randint(0, 4, (nr, 8), generator=g, device=dev)]
    return b


def pack_blocked(torch, lay, seq, qual, bc, nt, dst=None):
    """SoA matrices of nt*64 rows -> (input buffer, output buffer) of the tile-blocked layout (device-side byte moves).
    dst = an [nt, in_block] view of an existing input buffer to fill instead (no output buffer is made then)."""
    dev = seq[0].device
    bin_ = torch.zeros(nt * lay.in_block, dtype=torch.uint8, device=dev) if dst is None else None
    v = bin_.view(nt, lay.in_block) if dst is None else dst
    row = 64 * lay.stride
    for i in range(lay.n_mates):
        v[:, lay.in_qual[i]:lay.in_qual[i] + row] = qual[i].view(nt, row)
        if lay.in_seq[i] >= 0:
            v[:, lay.in_seq[i]:lay.in_seq[i] + row] = seq[i].view(nt, row)
    if lay.in_bc >= 0:
        v[:, lay.in_bc:lay.in_bc + 64 * lay.bc_stride] = bc.view(nt, 64 * lay.bc_stride)
    if dst is not None:
        return None, None
    bout = torch.empty(nt * lay.out_block, dtype=torch.uint8, device=dev)
    return bin_, bout


def unpack_blocked(torch, lay, bout, nt):
    """The first nt tiles of a blocked output buffer as SoA tensors (copies)."""
    v = bout[:nt * lay.out_block].view(nt, lay.out_block)
    row = 64 * lay.stride
    res = {"out_seq": [], "lowest_k": []}
    for i in range(lay.n_mates):
        if lay.out_seq[i] >= 0:
            res["out_seq"].append(v[:, lay.out_seq[i]:lay.out_seq[i] + row].reshape(nt * 64, lay.stride))
        if lay.out_lowest_k[i] >= 0:
            res["lowest_k"].append(v[:, lay.out_lowest_k[i]:lay.out_lowest_k[i] + 128].contiguous().view(torch.int16).reshape(nt * 64))
    if lay.out_assign >= 0:
        res["assign"] = v[:, lay.out_assign:lay.out_assign + 256].contiguous().view(torch.int32).reshape(nt * 64)
    return res


def dump_outputs(torch, out_dir, n, counts, lay=None, bout=None, assign=None, lowest_k=None, out_seq=None):
    """--dump-outputs: what the last timed step handed its caller, as float32 / float64 .npy files (exact: every value is an
    integer below 2^24, or 2^53 for the float64 sums).  counts = the u64[S+3] counters; rows = DUMP_ROWS clusters of this shard
    drawn with DUMP_SEED (sorted), with their assign, lowest_k [mate] and out_seq [mate][150]; over the whole shard, per mate:
    the byte sum and the 'N' count of every out_seq column, and the histogram of lowest_k (bin 151: anything above 150).
    SoA: assign / lowest_k / out_seq are the timed pass's tensors; blocked: its output buffer bout, read through the layout."""
    os.makedirs(out_dir, exist_ok=True)
    dev = counts.device

    def soa(r0, r1):
        """(assign, [lowest_k], [out_seq]) of rows r0:r1 (r0 a multiple of 64)"""
        if lay is None:
            return assign[r0:r1], [x[r0:r1] for x in lowest_k], [x[r0:r1] for x in out_seq]
        t0, t1 = r0 // 64, (r1 + 63) // 64
        u = unpack_blocked(torch, lay, bout[t0 * lay.out_block:t1 * lay.out_block], t1 - t0)
        m = r1 - r0
        return u["assign"][:m], [x[:m] for x in u["lowest_k"]], [x[:m] for x in u["out_seq"]]

    rows = np.sort(np.random.default_rng(DUMP_SEED).choice(n, size=min(DUMP_ROWS, n), replace=False))
    idx = torch.from_numpy(rows).to(dev)
    if lay is None:
        s_assign, s_k, s_seq = assign[idx], [x[idx] for x in lowest_k], [x[idx] for x in out_seq]
    else:
        tiles, inv = torch.unique(idx // 64, return_inverse=True)
        u = unpack_blocked(torch, lay, bout.view(-1, lay.out_block)[tiles].reshape(-1), tiles.numel())
        pos = inv * 64 + idx % 64
        s_assign, s_k, s_seq = u["assign"][pos], [x[pos] for x in u["lowest_k"]], [x[pos] for x in u["out_seq"]]
    col_sum = torch.zeros((2, L_READ), dtype=torch.int64, device=dev)
    col_n = torch.zeros((2, L_READ), dtype=torch.int64, device=dev)
    k_hist = torch.zeros((2, L_READ + 2), dtype=torch.int64, device=dev)
    chunk = 1 << 22
    for r0 in range(0, n, chunk):
        _, ks, ss = soa(r0, min(r0 + chunk, n))
        for i in range(2):
            col_sum[i] += ss[i].sum(0, dtype=torch.int64)
            col_n[i] += (ss[i] == ord("N")).sum(0)
            k = (ks[i].to(torch.int64) & 0xFFFF).clamp_(max=L_READ + 1)
            k_hist[i] += torch.bincount(k, minlength=L_READ + 2)
    arrays = {"counts": (counts.cpu().numpy(), np.float64), "rows": (rows, np.float64),
              "assign": (s_assign.cpu().numpy(), np.float32),
              "lowest_k": (np.stack([x.cpu().numpy().view(np.uint16) for x in s_k]), np.float32),
              "out_seq": (np.stack([x.cpu().numpy() for x in s_seq]), np.float32),
              "out_seq_column_sum": (col_sum.cpu().numpy(), np.float64), "out_seq_column_n": (col_n.cpu().numpy(), np.float64),
              "lowest_k_hist": (k_hist.cpu().numpy(), np.float64)}
    for name, (a, dt) in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a.astype(dt))


def usable_cores() -> int:
    """Cores this process may actually use: the affinity mask, cut by the cgroup's CPU quota when there is one."""
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    for path in ("/sys/fs/cgroup/cpu.max",):
        try:
            quota, period = open(path).read().split()[:2]
            if quota != "max":
                n = min(n, max(1, int(int(quota) / int(period))))
        except (OSError, ValueError):
            pass
    try:                                                    # cgroup v1
        q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
        per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
        if q > 0 and per > 0:
            n = min(n, max(1, q // per))
    except (OSError, ValueError):
        pass
    return max(1, n)


def library_digest() -> str:
    import seqkit_amd
    h = hashlib.sha256()
    with open(seqkit_amd.library_path(), "rb") as f:
        for blk in iter(lambda: f.read(1 << 20), b""):
            h.update(blk)
    return h.hexdigest()[:16]


def kernel_sources_digest() -> str:
    """Digest of everything libseqkit_hip.so is built from — kernels, launch code, the ABI layer, headers and the compiler
    flags: the PMC traffic record in profiles/ is only quoted for the build it was measured on."""
    from seqkit_amd import build
    return build.library_inputs_digest()


COLD_TRAFFIC = 512 << 20        # bytes of OTHER traffic between two uses of one buffer set (twice the 256 MiB Infinity Cache)


def cold_sets(footprint_bytes):
    """How many distinct input/output sets a call of this footprint needs so that, rotating over them, every set is met again
    only after >= COLD_TRAFFIC bytes of other sets went by: what it reads then comes from HBM, not from the Infinity Cache."""
    return int(-(-COLD_TRAFFIC // max(int(footprint_bytes), 1))) + 1


def measure_rotating(torch, ctx, dev, calls, rounds=5, warm=1):
    """Time `calls` (one closure per buffer set) in rotation on the ctx stream, ONE HIP event pair per call, nothing else between
    the pairs and no host synchronisation inside a round (the queue stays full: launch latency is not what is timed).  With
    len(calls) = cold_sets(footprint) a call never finds its bytes on-die.  Returns the median of the per-call durations (ms)."""
    stream = torch.cuda.ExternalStream(ctx.stream(), device=dev)
    torch.cuda.synchronize()
    ts = []
    with torch.cuda.stream(stream):
        for _ in range(warm):
            for fn in calls:
                fn()
        ctx.sync()
        for _ in range(rounds):
            evs = []
            for fn in calls:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fn()
                e1.record(stream)
                evs.append((e0, e1))
            ctx.sync()
            ts += [e0.elapsed_time(e1) for e0, e1 in evs]
    ts.sort()
    return ts[len(ts) // 2]


def secondary_rates(torch, ctx, dev):
    """extra.rates: device-resident rates of the other BASELINE configs on this GPU, a few ms each, outside the timed
    region.  Same workloads as tools/rates.py; `frac` is algorithmic bytes / time / 8 TB/s."""
    from seqkit_amd import capi, synth
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    out = []

    def measure(fn, iters, rounds):
        torch.cuda.synchronize()                 # the inputs were made on torch's stream; fn runs on the ctx stream
        for _ in range(2):
            fn()
        ctx.sync()
        ts = []
        for _ in range(rounds):
            ctx.timer_start()
            for _ in range(iters):
                fn()
            ts.append(ctx.timer_stop() / iters)
        return sorted(ts)[len(ts) // 2]

    def timeit(name, fn, units, bpu, iters=10, rounds=3, cands=None, sets=None, many=None):
        """cands = {array name: [candidate tensors with the same contents]} and fn(choice) — the streaming kernels are then also
        timed with the placement of their arrays chosen (one array at a time swapped for its other candidates, as
        sk_fused_tune_placement_dev does for the fused pass): `frac` is the chosen placement, `frac_as_placed` the first candidates.
        sets = one closure per distinct buffer set (cold_sets(footprint) of them) for a call whose bytes would fit the 256 MiB
        Infinity Cache: `frac` is then the call with its rows coming from HBM (rotation over the sets, one event pair per call),
        `frac_pipelined` the same rotation inside ONE event pair (launches overlap as in a stream of calls), `frac_warm` the
        call replayed on one set (what rounds 1-4 reported for these rows: an on-die number)."""
        first = None
        if sets is not None:
            warm = measure(sets[0], iters, rounds)
            ms = measure_rotating(torch, ctx, dev, sets, rounds=5)
            stream = torch.cuda.ExternalStream(ctx.stream(), device=dev)
            ts = []
            for _ in range(3):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                with torch.cuda.stream(stream):
                    e0.record(stream)
                    for f in sets:
                        f()
                    e1.record(stream)
                ctx.sync()
                ts.append(e0.elapsed_time(e1) / len(sets))
            piped = sorted(ts)[1]
            many_ms = many_piped = None
            if many is not None:
                # the same buffer sets through the many-batch entry point (sk_demux_assign_many_dev / sk_trim_by_quality_many_dev): ONE call,
                # one event pair around it; per batch = the call / len(sets)
                tm = []
                many()
                ctx.sync()
                for _ in range(5):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    with torch.cuda.stream(stream):
                        e0.record(stream)
                        many()
                        e1.record(stream)
                    ctx.sync()
                    tm.append(e0.elapsed_time(e1) / len(sets))
                many_ms = sorted(tm)[2]
                # ... and three such calls inside one event pair (as "pipelined" for the single calls: the host's part of a call hides behind
                # the launch before it)
                tm = []
                for _ in range(3):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    with torch.cuda.stream(stream):
                        e0.record(stream)
                        for _k in range(3):
                            many()
                        e1.record(stream)
                    ctx.sync()
                    tm.append(e0.elapsed_time(e1) / (3 * len(sets)))
                many_piped = sorted(tm)[1]
        elif cands is None:
            ms = measure(fn, iters, rounds)
        else:
            choice = {k: 0 for k in cands}
            first = best = measure(lambda: fn(choice), iters, 1)
            for _ in range(2):
                moved = False
                for k, lst in cands.items():
                    for j in range(len(lst)):
                        if j == choice[k]:
                            continue
                        trial = dict(choice, **{k: j})
                        t = measure(lambda: fn(trial), iters, 1)
                        if t < best * 0.998:
                            best, choice, moved = t, trial, True
                if not moved:
                    break
            ms = measure(lambda: fn(choice), iters, rounds)
        gbs = units * bpu / ms / 1e6
        row = {"config": name, "ms": round(ms, 4), "G_units_per_s": round(units / ms / 1e6, 2), "bytes_per_unit": bpu,
               "GBps": round(gbs, 1), "frac": round(gbs / HBM_PEAK_GBS, 4)}
        if first is not None:
            row["frac_as_placed"] = round(units * bpu / first / 1e6 / HBM_PEAK_GBS, 4)
        if sets is not None:
            row.update({"rows_from": f"HBM: rotation over {len(sets)} buffer sets, one event pair per call",
                        "ms_pipelined": round(piped, 4), "frac_pipelined": round(units * bpu / piped / 1e6 / HBM_PEAK_GBS, 4),
                        "ms_warm": round(warm, 4), "frac_warm": round(units * bpu / warm / 1e6 / HBM_PEAK_GBS, 4)})
            if many_ms is not None:
                row.update({"ms_many": round(many_ms, 4), "frac_many": round(units * bpu / many_ms / 1e6 / HBM_PEAK_GBS, 4),
                            "ms_many_pipelined": round(many_piped, 4), "frac_many_pipelined": round(units * bpu / many_piped / 1e6 / HBM_PEAK_GBS, 4),
                            "many": f"the {len(sets)} buffer sets as the batches of ONE many-batch call (rows from HBM), per batch; pipelined: three such calls inside one event pair"})
        out.append(row)

    n = 16_000_000
    q = torch.randint(35, 74, (n, 150), dtype=torch.uint8, device=dev, generator=g)
    s = torch.randint(65, 85, (n, 150), dtype=torch.uint8, device=dev, generator=g)
    o = torch.empty_like(s)
    lk = torch.empty((n,), dtype=torch.int16, device=dev)
    mc = {"seq": [s, s.clone(), s.clone()], "qual": [q, q.clone(), q.clone()], "out": [o, torch.empty_like(o), torch.empty_like(o)]}
    timeit("cfg1 shape: mask by quality 16M x 150bp",
           lambda ch: ctx.mask_by_quality_dev(mc["seq"][ch["seq"]].data_ptr(), mc["qual"][ch["qual"]].data_ptr(), 150, n, 20, mc["out"][ch["out"]].data_ptr()),
           n, 450, cands=mc)
    del mc
    timeit("cfg2 worst case: trim by quality 16M x 150bp, uniform Q2-Q40 (no early break)",
           lambda: ctx.trim_by_quality_dev(q.data_ptr(), 0, 150, n, 20, lk.data_ptr()), n, 152)
    k = cold_sets(1_000_000 * 152)                  # 1 M-row slices of the 16 M-row matrix, each met again after >= 512 MiB of the others
    timeit("cfg2: trim by quality 1M x 150bp, uniform Q2-Q40", None, 1_000_000, 152,
           sets=[(lambda i=i: ctx.trim_by_quality_dev(q[i * 1_000_000:].data_ptr(), 0, 150, 1_000_000, 20, lk[i * 1_000_000:].data_ptr())) for i in range(k)],
           many=lambda: ctx.trim_by_quality_many_dev([(q[i * 1_000_000:].data_ptr(), 0, 1_000_000, lk[i * 1_000_000:].data_ptr()) for i in range(k)], 150, 20))
    mu = 36.0 - 16.0 * (torch.arange(150, device=dev, dtype=torch.float32) / 149) ** 2
    for r0 in range(0, n, 2_000_000):
        q[r0:r0 + 2_000_000] = ((torch.randn((2_000_000, 150), generator=g, device=dev) * 6.0 + mu).round_().clamp_(2, 40) + 33).to(torch.uint8)
    timeit("cfg2 read-like qualities: trim by quality 16M x 150bp", lambda: ctx.trim_by_quality_dev(q.data_ptr(), 0, 150, n, 20, lk.data_ptr()), n, 152)
    # The fused pass in the forms BASELINE.md §3 names beside the paired headline: single-end 150 bp with an 8 bp barcode out of
    # 16 (the fused form of configs[2], 308 B read + 156 B written = 464 B/read), the same with ragged rows (a u16 length
    # column, +2 B), and the paired dual-index pass with the detail columns of matched rows (lowest_diff u8, first / last i16: +5 B).
    table = synth.make_sheet(16, 8, dual=False, seed=3)
    ctx.set_barcodes(table, 1)
    bc_np, _ = synth.observe_barcodes(table, 1_000_000, seed=3)
    bc1 = torch.from_numpy(bc_np).to(dev).repeat(16, 1).contiguous()
    assign = torch.empty((n,), dtype=torch.int32, device=dev)
    cnt = torch.zeros((16 + 3,), dtype=torch.int64, device=dev)
    # (the fused rows choose the placement of their big matrices among three candidates each, like the headline and the other
    # streaming rows: `frac` is the chosen placement, `frac_as_placed` the first candidates — one box's buffers as they come time
    # this pass 12 % apart from another's)
    fc = {"seq": [s, s.clone(), s.clone()], "qual": [q, q.clone(), q.clone()], "out": [o, torch.empty_like(o), torch.empty_like(o)]}

    def mate_of(ch, ln_ptr=0):
        return {"seq": fc["seq"][ch["seq"]].data_ptr(), "qual": fc["qual"][ch["qual"]].data_ptr(), "len": ln_ptr, "out_seq": fc["out"][ch["out"]].data_ptr(), "lowest_k": lk.data_ptr()}
    timeit("fused single-end: demultiplex + trim + mask, 16M x 150bp + 8bp, 16 barcodes",
           lambda ch: ctx.fused_pass_dev(n, 150, 20, [mate_of(ch)], bc=bc1.data_ptr(), bc_stride=8, assign=assign.data_ptr(), counts=cnt.data_ptr()), n, 464, cands=fc)
    ln = torch.randint(100, 151, (n,), dtype=torch.int16, device=dev, generator=g)
    timeit("fused single-end, ragged rows (u16 lengths 100-150): 16M x <=150bp + 8bp, 16 barcodes",
           lambda ch: ctx.fused_pass_dev(n, 150, 20, [mate_of(ch, ln.data_ptr())], bc=bc1.data_ptr(), bc_stride=8, assign=assign.data_ptr(), counts=cnt.data_ptr()), n, 466, cands=fc)
    del bc1, ln
    table = synth.make_sheet(96, 8, dual=True, seed=4)
    ctx.set_barcodes(table, 1)
    bc_np, _ = synth.observe_barcodes(table, 1_000_000, seed=4, halves=2)
    bc2 = torch.from_numpy(bc_np).to(dev).repeat(16, 1).contiguous()
    s2, q2 = s.flip(0).contiguous(), q.flip(0).contiguous()
    o2 = torch.empty_like(o)
    lk2 = torch.empty_like(lk)
    low = torch.empty((n,), dtype=torch.uint8, device=dev)
    first = torch.empty((n,), dtype=torch.int16, device=dev)
    last = torch.empty((n,), dtype=torch.int16, device=dev)
    cnt2 = torch.zeros((96 + 3,), dtype=torch.int64, device=dev)
    fc.update({"seq2": [s2, s2.clone(), s2.clone()], "qual2": [q2, q2.clone(), q2.clone()], "out2": [o2, torch.empty_like(o2), torch.empty_like(o2)]})

    def mates_of(ch):
        return [mate_of(ch), {"seq": fc["seq2"][ch["seq2"]].data_ptr(), "qual": fc["qual2"][ch["qual2"]].data_ptr(), "len": 0, "out_seq": fc["out2"][ch["out2"]].data_ptr(),
                              "lowest_k": lk2.data_ptr()}]
    ctx.set_detail_mode(capi.SK_DETAIL_MATCHED)
    timeit("fused paired with the detail columns of matched clusters (SK_DETAIL_MATCHED): 16M x 2x150bp, 96 dual-index",
           lambda ch: ctx.fused_pass_dev(n, 150, 20, mates_of(ch), bc=bc2.data_ptr(), bc_stride=17, assign=assign.data_ptr(), lowest_diff=low.data_ptr(),
                                         first_idx=first.data_ptr(), last_idx=last.data_ptr(), counts=cnt2.data_ptr()), n, 930, cands=fc)
    del fc
    ctx.set_detail_mode(capi.SK_DETAIL_FULL)
    del q, s, o, lk, s2, q2, o2, lk2, bc2, low, first, last, assign, cnt, cnt2
    n = 10_000_000
    table = synth.make_sheet(16, 8, dual=False, seed=3)
    ctx.set_barcodes(table, 1)
    bc_np, _ = synth.observe_barcodes(table, 1_000_000, seed=3)
    bc = torch.from_numpy(bc_np).to(dev).repeat(10, 1).contiguous()
    assign = torch.empty((n,), dtype=torch.int32, device=dev)

    def demux_sets(bc, L, bpu, detail=False):
        """cold_sets(n x bpu) copies of the barcode matrix, each with output columns of its own"""
        k = cold_sets(n * bpu)
        keep = []
        calls = []
        for i in range(k):
            b = bc if i == 0 else bc.clone()
            o = [torch.empty((n,), dtype=torch.int32, device=dev)]
            if detail:
                o += [torch.empty((n,), dtype=torch.uint8, device=dev), torch.empty((n,), dtype=torch.int16, device=dev), torch.empty((n,), dtype=torch.int16, device=dev)]
            keep.append((b, o))
            calls.append(lambda b=b, o=o: ctx.demux_assign_dev(b.data_ptr(), L, n, *[x.data_ptr() for x in o]))
        calls_many = lambda: ctx.demux_assign_many_dev([(b.data_ptr(), n, *[x.data_ptr() for x in o]) for b, o in keep], L)
        return calls, (keep, calls_many)

    calls, keep = demux_sets(bc, 8, 12)
    timeit("cfg3: demultiplex 10M x 8bp, 16 barcodes", None, n, 12, sets=calls, many=keep[1])
    # what `fasta demultiplex` asks for: the decision plus lowest_diff / first / last of the reads that matched something
    low = torch.empty((n,), dtype=torch.uint8, device=dev)
    first = torch.empty((n,), dtype=torch.int16, device=dev)
    last = torch.empty((n,), dtype=torch.int16, device=dev)
    ctx.set_detail_mode(capi.SK_DETAIL_MATCHED)
    calls, keep = demux_sets(bc, 8, 17, detail=True)
    timeit("cfg3 with the detail columns of matched reads (SK_DETAIL_MATCHED, as the fasta demultiplex host calls it), 10M x 8bp", None, n, 17, sets=calls, many=keep[1])
    del calls, keep
    ctx.set_detail_mode(capi.SK_DETAIL_FULL)
    bc_l = bc.repeat(10, 1).contiguous()          # the same sheet on a call ten times as long: what the lookup does once the launch is out of the way
    assign_l = torch.empty((10 * n,), dtype=torch.int32, device=dev)
    lc = {"bc": [bc_l, bc_l.clone(), bc_l.clone()], "assign": [assign_l, torch.empty_like(assign_l), torch.empty_like(assign_l)]}
    timeit("cfg3 sheet, 100M x 8bp in one call", lambda ch: ctx.demux_assign_dev(lc["bc"][ch["bc"]].data_ptr(), 8, 10 * n, lc["assign"][ch["assign"]].data_ptr()), 10 * n, 12, iters=3, cands=lc)
    del bc_l, assign_l, lc
    table = synth.make_sheet(96, 8, dual=True, seed=4)
    ctx.set_barcodes(table, 1)
    bc_np, _ = synth.observe_barcodes(table, 1_000_000, seed=4, halves=2)
    bc = torch.from_numpy(bc_np).to(dev).repeat(10, 1).contiguous()
    calls, keep = demux_sets(bc, 17, 21)
    timeit("demultiplex only 10M x 17ch, 96 dual-index", None, n, 21, sets=calls, many=keep[1])
    ctx.set_detail_mode(capi.SK_DETAIL_MATCHED)
    calls, keep = demux_sets(bc, 17, 26, detail=True)
    timeit("96 dual-index with the detail columns of matched reads (SK_DETAIL_MATCHED), 10M x 17ch", None, n, 26, sets=calls, many=keep[1])
    ctx.set_detail_mode(capi.SK_DETAIL_FULL)
    bc_l = bc.repeat(10, 1).contiguous()
    assign_l = torch.empty((10 * n,), dtype=torch.int32, device=dev)
    lc = {"bc": [bc_l, bc_l.clone(), bc_l.clone()], "assign": [assign_l, torch.empty_like(assign_l), torch.empty_like(assign_l)]}
    timeit("96 dual-index, 100M x 17ch in one call", lambda ch: ctx.demux_assign_dev(lc["bc"][ch["bc"]].data_ptr(), 17, 10 * n, lc["assign"][ch["assign"]].data_ptr()), 10 * n, 21, iters=3, cands=lc)
    del bc_l, assign_l, calls, keep, lc
    # the 96 dual-index sheet with every other sample typed in lower case — nine letters and the separator, where the table's
    # 3-bit classes hold seven (the reference compares raw bytes, src/fasta_demultiplex.rs:273-274, so such a sheet is legal).
    # Through round 4 it ran the S x L matchers (demux_tile_kernel: VALU-bound, ~350 instructions per read, 0.15-0.19); since round 5
    # it gets 4-bit classes and the factored form (sk_lut.h, "Wide classes") — the row says which, from sk_barcode_table_info.
    table_mc = table.copy()
    table_mc[1::2] = np.where((table_mc[1::2] >= 65) & (table_mc[1::2] <= 90), table_mc[1::2] + 32, table_mc[1::2])
    ctx.set_barcodes(table_mc, 1)
    bc_mc = bc.clone()
    odd = torch.arange(n, device=dev) % 2 == 1                  # (half of the reads in lower case too, so that both halves of the sheet are matched)
    bc_mc[odd] = torch.where((bc_mc[odd] >= 65) & (bc_mc[odd] <= 90), bc_mc[odd] + 32, bc_mc[odd])
    calls, keep = demux_sets(bc_mc, 17, 21)
    kind = ctx.barcode_table_info()["kind"]
    served = ("the matchers" if kind == capi.SK_TABLE_NONE else ("looked up half by half" if kind & capi.SK_TABLE_FACTORED else "full-key table")
              + (", wide classes" if kind & capi.SK_TABLE_WIDE_CLASSES else ""))
    timeit(f"demultiplex only 10M x 17ch, 96 dual-index, a mixed-case sheet (9 letters: {served})", None, n, 21, sets=calls)
    del calls, keep, bc_mc, odd
    # four plates: 384 dual-index samples (24 x 16 combinations).  The full-key table would be 512 KiB, so the sheet is looked
    # up half by half from LDS (sk_lut.h, the factored form)
    table = synth.make_sheet(384, 8, dual=True, seed=384)
    ctx.set_barcodes(table, 1)
    bc_np, _ = synth.observe_barcodes(table, 1_000_000, seed=4, halves=2)
    bc = torch.from_numpy(bc_np).to(dev).repeat(10, 1).contiguous()
    calls, keep = demux_sets(bc, 17, 21)
    timeit("demultiplex only 10M x 17ch, 384 dual-index (four plates)", None, n, 21, sets=calls, many=keep[1])
    del bc, assign, low, first, last, calls, keep
    n = 200_000_000
    flag_np, tid_np, mtid_np, tlen_np = synth.make_bam_cores(2_000_000, seed=5)
    flag = torch.from_numpy(flag_np.view(np.int16)).to(dev).repeat(100)
    tid = torch.from_numpy(tid_np).to(dev).repeat(100)
    mtid = torch.from_numpy(mtid_np).to(dev).repeat(100)
    tlen = torch.from_numpy(tlen_np).to(dev).repeat(100)
    outb = torch.zeros((4 + 5001,), dtype=torch.int64, device=dev)
    bcand = {"flag": [flag, flag.clone(), flag.clone()], "tid": [tid, tid.clone(), tid.clone()], "mtid": [mtid, mtid.clone(), mtid.clone()],
             "tlen": [tlen, tlen.clone(), tlen.clone()]}
    timeit("cfg5: sam statistics + fragment lengths 200M records",
           lambda ch: ctx.bam_flag_tlen_dev(bcand["flag"][ch["flag"]].data_ptr(), bcand["tid"][ch["tid"]].data_ptr(), bcand["mtid"][ch["mtid"]].data_ptr(),
                                            bcand["tlen"][ch["tlen"]].data_ptr(), n, 5000, outb.data_ptr()), n, 14, iters=3, cands=bcand)
    bits = torch.empty(((n + 7) // 8,), dtype=torch.uint8, device=dev)
    kept = torch.zeros((1,), dtype=torch.int64, device=dev)
    timeit("f2: sam fragments filter 200M records", lambda: ctx.bam_fragments_dev(flag.data_ptr(), tid.data_ptr(), mtid.data_ptr(), tlen.data_ptr(), n, 0, 5000,
                                                                                  bits.data_ptr(), kept.data_ptr()), n, 14.125, iters=3)
    del flag, tid, mtid, tlen, bcand, bits, kept
    # f4: sequence() of `sam to fastq`: 4-bit bases -> ASCII, reverse complement, q < 10 -> N
    n = 16_000_000
    s4 = torch.randint(0, 256, (n, 76), dtype=torch.uint8, device=dev, generator=g)
    q = torch.randint(0, 42, (n, 152), dtype=torch.uint8, device=dev, generator=g)
    ln = torch.full((n,), 150, dtype=torch.int16, device=dev)
    fl = torch.randint(0, 2, (n,), dtype=torch.int16, device=dev, generator=g) * 16
    o = torch.empty((n, 152), dtype=torch.uint8, device=dev)
    sc = {"seq4": [s4, s4.clone(), s4.clone()], "qual": [q, q.clone(), q.clone()], "out": [o, torch.empty_like(o), torch.empty_like(o)]}
    timeit("f4: sequence() 16M x 150 bases, both strands",
           lambda ch: ctx.bam_sequence_dev(sc["seq4"][ch["seq4"]].data_ptr(), 76, sc["qual"][ch["qual"]].data_ptr(), 152, ln.data_ptr(), fl.data_ptr(), n, 10,
                                           sc["out"][ch["out"]].data_ptr()),
           n, 76 + 152 + 152 + 4, iters=5, cands=sc)
    del s4, q, ln, fl, o, sc
    # f3: barcode census (`fasta statistics`, `--dry-run`): rows/s.  Every launch starts from an empty table, and emptying it is
    # part of the job: `ms` is the count alone (one event pair around sk_census_add_dev), `reset_ms` the sk_census_reset before it,
    # `reset_plus_count_ms` both inside one event pair.  The rows whose inputs are drawn independently are the census figure;
    # rounds 3-5 quoted one million drawn rows repeated 32 times (kept below them): their random halves come back 32 times each —
    # 110 k distinct keys in 32 M rows where the independent noisy mix has 1.6 M.
    table = synth.make_sheet(96, 8, dual=True, seed=4)
    ctx.set_barcodes(table, 1)

    def census_row(name, bc, L, reps=5):
        torch.cuda.synchronize()
        ts, rs, both = [], [], []
        for _ in range(reps):
            ctx.sync()
            ctx.timer_start()
            ctx.census_reset()
            rs.append(ctx.timer_stop())
            ctx.timer_start()
            ctx.census_add_dev(bc.data_ptr(), bc.shape[1], L, bc.shape[0], 0, 0)
            ts.append(ctx.timer_stop())
        for _ in range(3):
            ctx.sync()
            ctx.timer_start()
            ctx.census_reset()
            ctx.census_add_dev(bc.data_ptr(), bc.shape[1], L, bc.shape[0], 0, 0)
            both.append(ctx.timer_stop())
        ms, rms, bms = sorted(ts[1:])[len(ts[1:]) // 2], sorted(rs[1:])[len(rs[1:]) // 2], sorted(both)[1]
        rows = bc.shape[0]
        out.append({"config": name, "ms": round(ms, 4), "G_units_per_s": round(rows / ms / 1e6, 2), "bytes_per_unit": L,
                    "GBps": round(rows * L / ms / 1e6, 1), "frac": round(rows * L / ms / 1e6 / HBM_PEAK_GBS, 4),
                    "reset_ms": round(rms, 4), "reset_plus_count_ms": round(bms, 4),
                    "G_units_per_s_with_reset": round(rows / bms / 1e6, 2), "distinct": int(ctx.census_stats()["distinct"])})

    bases_t = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
    alpha_t = torch.tensor(list(b"ACGTN"), dtype=torch.uint8, device=dev)
    table_t = torch.tensor(table, dtype=torch.uint8, device=dev)
    for name, kw in (("f3: census 32M independently drawn rows, clean mix (97 % / 2.5 % / 0.5 % per index)", dict(p_exact=0.97, p_sub=0.025)),
                     ("f3: census 32M independently drawn rows, noisy mix (85 % / 10 % / 5 % per index)", {})):
        gi = torch.Generator(device=dev)
        gi.manual_seed(11)
        bc = torch.cat([observed_barcodes(torch, gi, dev, 4_000_000, table_t, bases_t, alpha_t, **kw) for _ in range(8)]).contiguous()
        census_row(name, bc, 17)
        del bc
    for name, kw in (("f3: census 32M rows (1 M drawn rows x 32: rounds 3-5's input), clean run (per index 97 % exact, 2.5 % one substitution, 0.5 % random)", dict(p_exact=0.97, p_sub=0.025)),
                     ("f3: census 32M rows (1 M drawn rows x 32: rounds 3-5's input), noisy run (per index 85 % / 10 % / 5 %)", {})):
        b_np, _ = synth.observe_barcodes(table, 1_000_000, seed=4, halves=2, **kw)
        bc = torch.from_numpy(b_np).to(dev).repeat(32, 1).contiguous()
        census_row(name, bc, 17)
        del bc
    # the floor of the census: every row a key never seen before (random 16-mers: 32 M distinct keys; level 1 of the table holds the first
    # four million, the rest go through to level 2 — and the reset behind such a launch clears level 2 as well)
    rows = 32_000_000
    bc = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)[torch.randint(0, 4, (rows, 16), device=dev, generator=g)].contiguous()
    census_row("f3: census 32M rows, every row a new key (random 16-mers)", bc, 16, reps=3)
    del bc
    ctx.census_reset()
    ctx.sync()
    return out


def bam_file_rows(ctx):
    """extra.bam_files: config 5 on a FILE — `sam statistics` + `sam fragment lengths` from the BGZF bytes (sk_bam_file_reduce: the compressed
    file crosses PCIe, the device inflates, walks the records and reduces) — on two synthetic BAMs, checked against the oracle's
    reduction of the same records.  `ms` is the whole call, file (page cache) to counters; the kernel's own rates are
    tools/r06/inflate_rate.py's."""
    import shutil
    import tempfile
    import time
    from oracle import oracle as orc
    from seqkit_amd import synth
    rows = []
    d = tempfile.mkdtemp(prefix="sk_bench_bam_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        for kind, n_rec, what in (("random", 4_000_000, "bases and qualities drawn uniformly: literals, 1.5 : 1 (an inflater's worst case)"),
                                  ("sorted", 8_000_000, "reads of a small genome in position order, binned qualities: 5 : 1")):
            path = os.path.join(d, kind + ".bam")
            n, flag, tid, mtid, tlen, reps = synth.write_bam_file(path, n_rec, seed=5, kind=kind)
            e_counters, e_hist, e_total = orc.bam_flag_tlen(flag, tid, mtid, tlen, 5000)
            ts, last = [], None
            for _ in range(4):
                t0 = time.perf_counter()
                last = ctx.bam_file_reduce(path, 5000)
                ts.append((time.perf_counter() - t0) * 1e3)
            handled, counters, hist, total, info = last
            ok = bool(handled) and (counters == e_counters * np.uint64(reps)).all() and (hist == e_hist * np.uint64(reps)).all() and total == e_total * reps
            ms = sorted(ts[1:])[1]
            rows.append({"config": f"cfg5 on a file: sam statistics + fragment lengths, {n // 1_000_000} M-record BAM ({what}), file to counters",
                         "ms": round(ms, 2), "M_records_per_s": round(n / ms / 1e3, 2), "compressed_GBps": round(info[0] / ms / 1e6, 2),
                         "inflated_GBps": round(info[1] / ms / 1e6, 2), "compressed_bytes": int(info[0]), "inflated_bytes": int(info[1]),
                         "bgzf_blocks": int(info[2]), "blocks_inflated_by_zlib_on_the_host": int(info[4]), "walk_rounds": int(info[5]),
                         "read_and_copy_ms": round(info[6], 2), "device_tail_ms": round(info[7], 2), "matches_oracle": bool(ok)})
    finally:
        shutil.rmtree(d, ignore_errors=True)
    return rows


def faithful_cpu(n_reads):
    """cpu_baseline.faithful: the line-at-a-time oracle CLI — same loops as the reference's commands,
    one thread — end to end on cfg 2 / cfg 3 text, stdout to /dev/null (per-sample gzip children included for
    demultiplex, as the reference spawns them)."""
    from oracle import oracle as orc
    from seqkit_amd import synth
    orc.build()
    d = tempfile.mkdtemp(prefix="sk_faithful_")
    res = {}
    try:
        nb = min(n_reads, 100_000)
        reps = max(1, n_reads // nb)
        seq, qual = synth.make_reads(nb, 150, seed=2)
        qual = synth.add_forced_classes(qual, seed=2)
        table = synth.make_sheet(16, 8, dual=False, seed=3)
        bc, _ = synth.observe_barcodes(table, nb, seed=3)
        headers = [f"@SIM:3:{i} 1:N:0".encode() + b" BC:" + bc[i].tobytes() for i in range(nb)]
        block = synth.fastq_text(seq, qual, headers=headers)
        fq = os.path.join(d, "in.fq")
        with open(fq, "wb") as f:
            for _ in range(reps):
                f.write(block)
        sheet = os.path.join(d, "sheet.tsv")
        with open(sheet, "wb") as f:
            for i in range(16):
                f.write(f"S{i:02d}\t".encode() + table[i].tobytes() + b"\n")
        n = nb * reps
        for key, argv in (("cfg2_trim_by_quality", ["trim", "by", "quality", fq, "20"]),
                          ("cfg1_mask_by_quality", ["mask", "by", "quality", fq, "20"]),
                          ("cfg3_demultiplex_16", ["demultiplex", sheet, fq])):
            t0 = time.perf_counter()
            r = subprocess.run([orc.FASTA_BIN] + argv, cwd=d, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            dt = time.perf_counter() - t0
            res[key] = {"M_reads_per_s": round(n / dt / 1e6, 3), "seconds": round(dt, 2), "reads": n, "rc": r.returncode}
        res["what"] = ("oracle CLI (C restatement of the reference's line-at-a-time command loops, 1 thread; demultiplex with its gzip "
                       "children), 150 bp text FASTQ -> /dev/null; not the Rust binary")
    finally:
        import shutil
        shutil.rmtree(d, ignore_errors=True)
    return res


def join_count_reduce(dist, rank, world, make_unique_id, init_rank, ready=None, timeout_s=None):
    """The ranks agree on how the counters are summed.  sk_comm_init_rank blocks until EVERY rank has called it, so nobody
    calls it before all ranks have said they can: (1) every rank makes its rank-local check (`ready`: librccl loadable, device
    bindable) and the answers are gathered; (2) rank 0 makes the communicator id (sk_comm_get_unique_id) and every rank gets
    it over the rendezvous backend; (3) all join.  Should any rank fail at (1) or (2), ALL ranks learn of it BEFORE the
    bootstrap and fall back together to a gloo sum with a host round trip — the JSON line then says so; a scaling run still
    gets numbers.  A join that RAISES on some rank is reported to all the same way afterwards.  A rank whose join does not
    return within `timeout_s` (the others may be gone) cannot be recovered in-process: it exits non-zero, and the launcher
    ends the other ranks.  Returns None (RCCL) or the reason (gloo)."""
    err = None
    if ready is not None:
        try:
            ready()
        except Exception as e:
            err = f"rank {rank}: {e}"
    flags = [None] * world
    dist.all_gather_object(flags, err)
    err = next((f for f in flags if f), None)
    box = [None]
    if err is None and rank == 0:
        try:
            box = [make_unique_id()]
        except Exception as e:
            box = [("error", str(e))]
    dist.broadcast_object_list(box, src=0)
    if err is None and isinstance(box[0], tuple):
        err = box[0][1]
    if err is not None:
        return err
    import threading
    done = {}

    def join():
        try:
            init_rank(box[0], rank, world)
            done["ok"] = True
        except Exception as e:
            done["err"] = str(e)
    th = threading.Thread(target=join, daemon=True)
    th.start()
    th.join(timeout_s if timeout_s is not None else float(os.environ.get("SK_BENCH_RCCL_TIMEOUT", "300")))
    if not done:
        # still inside the bootstrap: the ranks it waits for are gone or stuck, and the call cannot be taken back in-process
        sys.stderr.write(f"[bench] rank {rank}: joining the RCCL communicator did not return; this rank exits and the launcher ends the others\n")
        sys.stderr.flush()
        os._exit(3)
    # every rank that gets here came OUT of the join (a rank that did not has exited, which ends the run): they tell each other
    # how it went, and one failure (RCCL refusing the device set, say) sends all of them to the gloo sum together
    flags = [None] * world
    dist.all_gather_object(flags, done.get("err"))
    return next((f for f in flags if f), None)


def require_backend(rccl_err):
    """SK_BENCH_REQUIRE_RCCL=1: a run whose count reduce would go through gloo is an error (every rank holds the same rccl_err,
    so all of them leave together)."""
    if rccl_err is not None and os.environ.get("SK_BENCH_REQUIRE_RCCL") == "1":
        raise SystemExit(f"SK_BENCH_REQUIRE_RCCL=1 and the count reduce would go through gloo ({rccl_err})")


def reduce_report(distributed, rccl_err, rank_kernel_ms, rank_reduce_us):
    """The keys of the JSON line that say where a step of an N > 1 run went: which backend summed the counters, what the sum
    cost per step on the ctx stream (mean and slowest rank), and the spread of the ranks' own kernel times."""
    return {"count_reduce_backend": "none" if not distributed else ("rccl" if rccl_err is None else "gloo"),
            "allreduce_us": None if not distributed else round(sum(rank_reduce_us) / len(rank_reduce_us), 2),
            "allreduce_us_max": None if not distributed else round(max(rank_reduce_us), 2),
            "kernel_ms_ranks": {"min": round(min(rank_kernel_ms), 4), "max": round(max(rank_kernel_ms), 4)}}


def device_identity(index):
    """gpu_unique_id and the partition modes of the device the rank runs on, from rocm-smi (a separate process; nothing here
    touches the GPU): what two boxes whose fused pass streams differently could differ in."""
    out = {"gpu_unique_id": None, "memory_partition": None, "compute_partition": None}
    try:
        # rocm-smi is a script (`#!/usr/bin/env python3`: two exec hops).  Under `rocprofv3 --pmc` the profiler's preloaded library
        # would initialise the GPU in that child before the hops: it gets an environment without the preload.
        env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD" and not k.startswith(("ROCP", "ROCPROF", "HSA_TOOLS", "ROCTRACER"))}
        r = subprocess.run(["rocm-smi", "-d", str(index), "--showuniqueid", "--showmemorypartition", "--showcomputepartition", "--json"],
                           stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=30, env=env)
        j = json.loads(r.stdout.decode() or "{}")
        card = next(iter(j.values())) if j else {}
        for k, v in card.items():
            kl = k.lower()
            if "unique" in kl:
                out["gpu_unique_id"] = v
            elif "memory partition" in kl:
                out["memory_partition"] = v
            elif "compute partition" in kl:
                out["compute_partition"] = v
    except Exception as e:
        out["error"] = str(e)[:200]
    return out


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ and "RANK" not in os.environ:
        sys.exit(launch_ranks(args))
    # stdout carries exactly ONE line (the JSON).  Everything else that writes to fd 1 — RCCL's version banner comes out
    # of C stdio at exit, torch warnings, ... — is sent to stderr; the JSON line goes to the saved descriptor at the end.
    sys.stdout.flush()
    real_stdout = os.dup(1)
    os.dup2(2, 1)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if os.environ.get("SK_BENCH_SAME_DEVICE"):               # testing aid for one-GPU boxes: every rank on device 0 (RCCL refuses that: exercises the fallback)
        local_rank = 0
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    # --full: a child process, started before this one touches the GPU (every rank: its id goes into its line of `ranks`)
    device = device_identity(local_rank) if args.full else None

    import torch
    import torch.distributed as dist

    import seqkit_amd
    from seqkit_amd import capi, synth

    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: no HIP device visible (there is no CPU fallback to time)")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    # Placement tuning.  WHERE the pages of a device buffer lie moves the same kernel on the same bytes by up to 12 % on one
    # GPU — a property of the allocations that stays for their lifetime, bimodal, and relational (how the buffers of the
    # streams that are active together lie to each other; DESIGN.md §6, tools/soa_placement_search.py: 9.34 against 10.6 ms).
    # A long-lived process chooses once: the shard's big buffers are allocated --placements times over, before the
    # library's context, RCCL or any temporary exists; the input candidates get the same bytes; then, BEFORE the warm-up,
    # sk_fused_tune_placement_dev (SoA matrices) / a probe of every input x output pair (blocked) keeps the fastest
    # combination and the rest is freed.  What was probed and chosen goes into the JSON line (config.placement).
    # The job is ONE index space of args.pairs x world clusters (BASELINE configs[3]: 500 M over 8 GPUs), cut into contiguous
    # tile-aligned shards, one per rank (seqkit_amd/shard.py): weak scaling — every rank gets args.pairs clusters
    # to within a tile.  Nothing crosses shards but the S + 3 counters.
    from seqkit_amd import shard
    total_clusters = args.pairs * world
    shard_lo, shard_hi = shard.shard_bounds(total_clusters, rank, world)
    n = shard_hi - shard_lo
    nt = (n + 63) // 64
    npad = nt * 64                                           # whole tiles
    lay = None
    K = max(1, min(args.placements if args.placements is not None else (3 if world == 1 else 2), 8))
    # Pre-flight: the candidates are the bulk of what this rank allocates (K x 56 GB at the full shard).  Ask the device what is
    # free BEFORE allocating, take as many candidates as fit beside the fixed part, and say so — a rank that cannot hold even one
    # set ends here with a sentence instead of an allocator trace somewhere in the middle of the run.
    free_b, total_b = torch.cuda.mem_get_info(dev)
    per_candidate = npad * 930                               # six matrices of 150 B per cluster; a blocked candidate pair is 926 B per cluster
    fixed = npad * (L_BC + 2 * 2 + 4) + (3 << 30)             # barcodes, lowest_k x 2, assign, and room for the library's tables and the runtime
    if free_b < per_candidate + fixed:
        raise SystemExit(f"[bench] rank {rank}: {n} clusters need {(per_candidate + fixed) / 1e9:.1f} GB on device {local_rank}, "
                         f"{free_b / 1e9:.1f} of {total_b / 1e9:.1f} GB are free — a smaller --pairs, or a device nobody else is using")
    k_fit = int((free_b - fixed) // per_candidate)
    if k_fit < K:
        sys.stderr.write(f"[bench] rank {rank}: {k_fit} candidate allocation(s) per matrix fit the {free_b / 1e9:.1f} GB free on device {local_rank}, not {K}\n")
        K = max(1, k_fit)
    if args.layout == "blocked":
        lay = capi.blocked_layout(2, L_READ, L_BC, capi.SK_BLK_MASK | capi.SK_BLK_TRIM)
        cands = [(torch.empty(nt * lay.in_block, dtype=torch.uint8, device=dev), torch.empty(nt * lay.out_block, dtype=torch.uint8, device=dev))
                 for _ in range(K)]
        bin_, bout = cands[0]
        bin_.zero_()
    else:
        c_seq, c_qual, c_out = [[], []], [[], []], [[], []]              # [mate][candidate]
        for k in range(K):
            try:
                got = [torch.empty((npad, L_READ), dtype=torch.uint8, device=dev) for _ in range(6)]
            except torch.cuda.OutOfMemoryError:                          # less free memory than 3 x 56 GB: tune over what fits
                if k == 0:
                    raise
                sys.stderr.write(f"[bench] {k} candidate allocation(s) per matrix fit the free device memory, not {K}\n")
                K = k
                break
            for i in range(2):
                c_seq[i].append(got[3 * i]); c_qual[i].append(got[3 * i + 1]); c_out[i].append(got[3 * i + 2])
            del got
    torch.cuda.synchronize()
    ctx = seqkit_amd.Context(local_rank)                    # raises if libseqkit_hip.so is missing
    table = synth.make_sheet(S_SAMPLES, 8, dual=True, seed=4)
    ctx.set_barcodes(table, 1)

    # Ranks meet over gloo (plumbing: rendezvous, barrier, max of the elapsed times); the path's one collective —
    # the sum of the u64[S+3] counters — runs in the library's own RCCL communicator on the ctx stream.
    distributed = world > 1 or bool(os.environ.get("SK_BENCH_FORCE_DIST"))
    rccl_err = None
    if distributed:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        try:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        except Exception as e:
            if "address already in use" in str(e).lower() or "EADDRINUSE" in str(e):
                sys.stderr.write(f"[bench] rank {rank}: rendezvous port {os.environ['MASTER_PORT']} is taken\n")
                sys.stderr.flush()
                os._exit(EXIT_PORT_TAKEN)
            raise
        rccl_err = join_count_reduce(dist, rank, world, capi.comm_unique_id, ctx.comm_init_rank, ready=ctx.comm_ready)
        if rccl_err is not None:
            sys.stderr.write(f"[bench] RCCL unavailable ({rccl_err}); the count reduce goes through gloo\n")
            require_backend(rccl_err)
            try:
                ctx.comm_destroy()                                # a communicator some ranks did get
            except Exception:
                pass

    counts = torch.zeros((S_SAMPLES + 3,), dtype=torch.int64, device=dev)
    cpu_sample = args.cpu_sample if args.full else 0            # the parity sample and cpu_baseline are --full's
    if lay is not None:
        vin = bin_.view(nt, lay.in_block)
        ns_keep = (min(max(cpu_sample, 0), n) + 63) // 64 * 64
        seq = [torch.empty((ns_keep, L_READ), dtype=torch.uint8, device=dev) for _ in range(2)]     # only the parity sample stays in SoA form
        qual = [torch.empty((ns_keep, L_READ), dtype=torch.uint8, device=dev) for _ in range(2)]
        bc = torch.empty((ns_keep, L_BC), dtype=torch.uint8, device=dev)
        chunk = args.gen_chunk // 64 * 64

        def sink(r0, cs, cq, b):
            m = b.shape[0]
            pack_blocked(torch, lay, cs, cq, b, m // 64, dst=vin[r0 // 64:(r0 + m) // 64])
            k = min(max(ns_keep - r0, 0), m)
            if k:
                for i in range(2):
                    seq[i][r0:r0 + k] = cs[i][:k]
                    qual[i][r0:r0 + k] = cq[i][:k]
                bc[r0:r0 + k] = b[:k]
        gen_shard(torch, dev, npad, table, seed=4000 + rank, chunk=chunk, sink=sink)
        placement = {"candidates": len(cands), "probe_ms": None, "chosen": 0}
        if len(cands) > 1:
            for cin, _ in cands[1:]:
                cin.copy_(bin_)
            torch.cuda.synchronize()
            probe_ms = {}
            for i, (cin, _) in enumerate(cands):             # every input buffer with every output buffer
                for j, (_, cout) in enumerate(cands):
                    for _ in range(2):
                        ctx.fused_pass_blocked_dev(lay, cin.data_ptr(), cout.data_ptr(), n, MIN_BASEQ, counts=counts.data_ptr())
                    ctx.sync()
                    ctx.timer_start()
                    for _ in range(3):
                        ctx.fused_pass_blocked_dev(lay, cin.data_ptr(), cout.data_ptr(), n, MIN_BASEQ, counts=counts.data_ptr())
                    probe_ms[(i, j)] = round(ctx.timer_stop() / 3, 4)
            bi, bj = min(probe_ms, key=probe_ms.get)
            placement.update(probe_ms=[[probe_ms[(i, j)] for j in range(len(cands))] for i in range(len(cands))], chosen=[bi, bj])
            bin_, bout = cands[bi][0], cands[bj][1]
            vin = None
        del cands
        torch.cuda.empty_cache()
    else:
        seq, qual = [c_seq[i][0] for i in range(2)], [c_qual[i][0] for i in range(2)]
        bc = torch.empty((npad, L_BC), dtype=torch.uint8, device=dev)
        gen_shard(torch, dev, npad, table, seed=4000 + rank, chunk=args.gen_chunk, into=(seq, qual, bc))
        out_seq = [c_out[i][0] for i in range(2)]
        lowest_k = [torch.empty((npad,), dtype=torch.int16, device=dev) for _ in range(2)]     # raw u16 storage
        assign = torch.empty((npad,), dtype=torch.int32, device=dev)
        mates = [{"seq": seq[i].data_ptr(), "qual": qual[i].data_ptr(), "len": 0,
                  "out_seq": out_seq[i].data_ptr(), "lowest_k": lowest_k[i].data_ptr()} for i in range(2)]
        placement = {"candidates": K, "ms_before": None, "ms_after": None, "probes": 0}
        if K > 1:
            for i in range(2):
                for k in range(1, K):
                    c_seq[i][k].copy_(c_seq[i][0])
                    c_qual[i][k].copy_(c_qual[i][0])
            torch.cuda.synchronize()
            cd = [{"seq": [t.data_ptr() for t in c_seq[i]], "qual": [t.data_ptr() for t in c_qual[i]], "out_seq": [t.data_ptr() for t in c_out[i]]}
                  for i in range(2)]
            mates, ms0, ms1, probes = ctx.fused_tune_placement_dev(n, L_READ, MIN_BASEQ, mates, cd, bc=bc.data_ptr(), bc_stride=L_BC,
                                                                   assign=assign.data_ptr(), sweeps=2)
            by_ptr = {t.data_ptr(): t for grp in (c_seq, c_qual, c_out) for per_mate in grp for t in per_mate}
            seq = [by_ptr[mates[i]["seq"]] for i in range(2)]
            qual = [by_ptr[mates[i]["qual"]] for i in range(2)]
            out_seq = [by_ptr[mates[i]["out_seq"]] for i in range(2)]
            placement.update(ms_before=round(ms0, 4), ms_after=round(ms1, 4), probes=probes)
            del by_ptr, cd
        del c_seq, c_qual, c_out
        torch.cuda.empty_cache()
    torch.cuda.synchronize()

    # everything below runs on the ctx's own HIP stream (torch sees it as an external stream)
    stream = torch.cuda.ExternalStream(ctx.stream(), device=dev)

    def step(ev=None):
        with torch.cuda.stream(stream):
            counts.zero_()
            if ev is not None:
                ev[0].record(stream)
            if lay is not None:
                ctx.fused_pass_blocked_dev(lay, bin_.data_ptr(), bout.data_ptr(), n, MIN_BASEQ, counts=counts.data_ptr())
            else:
                ctx.fused_pass_dev(n, L_READ, MIN_BASEQ, mates, bc=bc.data_ptr(), bc_stride=L_BC,
                                   assign=assign.data_ptr(), counts=counts.data_ptr())
            if ev is not None:
                ev[1].record(stream)
            if rccl_err is None:
                ctx.allreduce_u64_dev(counts.data_ptr(), S_SAMPLES + 3)     # the path's only cross-shard state (nothing to do at N=1)
            else:
                h = counts.cpu()
                shard.reduce_counts(h)                                      # the same sum over gloo, with a host round trip
                counts.copy_(h)
            if ev is not None:
                ev[2].record(stream)

    def fence():
        if distributed:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        step()
    fence()
    events = [tuple(torch.cuda.Event(enable_timing=True) for _ in range(3)) for _ in range(args.steps)]
    t0 = time.perf_counter()
    for k in range(args.steps):
        step(events[k])
    fence()
    elapsed = time.perf_counter() - t0
    if distributed:
        t = torch.tensor([elapsed], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    kern_ms = sum(e[0].elapsed_time(e[1]) for e in events) / max(args.steps, 1)
    # the count reduce of a step on the ctx stream (RCCL: the collective itself, the kernel's end to the reduce's end; gloo:
    # the host round trip), and every rank's own kernel time: what a reader of an N > 1 line needs to see where a step went
    reduce_us = sum(e[1].elapsed_time(e[2]) for e in events) / max(args.steps, 1) * 1e3
    rank_kernel_ms = [kern_ms]
    rank_reduce_us = [reduce_us]
    # every rank's own line: its kernel time and what the placement probe found and chose on ITS device — a GPU in the slow
    # placement mode (some boxes have no fast one) shows here, not only in the max over the ranks
    mine = {"rank": rank, "local_rank": local_rank, "kernel_ms": round(kern_ms, 4), "count_reduce_us": round(reduce_us, 2),
            "placement_candidates": placement.get("candidates"), "placement_ms_before": placement.get("ms_before"),
            "placement_ms_after": placement.get("ms_after"), "gpu_unique_id": (device or {}).get("gpu_unique_id")}
    rank_lines = [mine]
    if distributed:
        both = [None] * world
        dist.all_gather_object(both, (kern_ms, reduce_us, mine))
        rank_kernel_ms, rank_reduce_us, rank_lines = [b[0] for b in both], [b[1] for b in both], [b[2] for b in both]

    # ---- size-independent checks on the full shard + bit-exact parity on a sample (oracle = checker only) -----
    total_counts = counts.cpu().numpy().astype(np.uint64)
    S = S_SAMPLES
    assert int(total_counts[S]) == total_clusters, (int(total_counts[S]), total_clusters)
    assert int(total_counts[:S].sum()) == int(total_counts[S + 1])
    if rank == 0 and args.dump_outputs:
        if lay is not None:
            dump_outputs(torch, args.dump_outputs, n, counts, lay=lay, bout=bout)
        else:
            dump_outputs(torch, args.dump_outputs, n, counts, assign=assign, lowest_k=lowest_k, out_seq=out_seq)
    cpu_baseline = None
    parity = None
    if rank == 0 and cpu_sample > 0:
        from oracle import oracle as orc
        ns = min(cpu_sample, n)
        if lay is not None:
            u = unpack_blocked(torch, lay, bout, (ns + 63) // 64)
            g_assign, g_k, g_m = u["assign"][:ns], [x[:ns] for x in u["lowest_k"]], [x[:ns] for x in u["out_seq"]]
        else:
            g_assign, g_k, g_m = assign[:ns], [x[:ns] for x in lowest_k], [x[:ns] for x in out_seq]
        h_bc = bc[:ns].cpu().numpy()
        h_seq = [seq[i][:ns].cpu().numpy() for i in range(2)]
        h_qual = [qual[i][:ns].cpu().numpy() for i in range(2)]
        def run_cpu(nthr):
            """the sampled clusters through the C restatement on nthr threads (contiguous slices; ctypes releases the GIL around
            the C calls): (per-slice results, seconds)"""
            cuts = [ns * k // nthr for k in range(nthr + 1)]

            def cpu_slice(k):
                lo, hi = cuts[k], cuts[k + 1]
                return (orc.demux_batch(table, h_bc[lo:hi], 1)[0],
                        [orc.trim_batch(h_qual[i][lo:hi], None, MIN_BASEQ) for i in range(2)],
                        [orc.mask_batch(h_seq[i][lo:hi], h_qual[i][lo:hi], None, MIN_BASEQ) for i in range(2)])
            t1 = time.perf_counter()
            if nthr == 1:
                res = [cpu_slice(0)]
            else:
                from concurrent.futures import ThreadPoolExecutor
                with ThreadPoolExecutor(nthr) as ex:
                    res = list(ex.map(cpu_slice, range(nthr)))
            return res, time.perf_counter() - t1

        nthr = max(1, min(args.cpu_threads, os.cpu_count() or 1))
        parts, cpu_s = run_cpu(nthr)
        e_assign = np.concatenate([p[0] for p in parts])
        e_k = [np.concatenate([p[1][i] for p in parts]) for i in range(2)]
        e_m = [np.concatenate([p[2][i] for p in parts]) for i in range(2)]
        ok = np.array_equal(g_assign.cpu().numpy(), e_assign)
        for i in range(2):
            ok = ok and np.array_equal(g_k[i].cpu().numpy().view(np.uint16), e_k[i])
            ok = ok and np.array_equal(g_m[i].cpu().numpy(), e_m[i])
        parity = bool(ok)
        cpu_baseline = {"value": round(ns / cpu_s / 1e6, 4), "unit": "M reads/s", "cores": nthr, "kind": "port",
                        "sample": f"first {ns} clusters of rank 0's shard, same fused work (demultiplex + 2x trim + 2x mask), "
                                  f"C restatement of the reference loops over the packed SoA batch, {nthr} thread(s) "
                                  f"({os.cpu_count()} host cores present; the reference's commands are single-threaded loops); "
                                  "not the Rust binary"}
        if not ok:
            raise SystemExit("PARITY FAILURE: GPU outputs differ from the oracle on the sampled clusters")
        # the same restatement on every core this process may use (1 thread AND all host cores, count stated)
        n_all = usable_cores()
        if n_all > nthr and not args.no_all_cores:
            best = min(run_cpu(n_all)[1] for _ in range(2))
            cpu_baseline["all_cores"] = {"value": round(ns / best / 1e6, 4), "unit": "M reads/s", "cores": n_all,
                                         "host_cores_present": os.cpu_count(),
                                         "how": f"the same {ns} clusters cut into {n_all} contiguous slices, one thread each (affinity mask and cgroup CPU quota "
                                                "of this process decide the count); best of two runs"}
        if args.faithful_reads > 0:
            try:
                cpu_baseline["faithful"] = faithful_cpu(args.faithful_reads)
            except Exception as e:                                   # a reported baseline must not take the bench line down
                cpu_baseline["faithful"] = {"error": str(e)}

    extra = None
    if rank == 0 and world == 1 and args.full and not args.no_extra:
        if lay is not None:
            del bin_, bout
        else:
            del out_seq, lowest_k, assign, mates
        del seq, qual, bc
        torch.cuda.empty_cache()
        try:
            extra = {"rates": secondary_rates(torch, ctx, dev), "bam_files": bam_file_rows(ctx),
                     "note": "device-resident, outside the timed region, HIP events on the ctx stream; frac = algorithmic bytes / time / 8 TB/s; "
                             "where frac_as_placed is given, frac is with the placement of the kernel's arrays chosen among 3 candidates each; "
                             "a row whose in+out bytes would fit the 256 MiB Infinity Cache says rows_from: its frac is measured with the rows "
                             "coming from HBM (buffer sets in rotation, one event pair per call, ~6 us of launch + event in every call), "
                             "frac_pipelined the same rotation inside one event pair, frac_warm the replay on one on-die set"}
        except Exception as e:
            extra = {"error": str(e)}

    if rank == 0:
        ms_per_step = elapsed / args.steps * 1e3
        value = total_clusters / (elapsed / args.steps) / 1e6
        achieved = BYTES_PER_PAIR * n / (kern_ms * 1e-3) / 1e9
        # HBM bytes per launch from the PMC counters are measured in separate rocprofv3 passes (tools/profile_bench.sh) and
        # recorded in profiles/pmc_traffic.json together with the digest of the kernel sources they were taken on; the record is
        # quoted only when it matches this build, layout and size — otherwise traffic is null.
        traffic = traffic_source = None
        tpath = os.path.join(REPO, "profiles", "pmc_traffic.json")
        if os.path.exists(tpath):
            try:
                tj = json.load(open(tpath))
                if tj.get("pairs") == n and tj.get("layout") == args.layout and tj.get("library_inputs_sha256_16") == kernel_sources_digest():
                    traffic = tj.get("hbm_bytes_per_launch")
                    traffic_source = {"file": "profiles/pmc_traffic.json", "how": "separate rocprofv3 --pmc passes of this build (FETCH_SIZE x 2 + WRITE_SIZE), not this run",
                                      "library_inputs_sha256_16": tj.get("library_inputs_sha256_16")}
            except Exception:
                traffic = traffic_source = None
        kernel = "sk::tile_blocked_kernel" if lay is not None else "sk::tile_pass_kernel"
        # the same pass on the buffers as they were allocated, before any placement was chosen (config.placement: ms_before of
        # the SoA tuner, probe_ms[0][0] of the blocked probe); null when only one candidate was allocated — frac is then as placed
        ms_placed = placement.get("ms_before") if lay is None else (placement["probe_ms"][0][0] if placement.get("probe_ms") else None)
        frac_as_placed = round(BYTES_PER_PAIR * n / (ms_placed * 1e-3) / 1e9 / HBM_PEAK_GBS, 4) if ms_placed else None
        line = {
            "metric": "M reads/s demultiplex (150bp, 96 barcodes) at 1/8 GPUs; % HBM roofline",
            "value": round(value, 3), "unit": "M reads/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 4), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "u8", "data": "synthetic", "full": args.full,
            "config": {"workload": "fasta add barcode + demultiplex fused with trim+mask by quality: "
                                   f"{n} clusters/GPU x 2x150bp paired, 96 dual-index 8+8 barcodes (17 chars), <=1 mismatch, "
                                   "min_baseq 20 (= BASELINE configs[3], 500M clusters read-sharded over 8 GPUs)",
                       "clusters_per_gpu": n, "clusters": total_clusters, "shard_of_rank_0": [shard_lo, shard_hi], "read_len": L_READ, "barcodes": S_SAMPLES, "barcode_len": L_BC,
                       "min_baseq": MIN_BASEQ, "read_unit": "cluster (as the reference's total_reads counts)",
                       "layout": args.layout,
                       "placement": dict(placement, what=("candidate input and output buffers allocated at start-up; the pass timed on every (input, output) "
                                                          "combination before the warm-up (probe_ms[i][j]); the fastest combination kept, the rest freed"
                                                          if lay is not None else
                                                          "candidate device buffers for each of the six big matrices allocated at start-up; sk_fused_tune_placement_dev "
                                                          "times the pass while one matrix at a time is swapped for its other candidates, before the warm-up; "
                                                          "the fastest combination kept, the rest freed")),
                       "count_reduce": ("none (1 GPU)" if not distributed else
                                        f"RCCL ncclAllReduce(sum, u64[{S + 3}]) per step on the ctx stream, {world} rank(s), communicator inside libseqkit_hip.so"
                                        if rccl_err is None else f"gloo all-reduce with a host round trip (RCCL unavailable: {rccl_err})")},
            "roofline": {"bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": round(achieved / HBM_PEAK_GBS, 4), "frac_as_placed": frac_as_placed,
                         "traffic": traffic, "traffic_source": traffic_source,
                         "kernel": kernel, "kernel_ms": round(kern_ms, 4),
                         "algorithmic_bytes_per_cluster": BYTES_PER_PAIR,
                         "read_frac": round((617 * n / (kern_ms * 1e-3) / 1e9) / HBM_PEAK_GBS, 4)},
            **reduce_report(distributed, rccl_err, rank_kernel_ms, rank_reduce_us),
            "ranks": rank_lines,
            "device": device,
            "cpu_baseline": cpu_baseline,
            "parity_sample_ok": parity,
            "identified_frac": round(float(total_counts[S + 1]) / float(total_counts[S]), 4),
            "library_sha256_16": library_digest(), "library_inputs_sha256_16": kernel_sources_digest(),
            "extra": extra,
        }
        os.write(real_stdout, (json.dumps(line) + "\n").encode())
    if distributed:
        ctx.comm_destroy()
    ctx.close()
    if distributed:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
