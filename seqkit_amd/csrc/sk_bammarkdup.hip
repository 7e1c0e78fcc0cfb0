// sk_bammarkdup.hip — the record passes of sk_bam_file_markdup (include/seqkit_hip.h): `sam mark duplicates`
// (src/sam_mark_duplicates.rs) over a verified BAM stream.  The BGZF half (cut, deflate, pack) is sk_bamwrite.hip's and sk_deflate.hip's.
//
// The reference keeps a FIFO of reads and, once a read's start position lies behind the file's current position, scans the FIFO for the
// reads that share its signature.  On a file it accepts as sorted the FIFO only bounds memory; what it writes is:
// a GROUP is the mapped reads of one run of equal tid in file order with one start_pos and strand; per group, in file order, the first
// read not yet in a cluster is a SEED and every later such read compatible with the seed (fragment length, UMI) joins it; all of a
// cluster get 0x400 except its longest read, the earliest on a tie.  In data-parallel form:
// bam_md_sig_kernel — a wave per BGZF block (sk_bamblock.h), a lane per record: the core fields, end_pos from the CIGAR for a mapped
//   reverse read, the aux walk to the first RX field; per record its stream and output offsets, (tid, pos), start_pos, l_seq, where its
//   UMI lies in the stream and how long it is, fraglen | strand | mapped, and its flag; the decline bits of include/seqkit_hip.h.
// bam_md_order_kernel — a lane per record: 1 where tid differs from the record before (the inclusive scan of that is the run index),
//   decline bit 2 where tid is the same and (u32) pos lower.
// bam_md_key_kernel — key = run << 33 | start_pos << 1 | strand for a mapped read, all ones for an unmapped one (sorted last, never
//   clustered), and the record's index; then sk_bamminimize.hip's stable radix sort of (key, index): a group is a stretch of equal keys
//   whose indices ascend.
// bam_md_cluster_kernel — a wave takes 64 sorted positions at a time.  A group of one member (head and tail at once) is settled by its
//   lane.  The heads of larger groups are taken one after another by the whole wave: up to 64 members sit a member per lane, in
//   registers; per round the ballot of unassigned lanes gives the seed (the lowest lane = the lowest file index), its fraglen, UMI length
//   and UMI address are broadcast, every unassigned lane tests itself against it (the UMI bytes are read where they lie in the stream,
//   a dword at a time), and a wave maximum of (l_seq, -lane) over the joiners names the one that keeps its flag.  A larger group goes
//   the same way with its members strided over the lanes, 64 positions at a time from the group's start, the "assigned" bit kept in the
//   record's signature word: position q is always lane (q - start) & 63's, so every word and every flag is read and written by one
//   lane only.  Rounds = clusters of the group.  No atomics: a record's flag is written by its owner lane.
// bam_md_count_kernel — the records that carry 0x400 afterwards.
// MdRecord in bam_write_kernel (sk_bamblock.h) — a window's records copied as sk_bamwrite.hip copies an unchanged record, bytes 18-19
//   from the flag column.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "../../include/seqkit_hip.h"
#include "sk_bamblock.h"
#include "sk_internal.h"

namespace sk {

namespace {

typedef uint32_t u32;
typedef unsigned long long u64;

constexpr int kMdThreads = 256;
constexpr u32 kStrand = 1u << 16, kMapped = 1u << 17, kAssigned = 1u << 31;      // bits of MdCols::fl above the fraglen
constexpr u64 kNoKey = ~0ull;

struct SigArgs {
	const uint8_t *stream;
	const u64 *bend, *entry, *rb;
	int64_t nb;
	int ignore_umi;
	u64 first;                // the stream offset of the first record: a record's output offset is its stream offset - first
	MdCols c;
	uint32_t *decline;
};

// The first RX field of the aux data r[a .. end) as the hosts' find_rx reads them: its type Z or H -> true with the value's offset and
// length; any other type, or no RX -> false.  *bad: the data stop parsing before that is known.
__device__ __forceinline__ bool md_find_rx(const uint8_t *r, u64 a, u32 end, u32 &voff, u32 &vl, bool &bad)
{
	while (a < end) {
		if (a + 3u > end) { bad = true; return false; }
		const u32 t0 = r[a], t1 = r[a + 1], ty = r[a + 2];
		a += 3u;
		const u32 v0 = (u32)a;
		if (ty == 'A' || ty == 'c' || ty == 'C') a += 1u;
		else if (ty == 's' || ty == 'S') a += 2u;
		else if (ty == 'i' || ty == 'I' || ty == 'f') a += 4u;
		else if (ty == 'Z' || ty == 'H') {
			while (a < end && r[a] != 0) a++;
			if (a >= end) { bad = true; return false; }
			a++;
		} else if (ty == 'B') {
			if (a + 5u > end) { bad = true; return false; }
			const u32 sub = r[a], cnt = bam_le32_bytes(r + a + 1);
			const u32 es = (sub == 'c' || sub == 'C') ? 1u : (sub == 's' || sub == 'S') ? 2u : (sub == 'i' || sub == 'I' || sub == 'f') ? 4u : 0u;
			if (!es) { bad = true; return false; }
			a += 5ull + (u64)cnt * es;
		} else { bad = true; return false; }
		if (a > end) { bad = true; return false; }
		if (t0 == 'R' && t1 == 'X') {
			if (ty != 'Z' && ty != 'H') return false;
			voff = v0; vl = (u32)(a - v0) - 1u;
			return true;
		}
	}
	return false;
}

__global__ __launch_bounds__(kBlockThreads) void bam_md_sig_kernel(const SigArgs a)
{
	// (block_open written out: with the helper this kernel measured 0.5 % slower, 2.747 against 2.734 ms on 20 M records)
	__shared__ uint16_t offs[kBlockWaves][kBlockRecs];
	const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	const int64_t c = (int64_t)blockIdx.x * kBlockWaves + w;
	if (c >= a.nb) return;
	uint16_t *off = offs[w];
	const u32 n = wave_record_offsets(a.stream, a.entry, a.bend, c, off, lane);
	const u64 entry = a.entry[c], k0 = a.rb[c];
	u32 dec = 0u;
	for (u32 j = (u32)lane; j < n; j += 64u) {
		const u64 ro = entry + off[j], k = k0 + j;
		const uint8_t *r = a.stream + ro;
		const u32 bs = bam_le32_bytes(r), lo = r[12], w16 = bam_le32_bytes(r + 16), S = bam_le32_bytes(r + 20);
		const u32 nc = w16 & 0xffffu, flag = w16 >> 16;
		const int32_t tid = (int32_t)bam_le32_bytes(r + 4), pos = (int32_t)bam_le32_bytes(r + 8), tlen = (int32_t)bam_le32_bytes(r + 32);
		u32 start = 0u, fl = 0u, uoff = 0u, ulen = 0u;
		if (bs < 32u || lo < 1u || S > 0x7fffffffu || 4ull * nc + lo + (((u64)S + 1) >> 1) + S > (u64)(bs - 32u)) dec |= 8u;
		else {
			if (flag & 0x900u) dec |= 1u;
			const bool mapped = !(flag & 4u), reverse = flag & 16u;
			if (mapped) {
				fl = kMapped | (reverse ? 0u : kStrand);
				if (pos < 0) dec |= 4u;
				long long e = pos;
				if (reverse) {
					const uint8_t *cg = r + 36 + lo;
					for (u32 q = 0; q < nc; q++) {
						const u32 op = bam_le32_bytes(cg + 4u * q), code = op & 15u;
						if (code > 8u) dec |= 32u;
						if (code == 0u || code == 2u || code == 3u || code == 7u || code == 8u) e += op >> 4;
					}
					if (e > 0x7fffffffll) dec |= 4u;
				}
				start = (u32)e;
				if (!a.ignore_umi) {
					bool bad = false;
					const u64 aux = 36ull + lo + 4ull * nc + (((u64)S + 1) >> 1) + S;
					if (!md_find_rx(r, aux, 4u + bs, uoff, ulen, bad)) { uoff = 0u; ulen = 0u; }
					if (bad) dec |= 16u;
				}
				if (ulen == 0u) {
					const long long t = tlen < 0 ? -(long long)tlen : (long long)tlen;
					fl |= (u32)(t < 65535 ? t : 65535);
				}
			}
		}
		a.c.krec[k] = ro;
		a.c.kout[k] = ro - a.first;
		a.c.tidpos[k] = ((u64)(u32)tid << 32) | (u32)pos;
		a.c.start[k] = start; a.c.fl[k] = fl; a.c.lseq[k] = S; a.c.uoff[k] = uoff; a.c.ulen[k] = ulen;
		a.c.nflag[k] = (uint16_t)flag;
	}
	if (__any((int)dec)) {
		for (int s = 32; s > 0; s >>= 1) dec |= (u32)__shfl_xor((int)dec, s);
		if (lane == 0) atomicOr(a.decline, dec);
	}
}

__global__ __launch_bounds__(kMdThreads) void bam_md_order_kernel(const u64 *tidpos, u64 n, u32 *runflag, uint32_t *decline)
{
	const u64 k = (u64)blockIdx.x * kMdThreads + threadIdx.x;
	bool bad = false;
	if (k < n) {
		const u64 me = tidpos[k], before = k ? tidpos[k - 1] : 0;
		const bool differs = k == 0 || (me >> 32) != (before >> 32);
		bad = !differs && (u32)me < (u32)before;
		runflag[k] = differs ? 1u : 0u;
	}
	if (__any((int)bad) && (threadIdx.x & 63) == 0) atomicOr(decline, 2u);
}

__global__ __launch_bounds__(kMdThreads) void bam_md_key_kernel(const u32 *run, const u32 *start, const u32 *fl, u64 n, u64 *key, u32 *idx)
{
	const u64 k = (u64)blockIdx.x * kMdThreads + threadIdx.x;
	if (k >= n) return;
	const u32 f = fl[k];
	key[k] = (f & kMapped) ? ((u64)(run[k] - 1u) << 33) | ((u64)start[k] << 1) | ((f & kStrand) ? 1u : 0u) : kNoKey;
	idx[k] = (u32)k;
}

// are two UMIs of the stream compatible (src/sam_mark_duplicates.rs:169-179): an empty one matches anything, different lengths never,
// else at most one position where the bytes differ and neither is 'N'.  (The stream is readable 64 bytes beyond its end.)
__device__ __forceinline__ bool md_umi_matches(const uint8_t *x, u32 lx, const uint8_t *y, u32 ly)
{
	if (lx == 0u || ly == 0u) return true;
	if (lx != ly) return false;
	u32 mm = 0u;
	for (u32 k = 0; k < lx && mm <= 1u; k += 4u) {
		const u32 vx = bam_le32(x + k), vy = bam_le32(y + k);
		if (vx == vy) continue;
		const u32 m = lx - k < 4u ? lx - k : 4u;
		for (u32 b = 0; b < m; b++) {
			const u32 bx = (vx >> (8u * b)) & 0xffu, by = (vy >> (8u * b)) & 0xffu;
			if (bx != by && bx != 'N' && by != 'N') mm++;
		}
	}
	return mm <= 1u;
}

__device__ __forceinline__ bool md_compatible(u32 fl, const uint8_t *u, u32 ul, u32 sfl, const uint8_t *su, u32 sul)
{
	const u32 f = fl & 0xffffu, sf = sfl & 0xffffu;
	if (f > 0u && sf > 0u && f != sf) return false;
	return md_umi_matches(u, ul, su, sul);
}

struct ClusterArgs {
	const uint8_t *stream;
	MdCols c;
	const u64 *key;
	const u32 *idx;
	u64 n;
};

// a group of at most 64 members, sorted positions g0 .. g0 + m - 1: a member per lane
__device__ __forceinline__ void md_small_group(const ClusterArgs &a, u64 g0, u32 m, int lane)
{
	const bool act = (u32)lane < m;
	const u32 i = act ? a.idx[g0 + (u32)lane] : 0u;
	u32 fl = 0u, ls = 0u, ul = 0u, f = 0u;
	const uint8_t *up = a.stream;
	if (act) { fl = a.c.fl[i]; ls = a.c.lseq[i]; ul = a.c.ulen[i]; up = a.stream + a.c.krec[i] + a.c.uoff[i]; f = a.c.nflag[i]; }
	bool un = act;
	for (;;) {
		const u64 um = __ballot(un);
		if (!um) break;
		const int sl = __ffsll((long long)um) - 1;                           // the seed: the lowest file index not yet in a cluster
		const u32 sfl = (u32)__shfl((int)fl, sl), sul = (u32)__shfl((int)ul, sl);
		const uint8_t *sup = (const uint8_t *)__shfl((u64)up, sl);
		const bool join = un && (lane == sl || md_compatible(fl, up, ul, sfl, sup, sul));
		u64 score = join ? ((((u64)ls << 6) | (u64)(63 - lane)) + 1ull) : 0ull;   // the largest l_seq, then the lowest lane
		for (int s = 32; s > 0; s >>= 1) { const u64 o = __shfl_xor(score, s); if (o > score) score = o; }
		const int best = 63 - (int)((score - 1ull) & 63ull);
		if (join) { f = lane == best ? f & ~0x400u : f | 0x400u; un = false; }
	}
	if (act) a.c.nflag[i] = (uint16_t)f;
}

// a group of more than 64 members, sorted positions g0 .. g1 - 1: position q belongs to lane (q - g0) & 63
__device__ __forceinline__ void md_large_group(const ClusterArgs &a, u64 g0, u64 g1, int lane)
{
	u64 lo = g0;                                                             // every position below it is in a cluster
	for (;;) {
		u64 sp = kNoKey;
		for (u64 q0 = g0 + ((lo - g0) & ~63ull); q0 < g1; q0 += 64u) {
			const u64 q = q0 + (u32)lane;
			const bool un = q >= lo && q < g1 && !(a.c.fl[a.idx[q]] & kAssigned);
			const u64 b = __ballot(un);
			if (b) { sp = q0 + (u32)(__ffsll((long long)b) - 1); break; }
		}
		if (sp == kNoKey) break;
		lo = sp + 1;
		const u32 si = a.idx[sp];                                             // the seed's signature: the same for every lane
		const u32 sfl = a.c.fl[si], sul = a.c.ulen[si];
		const uint8_t *sup = a.stream + a.c.krec[si] + a.c.uoff[si];
		u32 bl = 0u;                                                         // this lane's best joiner: l_seq and position
		u64 bq = kNoKey;
		for (u64 q0 = g0 + ((sp - g0) & ~63ull); q0 < g1; q0 += 64u) {
			const u64 q = q0 + (u32)lane;
			if (q < sp || q >= g1) continue;
			const u32 i = a.idx[q], fl = a.c.fl[i];
			if (fl & kAssigned) continue;
			const u32 ul = a.c.ulen[i];
			if (q != sp && !md_compatible(fl, a.stream + a.c.krec[i] + a.c.uoff[i], ul, sfl, sup, sul)) continue;
			a.c.fl[i] = fl | kAssigned;
			a.c.nflag[i] = (uint16_t)(a.c.nflag[i] | 0x400u);
			const u32 ls = a.c.lseq[i];
			if (bq == kNoKey || ls > bl) { bl = ls; bq = q; }               // (q ascends: the earliest of equal lengths stays)
		}
		for (int s = 32; s > 0; s >>= 1) {
			const u32 ol = (u32)__shfl_xor((int)bl, s);
			const u64 oq = __shfl_xor(bq, s);
			if (oq != kNoKey && (bq == kNoKey || ol > bl || (ol == bl && oq < bq))) { bl = ol; bq = oq; }
		}
		if ((u32)lane == (u32)((bq - g0) & 63ull)) {                         // (the lane that set the flag clears it)
			const u32 i = a.idx[bq];
			a.c.nflag[i] = (uint16_t)(a.c.nflag[i] & ~0x400u);
		}
	}
}

__global__ __launch_bounds__(kMdThreads) void bam_md_cluster_kernel(const ClusterArgs a)
{
	const int lane = threadIdx.x & 63;
	const u64 nw = (u64)gridDim.x * (kMdThreads / 64);
	for (u64 base = ((u64)blockIdx.x * (kMdThreads / 64) + (threadIdx.x >> 6)) * 64u; base < a.n; base += nw * 64u) {
		const u64 p = base + (u32)lane;
		const u64 k = p < a.n ? a.key[p] : kNoKey;
		const bool mapped = k != kNoKey;
		const bool head = mapped && (p == 0 || a.key[p - 1] != k);
		const bool tail = mapped && (p + 1 >= a.n || a.key[p + 1] != k);
		if (head && tail) {                                                  // alone in its group: not a duplicate
			const u32 i = a.idx[p];
			a.c.nflag[i] = (uint16_t)(a.c.nflag[i] & ~0x400u);
		}
		u64 multi = __ballot(head && !tail);
		const u64 tails = __ballot(tail);
		while (multi) {
			const int l = __ffsll((long long)multi) - 1;
			multi &= multi - 1;
			const u64 g0 = base + (u32)l, gk = __shfl(k, l);
			u64 g1;
			const u64 t = tails & (~0ull << l);
			if (t) g1 = base + (u32)__ffsll((long long)t);                   // its tail lies in these 64 positions
			else {
				g1 = base + 64u;
				for (;;) {
					const u64 q = g1 + (u32)lane;
					const u64 b = __ballot(q < a.n && a.key[q] == gk);
					if (b == ~0ull) { g1 += 64u; continue; }
					g1 += (u32)(__ffsll((long long)~b) - 1);
					break;
				}
			}
			if (g1 - g0 <= 64u) md_small_group(a, g0, (u32)(g1 - g0), lane);
			else md_large_group(a, g0, g1, lane);
		}
	}
}

__global__ __launch_bounds__(kMdThreads) void bam_md_count_kernel(const uint16_t *nflag, u64 n, u64 *count)
{
	u64 acc = 0;
	for (u64 k = (u64)blockIdx.x * kMdThreads + threadIdx.x; k < n; k += (u64)gridDim.x * kMdThreads) acc += (nflag[k] >> 10) & 1u;
	for (int s = 32; s > 0; s >>= 1) acc += __shfl_xor(acc, s);
	if ((threadIdx.x & 63) == 0 && acc) atomicAdd(count, acc);
}

// bam_write_kernel's record: two spans around bytes 18-19, those from the flag column
struct MdRecord {
	const uint16_t *nflag;
	template <class Put>
	__device__ void operator()(const uint8_t *r, int64_t k, const Put &put) const
	{
		const u32 len = 4u + bam_le32_bytes(r), f = nflag[k];
		auto byte = [&](u32 p) -> u32 { return p == 18u ? f & 0xffu : p == 19u ? f >> 8 : r[p]; };
		put(len, 0u, 18u, r, 20u, len - 20u, r + 20, 0u, 0u, r, byte);
	}
};

unsigned md_grid(uint64_t n) { return (unsigned)((n + kMdThreads - 1) / kMdThreads); }

}  // namespace

hipError_t launch_bam_md_sig(const uint8_t *stream, const uint64_t *bend, const uint64_t *entry, int64_t nb, const uint64_t *rb, int ignore_umi,
                             uint64_t first, const MdCols &cols, uint32_t *decline, hipStream_t st)
{
	if (nb <= 0) return hipSuccess;
	SigArgs a{};
	a.stream = stream; a.bend = (const u64 *)bend; a.entry = (const u64 *)entry; a.rb = (const u64 *)rb; a.nb = nb; a.ignore_umi = ignore_umi;
	a.first = first; a.c = cols; a.decline = decline;
	bam_md_sig_kernel<<<block_grid(nb), kBlockThreads, 0, st>>>(a);
	return hipGetLastError();
}

hipError_t launch_bam_md_order(const uint64_t *tidpos, uint64_t n, uint32_t *runflag, uint32_t *decline, hipStream_t st)
{
	if (n == 0) return hipSuccess;
	bam_md_order_kernel<<<md_grid(n), kMdThreads, 0, st>>>((const u64 *)tidpos, n, runflag, decline);
	return hipGetLastError();
}

hipError_t bam_md_run_scan(void *temp, size_t *temp_bytes, const uint32_t *runflag, uint32_t *run, uint64_t n, hipStream_t st)
{
	return rocprim::inclusive_scan(temp, *temp_bytes, runflag, run, (size_t)n, rocprim::plus<uint32_t>(), st);
}

hipError_t launch_bam_md_keys(const uint32_t *run, const MdCols &cols, uint64_t n, uint64_t *key, uint32_t *idx, hipStream_t st)
{
	if (n == 0) return hipSuccess;
	bam_md_key_kernel<<<md_grid(n), kMdThreads, 0, st>>>(run, cols.start, cols.fl, n, (u64 *)key, idx);
	return hipGetLastError();
}

hipError_t launch_bam_md_cluster(const uint8_t *stream, const MdCols &cols, const uint64_t *key, const uint32_t *idx, uint64_t n, uint64_t *count,
                                 int n_cu, hipStream_t st)
{
	if (hipError_t e = hipMemsetAsync(count, 0, 8, st)) return e;
	if (n == 0) return hipSuccess;
	ClusterArgs a{};
	a.stream = stream; a.c = cols; a.key = (const u64 *)key; a.idx = idx; a.n = n;
	const uint64_t cap = (uint64_t)(n_cu > 0 ? n_cu : 256) * 8;
	uint64_t grid = (n + kMdThreads - 1) / kMdThreads;                       // a wave per 64 sorted positions, up to 32 waves a CU
	if (grid > cap) grid = cap;
	bam_md_cluster_kernel<<<(unsigned)grid, kMdThreads, 0, st>>>(a);
	if (hipError_t e = hipGetLastError()) return e;
	bam_md_count_kernel<<<(unsigned)grid, kMdThreads, 0, st>>>(cols.nflag, n, (u64 *)count);
	return hipGetLastError();
}

hipError_t launch_bam_md_write(const WriteWindow &w, const uint16_t *nflag, int n_cu, hipStream_t st)
{
	return launch_bam_write(w, MdRecord{nflag}, n_cu, st);
}

}  // namespace sk
