// sk_bamcoverage.hip — the record passes of sk_bam_file_coverage (include/seqkit_hip.h): `sam coverage histogram`
// (src/sam_coverage_histogram.rs) over a verified BAM stream.
//
// The reference starts `samtools depth -a`, reads one text line per reference position back and counts the positions of every depth
// up to 10 000.  Here the depth is never laid out per position: memory and time follow the records, not the genome.
// A position's global coordinate is g = base[refID] + p, base = the running sum of l_ref over the header, in 64 bits.  A counted
// record (0 <= refID < n_ref, none of 0x4 0x100 0x200 0x400) covers the runs of its CIGAR: M = X cover and advance, D N advance, every
// other code does neither; covering ops with no D or N between them are one run; a run is cut to [0, l_ref).
// bam_cov_mark_kernel — a wave per BGZF block (sk_bamblock.h), a lane per record: the block's runs, the counted records, per
//   reference the bit "has a counted record" and, with BED intervals, the bit "has a counted record whose span [pos, end) overlaps an
//   interval" (binary search in that reference's merged intervals); decline bit 8 for a record whose variable part is shorter than
//   its fields.  A bit is set by an atomic OR only by a lane that has not read it set: a handful of atomics per reference, not one per record.
// bam_cov_emit_kernel — the same walk behind the scan of the blocks' runs: run q of the file writes events 2 q and 2 q + 1, (g_start,
//   kCovDepthUp) and (g_end, kCovDepthDown).  The target intervals follow as (g, kCovInsideUp) / (g, kCovInsideDown), written by the host: they are few.
// sk_bamminimize.hip's radix sort orders the events by g.  Events of one g stand in any order: the gap between them is zero.
// bam_cov_scan — one inclusive scan (rocprim) of depth + inside * 2^32 as one signed 64-bit sum: behind event i both running sums.
// bam_cov_hist_kernel — event i with inside > 0 and w = g[i + 1] - g[i] > 0 adds w to hist[depth], or for depth > 10 000 to the dropped
//   positions.  A workgroup sums in LDS, 10 001 32-bit counters (40 KB: four workgroups a CU) with the carry out of a counter added
//   to the global one by the lane that saw it wrap, and flushes the counters it touched; a gap of 2^16 positions or more, of which
//   a file has few, goes to the global counter at once.  No global atomic per event.
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
typedef long long i64;

constexpr int kCovThreads = 256;
constexpr int kCovBins = SK_COVERAGE_BINS;

struct CovDev {
	const uint8_t *stream;
	const u64 *bend, *entry;
	int64_t nb;
	CovArgs a;
};

// The runs of one record's CIGAR cut to [0, l_ref): f(start, end) for each that is not empty; returns their number, *end_out = the
// position behind the last reference-consuming op (pos without one).
template <class F>
__device__ __forceinline__ u32 cov_runs(const uint8_t *cg, u32 nc, i64 pos, i64 l_ref, i64 *end_out, const F &f)
{
	i64 p = pos, rs = 0;
	bool open = false;
	u32 n = 0u;
	auto close = [&]() {
		const i64 s = rs < 0 ? 0 : rs, e = p < l_ref ? p : l_ref;
		if (s < e) { f(s, e); n++; }
		open = false;
	};
	for (u32 q = 0; q < nc; q++) {
		const u32 op = bam_le32_bytes(cg + 4u * q), code = op & 15u;
		if (code == 0u || code == 7u || code == 8u) {
			if (!open) { rs = p; open = true; }
			p += op >> 4;
		} else if (code == 2u || code == 3u) {
			if (open) close();
			p += op >> 4;
		}
	}
	if (open) close();
	*end_out = p;
	return n;
}

// what both record passes read of a record: is it counted (valid, on a reference, none of 0x704), and then its reference, position,
// CIGAR and the reference's length.  *bad: its variable part is shorter than its fields.
struct CovRec { bool counted; int32_t tid; i64 pos, l_ref; u64 base; const uint8_t *cg; u32 nc; };
__device__ __forceinline__ CovRec cov_record(const uint8_t *r, const CovArgs &a, bool *bad)
{
	CovRec c;
	const u32 bs = bam_le32_bytes(r), lo = r[12], w16 = bam_le32_bytes(r + 16), S = bam_le32_bytes(r + 20);
	c.nc = w16 & 0xffffu;
	const u32 flag = w16 >> 16;
	c.tid = (int32_t)bam_le32_bytes(r + 4);
	c.pos = (int32_t)bam_le32_bytes(r + 8);
	c.cg = r + 36 + lo;
	c.counted = false; c.l_ref = 0; c.base = 0;
	if (bs < 32u || lo < 1u || S > 0x7fffffffu || 4ull * c.nc + lo + (((u64)S + 1) >> 1) + S > (u64)(bs - 32u)) { *bad = true; return c; }
	if (c.tid < 0 || c.tid >= a.n_ref || (flag & 0x704u)) return c;
	c.counted = true;
	c.base = a.base[c.tid];
	c.l_ref = (i64)(a.base[c.tid + 1] - c.base);
	return c;
}

__device__ __forceinline__ void cov_set_bit(u32 *bits, int32_t tid)
{
	const u32 m = 1u << (tid & 31);
	if (!(bits[tid >> 5] & m)) atomicOr(bits + (tid >> 5), m);
}

__global__ __launch_bounds__(kBlockThreads) void bam_cov_mark_kernel(const CovDev d)
{
	BlockPass b;
	if (!block_open(d.stream, d.entry, d.bend, d.nb, b)) return;
	const auto [lane, c, entry, n, off] = b;
	const CovArgs &a = d.a;
	u64 runs = 0, counted = 0;
	bool bad = false;
	for (u32 j = (u32)lane; j < n; j += 64u) {
		const CovRec r = cov_record(d.stream + entry + off[j], a, &bad);
		if (!r.counted) continue;
		counted++;
		i64 end = r.pos;
		runs += cov_runs(r.cg, r.nc, r.pos, r.l_ref, &end, [](i64, i64) {});
		cov_set_bit(a.has, r.tid);
		if (a.ioff) {
			if (end <= r.pos) end = r.pos + 1;
			// the first merged interval of the reference that ends behind pos: the only one the span can overlap first
			u32 lo = a.ioff[r.tid], hi = a.ioff[r.tid + 1];
			const u32 last = hi;
			while (lo < hi) {
				const u32 mid = lo + ((hi - lo) >> 1);
				if (a.iend[mid] > r.pos) hi = mid; else lo = mid + 1u;
			}
			if (lo < last && a.ibeg[lo] < end) cov_set_bit(a.hit, r.tid);
		}
	}
	for (int s = 32; s > 0; s >>= 1) {
		runs += __shfl_xor(runs, s);
		counted += __shfl_xor(counted, s);
	}
	if (lane == 0) {
		a.bruns[c] = runs;
		if (counted) atomicAdd(a.counted, counted);
	}
	if (__any((int)bad) && lane == 0) atomicOr(a.decline, 8u);
}

__global__ __launch_bounds__(kBlockThreads) void bam_cov_emit_kernel(const CovDev d, u64 *key, u32 *kind)
{
	// (block_open written out: with the helper this kernel measured 0.7 % slower, 1.909 against 1.896 ms on 20 M records)
	__shared__ uint16_t offs[kBlockWaves][kBlockRecs];
	const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	const int64_t c = (int64_t)blockIdx.x * kBlockWaves + w;
	if (c >= d.nb) return;
	uint16_t *off = offs[w];
	const u32 n = wave_record_offsets(d.stream, d.entry, d.bend, c, off, lane);
	const u64 entry = d.entry[c];
	const CovArgs &a = d.a;
	u64 q0 = a.bruns[c];                                                   // the block's first run
	const u64 q_end = a.bruns[c + 1];
	for (u32 j0 = 0; j0 < n; j0 += 64u) {
		const u32 j = j0 + (u32)lane;
		CovRec r;
		r.counted = false;
		bool bad = false;
		u64 mine = 0;
		i64 end = 0;
		if (j < n) {
			r = cov_record(d.stream + entry + off[j], a, &bad);
			if (r.counted) mine = cov_runs(r.cg, r.nc, r.pos, r.l_ref, &end, [](i64, i64) {});
		}
		const u64 il = wave_incl_scan(mine, lane);
		if (mine) {
			u64 q = q0 + il - mine;
			cov_runs(r.cg, r.nc, r.pos, r.l_ref, &end, [&](i64 s, i64 e) {
				if (q < q_end) {                                               // (what the mark pass counted: never beyond the block's share)
					key[2 * q] = r.base + (u64)s; kind[2 * q] = kCovDepthUp;
					key[2 * q + 1] = r.base + (u64)e; kind[2 * q + 1] = kCovDepthDown;
				}
				q++;
			});
		}
		q0 += __shfl(il, 63);
	}
}

struct CovDelta {
	__host__ __device__ i64 operator()(u32 kind) const
	{
		return kind == kCovDepthUp ? 1ll : kind == kCovDepthDown ? -1ll : kind == kCovInsideUp ? (1ll << 32) : -(1ll << 32);
	}
};

__global__ __launch_bounds__(kCovThreads) void bam_cov_hist_kernel(const u64 *key, const i64 *sums, u64 n, u64 *hist, u64 *totals)
{
	__shared__ u32 bins[kCovBins];
	for (int t = threadIdx.x; t < kCovBins; t += kCovThreads) bins[t] = 0u;
	__syncthreads();
	u64 n_pos = 0, n_drop = 0;
	for (u64 i = (u64)blockIdx.x * kCovThreads + threadIdx.x; i + 1 < n; i += (u64)gridDim.x * kCovThreads) {
		const i64 v = sums[i];
		const int32_t depth = (int32_t)(u32)(u64)v;
		const i64 inside = (v - (i64)depth) >> 32;
		const u64 w = key[i + 1] - key[i];
		if (inside <= 0 || w == 0) continue;
		n_pos += w;
		if ((u32)depth >= (u32)kCovBins) n_drop += w;                      // (behind a gap the depth is never negative)
		else if (w >= 65536ull) atomicAdd(hist + depth, w);
		else {
			const u32 old = atomicAdd(&bins[depth], (u32)w);
			if (old + (u32)w < old) atomicAdd(hist + depth, 1ull << 32);
		}
	}
	for (int s = 32; s > 0; s >>= 1) {
		n_pos += __shfl_xor(n_pos, s);
		n_drop += __shfl_xor(n_drop, s);
	}
	if ((threadIdx.x & 63) == 0) {
		if (n_pos) atomicAdd(totals, n_pos);
		if (n_drop) atomicAdd(totals + 1, n_drop);
	}
	__syncthreads();
	for (int t = threadIdx.x; t < kCovBins; t += kCovThreads) {
		const u32 v = bins[t];
		if (v) atomicAdd(hist + t, (u64)v);
	}
}

CovDev cov_dev(const uint8_t *stream, const uint64_t *bend, const uint64_t *entry, int64_t nb, const CovArgs &a)
{
	CovDev d;
	d.stream = stream; d.bend = (const u64 *)bend; d.entry = (const u64 *)entry; d.nb = nb; d.a = a;
	return d;
}

}  // namespace

hipError_t launch_bam_cov_mark(const uint8_t *stream, const uint64_t *bend, const uint64_t *entry, int64_t nb, const CovArgs &a, hipStream_t st)
{
	if (nb > 0) {
		bam_cov_mark_kernel<<<block_grid(nb), kBlockThreads, 0, st>>>(cov_dev(stream, bend, entry, nb, a));
		if (hipError_t e = hipGetLastError()) return e;
	}
	return launch_scan_u64(a.bruns, nb, st);
}

hipError_t launch_bam_cov_emit(const uint8_t *stream, const uint64_t *bend, const uint64_t *entry, int64_t nb, const CovArgs &a, uint64_t *key,
                               uint32_t *kind, hipStream_t st)
{
	if (nb <= 0) return hipSuccess;
	bam_cov_emit_kernel<<<block_grid(nb), kBlockThreads, 0, st>>>(cov_dev(stream, bend, entry, nb, a), (u64 *)key, kind);
	return hipGetLastError();
}

hipError_t bam_cov_scan(void *temp, size_t *temp_bytes, const uint32_t *kind, int64_t *sums, uint64_t n, hipStream_t st)
{
	auto delta = rocprim::make_transform_iterator(kind, CovDelta());
	if (!temp) return rocprim::inclusive_scan(nullptr, *temp_bytes, delta, (i64 *)sums, (size_t)n, rocprim::plus<i64>(), st);
	return rocprim::inclusive_scan(temp, *temp_bytes, delta, (i64 *)sums, (size_t)n, rocprim::plus<i64>(), st);
}

hipError_t launch_bam_cov_hist(const uint64_t *key, const int64_t *sums, uint64_t n, uint64_t *hist, uint64_t *totals, int n_cu, hipStream_t st)
{
	if (hipError_t e = hipMemsetAsync(hist, 0, (size_t)kCovBins * 8, st)) return e;
	if (hipError_t e = hipMemsetAsync(totals, 0, 16, st)) return e;
	if (n < 2) return hipSuccess;
	const u64 want = (n + kCovThreads - 1) / kCovThreads, cap = (u64)(n_cu > 0 ? n_cu : 256) * 4u;
	bam_cov_hist_kernel<<<(unsigned)(want < cap ? want : cap), kCovThreads, 0, st>>>((const u64 *)key, (const i64 *)sums, n, (u64 *)hist, (u64 *)totals);
	return hipGetLastError();
}

}  // namespace sk
