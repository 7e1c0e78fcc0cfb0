// sk_bamtext.hip — the order-dependent and text halves of `sam fragments` and `sam count` over device columns
// (include/seqkit_hip.h: sk_bam_fragments_bed_dev, sk_count_order_check_dev), and the passes behind sk_bam_file_reads (`sam to`).
//
// bam_bed_len_kernel / bam_bed_write_kernel — the BED line of every kept record (src/sam_fragments.rs:41), in record order.  A lane
// owns one byte of keep bits: 8 records.  The first pass sums each workgroup's line lengths, one workgroup turns the sums into
// offsets (bam_scan_u64_kernel), and the second pass recomputes the lengths, scans them inside the workgroup and writes the lines.
//
// count_order_tile_kernel / count_order_join_kernel — the loop of src/sam_count.rs:52-73 over the records its filter passes: each
// passing record is compared with the passing record before it (the initial state tid -1, pos 0 before the first).  A lane walks
// 16 records in order; inside a workgroup the predecessor of a lane's first passing record is the last passing record of the lanes
// before it (an LDS scan); the workgroups publish their first and last passing record and one workgroup checks the joins.  The
// answer is the smallest index at which the loop stops: every violation is checked against its true predecessor, so the smallest
// one is where the record-at-a-time loop ends.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <vector>

#include "../../include/seqkit_hip.h"
#include "sk_bamblock.h"
#include "sk_internal.h"

namespace sk {

typedef unsigned long long u64;

constexpr int kBedThreads = 256;                 // a lane = one keep byte = 8 records; a workgroup = 2048 records
constexpr int kScanThreads = 1024;

__device__ __forceinline__ uint32_t dec_digits(uint64_t v)
{
	uint32_t d = 1;
	while (v >= 10ull) { v /= 10ull; d++; }
	return d;
}
__device__ __forceinline__ uint32_t dec_len(int64_t v) { return v < 0 ? 1u + dec_digits(0ull - (uint64_t)v) : dec_digits((uint64_t)v); }
__device__ __forceinline__ uint8_t *dec_put(uint8_t *o, int64_t v)
{
	uint64_t m = (uint64_t)v;
	if (v < 0) { *o++ = '-'; m = 0ull - m; }
	const uint32_t d = dec_digits(m);
	for (uint32_t k = d; k-- > 0;) { o[k] = (uint8_t)('0' + m % 10ull); m /= 10ull; }
	return o + d;
}

struct BedArgs {
	const uint8_t *keep;
	const int32_t *tid, *pos, *tlen;
	int64_t n;
	const uint8_t *names;
	const u64 *name_off;
	int32_t n_ref;
	u64 *tile_sum;           // [tiles + 1]: sums, then (bam_scan_u64_kernel) exclusive offsets
	u64 *bad;                // smallest index of a kept record with a tid outside [0, n_ref)
	u64 *bad_off;            // where that record's line would begin
	uint8_t *text;
};

// the 8 records of keep byte k: their line lengths (0: not kept, or a bad tid)
__device__ __forceinline__ uint64_t bed_lens(const BedArgs &a, int64_t k, uint32_t len[8])
{
	uint64_t s = 0;
	const uint32_t bits = k * 8 < a.n ? a.keep[k] : 0u;
	for (int j = 0; j < 8; j++) {
		len[j] = 0u;
		const int64_t i = k * 8 + j;
		if (!(bits >> j & 1u) || i >= a.n) continue;
		const int32_t t = a.tid[i];
		if (t < 0 || t >= a.n_ref) { atomicMin(a.bad, (u64)i); continue; }
		const int64_t p = a.pos[i], tl = a.tlen[i];
		const int64_t e = p + (tl < 0 ? -tl : tl);
		len[j] = (uint32_t)(a.name_off[t + 1] - a.name_off[t]) + dec_len(p) + dec_len(e) + 3u;
		s += len[j];
	}
	return s;
}

__device__ __forceinline__ uint64_t block_sum_u64(uint64_t v, u64 *red)
{
	for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s);
	if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
	__syncthreads();
	uint64_t t = 0;
	for (int w = 0; w < (int)(blockDim.x >> 6); w++) t += red[w];
	return t;
}

// exclusive scan of one value per lane over the workgroup (blockDim.x <= 1024); *total = the sum
__device__ __forceinline__ uint64_t block_excl_scan_u64(uint64_t v, u64 *wsum, uint64_t *total)
{
	const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = (int)(blockDim.x >> 6);
	uint64_t x = v;
	for (int s = 1; s < 64; s <<= 1) {
		const uint64_t y = __shfl_up(x, s);
		if (lane >= s) x += y;
	}
	if (lane == 63) wsum[w] = x;
	__syncthreads();
	uint64_t before = 0, all = 0;
	for (int k = 0; k < nw; k++) { const uint64_t q = wsum[k]; if (k < w) before += q; all += q; }
	*total = all;
	return before + x - v;
}

__global__ __launch_bounds__(kBedThreads) void bam_bed_len_kernel(const BedArgs a)
{
	__shared__ u64 red[kBedThreads / 64];
	const int64_t k = (int64_t)blockIdx.x * kBedThreads + threadIdx.x;
	uint32_t len[8];
	const uint64_t s = bed_lens(a, k, len);
	const uint64_t t = block_sum_u64(s, red);
	if (threadIdx.x == 0) a.tile_sum[blockIdx.x] = t;
}

// v[0 .. n) -> exclusive offsets, v[n] = the sum; one workgroup
__global__ __launch_bounds__(kScanThreads) void bam_scan_u64_kernel(u64 *v, int64_t n)
{
	__shared__ u64 wsum[kScanThreads / 64];
	const int64_t per = (n + kScanThreads - 1) / kScanThreads;
	const int64_t lo = (int64_t)threadIdx.x * per, hi = lo + per < n ? lo + per : n;
	uint64_t s = 0;
	for (int64_t i = lo; i < hi; i++) s += v[i];
	uint64_t total;
	uint64_t run = block_excl_scan_u64(s, wsum, &total);
	for (int64_t i = lo; i < hi; i++) { const uint64_t x = v[i]; v[i] = run; run += x; }
	if (threadIdx.x == 0) v[n] = total;
}

__global__ __launch_bounds__(kBedThreads) void bam_bed_write_kernel(const BedArgs a)
{
	__shared__ u64 wsum[kBedThreads / 64];
	const int64_t k = (int64_t)blockIdx.x * kBedThreads + threadIdx.x;
	uint32_t len[8];
	const uint64_t s = bed_lens(a, k, len);
	uint64_t total;
	uint64_t at = a.tile_sum[blockIdx.x] + block_excl_scan_u64(s, wsum, &total);
	const u64 bad = *a.bad;
	for (int j = 0; j < 8; j++) {
		const int64_t i = k * 8 + j;
		if ((u64)i == bad) *a.bad_off = at;
		if (!len[j]) continue;
		const int32_t t = a.tid[i];
		const int64_t p = a.pos[i], tl = a.tlen[i];
		uint8_t *o = a.text + at;
		const u64 nb = a.name_off[t], ne = a.name_off[t + 1];
		for (u64 b = nb; b < ne; b++) *o++ = a.names[b];
		*o++ = '\t';
		o = dec_put(o, p);
		*o++ = '\t';
		o = dec_put(o, p + (tl < 0 ? -tl : tl));
		*o = '\n';
		at += len[j];
	}
}

// ---- sam count's order checks ----------------------------------------------------------------------------------------
constexpr int kOrdThreads = 256, kOrdPer = 16, kOrdTile = kOrdThreads * kOrdPer;

struct OrdArgs {
	const uint16_t *flag;
	const uint8_t *mapq;
	const int32_t *tid, *pos;
	int64_t n;
	uint32_t min_mapq;
	int32_t n_ref;
	int64_t *t_first;        // [tiles]: index of the tile's first passing record, -1 if none
	int32_t *t_ftid, *t_fpos, *t_ltid, *t_lpos;   // [tiles]: its tid / pos, and the last passing record's
	u64 *stop;               // min over (index << 1 | (1 = order, 0 = tid)) of the violations
};

__device__ __forceinline__ bool ord_pass(const OrdArgs &a, int64_t i)
{
	const uint32_t f = a.flag[i];
	return !(f & (0x4u | 0x400u | 0x100u | 0x800u)) && (uint32_t)a.mapq[i] >= a.min_mapq;          // src/sam_count.rs:46-49
}
// the record (tid, pos) against the state (ptid, ppos) its predecessor left: src/sam_count.rs:52-73
__device__ __forceinline__ void ord_check(const OrdArgs &a, int32_t ptid, int32_t ppos, int32_t tid, int32_t pos, int64_t i)
{
	if (tid != ptid) {
		if (tid < 0 || tid >= a.n_ref) atomicMin(a.stop, (u64)i << 1);
	} else if (pos < ppos) {
		atomicMin(a.stop, ((u64)i << 1) | 1ull);
	}
}

// inclusive "last non-empty" scan of (has, tid, pos) over the workgroup's lanes, in LDS; returns the state before lane t
__device__ __forceinline__ bool ord_pred(bool has, int32_t tid, int32_t pos, int32_t *s_has, int32_t *s_tid, int32_t *s_pos, int32_t &ptid, int32_t &ppos)
{
	const int t = threadIdx.x, nt = (int)blockDim.x;
	s_has[t] = has; s_tid[t] = tid; s_pos[t] = pos;
	__syncthreads();
	for (int d = 1; d < nt; d <<= 1) {
		int32_t h = 0, ti = 0, po = 0;
		const bool take = t >= d && !s_has[t];
		if (take) { h = s_has[t - d]; ti = s_tid[t - d]; po = s_pos[t - d]; }
		__syncthreads();
		if (take && h) { s_has[t] = 1; s_tid[t] = ti; s_pos[t] = po; }
		__syncthreads();
	}
	const bool any = t > 0 && s_has[t - 1];
	if (any) { ptid = s_tid[t - 1]; ppos = s_pos[t - 1]; }
	return any;
}

__global__ __launch_bounds__(kOrdThreads) void count_order_tile_kernel(const OrdArgs a)
{
	__shared__ int32_t s_has[kOrdThreads], s_tid[kOrdThreads], s_pos[kOrdThreads];
	__shared__ int64_t s_first;
	const int64_t i0 = (int64_t)blockIdx.x * kOrdTile + (int64_t)threadIdx.x * kOrdPer;
	bool has = false;
	int64_t first = -1;
	int32_t ftid = 0, fpos = 0, ltid = 0, lpos = 0;
	for (int j = 0; j < kOrdPer; j++) {
		const int64_t i = i0 + j;
		if (i >= a.n) break;
		if (!ord_pass(a, i)) continue;
		const int32_t t = a.tid[i], p = a.pos[i];
		if (!has) { has = true; first = i; ftid = t; fpos = p; }
		else ord_check(a, ltid, lpos, t, p, i);
		ltid = t; lpos = p;
	}
	if (threadIdx.x == 0) s_first = -1;
	int32_t ptid = 0, ppos = 0;
	const bool pred = ord_pred(has, ltid, lpos, s_has, s_tid, s_pos, ptid, ppos);
	if (has && pred) ord_check(a, ptid, ppos, ftid, fpos, first);
	if (has && !pred) {                                                   // the workgroup's first passing record: its predecessor is another tile's
		s_first = first;
		a.t_ftid[blockIdx.x] = ftid; a.t_fpos[blockIdx.x] = fpos;
	}
	if (threadIdx.x == blockDim.x - 1) {                                 // (the scan's last entry: the workgroup's last passing record)
		a.t_ltid[blockIdx.x] = s_tid[threadIdx.x]; a.t_lpos[blockIdx.x] = s_pos[threadIdx.x];
	}
	__syncthreads();
	if (threadIdx.x == 0) a.t_first[blockIdx.x] = s_first;
}

// the joins: every tile's first passing record against the last passing record of the tiles before it (tid -1, pos 0 when none)
__global__ __launch_bounds__(kScanThreads) void count_order_join_kernel(const OrdArgs a, int64_t tiles)
{
	__shared__ int32_t s_has[kScanThreads], s_tid[kScanThreads], s_pos[kScanThreads];
	const int64_t per = (tiles + kScanThreads - 1) / kScanThreads;
	const int64_t lo = (int64_t)threadIdx.x * per, hi = lo + per < tiles ? lo + per : tiles;
	bool has = false;
	int32_t ltid = 0, lpos = 0;
	for (int64_t b = lo; b < hi; b++)
		if (a.t_first[b] >= 0) { has = true; ltid = a.t_ltid[b]; lpos = a.t_lpos[b]; }
	int32_t ptid = -1, ppos = 0;                                           // src/sam_count.rs:40-41
	(void)ord_pred(has, ltid, lpos, s_has, s_tid, s_pos, ptid, ppos);
	for (int64_t b = lo; b < hi; b++) {
		const int64_t f = a.t_first[b];
		if (f < 0) continue;
		ord_check(a, ptid, ppos, a.t_ftid[b], a.t_fpos[b], f);
		ptid = a.t_ltid[b]; ppos = a.t_lpos[b];
	}
}

// ---- sam to raw|fasta|fastq: the reads of a verified BAM stream (sk_bam_file_reads) ------------------------------------------
// bam_reads_size_kernel / bam_reads_index_kernel — a wave per BGZF block follows the chain from entry[c] (sk_bamblock.h: lane 0
// leaves the records' offsets in LDS, then the lanes take consecutive records).  The first pass sums, per block, the kept records,
// their text bytes and their name bytes, and ORs every record's decline bits; after the scans, the second pass writes the kept
// records' columns at their kept index: stream offset, text offset, name offset, kind and qname key.
// bam_window_kernel — where each window of at most W bytes begins (the reads' text + name bytes; sk_bamwrite.hip's rewritten bytes).
// bam_reads_text_kernel — the text of one window: a 16-lane group owns a record and covers its output in consecutive dwords, each
// composed by output address (the dwords it shares with its neighbours are written bytewise).

struct ReadsArgs {
	const uint8_t *stream;
	const u64 *bend, *entry;
	int64_t nb;
	int fmt, want_unpaired;
	u64 *bk, *bt, *bn;       // [nb + 1]: per block kept records / text bytes / name bytes, then (bam_scan_u64_kernel) exclusive offsets
	uint32_t *decline;       // OR of the records' decline bits: 1 qname byte >= 0x80, 2 fastq quality, 4 l_seq > 65532, 8 invalid record
	u64 *krec, *ktoff, *knoff, *kkey;
	uint8_t *kkind;
};

struct ReadRec { uint32_t kept, kind, tlen, nlen; };

// the record at r: kept or not, its kind and text length (src/sam_to_fastq.rs:102,114-130,138-149); with `decline`, the reasons the
// host reader must serve the file instead (include/seqkit_hip.h)
__device__ __forceinline__ ReadRec reads_rec(const uint8_t *r, int fmt, int want_unpaired, uint32_t *decline)
{
	ReadRec o{0u, 0u, 0u, 0u};
	const uint32_t bs = bam_le32_bytes(r), w12 = bam_le32_bytes(r + 12), w16 = bam_le32_bytes(r + 16), S = bam_le32_bytes(r + 20);
	const uint32_t l_name = w12 & 0xffu, n_cigar = w16 & 0xffffu, f = w16 >> 16;
	if (bs < 32u || l_name < 1u || S > 0x7fffffffu || 4ull * n_cigar + l_name + (((u64)S + 1) >> 1) + S > (u64)(bs - 32u)) {
		if (decline) *decline |= 8u;                                       // htslib: "Invalid BAM record."
		return o;
	}
	if (f & (0x100u | 0x800u)) return o;                                   // :102
	const uint32_t L = l_name - 1u;
	if (decline) {
		uint32_t d = 0u;
		if (S > 65532u) d |= 4u;
		const uint8_t *nm = r + 36;
		for (uint32_t k = 0; k < L; k++) d |= (nm[k] & 0x80u) ? 1u : 0u;                  // :104 str::from_utf8
		if (fmt == 2 && S <= 65532u) {
			const uint8_t *q = nm + l_name + 4u * n_cigar + ((S + 1u) >> 1);
			uint32_t hi = 0u;
			for (uint32_t k = 0; k < S; k++) hi |= (uint32_t)(uint8_t)(33u + q[k]);     // char::from(33 + q) >= 0x80: two bytes
			if (hi & 0x80u) d |= 2u;
		}
		*decline |= d;
	}
	o.kind = !(f & 0x1u) ? 0u : (f & 0x40u) ? 1u : (f & 0x80u) ? 2u : 3u;
	o.kept = o.kind == 0u ? (want_unpaired ? 1u : 0u) : (o.kind != 3u ? 1u : 0u);
	if (!o.kept) return o;
	o.nlen = L;
	o.tlen = fmt == 2 ? L + 2u * S + 6u : fmt == 1 ? L + S + 3u : S + 1u;
	return o;
}

__global__ __launch_bounds__(kBlockThreads) void bam_reads_size_kernel(const ReadsArgs a)
{
	BlockPass b;
	if (!block_open(a.stream, a.entry, a.bend, a.nb, b)) return;
	const auto [lane, c, entry, n, off] = b;
	u64 kept = 0, tb = 0, nb = 0;
	uint32_t dec = 0u;
	for (uint32_t j = (uint32_t)lane; j < n; j += 64u) {
		const ReadRec rr = reads_rec(a.stream + entry + off[j], a.fmt, a.want_unpaired, &dec);
		kept += rr.kept; tb += rr.tlen; nb += rr.nlen;
	}
	for (int s = 32; s > 0; s >>= 1) {
		kept += __shfl_xor(kept, s); tb += __shfl_xor(tb, s); nb += __shfl_xor(nb, s);
		dec |= (uint32_t)__shfl_xor((int)dec, s);
	}
	if (lane == 0) {
		a.bk[c] = kept; a.bt[c] = tb; a.bn[c] = nb;
		if (dec) atomicOr(a.decline, dec);
	}
}

__global__ __launch_bounds__(kBlockThreads) void bam_reads_index_kernel(const ReadsArgs a)
{
	BlockPass b;
	if (!block_open(a.stream, a.entry, a.bend, a.nb, b)) return;
	const auto [lane, c, entry, n, off] = b;
	u64 kb = a.bk[c], tb = a.bt[c], nb = a.bn[c];                       // where the block's first kept record goes
	for (uint32_t j0 = 0; j0 < n; j0 += 64u) {
		const uint32_t j = j0 + (uint32_t)lane;
		ReadRec rr{0u, 0u, 0u, 0u};
		const uint8_t *r = a.stream + entry + (j < n ? off[j] : 0);
		if (j < n) rr = reads_rec(r, a.fmt, a.want_unpaired, nullptr);
		const u64 ik = wave_incl_scan(rr.kept, lane), it = wave_incl_scan(rr.tlen, lane), in = wave_incl_scan(rr.nlen, lane);
		if (rr.kept) {
			const u64 k = kb + ik - 1;
			a.krec[k] = entry + off[j];
			a.ktoff[k] = tb + it - rr.tlen;
			a.knoff[k] = nb + in - rr.nlen;
			a.kkind[k] = (uint8_t)rr.kind;
			a.kkey[k] = qname_key(r + 36, rr.nlen);
		}
		kb += __shfl(ik, 63); tb += __shfl(it, 63); nb += __shfl(in, 63);
	}
}

// window w = the records whose key off0[j] + off1[j] (off1 == nullptr: off0[j]) lies in [w W, (w + 1) W): ws[w] its first record, w0[w]
// / w1[w] its off0 / off1; entries past the last record's window hold (n, total0, total1).  nw entries in all.
__global__ __launch_bounds__(256) void bam_window_kernel(const u64 *off0, const u64 *off1, int64_t n, u64 W, u64 total0, u64 total1, u64 *ws, u64 *w0,
                                                         u64 *w1, int64_t nw)
{
	const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (j >= n) return;
	const u64 cur = (off0[j] + (off1 ? off1[j] : 0)) / W;
	const u64 from = j ? (off0[j - 1] + (off1 ? off1[j - 1] : 0)) / W + 1 : 0;
	for (u64 v = from; v <= cur && (int64_t)v < nw; v++) { ws[v] = (u64)j; w0[v] = off0[j]; if (off1) w1[v] = off1[j]; }
	if (j == n - 1)
		for (int64_t v = (int64_t)cur + 1; v < nw; v++) { ws[v] = (u64)n; w0[v] = total0; if (off1) w1[v] = total1; }
}

struct ReadsText {
	const uint8_t *stream;
	const u64 *krec, *ktoff, *knoff;
	int64_t first, n;
	u64 t0, n0;
	int fmt;
	uint32_t min_baseq;
	uint8_t *text, *names;
	u64 *toff;
	uint32_t *noff;
};

constexpr int kTextThreads = kGroupThreads;      // (launched on group_grid)
__global__ __launch_bounds__(kTextThreads) void bam_reads_text_kernel(const ReadsText a)
{
	const int gl = threadIdx.x & 15;
	const int64_t gstride = ((int64_t)gridDim.x * kTextThreads) >> 4;
	for (int64_t j = ((int64_t)blockIdx.x * kTextThreads + threadIdx.x) >> 4; j < a.n; j += gstride) {
		const int64_t k = a.first + j;
		const uint8_t *r = a.stream + a.krec[k];
		const uint32_t w12 = bam_le32_bytes(r + 12), w16 = bam_le32_bytes(r + 16), S = bam_le32_bytes(r + 20);
		const uint32_t l_name = w12 & 0xffu, n_cigar = w16 & 0xffffu, L = l_name - 1u;
		const bool rev = (w16 >> 16) & 0x10u;
		const uint8_t *name = r + 36, *seq4 = name + l_name + 4u * n_cigar, *qual = seq4 + ((S + 1u) >> 1);
		const uint32_t tlen = a.fmt == 2 ? L + 2u * S + 6u : a.fmt == 1 ? L + S + 3u : S + 1u;
		const u64 tb = a.ktoff[k] - a.t0, nbo = a.knoff[k] - a.n0;
		if (gl == 0) {
			a.toff[j] = tb; a.noff[j] = (uint32_t)nbo;
			if (j == a.n - 1) { a.toff[a.n] = tb + tlen; a.noff[a.n] = (uint32_t)(nbo + L); }
		}
		for (uint32_t q = (uint32_t)gl; q < L; q += 16u) a.names[nbo + q] = name[q];
		const u64 te = tb + tlen, d0 = tb >> 2, d1 = (te - 1) >> 2;
		for (u64 d = d0 + (u64)gl; d <= d1; d += 16u) {
			const u64 p0 = d << 2;
			if (p0 >= tb && p0 + 4 <= te) {
				const uint32_t p = (uint32_t)(p0 - tb);
				uint32_t wv = 0u;
				for (uint32_t b = 0; b < 4u; b++) wv |= reads_byte(p + b, a.fmt, name, L, seq4, qual, S, rev, a.min_baseq) << (8u * b);
				*reinterpret_cast<uint32_t *>(a.text + p0) = wv;
			} else {
				for (uint32_t b = 0; b < 4u; b++) {
					const u64 pp = p0 + b;
					if (pp >= tb && pp < te) a.text[pp] = (uint8_t)reads_byte((uint32_t)(pp - tb), a.fmt, name, L, seq4, qual, S, rev, a.min_baseq);
				}
			}
		}
	}
}

}  // namespace sk

namespace {
struct DevTmp {                                  // device scratch of one call, freed whichever way the call is left
	std::vector<void *> p;
	hipStream_t st = nullptr;
	~DevTmp() { if (st) (void)hipStreamSynchronize(st); for (void *q : p) (void)hipFree(q); }
	void *get(size_t bytes)
	{
		void *q = nullptr;
		if (hipMalloc(&q, bytes ? bytes : 16) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
		p.push_back(q);
		return q;
	}
};
inline bool a16(const void *p) { return ((uintptr_t)p & 15u) == 0; }
}  // namespace

#define BT_HIP(c, call)                                                                                                 \
	do {                                                                                                                \
		hipError_t e_ = (call);                                                                                         \
		if (e_ != hipSuccess) return sk::ctx_fail(c, SK_ERR_HIP, "%s: %s", #call, hipGetErrorString(e_));               \
	} while (0)

extern "C" int sk_bam_fragments_bed_dev(sk_ctx *c, const uint8_t *keep_bits, const int32_t *tid, const int32_t *pos, const int32_t *tlen, int64_t n,
                                        const uint8_t *names, const uint64_t *name_off, int32_t n_ref, const char **text, uint64_t *text_len, int64_t *bad)
{
	if (!c || !text || !text_len || !bad) return SK_ERR_INVALID;
	*text = nullptr; *text_len = 0; *bad = -1;
	if (n < 0 || n_ref < 0 || (n_ref > 0 && (!names || !name_off))) return sk::ctx_fail(c, SK_ERR_INVALID, "n = %lld, n_ref = %d", (long long)n, n_ref);
	if (n > 0 && (!keep_bits || !tid || !pos || !tlen)) return sk::ctx_fail(c, SK_ERR_INVALID, "NULL keep_bits or column");
	if (!a16(tid) || !a16(pos) || !a16(tlen)) return sk::ctx_fail(c, SK_ERR_INVALID, "columns must be 16-byte aligned");
	if (n_ref > 0 && name_off[0] != 0) return sk::ctx_fail(c, SK_ERR_INVALID, "name_off[0] must be 0");
	for (int32_t r = 0; r < n_ref; r++) if (name_off[r + 1] < name_off[r]) return sk::ctx_fail(c, SK_ERR_INVALID, "name_off must not decrease");
	if (int r = sk::ctx_bind(c)) return r;
	hipStream_t st = sk::ctx_stream(c);
	DevTmp tmp;
	tmp.st = st;
	const int64_t kbytes = (n + 7) / 8, tiles = (kbytes + sk::kBedThreads - 1) / sk::kBedThreads;
	const uint64_t name_bytes = n_ref > 0 ? name_off[n_ref] : 0;
	uint8_t *d_names = (uint8_t *)tmp.get((size_t)name_bytes);
	uint64_t *d_off = (uint64_t *)tmp.get((size_t)(n_ref + 1) * 8);
	uint64_t *d_tile = (uint64_t *)tmp.get((size_t)(tiles + 1) * 8 + 16);
	uint64_t *d_bad = d_tile + tiles + 1;
	if (!d_names || !d_off || !d_tile) return sk::ctx_fail(c, SK_ERR_NOMEM, "sk_bam_fragments_bed_dev: device scratch");
	std::vector<uint64_t> off0((size_t)n_ref + 1, 0);
	if (n_ref > 0) std::copy(name_off, name_off + n_ref + 1, off0.begin());
	if (name_bytes) BT_HIP(c, hipMemcpyAsync(d_names, names, (size_t)name_bytes, hipMemcpyHostToDevice, st));
	BT_HIP(c, hipMemcpyAsync(d_off, off0.data(), off0.size() * 8, hipMemcpyHostToDevice, st));
	BT_HIP(c, hipMemsetAsync(d_bad, 0xff, 8, st));
	BT_HIP(c, hipMemsetAsync(d_bad + 1, 0, 8, st));
	sk::BedArgs a;
	a.keep = keep_bits; a.tid = tid; a.pos = pos; a.tlen = tlen; a.n = n; a.names = d_names; a.name_off = (const sk::u64 *)d_off; a.n_ref = n_ref;
	a.tile_sum = (sk::u64 *)d_tile; a.bad = (sk::u64 *)d_bad; a.bad_off = (sk::u64 *)(d_bad + 1); a.text = nullptr;
	if (tiles > 0) {
		sk::bam_bed_len_kernel<<<(unsigned)tiles, sk::kBedThreads, 0, st>>>(a);
		BT_HIP(c, hipGetLastError());
	}
	sk::bam_scan_u64_kernel<<<1, sk::kScanThreads, 0, st>>>((sk::u64 *)d_tile, tiles);
	BT_HIP(c, hipGetLastError());
	uint64_t hb[3] = {0, 0, 0};                                           // total, bad
	BT_HIP(c, hipMemcpyAsync(hb, d_tile + tiles, 16, hipMemcpyDeviceToHost, st));
	BT_HIP(c, hipStreamSynchronize(st));
	const uint64_t total = hb[0];
	int krc = SK_OK;
	uint8_t *d_text = (uint8_t *)sk::ctx_keep(c, sk::kKeepText, (size_t)total + 16, false, &krc);
	if (!d_text) return krc;
	uint8_t *h_text = (uint8_t *)sk::ctx_keep(c, sk::kKeepTextPin, (size_t)total + 16, true, &krc);
	if (!h_text) return krc;
	a.text = d_text;
	if (tiles > 0) {
		sk::bam_bed_write_kernel<<<(unsigned)tiles, sk::kBedThreads, 0, st>>>(a);
		BT_HIP(c, hipGetLastError());
	}
	BT_HIP(c, hipMemcpyAsync(hb + 1, d_bad, 16, hipMemcpyDeviceToHost, st));
	BT_HIP(c, hipStreamSynchronize(st));
	const bool has_bad = hb[1] != ~0ull;
	const uint64_t len = has_bad ? hb[2] : total;
	if (len) BT_HIP(c, hipMemcpyAsync(h_text, d_text, (size_t)len, hipMemcpyDeviceToHost, st));
	BT_HIP(c, hipStreamSynchronize(st));
	*text = (const char *)h_text;
	*text_len = len;
	*bad = has_bad ? (int64_t)hb[1] : -1;
	return SK_OK;
}

extern "C" int sk_count_order_check_dev(sk_ctx *c, const uint16_t *flag, const uint8_t *mapq, const int32_t *tid, const int32_t *pos, int64_t n,
                                        uint8_t min_mapq, int32_t n_ref, int64_t *first_stop, int *code)
{
	if (!c || !first_stop || !code) return SK_ERR_INVALID;
	*first_stop = -1; *code = 0;
	if (n < 0) return sk::ctx_fail(c, SK_ERR_INVALID, "n = %lld", (long long)n);
	if (n == 0) return SK_OK;
	if (!flag || !mapq || !tid || !pos) return sk::ctx_fail(c, SK_ERR_INVALID, "NULL column");
	if (!a16(flag) || !a16(mapq) || !a16(tid) || !a16(pos)) return sk::ctx_fail(c, SK_ERR_INVALID, "columns must be 16-byte aligned");
	if (int r = sk::ctx_bind(c)) return r;
	hipStream_t st = sk::ctx_stream(c);
	DevTmp tmp;
	tmp.st = st;
	const int64_t tiles = (n + sk::kOrdTile - 1) / sk::kOrdTile;
	uint8_t *p = (uint8_t *)tmp.get((size_t)tiles * 24 + 64);
	if (!p) return sk::ctx_fail(c, SK_ERR_NOMEM, "sk_count_order_check_dev: device scratch");
	sk::OrdArgs a;
	a.flag = flag; a.mapq = mapq; a.tid = tid; a.pos = pos; a.n = n; a.min_mapq = min_mapq; a.n_ref = n_ref;
	a.stop = (sk::u64 *)p;
	a.t_first = (int64_t *)(p + 16);
	a.t_ftid = (int32_t *)(a.t_first + tiles); a.t_fpos = a.t_ftid + tiles; a.t_ltid = a.t_fpos + tiles; a.t_lpos = a.t_ltid + tiles;
	BT_HIP(c, hipMemsetAsync(a.stop, 0xff, 8, st));
	sk::count_order_tile_kernel<<<(unsigned)tiles, sk::kOrdThreads, 0, st>>>(a);
	BT_HIP(c, hipGetLastError());
	sk::count_order_join_kernel<<<1, sk::kScanThreads, 0, st>>>(a, tiles);
	BT_HIP(c, hipGetLastError());
	uint64_t s = 0;
	BT_HIP(c, hipMemcpyAsync(&s, a.stop, 8, hipMemcpyDeviceToHost, st));
	BT_HIP(c, hipStreamSynchronize(st));
	if (s != ~0ull) { *first_stop = (int64_t)(s >> 1); *code = (s & 1ull) ? 255 : 101; }
	return SK_OK;
}

// ---- launchers of the reads passes and the window plan (sk_bamfile_reads.cpp: sk_bam_file_reads; sk_bamfile_out.cpp: sk_bam_file_rewrite) ------------------
namespace sk {
hipError_t launch_bam_reads_size(const uint8_t *stream, const uint64_t *bend, const uint64_t *entry, int64_t nb, int fmt, int want_unpaired,
                                 uint64_t *bk, uint64_t *bt, uint64_t *bn, uint32_t *decline, hipStream_t st)
{
	ReadsArgs a{};
	a.stream = stream; a.bend = (const u64 *)bend; a.entry = (const u64 *)entry; a.nb = nb; a.fmt = fmt; a.want_unpaired = want_unpaired;
	a.bk = (u64 *)bk; a.bt = (u64 *)bt; a.bn = (u64 *)bn; a.decline = decline;
	if (nb > 0) {
		bam_reads_size_kernel<<<block_grid(nb), kBlockThreads, 0, st>>>(a);
		if (hipError_t e = hipGetLastError()) return e;
	}
	for (u64 *v : {a.bk, a.bt, a.bn}) {
		bam_scan_u64_kernel<<<1, kScanThreads, 0, st>>>(v, nb);
		if (hipError_t e = hipGetLastError()) return e;
	}
	return hipSuccess;
}

// v[0 .. n) -> exclusive offsets, v[n] = the sum (sk_bamwrite.hip's passes)
hipError_t launch_scan_u64(uint64_t *v, int64_t n, hipStream_t st)
{
	bam_scan_u64_kernel<<<1, kScanThreads, 0, st>>>((u64 *)v, n);
	return hipGetLastError();
}

hipError_t launch_bam_reads_index(const uint8_t *stream, const uint64_t *bend, const uint64_t *entry, int64_t nb, int fmt, int want_unpaired,
                                  const uint64_t *bk, const uint64_t *bt, const uint64_t *bn, uint64_t *krec, uint64_t *ktoff, uint64_t *knoff,
                                  uint64_t *kkey, uint8_t *kkind, hipStream_t st)
{
	if (nb <= 0) return hipSuccess;
	ReadsArgs a{};
	a.stream = stream; a.bend = (const u64 *)bend; a.entry = (const u64 *)entry; a.nb = nb; a.fmt = fmt; a.want_unpaired = want_unpaired;
	a.bk = (u64 *)bk; a.bt = (u64 *)bt; a.bn = (u64 *)bn;
	a.krec = (u64 *)krec; a.ktoff = (u64 *)ktoff; a.knoff = (u64 *)knoff; a.kkey = (u64 *)kkey; a.kkind = kkind;
	bam_reads_index_kernel<<<block_grid(nb), kBlockThreads, 0, st>>>(a);
	return hipGetLastError();
}

hipError_t launch_bam_windows(const uint64_t *off0, const uint64_t *off1, int64_t n, uint64_t W, uint64_t total0, uint64_t total1, uint64_t *ws,
                              uint64_t *w0, uint64_t *w1, int64_t nw, hipStream_t st)
{
	if (n <= 0) return hipSuccess;
	bam_window_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>((const u64 *)off0, (const u64 *)off1, n, W, total0, total1, (u64 *)ws, (u64 *)w0,
	                                                                (u64 *)w1, nw);
	return hipGetLastError();
}

hipError_t launch_bam_reads_text(const uint8_t *stream, const uint64_t *krec, const uint64_t *ktoff, const uint64_t *knoff, int64_t first, int64_t n,
                                 uint64_t t0, uint64_t n0, int fmt, uint8_t min_baseq, uint8_t *text, uint64_t *toff, uint8_t *names, uint32_t *noff,
                                 int n_cu, hipStream_t st)
{
	if (n <= 0) return hipSuccess;
	ReadsText a;
	a.stream = stream; a.krec = (const u64 *)krec; a.ktoff = (const u64 *)ktoff; a.knoff = (const u64 *)knoff; a.first = first; a.n = n;
	a.t0 = t0; a.n0 = n0; a.fmt = fmt; a.min_baseq = min_baseq; a.text = text; a.toff = (u64 *)toff; a.names = names; a.noff = noff;
	bam_reads_text_kernel<<<group_grid(n, n_cu), kTextThreads, 0, st>>>(a);
	return hipGetLastError();
}
}  // namespace sk
