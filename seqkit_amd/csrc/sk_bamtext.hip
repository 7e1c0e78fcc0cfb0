// sk_bamtext.hip — the order-dependent and text halves of `sam fragments` and `sam count` over device columns
// (include/seqkit_hip.h: sk_bam_fragments_bed_dev, sk_count_order_check_dev).
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
	enum { kKeepTextPin = 7, kKeepText = 8 };
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
	uint8_t *d_text = (uint8_t *)sk::ctx_keep(c, kKeepText, (size_t)total + 16, false, &krc);
	if (!d_text) return krc;
	uint8_t *h_text = (uint8_t *)sk::ctx_keep(c, kKeepTextPin, (size_t)total + 16, true, &krc);
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
