// sk_bamminimize.hip — the record passes of sk_bam_file_minimize (include/seqkit_hip.h): `sam minimize` (src/sam_minimize.rs) over a
// verified BAM stream.  The BGZF half (cut, deflate, pack) is sk_bamwrite.hip's and sk_deflate.hip's, unchanged.
//
// The read ids.  The reference keeps a map from a read's key — its name up to the first '/' — to a number: a key that is in the map
// takes the stored number and LEAVES the map, any other key takes the next number and enters it.  So the 1st, 3rd, 5th .. record of a
// key opens a number and the 2nd, 4th .. takes the number of the one just before it.  In data-parallel form:
// bam_min_key_kernel — a wave per BGZF block (sk_bamblock.h): per record its stream offset, the 64-bit hash of its key (qname_key,
//   cut to SK_MINIMIZE_KEY_BITS) and its index; invalid records set decline bit 8.
// a stable radix sort of (hash, index) by hash (rocprim::radix_sort_pairs): equal hashes stay in file order.
// bam_min_run_kernel — in sorted order a run is a stretch of equal hashes.  Where a run starts is a max-scan of the head positions
//   (a wave per tile of 1024 elements: min_agg_kernel, min_tile_scan_kernel, then the wave's own scan with its carry), so runs of any
//   length — a file whose names all begin with '/' is one run — cost the same.  An element whose key BYTES differ from its
//   predecessor's in the run sets decline bit 64 (a hash collision: the caller's reader serves the file).  With r the rank in the run:
//   r even: the record opens a number, src[idx] = idx; r odd: src[idx] = the index one place before it.
// bam_min_open_scan_kernel / bam_min_id_kernel — the inclusive count of openers in RECORD order, then id[k] = count[src[k]].
// The id passes serve sk_bam_file_subsample too (sk_bamsubsample.hip), under its IdRule (sk_internal.h): the whole name is the key, and
// a record with flag 0x800 takes no part — its key is the bit above the hash's alone, so it sorts behind every record that does, the run
// pass gives it no source (kNoSrc: neither an opener nor anybody's predecessor) and its id is 0.
//
// The records.  min_plan says what the flags make of one record (the name replaced by the id's digits or kept; `set`: only core, name,
// CIGAR, bases and qualities stay, the odd base count's pad nibble is cleared, the qualities are copied or filled), and
// bam_min_size_kernel / bam_min_index_kernel / MinRecord in bam_write_kernel follow sk_bamwrite.hip's three passes: per-block sums and decline
// bits (32: a CIGAR operation code above 8, where rust-htslib's cigar() panics), every record's output offset, and a window's bytes —
// the copied spans (core and kept name; CIGAR and bases; qualities or everything behind the name) as whole dwords through emit, the
// rest byte by byte.
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

constexpr int kMinThreads = 256;                  // scan kernels: 4 waves, a tile each
constexpr u32 kTile = 1024;                       // elements a wave scans: 16 rounds of 64
constexpr u32 kNoSrc = ~0u;                       // src of a record that takes no part (no record has this index: there are fewer than 2^32)

__device__ __forceinline__ u32 id_digits(u32 v)
{
	u32 d = 1u;
	while (v >= 10u) { v /= 10u; d++; }
	return d;
}

// is the record one htslib reads (sk_bamwrite.hip: rw_plan's bit 8)
__device__ __forceinline__ bool min_valid(const uint8_t *r)
{
	const u32 bs = bam_le32_bytes(r), lo = r[12], nc = bam_le32_bytes(r + 16) & 0xffffu, S = bam_le32_bytes(r + 20);
	return !(bs < 32u || lo < 1u || S > 0x7fffffffu || 4ull * nc + lo + (((u64)S + 1) >> 1) + S > (u64)(bs - 32u));
}

// the bytes of a valid record's key: its name up to the first '/', or (whole) all of it
__device__ __forceinline__ u32 key_len(const uint8_t *r, bool whole = false)
{
	const u32 L = (u32)r[12] - 1u;
	if (whole) return L;
	for (u32 k = 0; k < L; k++) if (r[36 + k] == '/') return k;
	return L;
}

// What the flags make of one valid record.  Output layout: block_size, the core (l_read_name = NL + 1), NL name bytes, NUL, then from
// T0 on the old record from tail_s on: `cs` bytes of CIGAR and bases and S qualities on the set path, everything to the record's end
// otherwise.
struct MinPlan {
	u32 NL, T0, tail_s, cs, S, out_len;
	u32 s0l;                  // span 0: out [13, 13 + s0l) = r + 13 (the core, and the kept name with its NUL)
	u32 s1l;                  // span 1: out [T0, T0 + s1l) = r + tail_s
	u32 s2o, s2l;             // span 2: out [s2o, s2o + s2l) = r + tail_s + cs (the qualities behind a patched pad nibble)
	u32 padp;                 // the output offset of the byte whose low nibble is cleared, ~0: none
};

__device__ __forceinline__ void min_plan(const uint8_t *r, int flags, u32 id, MinPlan &pl)
{
	const u32 bs = bam_le32_bytes(r), lo = r[12], nc = bam_le32_bytes(r + 16) & 0xffffu, S = bam_le32_bytes(r + 20);
	const bool ids = flags & SK_MINIMIZE_READ_IDS;
	pl.NL = ids ? id_digits(id) : lo - 1u;
	pl.T0 = 36u + pl.NL + 1u;
	pl.tail_s = 36u + lo;
	pl.cs = 4u * nc + ((S + 1u) >> 1);
	pl.S = S;
	pl.s0l = 23u + (ids ? 0u : lo);
	pl.s2o = 0u; pl.s2l = 0u; pl.padp = ~0u;
	if (!(flags & SK_MINIMIZE_TAGS)) {                                     // set_qname: every byte behind the name stays
		pl.s1l = 4u + bs - pl.tail_s;
		pl.out_len = pl.T0 + pl.s1l;
		return;
	}
	const u32 odd = S & 1u;
	pl.out_len = pl.T0 + pl.cs + S;
	pl.s1l = pl.cs - odd;
	if (odd) pl.padp = pl.T0 + pl.cs - 1u;
	if (!(flags & SK_MINIMIZE_BASE_QUALITIES)) {
		if (odd) { pl.s2o = pl.T0 + pl.cs; pl.s2l = S; }
		else pl.s1l += S;
	}
}

// byte p of a record's output
__device__ __forceinline__ u32 min_byte(const uint8_t *r, const MinPlan &pl, int flags, u32 fill, u32 id, u32 p)
{
	if (p < 4u) return ((pl.out_len - 4u) >> (8u * p)) & 0xffu;
	if (p == 12u) return pl.NL + 1u;
	if (p < 36u) return r[p];
	if (p < pl.T0) {
		const u32 q = p - 36u;
		if (q == pl.NL) return 0u;
		if (!(flags & SK_MINIMIZE_READ_IDS)) return r[p];
		u32 v = id;
		for (u32 k = pl.NL - 1u - q; k > 0u; k--) v /= 10u;
		return '0' + v % 10u;
	}
	const u32 t = p - pl.T0;
	if ((flags & SK_MINIMIZE_BASE_QUALITIES) && t >= pl.cs) return fill;
	const u32 v = r[pl.tail_s + t];
	return p == pl.padp ? v & 0xf0u : v;
}

struct MinArgs {
	const uint8_t *stream;
	const u64 *bend, *entry;
	int64_t nb;
	const u64 *rb;            // [nb]: the index of the block's first record
	int flags;
	u32 fill;
	u64 key_mask;
	IdRule rule;
	u64 skip_key;             // the key of a record that takes no part
	const u32 *ids;           // per record, with SK_MINIMIZE_READ_IDS
	u64 *bo;                  // [nb + 1]: per block output bytes, then (bam_scan_u64_kernel) exclusive offsets
	uint32_t *decline;
	u64 *krec, *kout, *key;
	u32 *idx;
};

__global__ __launch_bounds__(kBlockThreads) void bam_min_key_kernel(const MinArgs a)
{
	BlockPass b;
	if (!block_open(a.stream, a.entry, a.bend, a.nb, b)) return;
	const auto [lane, c, entry, n, off] = b;
	const u64 k0 = a.rb[c];
	u32 dec = 0u;
	for (u32 j = (u32)lane; j < n; j += 64u) {
		const uint8_t *r = a.stream + entry + off[j];
		u64 h = 0;
		if (!min_valid(r)) dec = 8u;
		else if ((bam_le32_bytes(r + 16) >> 16) & a.rule.skip_flags) h = a.skip_key;
		else h = qname_key(r + 36, key_len(r, a.rule.whole_name)) & a.key_mask;
		a.krec[k0 + j] = entry + off[j];
		a.key[k0 + j] = h;
		a.idx[k0 + j] = (u32)(k0 + j);
	}
	if (__any((int)dec) && lane == 0) atomicOr(a.decline, 8u);
}

// ---- scans of one u32 per element: a wave per tile of kTile elements ----
template <bool MAX>
__device__ __forceinline__ u32 op32(u32 x, u32 y) { return MAX ? (x > y ? x : y) : x + y; }

template <bool MAX>
__device__ __forceinline__ u32 wave_incl_scan32(u32 x, int lane)
{
	for (int s = 1; s < 64; s <<= 1) {
		const u32 y = (u32)__shfl_up((int)x, s);
		if (lane >= s) x = op32<MAX>(x, y);
	}
	return x;
}

// element p's value: the head positions of the sorted keys (MAX), or the openers of src (sum)
__device__ __forceinline__ u32 head_val(const u64 *key, u64 p) { return p == 0 || key[p] != key[p - 1] ? (u32)p : 0u; }
__device__ __forceinline__ u32 open_val(const u32 *src, u64 k) { return src[k] == (u32)k ? 1u : 0u; }

// agg[t] = the tile's maximum head position (HEADS) or its number of openers
template <bool HEADS>
__global__ __launch_bounds__(kMinThreads) void min_agg_kernel(const u64 *key, const u32 *src, u64 n, u32 *agg)
{
	const int lane = threadIdx.x & 63;
	const u64 t = (u64)blockIdx.x * (kMinThreads / 64) + (threadIdx.x >> 6);
	if (t * kTile >= n) return;
	u32 acc = 0u;
	for (u32 i = 0; i < kTile; i += 64u) {
		const u64 p = t * kTile + i + (u32)lane;
		if (p < n) acc = op32<HEADS>(acc, HEADS ? head_val(key, p) : open_val(src, p));
	}
	for (int s = 32; s > 0; s >>= 1) acc = op32<HEADS>(acc, (u32)__shfl_xor((int)acc, s));
	if (lane == 0) agg[t] = acc;
}

// agg[0 .. nt) -> what precedes each tile (one workgroup)
template <bool MAX>
__global__ __launch_bounds__(1024) void min_tile_scan_kernel(u32 *agg, u64 nt)
{
	__shared__ u32 ws[16];
	const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	u32 carry = 0u;
	for (u64 base = 0; base < nt; base += 1024u) {
		const u64 i = base + threadIdx.x;
		const u32 x = wave_incl_scan32<MAX>(i < nt ? agg[i] : 0u, lane);
		const u32 before = (u32)__shfl_up((int)x, 1);
		if (lane == 63) ws[w] = x;
		__syncthreads();
		u32 pre = carry, tot = carry;
		for (int k = 0; k < 16; k++) {
			if (k < w) pre = op32<MAX>(pre, ws[k]);
			tot = op32<MAX>(tot, ws[k]);
		}
		if (i < nt) agg[i] = lane ? op32<MAX>(pre, before) : pre;
		carry = tot;
		__syncthreads();
	}
}

// Sorted position p: the start of its run, its rank r in the run, the check of its key's bytes against its predecessor's, and src.
__global__ __launch_bounds__(kMinThreads) void bam_min_run_kernel(const uint8_t *stream, const u64 *krec, const u64 *key, const u32 *idx, u64 n,
                                                                  bool whole, u64 skip_bit, const u32 *agg, u32 *src, uint32_t *decline)
{
	const int lane = threadIdx.x & 63;
	const u64 t = (u64)blockIdx.x * (kMinThreads / 64) + (threadIdx.x >> 6);
	if (t * kTile >= n) return;
	u32 carry = agg[t];
	bool bad = false;
	for (u32 i = 0; i < kTile; i += 64u) {
		const u64 p = t * kTile + i + (u32)lane;
		const u32 x = wave_incl_scan32<true>(p < n ? head_val(key, p) : 0u, lane);
		const u32 rs = op32<true>(carry, x);
		carry = op32<true>(carry, (u32)__shfl((int)x, 63));
		if (p >= n) continue;
		const u32 r = (u32)p - rs, me = idx[p];
		u32 from = me;
		if (key[p] & skip_bit) from = kNoSrc;
		else if (r) {
			const u32 prev = idx[p - 1];
			const uint8_t *ra = stream + krec[me], *rb = stream + krec[prev];
			const u32 la = key_len(ra, whole);
			bool same = la == key_len(rb, whole);
			for (u32 k = 0; same && k < la; k++) same = ra[36 + k] == rb[36 + k];
			if (!same) bad = true;
			if (r & 1u) from = prev;
		}
		src[me] = from;
	}
	if (__any((int)bad) && lane == 0) atomicOr(decline, 64u);
}

// cnt[k] = the openers among records 0 .. k
__global__ __launch_bounds__(kMinThreads) void bam_min_open_scan_kernel(const u32 *src, u64 n, const u32 *agg, u32 *cnt)
{
	const int lane = threadIdx.x & 63;
	const u64 t = (u64)blockIdx.x * (kMinThreads / 64) + (threadIdx.x >> 6);
	if (t * kTile >= n) return;
	u32 carry = agg[t];
	for (u32 i = 0; i < kTile; i += 64u) {
		const u64 k = t * kTile + i + (u32)lane;
		const u32 x = wave_incl_scan32<false>(k < n ? open_val(src, k) : 0u, lane);
		if (k < n) cnt[k] = carry + x;
		carry += (u32)__shfl((int)x, 63);
	}
}

__global__ __launch_bounds__(256) void bam_min_id_kernel(const u32 *src, const u32 *cnt, u64 n, u32 *ids)
{
	const u64 k = (u64)blockIdx.x * blockDim.x + threadIdx.x;
	if (k >= n) return;
	const u32 s = src[k];
	ids[k] = s == kNoSrc ? 0u : cnt[s];
}

// ---- size, index, write ----
__global__ __launch_bounds__(kBlockThreads) void bam_min_size_kernel(const MinArgs a)
{
	BlockPass b;
	if (!block_open(a.stream, a.entry, a.bend, a.nb, b)) return;
	const auto [lane, c, entry, n, off] = b;
	const u64 k0 = a.rb[c];
	u64 bytes = 0;
	u32 dec = 0u;
	for (u32 j = (u32)lane; j < n; j += 64u) {
		const uint8_t *r = a.stream + entry + off[j];
		if (!min_valid(r)) { dec |= 8u; continue; }
		const u32 nc = bam_le32_bytes(r + 16) & 0xffffu;
		const uint8_t *cg = r + 36 + r[12];
		for (u32 k = 0; k < nc; k++) if ((cg[4u * k] & 15u) > 8u) dec |= 32u;        // cigar(): "Unexpected cigar operation"
		MinPlan pl;
		min_plan(r, a.flags, a.ids ? a.ids[k0 + j] : 0u, pl);
		bytes += pl.out_len;
	}
	block_close_size(bytes, dec, lane, a.bo + c, a.decline);
}

__global__ __launch_bounds__(kBlockThreads) void bam_min_index_kernel(const MinArgs a)
{
	BlockPass b;
	if (!block_open(a.stream, a.entry, a.bend, a.nb, b)) return;
	const auto [lane, c, entry, n, off] = b;
	const u64 k0 = a.rb[c];
	u64 ob = a.bo[c];                                                      // where the block's output begins
	for (u32 j0 = 0; j0 < n; j0 += 64u) {
		const u32 j = j0 + (u32)lane;
		u64 len = 0;
		if (j < n) { MinPlan pl; min_plan(a.stream + entry + off[j], a.flags, a.ids ? a.ids[k0 + j] : 0u, pl); len = pl.out_len; }
		const u64 il = wave_incl_scan(len, lane);
		if (j < n) { a.krec[k0 + j] = entry + off[j]; a.kout[k0 + j] = ob + il - len; }
		ob += __shfl(il, 63);
	}
}

// bam_write_kernel's record: the three spans of min_plan
struct MinRecord {
	const u32 *ids;
	int flags;
	u32 fill;
	template <class Put>
	__device__ void operator()(const uint8_t *r, int64_t k, const Put &put) const
	{
		const u32 id = ids ? ids[k] : 0u;
		MinPlan pl;
		min_plan(r, flags, id, pl);
		auto byte = [&](u32 p) -> u32 { return min_byte(r, pl, flags, fill, id, p); };
		put(pl.out_len, 13u, pl.s0l, r + 13, pl.T0, pl.s1l, r + pl.tail_s, pl.s2o, pl.s2l, r + pl.tail_s + pl.cs, byte);
	}
};

unsigned tiles_grid(uint64_t n) { return (unsigned)(((n + kTile - 1) / kTile + kMinThreads / 64 - 1) / (kMinThreads / 64)); }

MinArgs min_args(const uint8_t *stream, const uint64_t *bend, const uint64_t *entry, int64_t nb, const uint64_t *rb, int flags)
{
	MinArgs a{};
	a.stream = stream; a.bend = (const u64 *)bend; a.entry = (const u64 *)entry; a.nb = nb; a.rb = (const u64 *)rb; a.flags = flags;
	return a;
}

}  // namespace

hipError_t launch_bam_min_keys(const uint8_t *stream, const uint64_t *bend, const uint64_t *entry, int64_t nb, const uint64_t *rb, int key_bits,
                               IdRule rule, uint64_t *krec, uint64_t *key, uint32_t *idx, uint32_t *decline, hipStream_t st)
{
	if (nb <= 0) return hipSuccess;
	MinArgs a = min_args(stream, bend, entry, nb, rb, SK_MINIMIZE_READ_IDS);
	a.key_mask = key_bits >= 64 ? ~0ull : (1ull << key_bits) - 1ull;
	a.rule = rule; a.skip_key = id_skip_bit(rule, key_bits);
	a.krec = (u64 *)krec; a.key = (u64 *)key; a.idx = idx; a.decline = decline;
	bam_min_key_kernel<<<block_grid(nb), kBlockThreads, 0, st>>>(a);
	return hipGetLastError();
}

hipError_t bam_sort_pairs(void *temp, size_t *temp_bytes, uint64_t *key[2], uint32_t *idx[2], uint64_t n, int key_bits, int *sorted, hipStream_t st)
{
	rocprim::double_buffer<u64> k((u64 *)key[0], (u64 *)key[1]);
	rocprim::double_buffer<u32> v(idx[0], idx[1]);
	const hipError_t e = rocprim::radix_sort_pairs(temp, *temp_bytes, k, v, (size_t)n, 0u, (unsigned)key_bits, st);
	if (temp && sorted) *sorted = k.current() == (u64 *)key[0] ? 0 : 1;
	return e;
}

hipError_t launch_bam_min_ids(const uint8_t *stream, const uint64_t *krec, const uint64_t *key, const uint32_t *idx, uint64_t n, int key_bits,
                              IdRule rule, uint32_t *agg, uint32_t *src, uint32_t *cnt, uint32_t *ids, uint32_t *decline, hipStream_t st)
{
	if (n == 0) return hipSuccess;
	const u64 nt = (n + kTile - 1) / kTile;
	min_agg_kernel<true><<<tiles_grid(n), kMinThreads, 0, st>>>((const u64 *)key, nullptr, n, agg);
	min_tile_scan_kernel<true><<<1, 1024, 0, st>>>(agg, nt);
	bam_min_run_kernel<<<tiles_grid(n), kMinThreads, 0, st>>>(stream, (const u64 *)krec, (const u64 *)key, idx, n, rule.whole_name != 0,
	                                                              id_skip_bit(rule, key_bits), agg, src, decline);
	min_agg_kernel<false><<<tiles_grid(n), kMinThreads, 0, st>>>(nullptr, src, n, agg);
	min_tile_scan_kernel<false><<<1, 1024, 0, st>>>(agg, nt);
	bam_min_open_scan_kernel<<<tiles_grid(n), kMinThreads, 0, st>>>(src, n, agg, cnt);
	bam_min_id_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(src, cnt, n, ids);
	return hipGetLastError();
}

hipError_t launch_bam_min_size(const uint8_t *stream, const uint64_t *bend, const uint64_t *entry, int64_t nb, const uint64_t *rb, int flags,
                               const uint32_t *ids, uint64_t *bo, uint32_t *decline, hipStream_t st)
{
	if (nb > 0) {
		MinArgs a = min_args(stream, bend, entry, nb, rb, flags);
		a.ids = ids; a.bo = (u64 *)bo; a.decline = decline;
		bam_min_size_kernel<<<block_grid(nb), kBlockThreads, 0, st>>>(a);
		if (hipError_t e = hipGetLastError()) return e;
	}
	return launch_scan_u64(bo, nb, st);
}

hipError_t launch_bam_min_index(const uint8_t *stream, const uint64_t *bend, const uint64_t *entry, int64_t nb, const uint64_t *rb, int flags,
                                const uint32_t *ids, const uint64_t *bo, uint64_t *krec, uint64_t *kout, hipStream_t st)
{
	if (nb <= 0) return hipSuccess;
	MinArgs a = min_args(stream, bend, entry, nb, rb, flags);
	a.ids = ids; a.bo = (u64 *)bo; a.krec = (u64 *)krec; a.kout = (u64 *)kout;
	bam_min_index_kernel<<<block_grid(nb), kBlockThreads, 0, st>>>(a);
	return hipGetLastError();
}

hipError_t launch_bam_min_write(const WriteWindow &w, const uint32_t *ids, int flags, uint8_t fill, int n_cu, hipStream_t st)
{
	return launch_bam_write(w, MinRecord{ids, flags, fill}, n_cu, st);
}

}  // namespace sk
