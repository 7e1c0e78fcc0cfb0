// sk_bamtlen.hip — the record passes of sk_bam_file_recalc_tlen (include/seqkit_hip.h): `sam recalculate tlen`
// (src/sam_recalculate_tlen.rs) over a verified BAM stream.  The BGZF half (cut, deflate, pack) is sk_bamwrite.hip's and
// sk_deflate.hip's, unchanged.
//
// The reference sorts every record into one of three classes.  Z: not paired, unmapped, mate unmapped, or a discordant pair (tid !=
// mtid, |pos - mpos| > max_len, both mates on one strand): written with TLEN 0.  S: a paired, mapped record with a mapped mate and
// 0x100 or 0x800: the reference ends there (decline bit 1).  C, a candidate: every other record.  For the candidates it keeps a map
// from a read's name to the record waiting for its mate: a name that is in the map takes the stored record as its mate and LEAVES the
// map, any other name enters it.  That is the map of `sam minimize`, so the link between the mates is sk_bamminimize.hip's run pass
// under the rule {the whole name, Z records take no part}: among the candidates of one name, in file order, the 1st, 3rd, 5th .. opens
// (src[k] == k) and the 2nd, 4th .. closes, its mate the one just before it (src[k]).  An opener that nobody closes is never written.
// bam_tlen_key_kernel — a wave per BGZF block (sk_bamblock.h): per record its stream offset, its index and its key — the hash of its
//   whole name for a candidate, the bit above the hash's alone for a Z record, as launch_bam_min_keys writes them for a record its rule
//   passes over; decline bits 1 (an S record), 8 (an invalid record) and 16 (a name byte >= 0x80: the reference checks every name for
//   UTF-8, the caller's reader decides exactly; a NUL inside a name goes the same way).
// bam_tlen_resolve_kernel — a lane per record, a grid of at most 8 workgroups a CU striding over the file.  A Z record: TLEN 0 and its
//   bytes into len.  A closer reads both records and computes the pair's TLEN from the two 5' ends (for a reverse read the CIGAR's end
//   less one, in 64 bits), writes it and its negation into tlen and both records' bytes into len; decline bit 2 where the two have
//   equal 0x40 bits (the reference's assert).  len starts as 0, so afterwards a candidate with len 0 is one without a mate.  Every
//   word has one writer.  A reverse candidate with a CIGAR operation code above 8 sets decline bit 32, paired or not.
// bam_sub_scans, bam_sub_compact_kernel (sk_bamsubsample.hip) — the written records' stream and output offsets in written order.
// bam_tlen_gather_kernel — with the same places: a written record's TLEN to place pos[k]; a discarded record's stream offset to place
//   k - pos[k], its rank among the discarded, so that list is in file order too.
// TlenRecord in bam_write_kernel (sk_bamblock.h) — a window's records copied as sk_bamsubsample.hip copies them, bytes 32-35 from the
//   TLEN column.
// bam_tlen_names_kernel — a range of the discard list: a wave per record writes a slot of 256 bytes, the name and NULs behind it.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "../../include/seqkit_hip.h"
#include "sk_bamblock.h"
#include "sk_internal.h"

namespace sk {

namespace {

typedef uint32_t u32;
typedef unsigned long long u64;
typedef long long i64;

constexpr int kTlenThreads = 256;
constexpr u32 kNoSrc = ~0u;                       // launch_bam_min_ids: the src of a record that takes no part

// is the record one htslib reads (sk_bamwrite.hip: rw_plan's bit 8)
__device__ __forceinline__ bool tlen_valid(const uint8_t *r)
{
	const u32 bs = bam_le32_bytes(r), lo = r[12], nc = bam_le32_bytes(r + 16) & 0xffffu, S = bam_le32_bytes(r + 20);
	return !(bs < 32u || lo < 1u || S > 0x7fffffffu || 4ull * nc + lo + (((u64)S + 1) >> 1) + S > (u64)(bs - 32u));
}

enum TlenClass : u32 { kZero = 0u, kStop = 1u, kCandidate = 2u };

// src/sam_recalculate_tlen.rs:44-55
__device__ __forceinline__ u32 tlen_class(const uint8_t *r, i64 max_len)
{
	const u32 flag = bam_le32_bytes(r + 16) >> 16;
	if (!(flag & 0x1u) || (flag & 0xcu)) return kZero;
	if (flag & 0x900u) return kStop;
	const i64 tid = (int32_t)bam_le32_bytes(r + 4), pos = (int32_t)bam_le32_bytes(r + 8);
	const i64 mtid = (int32_t)bam_le32_bytes(r + 24), mpos = (int32_t)bam_le32_bytes(r + 28);
	const i64 d = pos > mpos ? pos - mpos : mpos - pos;
	if (tid != mtid || d > max_len || ((flag >> 4) & 1u) == ((flag >> 5) & 1u)) return kZero;
	return kCandidate;
}

struct TlenKeyArgs {
	const uint8_t *stream;
	const u64 *bend, *entry;
	int64_t nb;
	const u64 *rb;            // [nb]: the index of the block's first record
	i64 max_len;
	u64 key_mask, skip_key;   // the hash's bits; the key of a record that takes no part
	uint32_t *decline;
	u64 *krec, *key;
	u32 *idx;
};

__global__ __launch_bounds__(kBlockThreads) void bam_tlen_key_kernel(const TlenKeyArgs a)
{
	BlockPass b;
	if (!block_open(a.stream, a.entry, a.bend, a.nb, b)) return;
	const auto [lane, c, entry, n, off] = b;
	const u64 k0 = a.rb[c];
	u32 dec = 0u;
	for (u32 j = (u32)lane; j < n; j += 64u) {
		const uint8_t *r = a.stream + entry + off[j];
		u64 h = a.skip_key;
		if (!tlen_valid(r)) dec |= 8u;
		else {
			const u32 L = (u32)r[12] - 1u;
			bool odd = false;                                                   // a byte >= 0x80, or a NUL inside the name: a 256-byte slot could not say where such a name ends
			for (u32 k = 0; k < L; k++) odd = odd || (u32)r[36 + k] - 1u >= 0x7fu;
			if (odd) dec |= 16u;
			const u32 cls = tlen_class(r, a.max_len);
			if (cls == kStop) dec |= 1u;
			else if (cls == kCandidate) h = qname_key(r + 36, L) & a.key_mask;
		}
		a.krec[k0 + j] = entry + off[j];
		a.key[k0 + j] = h;
		a.idx[k0 + j] = (u32)(k0 + j);
	}
	for (int s = 32; s > 0; s >>= 1) dec |= (u32)__shfl_xor((int)dec, s);
	if (dec && lane == 0) atomicOr(a.decline, dec);
}

// The 5' end of a candidate (:60-61): pos, or for a reverse read cigar().end_pos() - 1 — pos and the lengths of the operations that
// consume the reference (M D N = X).  *dec: bit 32 at an operation code above 8, where cigar() panics.
__device__ __forceinline__ i64 tlen_start(const uint8_t *r, u32 flag, u32 &dec)
{
	i64 p = (int32_t)bam_le32_bytes(r + 8);
	if (!(flag & 0x10u)) return p;
	const u32 nc = bam_le32_bytes(r + 16) & 0xffffu;
	const uint8_t *cg = r + 36 + r[12];
	for (u32 k = 0; k < nc; k++) {
		const u32 op = bam_le32_bytes(cg + 4u * k), code = op & 15u;
		if (code > 8u) dec |= 32u;
		else if ((0x18du >> code) & 1u) p += op >> 4;                         // codes 0 2 3 7 8
	}
	return p - 1;
}

__global__ __launch_bounds__(kTlenThreads) void bam_tlen_resolve_kernel(const uint8_t *stream, const u64 *krec, const u32 *src, u64 n, int32_t *tlen, u32 *len,
                                                                        uint32_t *decline)
{
	u32 dec = 0u;
	for (u64 k = (u64)blockIdx.x * kTlenThreads + threadIdx.x; k < n; k += (u64)gridDim.x * kTlenThreads) {
		const u32 s = src[k];
		const uint8_t *rb = stream + krec[k];
		if (s == kNoSrc) { tlen[k] = 0; len[k] = 4u + bam_le32_bytes(rb); continue; }
		const u32 fb = bam_le32_bytes(rb + 16) >> 16;
		if (s == (u32)k) { (void)tlen_start(rb, fb, dec); continue; }          // an opener: its closer, if it has one, writes its words
		const uint8_t *ra = stream + krec[s];                                // the earlier mate
		const u32 fa = bam_le32_bytes(ra + 16) >> 16;
		if (!((fa ^ fb) & 0x40u)) dec |= 2u;                                  // :59
		const i64 sa = tlen_start(ra, fa, dec), sb = tlen_start(rb, fb, dec);
		i64 t = (sb > sa ? sb - sa : sa - sb) + 1;                            // :65-73
		if ((int32_t)bam_le32_bytes(rb + 8) > (int32_t)bam_le32_bytes(ra + 8)) t = -t;
		const bool rev = fb & 0x10u;
		if ((sb < sa && rev) || (sb > sa && !rev)) t = 0;
		tlen[k] = (int32_t)(u32)(u64)t;                                      // `as i32`: the low 32 bits
		tlen[s] = (int32_t)(u32)(u64)(-t);
		len[k] = 4u + bam_le32_bytes(rb);
		len[s] = 4u + bam_le32_bytes(ra);
	}
	for (int sh = 32; sh > 0; sh >>= 1) dec |= (u32)__shfl_xor((int)dec, sh);
	if (dec && (threadIdx.x & 63) == 0) atomicOr(decline, dec);
}

__global__ __launch_bounds__(kTlenThreads) void bam_tlen_gather_kernel(const u64 *krec, const u32 *len, const u32 *pos, const int32_t *tlen, u64 n,
                                                                       int32_t *tlen_out, u64 *disc)
{
	for (u64 k = (u64)blockIdx.x * kTlenThreads + threadIdx.x; k < n; k += (u64)gridDim.x * kTlenThreads) {
		const u32 q = pos[k];                                                // (q <= k: the written records before k)
		if (len[k]) tlen_out[q] = tlen[k];
		else disc[k - q] = krec[k];
	}
}

// bam_write_kernel's record: one span before the TLEN and one behind it
struct TlenRecord {
	const int32_t *tlen;
	template <class Put>
	__device__ void operator()(const uint8_t *r, int64_t k, const Put &put) const
	{
		const u32 len = 4u + bam_le32_bytes(r), t = (u32)tlen[k];
		auto byte = [&](u32 p) -> u32 { return p - 32u < 4u ? (t >> (8u * (p - 32u))) & 0xffu : r[p]; };
		put(len, 0u, 32u, r, 36u, len - 36u, r + 36, 0u, 0u, r, byte);
	}
};

__global__ __launch_bounds__(kTlenThreads) void bam_tlen_names_kernel(const uint8_t *stream, const u64 *disc, int64_t first, int64_t n, uint8_t *out)
{
	const u32 lane = threadIdx.x & 63u;
	const int64_t wstride = ((int64_t)gridDim.x * kTlenThreads) >> 6;
	for (int64_t j = ((int64_t)blockIdx.x * kTlenThreads + threadIdx.x) >> 6; j < n; j += wstride) {
		const uint8_t *r = stream + disc[first + j];
		const u32 L = (u32)r[12] - 1u;                                       // (at most 254: the slot ends with two NULs or more)
		u32 v = 0u;
		for (u32 b = 0; b < 4u; b++) {
			const u32 p = 4u * lane + b;
			if (p < L) v |= (u32)r[36 + p] << (8u * b);
		}
		reinterpret_cast<u32 *>(out + (u64)j * 256u)[lane] = v;
	}
}

// a lane per element, at most 8 workgroups a planned CU: the lanes stride over the rest
unsigned tlen_grid(uint64_t n, int n_cu)
{
	const uint64_t want = (n + kTlenThreads - 1) / kTlenThreads, cap = (uint64_t)(n_cu > 0 ? n_cu : 256) * 8u;
	return (unsigned)(want < cap ? want : cap);
}

}  // namespace

hipError_t launch_bam_tlen_keys(const uint8_t *stream, const uint64_t *bend, const uint64_t *entry, int64_t nb, const uint64_t *rb, int64_t max_len,
                                int key_bits, uint64_t *krec, uint64_t *key, uint32_t *idx, uint32_t *decline, hipStream_t st)
{
	if (nb <= 0) return hipSuccess;
	TlenKeyArgs a{};
	a.stream = stream; a.bend = (const u64 *)bend; a.entry = (const u64 *)entry; a.nb = nb; a.rb = (const u64 *)rb; a.max_len = max_len;
	a.key_mask = ((u64)1 << key_bits) - 1ull; a.skip_key = id_skip_bit(kTlenIdRule, key_bits);
	a.decline = decline; a.krec = (u64 *)krec; a.key = (u64 *)key; a.idx = idx;
	bam_tlen_key_kernel<<<block_grid(nb), kBlockThreads, 0, st>>>(a);
	return hipGetLastError();
}

hipError_t launch_bam_tlen_resolve(const uint8_t *stream, const uint64_t *krec, const uint32_t *src, uint64_t n, int32_t *tlen, uint32_t *len,
                                   uint32_t *decline, int n_cu, hipStream_t st)
{
	if (n == 0) return hipSuccess;
	if (hipError_t e = hipMemsetAsync(len, 0, (size_t)n * 4, st)) return e;
	bam_tlen_resolve_kernel<<<tlen_grid(n, n_cu), kTlenThreads, 0, st>>>(stream, (const u64 *)krec, src, n, tlen, len, decline);
	return hipGetLastError();
}

hipError_t launch_bam_tlen_gather(const uint64_t *krec, const uint32_t *len, const uint32_t *pos, const int32_t *tlen, uint64_t n, int32_t *tlen_out,
                                  uint64_t *disc, int n_cu, hipStream_t st)
{
	if (n == 0) return hipSuccess;
	bam_tlen_gather_kernel<<<tlen_grid(n, n_cu), kTlenThreads, 0, st>>>((const u64 *)krec, len, pos, tlen, n, tlen_out, (u64 *)disc);
	return hipGetLastError();
}

hipError_t launch_bam_tlen_write(const WriteWindow &w, const int32_t *tlen, int n_cu, hipStream_t st)
{
	return launch_bam_write(w, TlenRecord{tlen}, n_cu, st);
}

hipError_t launch_bam_tlen_names(const uint8_t *stream, const uint64_t *disc, int64_t first, int64_t n, uint8_t *out, int n_cu, hipStream_t st)
{
	if (n <= 0) return hipSuccess;
	bam_tlen_names_kernel<<<tlen_grid((uint64_t)n * 64u, n_cu), kTlenThreads, 0, st>>>(stream, (const u64 *)disc, first, n, out);
	return hipGetLastError();
}

}  // namespace sk
