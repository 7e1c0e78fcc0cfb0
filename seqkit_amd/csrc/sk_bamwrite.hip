// sk_bamwrite.hip — the BAM-out half of sk_bam_file_rewrite (include/seqkit_hip.h): the per-record rewrite of `sam trim qnames`,
// `sam tags from qname` and `sam qname from tags` over a verified BAM stream, and the packing of deflated blocks into BGZF members.
//
// bam_rw_size_kernel / bam_rw_index_kernel — a wave per BGZF block follows the chain from entry[c] (sk_bamblock.h: block_open; lane 0
// leaves the records' offsets in LDS, then the lanes take consecutive records).  rw_plan reads one record and says what the
// command makes of it: unchanged, or a new name (a prefix of the old one, followed by " RX:" + the RX value for qname from tags) and
// appended Z fields (tags from qname).  The first pass sums the rewritten bytes per block and ORs the decline bits: every record the
// reference would end on (src/sam_trim_qnames.rs:23 qname[trim - 2]; src/sam_tags_from_qname.rs:46 error!; set_qname's 254-byte
// limit), and, for qname from tags, aux data that do not parse to the record's end.  After the scan, the second pass writes every
// record's stream offset and output offset.
// (where each window of at most W rewritten bytes begins: sk_bamtext.hip's bam_window_kernel)
// bam_rw_write_kernel — one window's records: a 16-lane group owns a record and covers its output in consecutive dwords.  A dword
// that lies inside one of the record's copied spans (the core and the kept name; CIGAR, bases, qualities and aux) is built from two
// aligned loads with a funnel shift (v_alignbyte) and stored whole; the rest — the block_size and l_read_name bytes, the spans' edges,
// the appended bytes and the dwords shared with the neighbouring records — is composed byte by byte (sk_bamblock.h: emit).
// bgzf_cut_kernel / bgzf_member_size_kernel / bgzf_pack_kernel — a window as blocks of at most 0xff00 bytes for bgzf_deflate_kernel
// (sk_deflate.hip), then the members (SAMv1 §4.1: 18-byte header with BC = BSIZE - 1, payload, CRC32, ISIZE) back to back: a wave
// per member, the payload copied as the records are.  A block that does not shrink, and every block at level 0, is framed as a
// stored block (RFC 1951 §3.2.4).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/seqkit_hip.h"
#include "sk_bamblock.h"
#include "sk_internal.h"

namespace sk {

namespace {

typedef uint32_t u32;
typedef unsigned long long u64;

constexpr u32 kMaxIn = 0xff00u;

// What a command makes of one record.  Output layout of a changed record: block_size, the core (l_read_name new), the first P bytes of
// the old name, X bytes (NUL, or " RX:" value NUL), the old record from the end of the name on (tail_len bytes: CIGAR .. aux), then
// alen bytes of appended Z fields.
struct RwPlan {
	u32 same;                 // 1: the record passes unchanged (out_len = 4 + block_size)
	u32 P, X, voff, vl, sp;   // kept name bytes; bytes behind them; qname from tags: the RX value's offset and length; tags from qname: the first space
	u32 tail_s, tail_len, alen, out_len;
};

__device__ __forceinline__ u32 rw_plan(const uint8_t *r, int op, RwPlan &pl)
{
	const u32 bs = bam_le32_bytes(r), w12 = bam_le32_bytes(r + 12), w16 = bam_le32_bytes(r + 16), S = bam_le32_bytes(r + 20);
	const u32 lo = w12 & 0xffu, nc = w16 & 0xffffu;
	pl.same = 1u; pl.P = 0u; pl.X = 0u; pl.voff = 0u; pl.vl = 0u; pl.sp = 0u; pl.tail_s = 0u; pl.tail_len = 0u; pl.alen = 0u;
	pl.out_len = 4u + bs;
	if (bs < 32u || lo < 1u || S > 0x7fffffffu || 4ull * nc + lo + (((u64)S + 1) >> 1) + S > (u64)(bs - 32u)) return 8u;   // "Invalid BAM record."
	const uint8_t *name = r + 36;
	const u32 L = lo - 1u;
	u32 sp = L;
	if (op != SK_REWRITE_QNAME_FROM_TAGS)
		for (u32 k = 0; k < L; k++) if (name[k] == ' ') { sp = k; break; }
	if (op == SK_REWRITE_TRIM_QNAMES) {                                     // src/sam_trim_qnames.rs:20-26
		if (sp == L) return 0u;
		if (sp < 2u) return 1u;                                            // qname[trim - 2]: a panic
		u32 t = sp;
		if (name[t - 2u] == '/' && (name[t - 1u] == '1' || name[t - 1u] == '2')) t -= 2u;
		pl.P = t; pl.X = 1u;
	} else if (op == SK_REWRITE_TAGS_FROM_QNAME) {                          // src/sam_tags_from_qname.rs:33-48
		if (sp == L) return 0u;
		u32 alen = 0u;
		for (u32 s = sp + 1u;;) {
			u32 e = s;
			while (e < L && name[e] != ' ') e++;
			const u32 m = e - s;
			if (m >= 4u && name[s] == 'U' && name[s + 1u] == 'M' && name[s + 2u] == 'I' && name[s + 3u] == ':') alen += m;     // RX Z value NUL
			else if (m >= 3u && name[s + 2u] == ':') alen += m + 1u;                                                            // tag Z value NUL
			else return 2u;                                                                                                     // error! (or a panic)
			if (e >= L) break;
			s = e + 1u;
		}
		pl.P = sp; pl.X = 1u; pl.sp = sp; pl.alen = alen;
	} else {                                                                // src/sam_qname_from_tags.rs:32-38
		const u32 end = 4u + bs;
		u64 a = 36ull + lo + 4ull * nc + (((u64)S + 1) >> 1) + S;
		bool found = false;
		u32 rty = 0u, voff = 0u, vl = 0u;
		while (a < end) {
			if (a + 3u > end) return 16u;
			const u32 t0 = r[a], t1 = r[a + 1], ty = r[a + 2];
			a += 3u;
			const u32 v0 = (u32)a;
			if (ty == 'A' || ty == 'c' || ty == 'C') a += 1u;
			else if (ty == 's' || ty == 'S') a += 2u;
			else if (ty == 'i' || ty == 'I' || ty == 'f') a += 4u;
			else if (ty == 'Z' || ty == 'H') {
				while (a < end && r[a] != 0) a++;
				if (a >= end) return 16u;
				a++;
			} else if (ty == 'B') {
				if (a + 5u > end) return 16u;
				const u32 sub = r[a], cnt = bam_le32_bytes(r + a + 1);
				const u32 es = (sub == 'c' || sub == 'C') ? 1u : (sub == 's' || sub == 'S') ? 2u : (sub == 'i' || sub == 'I' || sub == 'f') ? 4u : 0u;
				if (!es) return 16u;
				a += 5ull + (u64)cnt * es;
			} else return 16u;
			if (a > end) return 16u;
			if (!found && t0 == 'R' && t1 == 'X') { found = true; rty = ty; voff = v0; vl = (u32)(a - v0) - 1u; }
		}
		if (!found || (rty != 'Z' && rty != 'H')) return 0u;
		if (L + 4u + vl > 254u) return 4u;                                 // set_qname: a name of 255 bytes or more panics
		pl.P = L; pl.X = 4u + vl + 1u; pl.voff = voff; pl.vl = vl;
	}
	pl.same = 0u;
	pl.tail_s = 36u + lo;
	pl.tail_len = 4u + bs - pl.tail_s;
	pl.out_len = 36u + pl.P + pl.X + pl.tail_len + pl.alen;
	return 0u;
}

// byte p of a record's output
__device__ __forceinline__ u32 rw_byte(const uint8_t *r, int op, const RwPlan &pl, u32 p)
{
	if (pl.same) return r[p];
	if (p < 4u) return ((pl.out_len - 4u) >> (8u * p)) & 0xffu;
	if (p == 12u) return pl.P + pl.X;
	if (p < 36u + pl.P) return r[p];
	u32 q = p - 36u - pl.P;
	if (q < pl.X) {
		if (op != SK_REWRITE_QNAME_FROM_TAGS) return 0u;
		if (q < 4u) return q == 0u ? ' ' : q == 1u ? 'R' : q == 2u ? 'X' : ':';
		return q < 4u + pl.vl ? r[pl.voff + q - 4u] : 0u;
	}
	q -= pl.X;
	if (q < pl.tail_len) return r[pl.tail_s + q];
	q -= pl.tail_len;
	const uint8_t *name = r + 36;                                           // the appended fields, one per part of the old name
	const u32 L = (u32)r[12] - 1u;
	for (u32 s = pl.sp + 1u; s < L + 1u;) {
		u32 e = s;
		while (e < L && name[e] != ' ') e++;
		const u32 m = e - s;
		const bool umi = m >= 4u && name[s] == 'U' && name[s + 1u] == 'M' && name[s + 2u] == 'I' && name[s + 3u] == ':';
		const u32 f = umi ? m : m + 1u;
		if (q < f) {
			if (umi) return q == 0u ? 'R' : q == 1u ? 'X' : q == 2u ? 'Z' : q + 1u < m ? name[s + q + 1u] : 0u;
			return q == 2u ? 'Z' : q < m ? name[s + q] : 0u;
		}
		q -= f;
		s = e + 1u;
	}
	return 0u;
}

struct RwArgs {
	const uint8_t *stream;
	const u64 *bend, *entry;
	int64_t nb;
	int op;
	u64 *bo;                  // [nb + 1]: per block rewritten bytes, then (bam_scan_u64_kernel) exclusive offsets
	const u64 *rb;            // [nb]: the index of the block's first record
	uint32_t *decline;        // OR of the records' decline bits (include/seqkit_hip.h: sk_bam_file_rewrite)
	u64 *krec, *kout;
};

__global__ __launch_bounds__(kBlockThreads) void bam_rw_size_kernel(const RwArgs a)
{
	BlockPass b;
	if (!block_open(a.stream, a.entry, a.bend, a.nb, b)) return;
	const auto [lane, c, entry, n, off] = b;
	u64 bytes = 0;
	u32 dec = 0u;
	for (u32 j = (u32)lane; j < n; j += 64u) {
		RwPlan pl;
		dec |= rw_plan(a.stream + entry + off[j], a.op, pl);
		bytes += pl.out_len;
	}
	block_close_size(bytes, dec, lane, a.bo + c, a.decline);
}

__global__ __launch_bounds__(kBlockThreads) void bam_rw_index_kernel(const RwArgs a)
{
	BlockPass b;
	if (!block_open(a.stream, a.entry, a.bend, a.nb, b)) return;
	const auto [lane, c, entry, n, off] = b;
	u64 k0 = a.rb[c], ob = a.bo[c];                                        // the block's first record and where its output begins
	for (u32 j0 = 0; j0 < n; j0 += 64u) {
		const u32 j = j0 + (u32)lane;
		u64 len = 0;
		if (j < n) { RwPlan pl; (void)rw_plan(a.stream + entry + off[j], a.op, pl); len = pl.out_len; }
		const u64 il = wave_incl_scan(len, lane);
		if (j < n) { a.krec[k0 + j] = entry + off[j]; a.kout[k0 + j] = ob + il - len; }
		ob += __shfl(il, 63);
	}
}

// (bam_write_kernel's loop written out: as the descriptor of that template this writer measured 0.5 % slower, 10.004 against 9.949 ms
// over the 82 windows of 20 M records, above the parent's own repeats in two tables of three)
__global__ __launch_bounds__(kGroupThreads) void bam_rw_write_kernel(const uint8_t *stream, const u64 *krec, const u64 *kout, int64_t first, int64_t n,
                                                                     u64 o0, int op, uint8_t *out)
{
	const u32 gl = threadIdx.x & 15u;
	const int64_t gstride = ((int64_t)gridDim.x * kGroupThreads) >> 4;
	for (int64_t j = ((int64_t)blockIdx.x * kGroupThreads + threadIdx.x) >> 4; j < n; j += gstride) {
		const int64_t k = first + j;
		const uint8_t *r = stream + krec[k];
		RwPlan pl;
		(void)rw_plan(r, op, pl);
		const u64 ob = kout[k] - o0;
		auto byte = [&](u32 p) -> u32 { return rw_byte(r, op, pl, p); };
		if (pl.same) emit(out, ob, pl.out_len, 0u, pl.out_len, r, 0u, 0u, r, 0u, 0u, r, byte, gl, 16u);
		else emit(out, ob, pl.out_len, 13u, 23u + pl.P, r + 13, 36u + pl.P + pl.X, pl.tail_len, r + pl.tail_s, 0u, 0u, r, byte, gl, 16u);
	}
}

struct Blk { u64 in_off; u32 in_len, pad; };      // == sk_deflate_block

__global__ __launch_bounds__(256) void bgzf_cut_kernel(u64 raw_len, Blk *blocks, int64_t n)
{
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const u64 o = (u64)i * kMaxIn;
	blocks[i].in_off = o;
	blocks[i].in_len = (u32)(raw_len - o < kMaxIn ? raw_len - o : kMaxIn);
	blocks[i].pad = 0u;
}

// a member's payload: stored (5 bytes of framing + the input) or the deflate kernel's bytes
__device__ __forceinline__ bool member_stored(const Blk &b, const u32 *result, int64_t i, int stored_only)
{
	if (stored_only) return true;
	const u32 pay = result[2 * i];
	return pay >= b.in_len + 5u || pay + 26u > 65536u;
}

__global__ __launch_bounds__(256) void bgzf_member_size_kernel(const Blk *blocks, int64_t n, const u32 *result, int stored_only, u64 *msz)
{
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const Blk b = blocks[i];
	msz[i] = 26u + (member_stored(b, result, i, stored_only) ? b.in_len + 5u : result[2 * i]);
}

__global__ __launch_bounds__(256) void bgzf_pack_kernel(const uint8_t *raw, const Blk *blocks, int64_t n, const uint8_t *slots, u32 slot_stride,
                                                        const u32 *result, const u32 *crc, int stored_only, const u64 *moff, uint8_t *out)
{
	const u32 lane = threadIdx.x & 63u;
	const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
	if (i >= n) return;
	const Blk b = blocks[i];
	const bool stored = member_stored(b, result, i, stored_only);
	const u32 len = b.in_len, clen = stored ? len + 5u : result[2 * i], bsize = 26u + clen, c = crc[i];
	const u32 p0 = stored ? 23u : 18u;                                     // where the copied payload begins
	const uint8_t *src = stored ? raw + b.in_off : slots + (u64)i * slot_stride;
	auto byte = [&](u32 p) -> u32 {
		if (p < 16u) {
			const u32 h = p < 4u ? (0x04088b1fu >> (8u * p)) : p < 8u ? 0u : p < 12u ? (0x0006ff00u >> (8u * (p - 8u))) : (0x00024342u >> (8u * (p - 12u)));
			return h & 0xffu;
		}
		if (p < 18u) return ((bsize - 1u) >> (8u * (p - 16u))) & 0xffu;
		if (p < p0) {                                                      // BFINAL = 1, BTYPE = 00, LEN, NLEN
			const u32 q = p - 18u;
			return q == 0u ? 1u : q < 3u ? (len >> (8u * (q - 1u))) & 0xffu : (~len >> (8u * (q - 3u))) & 0xffu;
		}
		if (p < 18u + clen) return src[p - p0];
		const u32 q = p - 18u - clen;
		return q < 4u ? (c >> (8u * q)) & 0xffu : (len >> (8u * (q - 4u))) & 0xffu;
	};
	const u32 plen = stored ? len : clen;
	emit(out, moff[i], bsize, p0, plen, src, 0u, 0u, src, 0u, 0u, src, byte, lane, 64u);
}

}  // namespace

hipError_t launch_bam_rw_size(const uint8_t *stream, const uint64_t *bend, const uint64_t *entry, int64_t nb, int op, uint64_t *bo, uint32_t *decline,
                              hipStream_t st)
{
	RwArgs a{};
	a.stream = stream; a.bend = (const u64 *)bend; a.entry = (const u64 *)entry; a.nb = nb; a.op = op; a.bo = (u64 *)bo; a.decline = decline;
	if (nb > 0) {
		bam_rw_size_kernel<<<block_grid(nb), kBlockThreads, 0, st>>>(a);
		if (hipError_t e = hipGetLastError()) return e;
	}
	return launch_scan_u64(bo, nb, st);
}

hipError_t launch_bam_rw_index(const uint8_t *stream, const uint64_t *bend, const uint64_t *entry, int64_t nb, int op, const uint64_t *bo,
                               const uint64_t *rb, uint64_t *krec, uint64_t *kout, hipStream_t st)
{
	if (nb <= 0) return hipSuccess;
	RwArgs a{};
	a.stream = stream; a.bend = (const u64 *)bend; a.entry = (const u64 *)entry; a.nb = nb; a.op = op; a.bo = (u64 *)bo; a.rb = (const u64 *)rb;
	a.krec = (u64 *)krec; a.kout = (u64 *)kout;
	bam_rw_index_kernel<<<block_grid(nb), kBlockThreads, 0, st>>>(a);
	return hipGetLastError();
}

hipError_t launch_bam_rw_write(const WriteWindow &w, int op, int n_cu, hipStream_t st)
{
	if (w.n <= 0) return hipSuccess;
	bam_rw_write_kernel<<<group_grid(w.n, n_cu), kGroupThreads, 0, st>>>(w.stream, (const u64 *)w.krec, (const u64 *)w.kout, w.first, w.n, w.o0, op, w.out);
	return hipGetLastError();
}

hipError_t launch_bgzf_cut(uint64_t raw_len, void *blocks, int64_t n, hipStream_t st)
{
	if (n <= 0) return hipSuccess;
	bgzf_cut_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(raw_len, reinterpret_cast<Blk *>(blocks), n);
	return hipGetLastError();
}

hipError_t launch_bgzf_pack(const uint8_t *raw, const void *blocks, int64_t n, const uint8_t *slots, uint32_t slot_stride, const uint32_t *result,
                            const uint32_t *crc, int stored_only, uint64_t *msz, uint8_t *out, int n_cu, hipStream_t st)
{
	(void)n_cu;
	if (n <= 0) return hipSuccess;
	const Blk *b = reinterpret_cast<const Blk *>(blocks);
	bgzf_member_size_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(b, n, result, stored_only, (u64 *)msz);
	if (hipError_t e = hipGetLastError()) return e;
	if (hipError_t e = launch_scan_u64(msz, n, st)) return e;
	bgzf_pack_kernel<<<(unsigned)((n + 3) / 4), 256, 0, st>>>(raw, b, n, slots, slot_stride, result, crc, stored_only, (const u64 *)msz, out);
	return hipGetLastError();
}

}  // namespace sk
