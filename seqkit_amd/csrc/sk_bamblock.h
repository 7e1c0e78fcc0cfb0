// sk_bamblock.h — what the per-block passes over a verified BAM stream share (sk_inflate.hip: bam_gather_kernel; sk_bamtext.hip: the
// reads passes; sk_bamwrite.hip, sk_bamminimize.hip, sk_bammarkdup.hip, sk_bammerge.hip, sk_bamcoverage.hip: theirs).  Such a pass is a
// wave per BGZF block: lane 0 follows the chain of records from the block's entry to its end and leaves every record's offset in LDS,
// then the 64 lanes take consecutive records: block_open is how such a kernel begins (two write it out, where they say why),
// block_grid its launch, block_close_size how a sizing pass ends.  Also the name hash (reads, minimize), the byte composition of
// `sam to`'s texts (sk_bamtext.hip, sk_bampair.hip), the span copy (emit) and, around it, the window writer of the BAM-writing calls:
// bam_write_kernel and launch_bam_write over a command's record descriptor, on the grid rule (group_grid) that every window and
// text writer is launched by.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sk_internal.h"

namespace sk {

// waves per workgroup, and the records that can begin in one block: each takes at least 36 bytes of its 64 KiB
constexpr int kBlockWaves = 4, kBlockRecs = 1824, kBlockThreads = kBlockWaves * 64;
inline unsigned block_grid(int64_t nb) { return (unsigned)((nb + kBlockWaves - 1) / kBlockWaves); }

// four bytes at any alignment, little-endian: two aligned dwords and a byte shift (the buffer is readable to the next dword behind
// its last byte; the inflated stream is, 64 bytes beyond)
__device__ __forceinline__ uint32_t bam_le32(const uint8_t *p)
{
	const uintptr_t a = (uintptr_t)p;
	const uint32_t *q = reinterpret_cast<const uint32_t *>(a & ~(uintptr_t)3);
	const uint32_t sh = (uint32_t)(a & 3u);
	const uint32_t lo = q[0];
	if (sh == 0u) return lo;
	return __builtin_amdgcn_alignbyte(q[1], lo, sh);
}

// the same from four byte loads, for the per-record parsers (reads_rec, rw_plan, the text kernel): there the two-dword form measured
// slower (bam_reads_index_kernel 2.74 ms against 2.39 ms on 20 M records) and took more registers
__device__ __forceinline__ uint32_t bam_le32_bytes(const uint8_t *p)
{
	return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// is the record one htslib reads (sk_bamwrite.hip: rw_plan's bit 8): the decline rule of the merge and concatenate passes
__device__ __forceinline__ bool bam_record_valid(const uint8_t *r)
{
	const uint32_t bs = bam_le32_bytes(r), lo = r[12], nc = bam_le32_bytes(r + 16) & 0xffffu, S = bam_le32_bytes(r + 20);
	return !(bs < 32u || lo < 1u || S > 0x7fffffffu || 4ull * nc + lo + (((unsigned long long)S + 1) >> 1) + S > (unsigned long long)(bs - 32u));
}

// lane 0's walk: the offsets (from entry) of the records that begin in [entry, end) into off[], at most kBlockRecs; returns their count
__device__ __forceinline__ uint32_t block_record_offsets(const uint8_t *stream, unsigned long long entry, unsigned long long end, uint16_t *off)
{
	uint32_t k = 0u;
	for (unsigned long long o = entry; o < end && k < (uint32_t)kBlockRecs; k++) {
		off[k] = (uint16_t)(o - entry);
		o += 4 + (unsigned long long)bam_le32(stream + o);
	}
	return k;
}

// the same for a wave that waits for no other: lane 0 walks, every lane gets the count
__device__ __forceinline__ uint32_t wave_record_offsets(const uint8_t *stream, const unsigned long long *entry, const unsigned long long *bend, int64_t c,
                                                        uint16_t *off, int lane)
{
	uint32_t k = 0u;
	if (lane == 0) k = block_record_offsets(stream, entry[c], bend[c], off);
	__builtin_amdgcn_wave_barrier();
	return (uint32_t)__shfl((int)k, 0);
}

// How a per-block pass begins: this wave's lane and block c, the block's entry, and the offsets (from entry) of its n records in the
// wave's own part of the workgroup's LDS.  false: there is no block for this wave, and the kernel returns.  No workgroup barrier may
// follow in such a kernel: the waves without a block have left, and each wave uses its own LDS.
struct BlockPass {
	int lane;
	int64_t c;
	unsigned long long entry;
	uint32_t n;
	const uint16_t *off;
};
__device__ __forceinline__ bool block_open(const uint8_t *stream, const unsigned long long *entry, const unsigned long long *bend, int64_t nb, BlockPass &b)
{
	__shared__ uint16_t offs[kBlockWaves][kBlockRecs];
	const int w = threadIdx.x >> 6;
	b.lane = threadIdx.x & 63;
	b.c = (int64_t)blockIdx.x * kBlockWaves + w;
	if (b.c >= nb) return false;
	b.off = offs[w];
	b.n = wave_record_offsets(stream, entry, bend, b.c, offs[w], b.lane);
	b.entry = entry[b.c];
	return true;
}

// How a sizing pass ends: the lanes' output bytes summed and their records' decline bits ORed over the wave, then lane 0 stores
__device__ __forceinline__ void block_close_size(unsigned long long bytes, uint32_t dec, int lane, unsigned long long *block_bytes, uint32_t *decline)
{
	for (int s = 32; s > 0; s >>= 1) {
		bytes += __shfl_xor(bytes, s);
		dec |= (uint32_t)__shfl_xor((int)dec, s);
	}
	if (lane == 0) {
		*block_bytes = bytes;
		if (dec) atomicOr(decline, dec);
	}
}

// inclusive prefix sum over the wave's 64 lanes
__device__ __forceinline__ unsigned long long wave_incl_scan(unsigned long long x, int lane)
{
	for (int s = 1; s < 64; s <<= 1) {
		const unsigned long long y = __shfl_up(x, s);
		if (lane >= s) x += y;
	}
	return x;
}

// FNV-1a over a name's bytes, then a finalizer (murmur3's fmix64): the pairing key of the reads passes and of sk_bam_file_minimize
__device__ __forceinline__ unsigned long long qname_key(const uint8_t *p, uint32_t n)
{
	unsigned long long h = 0xcbf29ce484222325ull;
	for (uint32_t k = 0; k < n; k++) h = (h ^ p[k]) * 0x100000001b3ull;
	h ^= h >> 33; h *= 0xff51afd7ed558ccdull; h ^= h >> 33; h *= 0xc4ceb9fe1a85ec53ull; h ^= h >> 33;
	return h;
}

// byte p of a kept record's text in `sam to` (sk_bamtext.hip, sk_bampair.hip: write_read, src/sam_to_fastq.rs:138-149; SEQ as sequence(), :31-59)
__device__ __forceinline__ uint32_t reads_byte(uint32_t p, int fmt, const uint8_t *name, uint32_t L, const uint8_t *seq4, const uint8_t *qual, uint32_t S,
                                               bool rev, uint32_t min_baseq)
{
	if (fmt != 0) {
		if (p == 0u) return fmt == 2 ? '@' : '>';
		if (p <= L) return name[p - 1u];
		if (p == L + 1u) return '\n';
		p -= L + 2u;
	}
	if (p < S) {
		const uint32_t s = rev ? S - 1u - p : p;
		if (qual[s] < min_baseq) return 'N';
		const uint32_t code = (seq4[s >> 1] >> ((s & 1u) ? 0 : 4)) & 15u;
		// 1 2 4 8 -> A C G T (reverse strand: T G C A), anything else N
		const uint32_t fw = code == 1u ? 'A' : code == 2u ? 'C' : code == 4u ? 'G' : code == 8u ? 'T' : 'N';
		if (!rev) return fw;
		return fw == 'A' ? 'T' : fw == 'C' ? 'G' : fw == 'G' ? 'C' : fw == 'T' ? 'A' : 'N';
	}
	if (p == S || fmt != 2) return '\n';
	if (p == S + 1u) return '+';
	if (p == S + 2u) return '\n';
	p -= S + 3u;
	if (p < S) return (uint8_t)(33u + qual[p]);
	return '\n';
}

// out[o0 .. o0 + len) by `nl` lanes from lane `lane` on: the bytes in [ro0, ro0 + rl0), [ro1, ro1 + rl1) and [ro2, ro2 + rl2) (relative
// to o0) are src0[p - ro0], src1[p - ro1] and src2[p - ro2], the others byte(p); a span of length 0 takes nothing.  Whole dwords inside
// one span: two aligned loads and one dword store; the others byte by byte (the first and last dwords are shared with what lies around).
template <class ByteFn>
__device__ __forceinline__ void emit(uint8_t *out, unsigned long long o0, unsigned long long len, uint32_t ro0, uint32_t rl0, const uint8_t *src0,
                                     uint32_t ro1, uint32_t rl1, const uint8_t *src1, uint32_t ro2, uint32_t rl2, const uint8_t *src2, const ByteFn &byte,
                                     uint32_t lane, uint32_t nl)
{
	if (len == 0) return;
	const unsigned long long e = o0 + len, d0 = o0 >> 2, d1 = (e - 1) >> 2;
	for (unsigned long long d = d0 + lane; d <= d1; d += nl) {
		const unsigned long long a = d << 2;
		if (a >= o0 && a + 4 <= e) {
			const uint32_t p = (uint32_t)(a - o0);
			uint32_t v;
			if (p >= ro0 && p + 4u <= ro0 + rl0) v = bam_le32(src0 + (p - ro0));
			else if (p >= ro1 && p + 4u <= ro1 + rl1) v = bam_le32(src1 + (p - ro1));
			else if (p >= ro2 && p + 4u <= ro2 + rl2) v = bam_le32(src2 + (p - ro2));
			else v = byte(p) | (byte(p + 1u) << 8) | (byte(p + 2u) << 16) | (byte(p + 3u) << 24);
			*reinterpret_cast<uint32_t *>(out + a) = v;
		} else {
			for (uint32_t b = 0; b < 4u; b++) {
				const unsigned long long pp = a + b;
				if (pp >= o0 && pp < e) out[pp] = (uint8_t)byte((uint32_t)(pp - o0));
			}
		}
	}
}

// ---- a window's records, 16 lanes a record (the window writers here; the text writers of sk_bamtext.hip and sk_bampair.hip) ----
constexpr int kGroupThreads = 256;               // a workgroup: 16 groups of 16 lanes, a record a group
// a group per record, at most 16 workgroups a planned CU: the groups stride over the rest
inline unsigned group_grid(int64_t n, int n_cu)
{
	const int64_t want = (n + kGroupThreads / 16 - 1) / (kGroupThreads / 16), cap = (int64_t)(n_cu > 0 ? n_cu : 256) * 16;
	return (unsigned)(want < cap ? want : cap);
}

// The window writer of the BAM-writing calls.  What a command makes of a record is its descriptor `rec`, passed by value with the
// command's device pointers and flags: rec(r, k, put) reads record k at r and calls put(len, <the three spans of emit>, byte) once.
template <class Rec>
__global__ __launch_bounds__(kGroupThreads) void bam_write_kernel(const WriteWindow w, const Rec rec)
{
	const uint32_t gl = threadIdx.x & 15u;
	const int64_t gstride = ((int64_t)gridDim.x * kGroupThreads) >> 4;
	for (int64_t j = ((int64_t)blockIdx.x * kGroupThreads + threadIdx.x) >> 4; j < w.n; j += gstride) {
		const int64_t k = w.first + j;
		rec(w.stream + w.krec[k], k, [&](unsigned long long len, uint32_t ro0, uint32_t rl0, const uint8_t *src0, uint32_t ro1, uint32_t rl1,
		                                 const uint8_t *src1, uint32_t ro2, uint32_t rl2, const uint8_t *src2, const auto &byte) {
			emit(w.out, w.kout[k] - w.o0, len, ro0, rl0, src0, ro1, rl1, src1, ro2, rl2, src2, byte, gl, 16u);
		});
	}
}

template <class Rec>
hipError_t launch_bam_write(const WriteWindow &w, const Rec &rec, int n_cu, hipStream_t st)
{
	if (w.n <= 0) return hipSuccess;
	bam_write_kernel<<<group_grid(w.n, n_cu), kGroupThreads, 0, st>>>(w, rec);
	return hipGetLastError();
}

}  // namespace sk
