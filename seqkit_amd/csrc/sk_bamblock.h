// sk_bamblock.h — what the per-block passes over a verified BAM stream share (sk_inflate.hip: bam_gather_kernel; sk_bamtext.hip: the
// reads passes; sk_bamwrite.hip: the rewrite passes).  Such a pass is a wave per BGZF block: lane 0 follows the chain of records from
// the block's entry to its end and leaves every record's offset in LDS, then the 64 lanes take consecutive records.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sk {

// waves per workgroup, and the records that can begin in one block: each takes at least 36 bytes of its 64 KiB
constexpr int kBlockWaves = 4, kBlockRecs = 1824;

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

// inclusive prefix sum over the wave's 64 lanes
__device__ __forceinline__ unsigned long long wave_incl_scan(unsigned long long x, int lane)
{
	for (int s = 1; s < 64; s <<= 1) {
		const unsigned long long y = __shfl_up(x, s);
		if (lane >= s) x += y;
	}
	return x;
}

}  // namespace sk
