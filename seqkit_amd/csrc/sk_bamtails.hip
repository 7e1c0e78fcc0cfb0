// sk_bamtails.hip — the record passes of sk_bam_file_discard_tails (include/seqkit_hip.h): `sam discard tail artifacts`
// (src/sam_discard_tail_artifacts.rs) over a verified BAM stream and a genome whose chromosomes lie raw — newlines included — in device
// memory.  The stream offsets and lengths come from sk_bamconcat.hip's sizing pass, the scans, the compaction and the window copy are
// sk_bamsubsample.hip's, the BGZF half (cut, deflate, pack) sk_bamwrite.hip's and sk_deflate.hip's, unchanged.
//
// bam_tail_used_kernel — a lane per record on a grid capped by the CU count: used[tid] = 1 for every mapped record whose refID the
//   header knows, so that only those chromosomes are read from the FASTA file.
// bam_tail_keep_kernel — a lane per record, the same grid, bam_sub_keep_kernel's shape: an unmapped record (0x4) is written; a mapped
//   one is walked from both ends (count_mismatches, :257-348, in signed 64-bit arithmetic: wherever a value the reference holds in an
//   i32 or an index would leave its range the file is declined, so no wrap is ever modelled here) and written iff both counts stay
//   below min_mismatches.  len[k] = the record's bytes where it is written, else 0; tidc[k] = its refID, kTailUnmapped for an unmapped
//   record; total, failed, passed, written and the written bytes are summed per lane, then per wave, one atomic a wave.  Decline bits:
//   1 a mapped record with an operation outside M I D = X anywhere in its CIGAR, 2 an examined base outside the read or the chromosome,
//   4 a mapped record whose refID has no chromosome, 16 a value outside the i32 range.  Base p of a chromosome is byte
//   p / line_bases * line_width + p % line_bases of its span: the .fai's arithmetic, applied here.
// bam_tail_loads — the chromosome loads after the first, in file order (rocprim): last[k] = the refID of the last mapped record among
//   0 .. k (an inclusive scan under "the right one unless it is unmapped"), then the refIDs of the mapped records that differ from
//   last[k - 1] — from 0 where there is none — selected into loads.
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

constexpr int kTailThreads = 256;
constexpr i64 kI32Min = -2147483648ll, kI32Max = 2147483647ll;

__device__ __forceinline__ bool in_i32(i64 v) { return v >= kI32Min && v <= kI32Max; }

// one walk: the mismatches of the tail, *dec |= the bits of what the reference would stop at or wrap around.  step +1: the operations
// in order from base si on; -1: in reverse.
__device__ __forceinline__ u32 tail_walk(const uint8_t *cigar, u32 n_cigar, const uint8_t *seq4, i64 l_seq, i64 si, i64 ro, const uint8_t *chrom,
                                         const TailRef &ref, u32 T, int step, u32 *dec)
{
	u32 examined = 0u, mm = 0u;
	for (u32 j = 0; j < n_cigar && examined < T; j++) {
		const u32 op = bam_le32_bytes(cigar + 4u * (step > 0 ? j : n_cigar - 1u - j)), code = op & 15u;
		const i64 l = (i64)(op >> 4) * step;
		if (code == 1u) {
			mm++;
			si += l; ro -= l;
			if (!in_i32(si) || !in_i32(ro)) { *dec |= 16u; return mm; }
		} else if (code == 2u) {
			mm++;
			ro += l;
			if (!in_i32(ro)) { *dec |= 16u; return mm; }
		} else {                                                               // M = X (the caller has declined every other code)
			for (u32 k = op >> 4; k > 0u && examined < T; k--) {
				examined++;
				const i64 ri = ro + si;
				if (si < 0 || si >= l_seq || ri < 0 || (u64)ri >= ref.length) { *dec |= 2u; return mm; }
				const u32 c4 = (seq4[si >> 1] >> ((si & 1) ? 0 : 4)) & 15u;
				const u32 rd = c4 == 1u ? 'A' : c4 == 2u ? 'C' : c4 == 4u ? 'G' : c4 == 8u ? 'T' : 'N';
				u32 g = chrom[(u64)ri / ref.line_bases * ref.line_width + (u64)ri % ref.line_bases];
				if (g >= 'a' && g <= 'z') g -= 32u;
				if (!(rd == g || g == 'N' || rd == 'N')) mm++;
				si += step;
			}
		}
	}
	return mm;
}

__global__ __launch_bounds__(kTailThreads) void bam_tail_used_kernel(const uint8_t *stream, const u64 *krec, u64 n, int32_t n_refs, u32 *used)
{
	for (u64 k = (u64)blockIdx.x * kTailThreads + threadIdx.x; k < n; k += (u64)gridDim.x * kTailThreads) {
		const uint8_t *r = stream + krec[k];
		const int32_t tid = (int32_t)bam_le32_bytes(r + 4);
		if (!((bam_le32_bytes(r + 16) >> 16) & 4u) && tid >= 0 && tid < n_refs) used[tid] = 1u;
	}
}

__global__ __launch_bounds__(kTailThreads) void bam_tail_keep_kernel(const uint8_t *stream, const u64 *krec, u64 n, const uint8_t *genome, const TailRef *refs,
                                                                     int32_t n_refs, u32 T, u32 min_mm, u32 *len, int32_t *tidc, u64 *counts, uint32_t *decline)
{
	u64 total = 0, failed = 0, passed = 0, written = 0, bytes = 0;
	u32 dec = 0u;
	for (u64 k = (u64)blockIdx.x * kTailThreads + threadIdx.x; k < n; k += (u64)gridDim.x * kTailThreads) {
		const uint8_t *r = stream + krec[k];
		const u32 rec_bytes = 4u + bam_le32_bytes(r), fl = bam_le32_bytes(r + 16), n_cigar = fl & 0xffffu, l_read_name = r[12];
		const int32_t tid = (int32_t)bam_le32_bytes(r + 4);
		total++;
		u32 l = 0u;
		int32_t tc = kTailUnmapped;
		if ((fl >> 16) & 4u) l = rec_bytes;
		else {
			tc = tid;
			const uint8_t *cigar = r + 36 + l_read_name, *seq4 = cigar + 4u * n_cigar;
			const i64 l_seq = (i64)bam_le32_bytes(r + 20), pos = (int32_t)bam_le32_bytes(r + 8);
			u32 d = 0u;
			i64 shift = 0;                                                   // the deletions' lengths less the insertions'
			for (u32 j = 0; j < n_cigar; j++) {
				const u32 op = bam_le32_bytes(cigar + 4u * j), code = op & 15u;
				if (code == 1u) shift -= (i64)(op >> 4);
				else if (code == 2u) shift += (i64)(op >> 4);
				else if (code != 0u && code != 7u && code != 8u) d |= 1u;
			}
			if (tid < 0 || tid >= n_refs || refs[tid < 0 || tid >= n_refs ? 0 : tid].line_bases == 0ull) d |= 4u;
			if (!in_i32(shift) || !in_i32(pos + shift)) d |= 16u;
			if (!d) {
				const TailRef ref = refs[tid];
				const uint8_t *chrom = genome + ref.base;
				const u32 left = tail_walk(cigar, n_cigar, seq4, l_seq, 0, pos, chrom, ref, T, 1, &d);
				const u32 right = tail_walk(cigar, n_cigar, seq4, l_seq, l_seq - 1, pos + shift, chrom, ref, T, -1, &d);
				if (!d) {
					if (left >= min_mm || right >= min_mm) failed++;
					else { passed++; l = rec_bytes; }
				}
			}
			dec |= d;
		}
		if (l) { written++; bytes += l; }
		len[k] = l;
		tidc[k] = tc;
	}
	for (int s = 32; s > 0; s >>= 1) {
		total += __shfl_xor(total, s);
		failed += __shfl_xor(failed, s);
		passed += __shfl_xor(passed, s);
		written += __shfl_xor(written, s);
		bytes += __shfl_xor(bytes, s);
		dec |= (u32)__shfl_xor((int)dec, s);
	}
	if ((threadIdx.x & 63) == 0) {
		if (total) atomicAdd(counts, total);
		if (failed) atomicAdd(counts + 1, failed);
		if (passed) atomicAdd(counts + 2, passed);
		if (written) { atomicAdd(counts + 3, written); atomicAdd(counts + 4, bytes); }
		if (dec) atomicOr(decline, dec);
	}
}

struct LastMapped {
	__host__ __device__ int32_t operator()(int32_t a, int32_t b) const { return b == kTailUnmapped ? a : b; }
};
// does record k load a chromosome: it is mapped, and the last mapped record before it — chromosome 0 where there is none — had another refID
struct IsLoad {
	const int32_t *tidc, *last;
	__host__ __device__ uint8_t operator()(size_t k) const
	{
		const int32_t t = tidc[k];
		if (t == kTailUnmapped) return 0;
		const int32_t before = k ? last[k - 1] : kTailUnmapped;
		return t != (before == kTailUnmapped ? 0 : before) ? 1 : 0;
	}
};

unsigned tail_grid(uint64_t n, int n_cu)
{
	const uint64_t want = (n + kTailThreads - 1) / kTailThreads, cap = (uint64_t)(n_cu > 0 ? n_cu : 256) * 8u;
	return (unsigned)(want < cap ? want : cap);
}

}  // namespace

hipError_t launch_bam_tail_used(const uint8_t *stream, const uint64_t *krec, uint64_t n, int32_t n_refs, uint32_t *used, int n_cu, hipStream_t st)
{
	if (hipError_t e = hipMemsetAsync(used, 0, (size_t)n_refs * 4, st)) return e;
	if (n == 0) return hipSuccess;
	bam_tail_used_kernel<<<tail_grid(n, n_cu), kTailThreads, 0, st>>>(stream, (const u64 *)krec, n, n_refs, used);
	return hipGetLastError();
}

hipError_t launch_bam_tail_keep(const uint8_t *stream, const uint64_t *krec, uint64_t n, const uint8_t *genome, const TailRef *refs, int32_t n_refs,
                                uint32_t tail_length, uint32_t min_mismatches, uint32_t *len, int32_t *tidc, uint64_t *counts, uint32_t *decline, int n_cu,
                                hipStream_t st)
{
	if (hipError_t e = hipMemsetAsync(counts, 0, 40, st)) return e;
	if (n == 0) return hipSuccess;
	bam_tail_keep_kernel<<<tail_grid(n, n_cu), kTailThreads, 0, st>>>(stream, (const u64 *)krec, n, genome, refs, n_refs, tail_length, min_mismatches, len, tidc,
	                                                                  (u64 *)counts, decline);
	return hipGetLastError();
}

hipError_t bam_tail_loads(void *temp, size_t *temp_bytes, const int32_t *tidc, int32_t *last, int32_t *loads, uint64_t *n_loads, uint64_t n, hipStream_t st)
{
	auto flags = rocprim::make_transform_iterator(rocprim::counting_iterator<size_t>(0), IsLoad{tidc, last});
	if (!temp) {
		size_t a = 0, b = 0;
		if (hipError_t e = rocprim::inclusive_scan(nullptr, a, tidc, last, (size_t)n, LastMapped(), st)) return e;
		if (hipError_t e = rocprim::select(nullptr, b, tidc, flags, loads, (size_t *)n_loads, (size_t)n, st)) return e;
		*temp_bytes = a > b ? a : b;
		return hipSuccess;
	}
	if (hipError_t e = rocprim::inclusive_scan(temp, *temp_bytes, tidc, last, (size_t)n, LastMapped(), st)) return e;
	return rocprim::select(temp, *temp_bytes, tidc, flags, loads, (size_t *)n_loads, (size_t)n, st);
}

}  // namespace sk
