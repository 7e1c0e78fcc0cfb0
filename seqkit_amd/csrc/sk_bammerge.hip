// sk_bammerge.hip — the record passes of sk_bam_file_merge (include/seqkit_hip.h): `sam merge` (src/sam_merge.rs) over several verified
// BAM streams that lie in one address space.  The BGZF half (cut, deflate, pack) is sk_bamwrite.hip's and sk_deflate.hip's, unchanged.
//
// The reference pops the smallest (u32 refID, i32 pos) among the inputs' current first records from a heap.  With ties going to the
// lowest input that loop is, for inputs each sorted by the key, the stable merge — and a stable merge is a stable sort of the
// concatenated inputs:
// bam_merge_key_kernel — a wave per BGZF block of ONE input (sk_bamblock.h), launched once per input: per record its address as an
//   offset from input 1's stream (mod 2^64: the window writers add it to that one base again), its key (u32 refID) << 32 | (u32 pos ^
//   0x80000000), its global index (input 1's records first, then input 2's ..), its output length block_size + 4 + the suffix's bytes,
//   and its input number; decline bit 8: an invalid record; bit 1: with a suffix, a name that would exceed 254 bytes.
// bam_merge_order_kernel — a lane per record over the key column in input order: a key below its predecessor's in the same input sets
//   decline bit 2 (block boundaries are nothing special there: the predecessor is the element before).
// the shared stable radix sort of (key, index) (sk_bamminimize.hip: bam_sort_pairs).
// bam_merge_gather_kernel — output place p takes the address, length and input number of record idx[p]; bam_merge_scan (rocprim, in
//   place over n + 1 elements) then turns the lengths into output offsets, the total behind them.
// MergeRecord in bam_write_kernel (sk_bamblock.h) — with a suffix, a window's records: 16 lanes a record through emit.  The core behind block_size and the name
//   without its NUL are one span of the source (bytes 13 ..), refID and pos a second, everything from the CIGAR on a third, all copied
//   as whole dwords; block_size, l_read_name, '.', the digits, the NUL and the spans' edges go byte by byte.  Without a suffix a record
//   is one copied span: sk_bamsubsample.hip's copy writer serves as it stands.
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

constexpr int kMergeThreads = 256;

__global__ __launch_bounds__(kBlockThreads) void bam_merge_key_kernel(const uint8_t *stream, const u64 *bend, const u64 *entry_of, int64_t nb, const u64 *rb,
                                                                         u64 delta, u32 input, u32 sl, const MergeCols m, uint32_t *decline)
{
	BlockPass b;
	if (!block_open(stream, entry_of, bend, nb, b)) return;
	const auto [lane, c, entry, n, off] = b;
	const u64 k0 = rb[c];
	u32 dec = 0u;
	for (u32 j = (u32)lane; j < n; j += 64u) {
		const uint8_t *r = stream + entry + off[j];
		const u64 k = k0 + j;
		if (!bam_record_valid(r)) dec |= 8u;
		else if (sl && (u32)r[12] - 1u + sl > 254u) dec |= 1u;
		m.addr[k] = delta + entry + off[j];
		m.key[k] = ((u64)bam_le32_bytes(r + 4) << 32) | (u64)(bam_le32_bytes(r + 8) ^ 0x80000000u);
		m.idx[k] = (u32)k;
		m.len[k] = 4u + bam_le32_bytes(r) + sl;
		m.in[k] = (uint8_t)input;
	}
	for (int s = 32; s > 0; s >>= 1) dec |= (u32)__shfl_xor((int)dec, s);
	if (dec && lane == 0) atomicOr(decline, dec);
}

__global__ __launch_bounds__(kMergeThreads) void bam_merge_order_kernel(const u64 *key, const uint8_t *in, u64 n, uint32_t *decline)
{
	const u64 k = (u64)blockIdx.x * kMergeThreads + threadIdx.x;
	const bool bad = k > 0 && k < n && in[k] == in[k - 1] && key[k] < key[k - 1];
	if (__any((int)bad) && (threadIdx.x & 63) == 0) atomicOr(decline, 2u);
}

__global__ __launch_bounds__(kMergeThreads) void bam_merge_gather_kernel(const u32 *idx, const MergeCols m, u64 n, u64 *krec, u64 *kout, uint8_t *kin)
{
	const u64 p = (u64)blockIdx.x * kMergeThreads + threadIdx.x;
	if (p >= n) return;
	const u32 g = idx[p];
	krec[p] = m.addr[g];
	kout[p] = m.len[g];
	kin[p] = m.in[g];
}

// bam_write_kernel's record: ".N" behind the name, N from the input column
struct MergeRecord {
	const uint8_t *kin;
	template <class Put>
	__device__ void operator()(const uint8_t *r, int64_t k, const Put &put) const
	{
		const u32 input = kin[k], sl = input >= 10u ? 3u : 2u;
		const u32 bs = bam_le32_bytes(r), lo = r[12];
		const u32 T = 35u + lo;                                            // where the old name's NUL stood: the suffix begins here
		const u32 len = 4u + bs + sl;
		auto byte = [&](u32 p) -> u32 {
			if (p < 4u) return ((bs + sl) >> (8u * p)) & 0xffu;
			if (p == 12u) return lo + sl;
			if (p < T) return r[p];
			if (p == T) return '.';
			if (p == T + sl) return 0u;
			if (p > T + sl) return r[p - sl];
			return '0' + ((sl == 3u && p == T + 1u) ? input / 10u : input % 10u);
		};
		put(len, 13u, T - 13u, r + 13, 4u, 8u, r + 4, T + sl + 1u, len - (T + sl + 1u), r + T + 1u, byte);
	}
};

unsigned merge_grid(uint64_t n) { return (unsigned)((n + kMergeThreads - 1) / kMergeThreads); }

}  // namespace

hipError_t launch_bam_merge_keys(const uint8_t *stream, const uint64_t *bend, const uint64_t *entry, int64_t nb, const uint64_t *rb, uint64_t delta,
                                 uint32_t input, uint32_t suffix_len, const MergeCols &cols, uint32_t *decline, hipStream_t st)
{
	if (nb <= 0) return hipSuccess;
	bam_merge_key_kernel<<<block_grid(nb), kBlockThreads, 0, st>>>(stream, (const u64 *)bend, (const u64 *)entry, nb,
	                                                                                                     (const u64 *)rb, delta, input, suffix_len, cols, decline);
	return hipGetLastError();
}

hipError_t launch_bam_merge_order(const MergeCols &cols, uint64_t n, uint32_t *decline, hipStream_t st)
{
	if (n < 2) return hipSuccess;
	bam_merge_order_kernel<<<merge_grid(n), kMergeThreads, 0, st>>>((const u64 *)cols.key, cols.in, n, decline);
	return hipGetLastError();
}

hipError_t launch_bam_merge_gather(const uint32_t *idx, const MergeCols &cols, uint64_t n, uint64_t *krec, uint64_t *kout, uint8_t *kin, hipStream_t st)
{
	if (n == 0) return hipSuccess;
	bam_merge_gather_kernel<<<merge_grid(n), kMergeThreads, 0, st>>>(idx, cols, n, (u64 *)krec, (u64 *)kout, kin);
	return hipGetLastError();
}

hipError_t bam_merge_scan(void *temp, size_t *temp_bytes, uint64_t *kout, uint64_t n, hipStream_t st)
{
	if (!temp) return rocprim::exclusive_scan(nullptr, *temp_bytes, (u64 *)kout, (u64 *)kout, (u64)0, (size_t)n + 1, rocprim::plus<u64>(), st);
	if (hipError_t e = hipMemsetAsync(kout + n, 0, 8, st)) return e;
	return rocprim::exclusive_scan(temp, *temp_bytes, (u64 *)kout, (u64 *)kout, (u64)0, (size_t)n + 1, rocprim::plus<u64>(), st);
}

hipError_t launch_bam_merge_write(const WriteWindow &w, const uint8_t *kin, int n_cu, hipStream_t st)
{
	return launch_bam_write(w, MergeRecord{kin}, n_cu, st);
}

}  // namespace sk
