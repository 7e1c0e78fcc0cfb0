// sk_bamconcat.hip — the record passes of sk_bam_file_concatenate (include/seqkit_hip.h): ONE input of `sam concatenate`
// (src/sam_concatenate.rs), every record in file order with '.' and the decimal input number behind its name.  The BGZF half (cut,
// deflate, pack) is sk_bamwrite.hip's and sk_deflate.hip's, unchanged.
//
// bam_concat_size_kernel — a wave per BGZF block (sk_bamblock.h), as bam_merge_key_kernel is launched: per record its offset in the
//   stream and its output length block_size + 4 + the suffix's bytes, straight into the two columns the window writers read (16 B per
//   record, no key, no sort, no gather); decline bit 8: an invalid record; bit 1: a name that would exceed 254 bytes.
//   bam_merge_scan (sk_bammerge.hip; in place over n + 1 elements) then turns the lengths into output offsets, the total behind them.
// ConcatRecord in bam_write_kernel (sk_bamblock.h) — a window's records, 16 lanes a record through emit.  MergeRecord's three spans:
//   the core behind block_size and the name without its NUL (bytes 13 ..), refID and pos, everything behind the old NUL, all copied as
//   whole dwords; block_size, l_read_name, '.', the one to ten digits, the NUL and the spans' edges go byte by byte.  The number is the
//   launch's, not a column's: digit d of D is (number / 10^(D - 1 - d)) % 10, the power from a table.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/seqkit_hip.h"
#include "sk_bamblock.h"
#include "sk_internal.h"

namespace sk {

namespace {

typedef uint32_t u32;
typedef unsigned long long u64;

__constant__ u32 kPow10[10] = {1u, 10u, 100u, 1000u, 10000u, 100000u, 1000000u, 10000000u, 100000000u, 1000000000u};

__global__ __launch_bounds__(kBlockThreads) void bam_concat_size_kernel(const uint8_t *stream, const u64 *bend, const u64 *entry_of, int64_t nb, const u64 *rb,
                                                                           u32 sl, u64 *krec, u64 *kout, uint32_t *decline)
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
		else if ((u32)r[12] - 1u + sl > 254u) dec |= 1u;
		krec[k] = entry + off[j];
		kout[k] = 4ull + bam_le32_bytes(r) + sl;
	}
	for (int s = 32; s > 0; s >>= 1) dec |= (u32)__shfl_xor((int)dec, s);
	if (dec && lane == 0) atomicOr(decline, dec);
}

// bam_write_kernel's record: ".N" behind the name, N the launch's (sl: the bytes of ".N", 2 .. 11)
struct ConcatRecord {
	u32 number, sl;
	template <class Put>
	__device__ void operator()(const uint8_t *r, int64_t, const Put &put) const
	{
		const u32 n = number, s = sl;
		const u32 bs = bam_le32_bytes(r), lo = r[12];
		const u32 T = 35u + lo;                                            // where the old name's NUL stood: the suffix begins here
		const u32 len = 4u + bs + s;
		auto byte = [&](u32 p) -> u32 {
			if (p < 4u) return ((bs + s) >> (8u * p)) & 0xffu;
			if (p == 12u) return lo + s;
			if (p < T) return r[p];
			if (p == T) return '.';
			if (p == T + s) return 0u;
			if (p > T + s) return r[p - s];
			return '0' + (n / kPow10[T + s - 1u - p]) % 10u;                 // (the last digit stands at T + s - 1)
		};
		put(len, 13u, T - 13u, r + 13, 4u, 8u, r + 4, T + s + 1u, len - (T + s + 1u), r + T + 1u, byte);
	}
};

}  // namespace

hipError_t launch_bam_concat_size(const uint8_t *stream, const uint64_t *bend, const uint64_t *entry, int64_t nb, const uint64_t *rb, uint32_t suffix_len,
                                  uint64_t *krec, uint64_t *kout, uint32_t *decline, hipStream_t st)
{
	if (nb <= 0) return hipSuccess;
	bam_concat_size_kernel<<<block_grid(nb), kBlockThreads, 0, st>>>(stream, (const u64 *)bend, (const u64 *)entry, nb, (const u64 *)rb, suffix_len,
	                                                                 (u64 *)krec, (u64 *)kout, decline);
	return hipGetLastError();
}

hipError_t launch_bam_concat_write(const WriteWindow &w, uint32_t number, uint32_t suffix_len, int n_cu, hipStream_t st)
{
	return launch_bam_write(w, ConcatRecord{number, suffix_len}, n_cu, st);
}

}  // namespace sk
