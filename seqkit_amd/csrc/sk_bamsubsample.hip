// sk_bamsubsample.hip — the record passes of sk_bam_file_subsample (include/seqkit_hip.h): `sam subsample` (src/sam_subsample.rs)
// over a verified BAM stream.  The BGZF half (cut, deflate, pack) is sk_bamwrite.hip's and sk_deflate.hip's, unchanged.
//
// The reference keeps a map from a read's name to a decision: a name that is in the map takes the stored decision and LEAVES the map,
// any other name draws a fresh one and enters it; a record with 0x800 is passed over before the map is looked at.  That is the map of
// `sam minimize` with a draw in place of the next number, so the fragment numbers are sk_bamminimize.hip's id passes under the rule
// {the whole name, 0x800 takes no part}: the 1st, 3rd, 5th .. counted record of a name gets the next number d = 1, 2, 3 .. in file
// order, the 2nd, 4th .. the number of the one just before it.  With draw d a pure function of (seed, d) (sk_internal.h:
// subsample_keeps) a record's fate needs nothing but its own number:
// bam_sub_keep_kernel — a lane per record, a grid of at most 8 workgroups a CU striding over the file: len[k] = the record's bytes when
//   it is counted and its draw keeps it, else 0; the counted and the kept records and the kept bytes are summed per lane, then per wave,
//   and added to three counters (with a wave per 64 records, 0.9 M atomic adds to three words made the pass 11.3 ms for 20 M records); a counted record without 0x1 sets decline
//   bit 1 (the reference ends there: the caller's reader serves the file).
// bam_sub_scans — two exclusive scans in record order (rocprim): pos[k] = the kept records before k, off[k] = their bytes.
// bam_sub_compact_kernel — a kept record's stream offset and output offset go to place pos[k]: from here on (the window plan, the
//   deflate windows, the packing) only the kept records exist.
// bam_copy_write_kernel — a window's kept records copied byte for byte, 16 lanes a record, as whole dwords through emit: one span, no
//   patched byte; `sam merge` without --suffix writes its windows with it too.  (A kernel of its own rather than sk_bammarkdup.hip's
//   record with its flag column switched off: that one reads a u16 per record and cuts every record into two spans around bytes
//   18-19, neither of which a plain copy needs.)
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

constexpr int kSubThreads = 256;

__global__ __launch_bounds__(kSubThreads) void bam_sub_keep_kernel(const uint8_t *stream, const u64 *krec, const u32 *ids, u64 n, u64 seed, u32 T,
                                                                   u32 *len, u64 *counts, uint32_t *decline)
{
	u64 counted = 0, kept = 0, bytes = 0;
	bool bad = false;
	for (u64 k = (u64)blockIdx.x * kSubThreads + threadIdx.x; k < n; k += (u64)gridDim.x * kSubThreads) {
		const uint8_t *r = stream + krec[k];
		const u32 flag = bam_le32_bytes(r + 16) >> 16;
		u32 l = 0u;
		if (!(flag & 0x800u)) {
			counted++;
			bad = bad || !(flag & 1u);
			if (subsample_keeps(seed, ids[k], T)) { l = 4u + bam_le32_bytes(r); kept++; bytes += l; }
		}
		len[k] = l;
	}
	for (int s = 32; s > 0; s >>= 1) {
		counted += __shfl_xor(counted, s);
		kept += __shfl_xor(kept, s);
		bytes += __shfl_xor(bytes, s);
	}
	if ((threadIdx.x & 63) == 0) {
		if (counted) atomicAdd(counts, counted);
		if (kept) { atomicAdd(counts + 1, kept); atomicAdd(counts + 2, bytes); }
	}
	if (__any((int)bad) && (threadIdx.x & 63) == 0) atomicOr(decline, 1u);
}

struct IsKept { __host__ __device__ u32 operator()(u32 len) const { return len ? 1u : 0u; } };
struct Widen { __host__ __device__ u64 operator()(u32 len) const { return len; } };

__global__ __launch_bounds__(kSubThreads) void bam_sub_compact_kernel(const u64 *krec, const u32 *len, const u32 *pos, const u64 *off, u64 n, u64 *kept_rec,
                                                                      u64 *kept_out)
{
	const u64 k = (u64)blockIdx.x * kSubThreads + threadIdx.x;
	if (k >= n || !len[k]) return;
	const u32 q = pos[k];                                                  // (q <= k: the kept records before k)
	kept_rec[q] = krec[k];
	kept_out[q] = off[k];
}

// (bam_write_kernel's loop written out: as a descriptor without members, which moves nothing but the launch's hidden arguments, the
// copy measured 0.7 % slower, 5.421 against 5.385 ms over the 82 windows of 20 M records)
__global__ __launch_bounds__(kGroupThreads) void bam_copy_write_kernel(const uint8_t *stream, const u64 *krec, const u64 *kout, int64_t first, int64_t n, u64 o0,
                                                                       uint8_t *out)
{
	const u32 gl = threadIdx.x & 15u;
	const int64_t gstride = ((int64_t)gridDim.x * kGroupThreads) >> 4;
	for (int64_t j = ((int64_t)blockIdx.x * kGroupThreads + threadIdx.x) >> 4; j < n; j += gstride) {
		const int64_t k = first + j;
		const uint8_t *r = stream + krec[k];
		const u32 len = 4u + bam_le32_bytes(r);
		auto byte = [&](u32 p) -> u32 { return r[p]; };
		emit(out, kout[k] - o0, len, 0u, len, r, 0u, 0u, r, 0u, 0u, r, byte, gl, 16u);
	}
}

unsigned sub_grid(uint64_t n) { return (unsigned)((n + kSubThreads - 1) / kSubThreads); }

}  // namespace

hipError_t launch_bam_sub_keep(const uint8_t *stream, const uint64_t *krec, const uint32_t *ids, uint64_t n, uint64_t seed, uint32_t T, uint32_t *len,
                               uint64_t *counts, uint32_t *decline, int n_cu, hipStream_t st)
{
	if (hipError_t e = hipMemsetAsync(counts, 0, 24, st)) return e;
	if (n == 0) return hipSuccess;
	const unsigned cap = (unsigned)(n_cu > 0 ? n_cu : 256) * 8u;
	bam_sub_keep_kernel<<<sub_grid(n) < cap ? sub_grid(n) : cap, kSubThreads, 0, st>>>(stream, (const u64 *)krec, ids, n, seed, T, len, (u64 *)counts, decline);
	return hipGetLastError();
}

hipError_t bam_sub_scans(void *temp, size_t *temp_bytes, const uint32_t *len, uint32_t *pos, uint64_t *off, uint64_t n, hipStream_t st)
{
	auto kept = rocprim::make_transform_iterator(len, IsKept());
	auto wide = rocprim::make_transform_iterator(len, Widen());
	if (!temp) {
		size_t a = 0, b = 0;
		if (hipError_t e = rocprim::exclusive_scan(nullptr, a, kept, pos, 0u, (size_t)n, rocprim::plus<u32>(), st)) return e;
		if (hipError_t e = rocprim::exclusive_scan(nullptr, b, wide, (u64 *)off, (u64)0, (size_t)n, rocprim::plus<u64>(), st)) return e;
		*temp_bytes = a > b ? a : b;
		return hipSuccess;
	}
	if (hipError_t e = rocprim::exclusive_scan(temp, *temp_bytes, kept, pos, 0u, (size_t)n, rocprim::plus<u32>(), st)) return e;
	return rocprim::exclusive_scan(temp, *temp_bytes, wide, (u64 *)off, (u64)0, (size_t)n, rocprim::plus<u64>(), st);
}

hipError_t launch_bam_sub_compact(const uint64_t *krec, const uint32_t *len, const uint32_t *pos, const uint64_t *off, uint64_t n, uint64_t *kept_rec,
                                  uint64_t *kept_out, hipStream_t st)
{
	if (n == 0) return hipSuccess;
	bam_sub_compact_kernel<<<sub_grid(n), kSubThreads, 0, st>>>((const u64 *)krec, len, pos, (const u64 *)off, n, (u64 *)kept_rec, (u64 *)kept_out);
	return hipGetLastError();
}

hipError_t launch_bam_copy_write(const WriteWindow &w, int n_cu, hipStream_t st)
{
	if (w.n <= 0) return hipSuccess;
	bam_copy_write_kernel<<<group_grid(w.n, n_cu), kGroupThreads, 0, st>>>(w.stream, (const u64 *)w.krec, (const u64 *)w.kout, w.first, w.n, w.o0, w.out);
	return hipGetLastError();
}

}  // namespace sk
