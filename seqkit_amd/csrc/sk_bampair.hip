// sk_bampair.hip — the mate pairing of `sam to [interleaved] raw|fasta|fastq` (src/sam_to_fastq.rs:113-137) over the kept records of
// sk_bamtext.hip's reads passes, and the text of an output window in the order it is written (include/seqkit_hip.h: sk_bam_file_pairs).
//
// The reference keeps two maps, reads_1 and reads_2, from a name to the pending text of that name's first / last mate.  A first mate
// whose name is in reads_2 completes a pair (it leaves the map), else it enters reads_1, where a second insert REPLACES the text; a last
// mate mirrors that.  Per name at most one of the two maps holds an entry — to enter reads_1 the name must be absent from reads_2 and
// the other way round — and what it holds is always the record of that name seen LAST.  So per name, over its records r[0], r[1] .. in
// file order: r[i] completes a pair iff r[i - 1] is held and is of the other kind, c[i] = d[i] & !c[i - 1] with d[i] = (kind[i] !=
// kind[i - 1]) and d[0] = 0.  Behind a position z with d[z] = 0 the c alternate 1 0 1 0 .. as long as d stays 1: c[i] = (i - z(i)) & 1
// with z(i) the last position <= i where d is 0.  A record with c = 0 is held; the next record of its name decides its fate: of the other
// kind, it completes the pair; of the same kind, it replaces the held record, which is written nowhere; none, the held record is a
// leftover.  The map entry's ORDER is that of the first insert since the name was last absent: the first record of the stretch of held
// records that ends with the leftover, h(i) = the last position <= i with c = 0 whose predecessor is not held (c = 1, or none).
// In data-parallel form:
// bam_pair_compact_kernel — the paired kept records' (key, index) in file order (their places: an inclusive scan of kind != 0), and every
//   kept record's initial fate.
// the shared stable radix sort by key (sk_bamminimize.hip: bam_sort_pairs): a name's records are adjacent, in file order.
// bam_pair_heads_kernel — per sorted position p the value p where d = 0 (a run's head, or the kind of the record before); two
//   records of one run whose NAMES differ set decline bit 64 (a key collision: nothing is guessed).  A max-scan gives z.
// bam_pair_holds_kernel — the value p where a stretch of held records begins; a max-scan gives h.
// bam_pair_fates_kernel — per record its fate and partner: the completer's index for both records of a pair, the order record for a
//   leftover; and per record its class for the ranks: unpaired, completer, order record of a leftover first / last mate.  A record has
//   one class at most.  Runs of any length — one name on every record of the file — cost the same.
// the ranks: one inclusive scan in FILE order of the four class counts.  An unpaired record's place in the single stream is its rank;
//   a pair's number is its completer's rank (pairs are written when they complete); a leftover's is its order record's rank.
// bam_pair_place_kernel — every written record into its stream's permutation rank -> record, and its text length beside it; an exclusive
//   scan per stream gives the 64-bit stream offsets.
// bam_pair_text_kernel — sk_bamtext.hip's text writer with the records taken through the permutation and the destinations from the
//   stream offsets: a window is a rank range of one stream, its sources lie anywhere in the resident stream.
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

constexpr int kPairThreads = kPairBlock;

struct IsPaired { __host__ __device__ u32 operator()(uint8_t kind) const { return kind ? 1u : 0u; } };
struct ClassCount {
	__host__ __device__ PairRanks operator()(uint8_t cls) const { return PairRanks{cls == kPairClsSingle, cls == kPairClsCompleter, cls == kPairClsOrder1, cls == kPairClsOrder2}; }
};
struct RanksPlus {
	__host__ __device__ PairRanks operator()(const PairRanks &a, const PairRanks &b) const
	{
		return PairRanks{a.single + b.single, a.pair + b.pair, a.order1 + b.order1, a.order2 + b.order2};
	}
};

__global__ __launch_bounds__(kPairThreads) void bam_pair_compact_kernel(const uint8_t *kkind, const u64 *kkey, const u32 *ipos, u64 K, u64 key_mask, u64 *key,
                                                                        u32 *idx, uint8_t *fate, u32 *aux, uint8_t *cls)
{
	const u64 k = (u64)blockIdx.x * kPairThreads + threadIdx.x;
	if (k >= K) return;
	const uint8_t kind = kkind[k];
	fate[k] = kind ? kPairNowhere : kPairSingle;
	cls[k] = kind ? kPairClsNone : kPairClsSingle;
	aux[k] = (u32)k;
	if (kind) {
		const u32 p = ipos[k] - 1u;
		key[p] = kkey[k] & key_mask;
		idx[p] = (u32)k;
	}
}

__device__ __forceinline__ bool same_name(const uint8_t *a, const uint8_t *b)
{
	const u32 la = a[12];
	if (la != (u32)b[12]) return false;
	for (u32 q = 0; q + 1u < la; q++) if (a[36 + q] != b[36 + q]) return false;
	return true;
}

__global__ __launch_bounds__(kPairThreads) void bam_pair_heads_kernel(const uint8_t *stream, const u64 *krec, const uint8_t *kkind, const u64 *key, const u32 *idx,
                                                                      u64 P, u32 *lz, uint32_t *decline)
{
	const u64 p = (u64)blockIdx.x * kPairThreads + threadIdx.x;
	if (p >= P) return;
	bool zero = p == 0 || key[p] != key[p - 1];
	if (!zero) {
		const u32 me = idx[p], prev = idx[p - 1];
		if (!same_name(stream + krec[me], stream + krec[prev])) atomicOr(decline, 64u);
		zero = kkind[me] == kkind[prev];
	}
	lz[p] = zero ? (u32)p : 0u;
}

// (after the max-scan of lz) hs[p] = p where a stretch of held records begins
__global__ __launch_bounds__(kPairThreads) void bam_pair_holds_kernel(const u64 *key, const u32 *lz, u64 P, u32 *hs)
{
	const u64 p = (u64)blockIdx.x * kPairThreads + threadIdx.x;
	if (p >= P) return;
	const bool c = ((u32)p - lz[p]) & 1u;
	const bool head = p == 0 || key[p] != key[p - 1];
	const bool begins = !c && (head || (((u32)(p - 1) - lz[p - 1]) & 1u));
	hs[p] = begins ? (u32)p : 0u;
}

__global__ __launch_bounds__(kPairThreads) void bam_pair_fates_kernel(const u64 *key, const u32 *idx, const uint8_t *kkind, const u32 *lz, const u32 *hs, u64 P,
                                                                      uint8_t *fate, u32 *aux, uint8_t *cls)
{
	const u64 p = (u64)blockIdx.x * kPairThreads + threadIdx.x;
	if (p >= P) return;
	const u32 k = idx[p];
	const uint8_t kind = kkind[k];
	const uint8_t to_stream = kind == 1 ? kPairStream1 : kPairStream2;
	if (((u32)p - lz[p]) & 1u) {                                            // completes a pair with the record before it
		fate[k] = to_stream; aux[k] = k; cls[k] = kPairClsCompleter;
		return;
	}
	if (p + 1 < P && key[p + 1] == key[p]) {                              // held, and the name comes again
		const u32 nx = idx[p + 1];
		if (kkind[nx] != kind) { fate[k] = to_stream; aux[k] = nx; }
		else fate[k] = kPairNowhere;                                       // HashMap::insert replaces the value
		return;
	}
	const u32 o = idx[hs[p]];                                               // held to the end: a leftover, ordered by its entry's first insert
	fate[k] = kind == 1 ? kPairLeft1 : kPairLeft2;
	aux[k] = o;
	cls[o] = kind == 1 ? kPairClsOrder1 : kPairClsOrder2;
}

// stream s holds n[s] records; its permutation and lengths / offsets begin at entry base[s] + s (n[s] + 1 entries: the last one the total)
struct PairPlan {
	u64 n[3], base[3];
	u32 n_single, n_left1;
	int interleaved;
};

__global__ __launch_bounds__(kPairThreads) void bam_pair_place_kernel(const uint8_t *fate, const u32 *aux, const PairRanks *ranks, const u64 *ktoff, u64 K, u64 T,
                                                                      const PairPlan pl, u32 *perm, u64 *slen)
{
	const u64 k = (u64)blockIdx.x * kPairThreads + threadIdx.x;
	if (k == 0) for (int s = 0; s < 3; s++) slen[pl.base[s] + s + pl.n[s]] = 0;
	if (k >= K) return;
	const uint8_t f = fate[k];
	int s;
	u64 r;
	if (f == kPairSingle) { s = 2; r = ranks[k].single - 1u; }
	else if (f == kPairStream1 || f == kPairStream2) {
		const u64 pair = ranks[aux[k]].pair - 1u;
		if (pl.interleaved) { s = 0; r = 2 * pair + (f == kPairStream2 ? 1 : 0); }
		else { s = f == kPairStream1 ? 0 : 1; r = pair; }
	} else if (f == kPairLeft1) { s = 2; r = (u64)pl.n_single + ranks[aux[k]].order1 - 1u; }
	else if (f == kPairLeft2) { s = 2; r = (u64)pl.n_single + pl.n_left1 + ranks[aux[k]].order2 - 1u; }
	else return;
	if (r >= pl.n[s]) return;                                               // (interleaved: the single stream is not produced)
	const u64 g = pl.base[s] + s + r;
	perm[g] = (u32)k;
	slen[g] = (k + 1 < K ? ktoff[k + 1] : T) - ktoff[k];
}

struct PairText {
	const uint8_t *stream;
	const u64 *krec;
	const u32 *perm;         // the stream's: rank -> kept record
	const u64 *soff;         // the stream's: rank -> offset of the record's text in the stream's output
	int64_t first, n;
	int fmt;
	uint32_t min_baseq;
	uint8_t *text;
};

__global__ __launch_bounds__(kPairThreads) void bam_pair_text_kernel(const PairText a)
{
	const int gl = threadIdx.x & 15;
	const int64_t gstride = ((int64_t)gridDim.x * kPairThreads) >> 4;
	const u64 t0 = a.soff[a.first];
	for (int64_t j = ((int64_t)blockIdx.x * kPairThreads + threadIdx.x) >> 4; j < a.n; j += gstride) {
		const uint8_t *r = a.stream + a.krec[a.perm[a.first + j]];
		const uint32_t w12 = bam_le32_bytes(r + 12), w16 = bam_le32_bytes(r + 16), S = bam_le32_bytes(r + 20);
		const uint32_t l_name = w12 & 0xffu, n_cigar = w16 & 0xffffu, L = l_name - 1u;
		const bool rev = (w16 >> 16) & 0x10u;
		const uint8_t *name = r + 36, *seq4 = name + l_name + 4u * n_cigar, *qual = seq4 + ((S + 1u) >> 1);
		const u64 tb = a.soff[a.first + j] - t0, te = a.soff[a.first + j + 1] - t0;
		if (te == tb) continue;
		const u64 d0 = tb >> 2, d1 = (te - 1) >> 2;
		for (u64 d = d0 + (u64)gl; d <= d1; d += 16u) {
			const u64 p0 = d << 2;
			if (p0 >= tb && p0 + 4 <= te) {
				const uint32_t p = (uint32_t)(p0 - tb);
				uint32_t wv = 0u;
				for (uint32_t b = 0; b < 4u; b++) wv |= reads_byte(p + b, a.fmt, name, L, seq4, qual, S, rev, a.min_baseq) << (8u * b);
				*reinterpret_cast<uint32_t *>(a.text + p0) = wv;
			} else {
				for (uint32_t b = 0; b < 4u; b++) {
					const u64 pp = p0 + b;
					if (pp >= tb && pp < te) a.text[pp] = (uint8_t)reads_byte((uint32_t)(pp - tb), a.fmt, name, L, seq4, qual, S, rev, a.min_baseq);
				}
			}
		}
	}
}

unsigned grid_of(u64 n) { return (unsigned)((n + kPairThreads - 1) / kPairThreads); }

}  // namespace

// the scans: temp_bytes serves every one of them over n (offsets: n + 1) elements
hipError_t bam_pair_scan_bytes(uint64_t n, size_t *temp_bytes, hipStream_t st)
{
	size_t a = 0, b = 0, m = 0, o = 0;
	if (hipError_t e = rocprim::inclusive_scan(nullptr, a, rocprim::make_transform_iterator((const uint8_t *)nullptr, IsPaired()), (u32 *)nullptr, (size_t)n, rocprim::plus<u32>(), st)) return e;
	if (hipError_t e = rocprim::inclusive_scan(nullptr, b, rocprim::make_transform_iterator((const uint8_t *)nullptr, ClassCount()), (PairRanks *)nullptr, (size_t)n, RanksPlus(), st)) return e;
	if (hipError_t e = rocprim::inclusive_scan(nullptr, m, (u32 *)nullptr, (u32 *)nullptr, (size_t)n, rocprim::maximum<u32>(), st)) return e;
	if (hipError_t e = rocprim::exclusive_scan(nullptr, o, (u64 *)nullptr, (u64 *)nullptr, (u64)0, (size_t)n + 1, rocprim::plus<u64>(), st)) return e;
	*temp_bytes = a > b ? a : b;
	if (m > *temp_bytes) *temp_bytes = m;
	if (o > *temp_bytes) *temp_bytes = o;
	return hipSuccess;
}
// ipos[k] = the paired records among kept records 0 .. k
hipError_t bam_pair_scan_paired(void *temp, size_t temp_bytes, const uint8_t *kkind, uint32_t *ipos, uint64_t n, hipStream_t st)
{
	if (n == 0) return hipSuccess;
	return rocprim::inclusive_scan(temp, temp_bytes, rocprim::make_transform_iterator(kkind, IsPaired()), ipos, (size_t)n, rocprim::plus<u32>(), st);
}
// v[p] = max(v[0 .. p]), in place
hipError_t bam_pair_scan_max(void *temp, size_t temp_bytes, uint32_t *v, uint64_t n, hipStream_t st)
{
	if (n == 0) return hipSuccess;
	return rocprim::inclusive_scan(temp, temp_bytes, v, v, (size_t)n, rocprim::maximum<u32>(), st);
}
// ranks[k] = per class the records of that class among kept records 0 .. k
hipError_t bam_pair_scan_ranks(void *temp, size_t temp_bytes, const uint8_t *cls, PairRanks *ranks, uint64_t n, hipStream_t st)
{
	if (n == 0) return hipSuccess;
	return rocprim::inclusive_scan(temp, temp_bytes, rocprim::make_transform_iterator(cls, ClassCount()), ranks, (size_t)n, RanksPlus(), st);
}
// lens[0 .. n] (lens[n] = 0) -> exclusive offsets, lens[n] the sum; in place
hipError_t bam_pair_scan_offsets(void *temp, size_t temp_bytes, uint64_t *lens, uint64_t n, hipStream_t st)
{
	return rocprim::exclusive_scan(temp, temp_bytes, (u64 *)lens, (u64 *)lens, (u64)0, (size_t)n + 1, rocprim::plus<u64>(), st);
}

hipError_t launch_bam_pair_compact(const uint8_t *kkind, const uint64_t *kkey, const uint32_t *ipos, uint64_t K, int key_bits, uint64_t *key, uint32_t *idx,
                                   uint8_t *fate, uint32_t *aux, uint8_t *cls, hipStream_t st)
{
	if (K == 0) return hipSuccess;
	const u64 mask = key_bits >= 64 ? ~0ull : (1ull << key_bits) - 1ull;
	bam_pair_compact_kernel<<<grid_of(K), kPairThreads, 0, st>>>(kkind, (const u64 *)kkey, ipos, K, mask, (u64 *)key, idx, fate, aux, cls);
	return hipGetLastError();
}

hipError_t launch_bam_pair_heads(const uint8_t *stream, const uint64_t *krec, const uint8_t *kkind, const uint64_t *key, const uint32_t *idx, uint64_t P,
                                 uint32_t *lz, uint32_t *decline, hipStream_t st)
{
	if (P == 0) return hipSuccess;
	bam_pair_heads_kernel<<<grid_of(P), kPairThreads, 0, st>>>(stream, (const u64 *)krec, kkind, (const u64 *)key, idx, P, lz, decline);
	return hipGetLastError();
}

hipError_t launch_bam_pair_holds(const uint64_t *key, const uint32_t *lz, uint64_t P, uint32_t *hs, hipStream_t st)
{
	if (P == 0) return hipSuccess;
	bam_pair_holds_kernel<<<grid_of(P), kPairThreads, 0, st>>>((const u64 *)key, lz, P, hs);
	return hipGetLastError();
}

hipError_t launch_bam_pair_fates(const uint64_t *key, const uint32_t *idx, const uint8_t *kkind, const uint32_t *lz, const uint32_t *hs, uint64_t P,
                                 uint8_t *fate, uint32_t *aux, uint8_t *cls, hipStream_t st)
{
	if (P == 0) return hipSuccess;
	bam_pair_fates_kernel<<<grid_of(P), kPairThreads, 0, st>>>((const u64 *)key, idx, kkind, lz, hs, P, fate, aux, cls);
	return hipGetLastError();
}

hipError_t launch_bam_pair_place(const uint8_t *fate, const uint32_t *aux, const PairRanks *ranks, const uint64_t *ktoff, uint64_t K, uint64_t T,
                                 const uint64_t n[3], const uint64_t base[3], uint32_t n_single, uint32_t n_left1, int interleaved, uint32_t *perm,
                                 uint64_t *slen, hipStream_t st)
{
	PairPlan pl;
	for (int s = 0; s < 3; s++) { pl.n[s] = n[s]; pl.base[s] = base[s]; }
	pl.n_single = n_single; pl.n_left1 = n_left1; pl.interleaved = interleaved;
	bam_pair_place_kernel<<<grid_of(K ? K : 1), kPairThreads, 0, st>>>(fate, aux, ranks, (const u64 *)ktoff, K, T, pl, perm, (u64 *)slen);
	return hipGetLastError();
}

hipError_t launch_bam_pair_text(const uint8_t *stream, const uint64_t *krec, const uint32_t *perm, const uint64_t *soff, int64_t first, int64_t n, int fmt,
                                uint8_t min_baseq, uint8_t *text, int n_cu, hipStream_t st)
{
	if (n <= 0) return hipSuccess;
	PairText a;
	a.stream = stream; a.krec = (const u64 *)krec; a.perm = perm; a.soff = (const u64 *)soff; a.first = first; a.n = n; a.fmt = fmt; a.min_baseq = min_baseq;
	a.text = text;
	static_assert(kPairThreads == kGroupThreads, "bam_pair_text_kernel is launched on group_grid");
	bam_pair_text_kernel<<<group_grid(n, n_cu), kPairThreads, 0, st>>>(a);
	return hipGetLastError();
}

}  // namespace sk
