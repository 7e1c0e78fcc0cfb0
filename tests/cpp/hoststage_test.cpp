// hoststage_test.cpp — sk_hoststage.h (what the host-pointer entry points of sk_capi_*.cpp stage through the ctx's workspace) on the host,
// built with the address and undefined-behaviour sanitizers (tests/test_hoststage_cpu.py).  The column lists of the entry points are
// restated here as sk_capi_*.cpp give them, in every mode that changes the list; the chunk rules and the bytes of a half are written
// out a second time as the plain arithmetic the entry points did by hand before the header existed.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sanitizer/asan_interface.h>

#include <set>
#include <utility>
#include <vector>

#include "sk_hoststage.h"

using namespace hoststage;

static long g_checks = 0;
static char g_what[256] = "";                    // the case at hand, for a failing CHECK
#define CHECK(cond)                                                                                                     \
	do {                                                                                                                \
		g_checks++;                                                                                                     \
		if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed [%s]\n", __FILE__, __LINE__, #cond, g_what); exit(1); }   \
	} while (0)

static const int64_t kNs[] = {1, 7, 8, 9, 63, 64, 65, 255, 256, 257, 5003, 70001};
static const int kStrides[] = {1, 17, 150, 152, 65535};
static const size_t kPipeChunkBytes = 48u << 20;
// SK_HOST_CHUNK_LOG2 = 6, 7, 12, 15, and the call's own budget
static std::vector<uint64_t> budgets(uint64_t dflt) { return {1u << 6, 1u << 7, 1u << 12, 1u << 15, dflt}; }

// ---- one call's list, with what the test knows about each column ------------------------------------------------------------------
struct Call {
	Stage st;
	uint8_t *dev[16];                                // what carve() sets
	struct Want { uint64_t row_bits; Dir dir; bool host; };
	std::vector<Want> want;
	uint8_t *host_base = (uint8_t *)(uintptr_t)0x10000000;      // never touched, only compared
	void add_bits(uint64_t row_bits, Dir dir, bool present)
	{
		const size_t i = want.size();
		dev[i] = (uint8_t *)(uintptr_t)1;
		st.add_bits(dev[i], row_bits, dir, present && dir != kDev ? host_base + i * 0x1000000 : nullptr);
		want.push_back({row_bits, dir, present && dir != kDev});
	}
	void add(uint64_t row_bytes, Dir dir, bool present = true) { add_bits(row_bytes * 8, dir, present); }
	bool region(size_t i) const { return want[i].dir == kDev || want[i].host; }
	size_t bytes(size_t i, int64_t rows) const { return (size_t)(((uint64_t)rows * want[i].row_bits + 7) / 8); }
};

// Everything the issue asks of one (list, chunk, n): the chunk against the table's arithmetic and its granule and minimum, the half
// against the hand-written sum, alignment, disjointness, the total, the chunks' cover of [0, n), the carved pointers and the copies of
// every chunk, and every region of every chunk memset in a heap buffer of exactly the total.  (A region's extent depends on the half
// and on the chunk's rows alone: each distinct pair is memset once — the first chunk of each half and the last one.  A region above
// 256 KiB — a pitch of 65535 makes halves of 50 MB, 20 000 times — is memset at its two ends, 64 KiB each, and the sanitizer is asked
// about every byte between them: the buffer is one piece, so a region whose ends are inside it is inside it.)
static void fill_region(uint8_t *p, size_t bytes, int fill)
{
	const size_t edge = 64 << 10;
	if (bytes <= 4 * edge) { memset(p, fill, bytes); return; }
	memset(p, fill, edge);
	memset(p + bytes - edge, fill, edge);
	if (__asan_region_is_poisoned(p, bytes) != nullptr) { fprintf(stderr, "region of %zu bytes leaves the buffer\n", bytes); exit(1); }
}

static void check(Call &c, int64_t chunk, int64_t table_chunk, int64_t granule, int64_t min_rows, int64_t n, size_t expect_half, size_t tail, int lanes,
                  int64_t first_row_granule)
{
	Stage &st = c.st;
	CHECK(chunk == table_chunk);
	CHECK(chunk % granule == 0 && chunk >= min_rows && chunk >= 1);
	st.plan(chunk, tail, lanes);
	CHECK(st.chunk() == chunk);
	CHECK(st.half() == expect_half);
	CHECK(st.half() % 256 == 0 && st.tail_at() == (size_t)lanes * st.half());
	CHECK(st.total() == (size_t)lanes * st.half() + up(tail));
	// the regions of a half at the full chunk: on multiples of 256, in order, disjoint, inside the half
	std::vector<std::pair<size_t, size_t>> full;
	st.each_region(chunk, [&](size_t at, size_t bytes) { full.push_back({at, bytes}); });
	size_t n_regions = 0, end = 0;
	for (size_t i = 0; i < c.want.size(); i++) n_regions += c.region(i) ? 1 : 0;
	CHECK(full.size() == n_regions);
	for (auto &r : full) {
		CHECK(r.first % 256 == 0 && r.first >= end && r.second > 0);
		end = r.first + r.second;
	}
	CHECK(end <= st.half() && up(end) == st.half());
	// (a heap buffer of exactly the total; the case before this one left its own when it had the same total)
	static uint8_t *base = nullptr;
	static size_t base_bytes = 0;
	if (!base || base_bytes != st.total()) { free(base); base = (uint8_t *)malloc(st.total()); base_bytes = st.total(); }
	CHECK(base != nullptr && st.total() > 0);
	std::vector<size_t> idx[3];                                              // the columns that have a copy, by direction
	for (size_t i = 0; i < c.want.size(); i++) if (c.want[i].host) idx[c.want[i].dir].push_back(i);
	std::set<std::pair<int, int64_t>> seen;
	// (the byte stream of sk_mask_by_quality at 2^6 bytes a chunk is 70 M chunks, all but the last alike: beyond 4096 chunks the first
	// and the last 2048 are walked, the rows between them are whole chunks by the same arithmetic)
	const int64_t n_chunks = (n + chunk - 1) / chunk;
	int64_t r0 = 0;
	for (int64_t k = 0; r0 < n; k++) {
		if (k == 2048 && n_chunks > 4096) { k = n_chunks - 2048; r0 = k * chunk; }
		const int64_t nr = st.rows_at(r0, n);
		CHECK(nr >= 1 && nr <= chunk && (nr == chunk || r0 + nr == n));       // every chunk but the last is a whole one
		CHECK(r0 % first_row_granule == 0);
		const int h = (int)(k % lanes);
		uint8_t *half = base + (size_t)h * st.half();
		st.carve(half);
		size_t at = 0, i_copy[3] = {0, 0, 0};
		for (size_t i = 0; i < c.want.size(); i++) {
			if (!c.region(i)) { CHECK(c.dev[i] == nullptr); continue; }        // absent: NULL for the kernel
			CHECK(c.dev[i] == half + at && ((uintptr_t)(c.dev[i] - base) & 255) == 0);
			CHECK(c.bytes(i, nr) <= c.bytes(i, chunk));
			at += up(c.bytes(i, chunk));
		}
		for (Dir dir : {kIn, kOut, kDev}) {
			st.each_copy(dir, r0, nr, [&](size_t off, uint8_t *host, size_t bytes) {
				CHECK(i_copy[dir] < idx[dir].size());
				const size_t i = idx[dir][i_copy[dir]++];
				CHECK(half + off == c.dev[i] && bytes == c.bytes(i, nr) && bytes > 0);
				CHECK(host == c.host_base + i * 0x1000000 + (uint64_t)r0 * c.want[i].row_bits / 8 && (uint64_t)r0 * c.want[i].row_bits % 8 == 0);
			});
			CHECK(i_copy[dir] == idx[dir].size());
		}
		if (seen.insert({h, nr}).second) {
			int fill = 0x40;
			st.each_region(nr, [&](size_t off, size_t bytes) { fill_region(half + off, bytes, fill++); });      // (ASan: inside the buffer)
			fill = 0x40;
			st.each_region(nr, [&](size_t off, size_t bytes) { CHECK(half[off] == fill && half[off + bytes - 1] == fill); fill++; });   // (and no region on another)
		}
		r0 += chunk;
	}
	CHECK(r0 >= n && r0 - n < chunk);                                        // [0, n) exactly once, in order
	if (tail) memset(base + st.tail_at(), 0x3f, up(tail));
}

// ---- the table of the chunk rules, as plain arithmetic (what the entry points computed by hand) -----------------------------------
static int64_t table_fused(uint64_t budget_bytes, size_t per_row, int64_t n)
{
	int64_t chunk = (int64_t)(budget_bytes / (per_row ? per_row : 1));
	chunk &= ~(int64_t)63;
	if (chunk < 64) chunk = 64;
	if (chunk > n) chunk = (n + 63) & ~(int64_t)63;
	return chunk;
}
static int64_t table_mask(uint64_t budget_bytes, int64_t total)
{
	int64_t chunk = (int64_t)budget_bytes;
	if (chunk > total) chunk = (total + 15) & ~(int64_t)15;
	return chunk;
}
static int64_t table_rows(uint64_t budget_rows, int64_t n)                   // sk_bam_flag_tlen, sk_count_add, sk_on_target_add
{
	int64_t chunk = (int64_t)budget_rows;
	if (chunk > n) chunk = n;
	return chunk;
}
static int64_t table_fragments(uint64_t budget_rows, int64_t n)
{
	int64_t chunk = (int64_t)budget_rows;
	if (chunk > n) chunk = (n + 7) & ~(int64_t)7;
	return chunk;
}
static int64_t table_sequence(uint64_t budget_bytes, size_t per_row, int64_t n)
{
	int64_t chunk = (int64_t)(budget_bytes / per_row);
	if (chunk < 1) chunk = 1;
	if (chunk > n) chunk = n;
	return chunk;
}
static int64_t table_census(uint64_t budget_bytes, int bc_stride, int64_t n)
{
	int64_t chunk = (int64_t)(budget_bytes / (size_t)(bc_stride + 4));
	if (chunk < 1) chunk = 1;          // (a budget below one row — SK_HOST_CHUNK_LOG2=6 at bc_stride 61..64 — was 0 rows by hand, a loop that never ended)
	if (chunk > n) chunk = n;
	return chunk;
}

// ---- the entry points -------------------------------------------------------------------------------------------------------------
static void test_fused()
{
	// mates: 0, 1, 2; each active mate with or without out_seq, lowest_k and len; the barcode phase absent, alone, with lowest_diff
	// alone and with its three detail columns (2 mates, everything: 15 regions)
	for (int n_mates = 0; n_mates <= 2; n_mates++)
		for (int f = 0; f < (n_mates ? 8 : 1); f++)
			for (int bc = 0; bc < 4; bc++) {
				const bool out = f & 1, lk = f & 2, len = f & 4, mate = n_mates > 0 && (out || lk);
				if (!mate && !bc) continue;                                  // nothing to do: refused before any list is made
				for (int stride : kStrides) {
					const int bc_stride = (stride - 1) % 200 + 1;
					for (uint64_t budget : budgets(kPipeChunkBytes))
						for (int64_t n : kNs) {
							snprintf(g_what, sizeof g_what, "fused mates %d flags %d bc %d stride %d budget %llu n %lld", n_mates, f, bc, stride, (unsigned long long)budget, (long long)n);
							Call c;
							size_t per_row = 0, regions = 0;
							for (int m = 0; m < n_mates && mate; m++) {
								c.add(stride, kIn); per_row += stride; regions++;
								if (out) { c.add(stride, kIn); c.add(stride, kOut); per_row += 2 * (size_t)stride; regions += 2; }
								if (len) { c.add(2, kIn); per_row += 2; regions++; }
								if (lk) { c.add(2, kOut); per_row += 2; regions++; }
							}
							if (bc) {
								c.add(bc_stride, kIn); c.add(4, kOut); c.add(1, kOut, bc >= 2); c.add(2, kOut, bc == 3); c.add(2, kOut, bc == 3);
								per_row += (size_t)bc_stride + 4 + 1 + 2 + 2;
								regions += 2 + (bc >= 2) + 2 * (bc == 3);
							}
							CHECK(c.st.per_row() == per_row);
							CHECK(n_mates < 2 || f != 7 || bc != 3 || regions == 15);
							const int64_t chunk = c.st.rows_for_bytes(budget, 64, n);
							size_t half = 0;
							for (int m = 0; m < n_mates && mate; m++) half += up(chunk * stride) * (out ? 3 : 1) + up(chunk * 2) * ((len ? 1 : 0) + (lk ? 1 : 0));
							if (bc) half += up(chunk * bc_stride) + up(chunk * 4) + (bc >= 2 ? up(chunk) : 0) + (bc == 3 ? 2 * up(chunk * 2) : 0);
							check(c, chunk, table_fused(budget, per_row, n), 64, 64, n, half, 0, 2, 64);
						}
				}
			}
}

static void test_mask()
{
	for (int stride : kStrides)
		for (uint64_t budget : budgets((size_t)16 << 20))
			for (int64_t n : kNs) {
				const int64_t total = n * stride;                            // the whole matrix as one byte stream
				snprintf(g_what, sizeof g_what, "mask stride %d budget %llu n %lld", stride, (unsigned long long)budget, (long long)n);
				Call c;
				c.add(1, kIn); c.add(1, kIn); c.add(1, kOut);
				const int64_t chunk = rows_per_chunk(budget, 16, total);
				check(c, chunk, table_mask(budget, total), 16, 16, total, 3 * up(chunk), 0, 2, 16);
			}
}

static void test_bam_columns()
{
	for (int64_t n : kNs) {
		for (uint64_t budget : budgets((size_t)4 << 20)) {
			for (int hist = 0; hist < 2; hist++) {                           // counters only: tid, mtid and tlen are carved and not copied
				snprintf(g_what, sizeof g_what, "flag_tlen hist %d budget %llu n %lld", hist, (unsigned long long)budget, (long long)n);
				Call c;
				c.add(2, kIn); c.add(4, hist ? kIn : kDev); c.add(4, hist ? kIn : kDev); c.add(4, hist ? kIn : kDev);
				const size_t nout = 4 + (hist ? 5000 + 1 : 0);
				const int64_t chunk = rows_per_chunk(budget, 1, n);
				check(c, chunk, table_rows(budget, n), 1, 1, n, up(chunk * 2) + 3 * up(chunk * 4), nout * 8, 2, 1);
				CHECK(c.st.total() == 2 * c.st.half() + up(nout * 8));
			}
			{
				snprintf(g_what, sizeof g_what, "fragments budget %llu n %lld", (unsigned long long)budget, (long long)n);
				Call c;
				c.add(2, kIn); c.add(4, kIn); c.add(4, kIn); c.add(4, kIn); c.add_bits(1, kOut, true);
				const int64_t chunk = rows_per_chunk(budget, 8, n);
				check(c, chunk, table_fragments(budget, n), 8, 8, n, up(chunk * 2) + 3 * up(chunk * 4) + up(chunk / 8), 8, 2, 8);
				CHECK(c.st.total() == 2 * c.st.half() + 256);
			}
		}
		for (uint64_t budget : budgets((size_t)2 << 20)) {
			for (int single_end = 0; single_end < 2; single_end++) {         // the other mode's columns are carved and not copied
				snprintf(g_what, sizeof g_what, "count single_end %d budget %llu n %lld", single_end, (unsigned long long)budget, (long long)n);
				Call c;
				const Dir pair = single_end ? kDev : kIn, single = single_end ? kIn : kDev;
				c.add(2, kIn); c.add(1, kIn); c.add(4, kIn); c.add(4, pair); c.add(4, kIn); c.add(4, pair); c.add(4, pair); c.add(4, single);
				const int64_t chunk = rows_per_chunk(budget, 1, n);
				check(c, chunk, table_rows(budget, n), 1, 1, n, up(chunk * 2) + up(chunk) + 6 * up(chunk * 4), 0, 2, 1);
			}
			snprintf(g_what, sizeof g_what, "on_target budget %llu n %lld", (unsigned long long)budget, (long long)n);
			Call c;
			c.add(2, kIn);
			for (int k = 0; k < 6; k++) c.add(4, kIn);
			const int64_t chunk = rows_per_chunk(budget, 1, n);
			check(c, chunk, table_rows(budget, n), 1, 1, n, up(chunk * 2) + 6 * up(chunk * 4), 0, 2, 1);
		}
	}
}

static void test_sequence()
{
	for (int stride : kStrides)
		for (int with_len = 0; with_len < 2; with_len++)
			for (uint64_t budget : budgets(kPipeChunkBytes))
				for (int64_t n : kNs) {
					const int seq4_stride = (stride + 7) / 8 * 4;
					snprintf(g_what, sizeof g_what, "sequence stride %d len %d budget %llu n %lld", stride, with_len, (unsigned long long)budget, (long long)n);
					Call c;
					c.add(seq4_stride, kIn); c.add(stride, kIn); c.add(stride, kOut); c.add(2, kIn, with_len); c.add(2, kIn);
					const size_t per_row = (size_t)seq4_stride + 2 * (size_t)stride + 4;
					CHECK(c.st.per_row() == per_row);
					const int64_t chunk = c.st.rows_for_bytes(budget, 1, n);
					check(c, chunk, table_sequence(budget, per_row, n), 1, 1, n, up(chunk * seq4_stride) + 2 * up(chunk * stride) + (1 + with_len) * up(chunk * 2), 0, 2, 1);
				}
}

static void test_census()
{
	for (int bc_stride : {1, 17, 64})                                       // (the entry point takes 1..64)
		for (int with_assign = 0; with_assign < 2; with_assign++)
			for (uint64_t budget : budgets((size_t)64 << 20))
				for (int64_t n : kNs) {
					snprintf(g_what, sizeof g_what, "census bc_stride %d assign %d budget %llu n %lld", bc_stride, with_assign, (unsigned long long)budget, (long long)n);
					Call c;
					c.add(bc_stride, kIn); c.add(4, kIn, with_assign);
					CHECK(c.st.per_row() == (size_t)bc_stride + 4);
					const int64_t chunk = c.st.rows_for_bytes(budget, 1, n);
					check(c, chunk, table_census(budget, bc_stride, n), 1, 1, n, up(chunk * bc_stride) + (with_assign ? up(chunk * 4) : 0), 0, 1, 1);   // one stream, one half
					CHECK(c.st.total() == c.st.half());
				}
}

int main()
{
	test_fused();
	test_mask();
	test_bam_columns();
	test_sequence();
	test_census();
	printf("ok: %ld checks\n", g_checks);
	return 0;
}
