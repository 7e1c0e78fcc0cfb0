// sk_censusplan.h — the launch decisions of the barcode census (sk_census.hip), each stated once: how many tiles a wave step takes,
// which census_kernel<R, NW, SPILL> runs, the wave's LDS slot and what the rest of the workgroup's LDS buys the front table, the grid,
// whether a launch writes records (the partition path) and how large a (workgroup, bucket) region is, how large a bite of the input a
// launch takes and when the HBM table grows instead.  Pure arithmetic on plain facts (Knobs: the SK_CENSUS_* variables as read): no
// HIP, no heap, no getenv.  sk_census.hip reads the environment (census_knobs), asks here, reserves and launches; the kernels' side of
// the LDS layout is tied to this one by static_asserts there.  tests/cpp/censusplan_test.cpp holds every rule to expectations written
// out by hand, on the CPU.
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "sk_tileplan.h"      // kLdsPerCu

namespace sk {

// ---- what host and device share ----------------------------------------------------------------------------------------------------
// The partition path (large launches): keys the front tables had no room for leave the front kernel as 16-byte records,
// partitioned by the region of the HBM table their slot lies in (kSpillBuckets regions) INSIDE that kernel: a record draws
// its place in the (workgroup, bucket) region of the record array from the workgroup's cursor of that bucket (an LDS add with
// return) and goes there with one 16-byte store.  A wave's 64 records go to 64 different lines; the lines of the
// workgroups' open regions (256 x 128 x 128 B = 4 MiB) stay in L2 until they are full.  The records are combined per bucket in
// LDS before they touch the table (census_add).  (Through round 4 the records were written as they came, then
// counted, scanned and moved to 1 024 buckets by two more kernels: every record crossed HBM four times — 62 + 7 of a noisy
// launch's 314 us of kernels and two of its five kernel boundaries.  A first form of this round staged the records per
// bucket in each wave's LDS and flushed whole pieces: the stages took the front table's room and the flushes its time.)
constexpr int kSpillBucketsLog2 = 8;
constexpr int kSpillBuckets = 1 << kSpillBucketsLog2;
constexpr int kSpillMaxLen = 24;         // 24 characters = 96 bits; the key's fourth dword is then the marker alone
constexpr int kSpillMaxGrid = 1024;      // workgroups of the front kernel the combine pass can address

// A record's fourth dword: the row index within the launch (a launch is at most 2^25 rows: kCensusChunk) and how many rows
// the record stands for — digit d = 1..31 at level v = 0..3, d << (5 v) rows: a row the front tables had no room for is
// (d, v) = (1, 0); a front-table key counted c times leaves the workgroup as the non-zero base-32 digits of c.
constexpr int kRecRowBits = 25;

constexpr uint64_t kInitialSlots = 1ull << 26;   // 2 GiB of the 288: one launch may then take 32 M rows (SK_CENSUS_SLOTS_LOG2 overrides; tests use it)
constexpr uint32_t kLogCap = 1u << 16;           // claim-log entries per region: 256 x 65 536 slots = 64 MiB (SK_CENSUS_LOG_CAP_LOG2 overrides; tests shrink it)
constexpr int64_t kCensusChunk = 1 << 25;   // most rows per launch; the table is grown between launches so that it is never
constexpr int64_t kCensusMinChunk = 1 << 22;   // more than half full even if every row of the next launch is a new key

constexpr int kCensusWaves = 16;          // waves per workgroup (one per CU): they share the front table
constexpr int kCensusMaxStride = 64;      // a row's span is at most 9 dwords (census_load_rows)
constexpr int kCensusMaxSub = 2;          // 64-row tiles per wave and step (three and four timed the same and needed scratch for the longest strings)
constexpr int kCensusStepBytes = 5120;    // most bytes per wave and step before the cap on R (censusplan::tiles_per_step)
constexpr int kCensusQueue = 128;         // flush queue entries (16 B key + 4 B row): fewer than 64 left over + one tile's 64

constexpr int64_t kSpillMinRows = 1 << 19;      // smaller launches insert directly: the partition path is four more kernels.  Measured (tools/census_small.py, round 4,
                                                // insert-in-place / partition, noisy run): 250 k rows 58 / 68 us, 1 M 100 / 80, 4 M 187 / 110, 8 M 308 / 149; rows that
                                                // are all sheet barcodes: 250 k 40 / 47, 1 M 65 / 55, 4 M 84 / 68 (round 3's crossover was at 8 M rows)

namespace censusplan {

// The SK_CENSUS_* variables as sk_census.hip: census_knobs() found them, each already held to the range the code accepts (set_knob):
// a value outside its range leaves the default.
struct Knobs {
	bool tiles_set = false;                  // SK_CENSUS_TILES is in the environment, whatever its value (tiles_for_launch) ...
	int tiles = 0;                           // ... and its value when that is at least 1 (at most R: tiles_per_step); experiments
	int front_entries = 0;                   // SK_CENSUS_FRONT_ENTRIES & ~63 when at least 64 (at most what the layout leaves: lds_layout): tests shrink the
	                                         // front table so that small inputs walk "no room in either place"
	int wgs_per_cu = 1;                      // SK_CENSUS_WGS, 1..4 (experiments)
	int direct_pct = 50;                     // SK_CENSUS_SPILL_MAX_PCT, 0..100: more spilled rows than this share of a launch are inserted directly
	int64_t spill_min_rows = kSpillMinRows;  // SK_CENSUS_SPILL_MIN_ROWS_LOG2, 6..30: tests lower it
	int direct_split = 8;                    // SK_CENSUS_DIRECT_SPLIT, 1..64: workgroups per region of census_direct_kernel (experiments)
	bool merge_records = true;               // SK_CENSUS_MERGE_RECORDS=0: the front kernel inserts its tables itself, as small launches do (A/B, tests)
	int spill_mode = -1;                     // SK_CENSUS_SPILL=0/1: never / always (tests, experiments)
	int64_t chunk = kCensusChunk;            // SK_CENSUS_CHUNK_LOG2, 6..kRecRowBits (a record's row index has kRecRowBits bits) and
	int64_t min_chunk = kCensusMinChunk;     // SK_CENSUS_MIN_CHUNK_LOG2, 6..30: tests shrink the launches to walk the grow / smaller-bite decisions
	bool trust_slots = false;                // SK_CENSUS_TRUST_SLOTS: experiments with a table that is known to be large enough
	bool long_way_only = false;              // SK_CENSUS_LONG_WAY_ONLY=1 (CensusArgs::long_way_only)
	// census_create:
	uint64_t initial_slots = kInitialSlots;  // SK_CENSUS_SLOTS_LOG2, 10..32
	uint32_t log_cap = kLogCap;              // SK_CENSUS_LOG_CAP_LOG2, 0..20, or -1: no log, every reset clears the whole table
};

// one variable: `name` is what follows "SK_CENSUS_" (len characters of it), `value` the text behind the '='
inline void set_knob(Knobs &k, const char *name, size_t len, const char *value)
{
	auto is = [&](const char *n) { return strlen(n) == len && memcmp(n, name, len) == 0; };
	const int v = atoi(value);
	if (is("TILES")) { k.tiles_set = true; if (v >= 1) k.tiles = v; }
	else if (is("FRONT_ENTRIES")) { if ((v & ~63) >= 64) k.front_entries = v & ~63; }
	else if (is("WGS")) { if (v >= 1 && v <= 4) k.wgs_per_cu = v; }
	else if (is("SPILL_MAX_PCT")) { if (v >= 0 && v <= 100) k.direct_pct = v; }
	else if (is("SPILL_MIN_ROWS_LOG2")) { if (v >= 6 && v <= 30) k.spill_min_rows = (int64_t)1 << v; }
	else if (is("DIRECT_SPLIT")) { if (v >= 1 && v <= 64) k.direct_split = v; }
	else if (is("MERGE_RECORDS")) k.merge_records = v != 0;
	else if (is("SPILL")) k.spill_mode = v != 0;
	else if (is("CHUNK_LOG2")) { if (v >= 6 && v <= kRecRowBits) k.chunk = (int64_t)1 << v; }
	else if (is("MIN_CHUNK_LOG2")) { if (v >= 6 && v <= 30) k.min_chunk = (int64_t)1 << v; }
	else if (is("TRUST_SLOTS")) k.trust_slots = true;
	else if (is("LONG_WAY_ONLY")) k.long_way_only = v != 0;
	else if (is("SLOTS_LOG2")) { if (v >= 10 && v <= 32) k.initial_slots = 1ull << v; }
	else if (is("LOG_CAP_LOG2")) { if (v >= 0 && v <= 20) k.log_cap = 1u << v; else if (v == -1) k.log_cap = 0u; }
}

// ---- which kernel ------------------------------------------------------------------------------------------------------------------
// 64-row tiles per wave and step: what kCensusStepBytes holds, two at most (more bought nothing — R = 1 ... 4 timed the same within
// the boxes' noise in round 4 — and a tile's 64 queue entries are 43 front-table entries of a 17-byte sheet).  0: the pitch is refused.
inline int tiles_per_step(const Knobs &k, int bc_stride)
{
	if (bc_stride < 1 || bc_stride > kCensusMaxStride) return 0;
	int R = kCensusStepBytes / (64 * bc_stride);
	R = R < 1 ? 1 : (R > kCensusMaxSub ? kCensusMaxSub : R);
	if (k.tiles >= 1 && k.tiles <= R) R = k.tiles;
	return R;
}
// the kernels' row widths: barcodes of at most 8, 20, 31 characters are 2, 5, 8 dwords
inline int nw_class(int L) { return L <= 8 ? 0 : (L <= 20 ? 1 : 2); }
inline int nw_dwords(int L) { return L <= 8 ? 2 : (L <= 20 ? 5 : 8); }
constexpr int class_dwords(int nw_class) { return nw_class == 0 ? 2 : (nw_class == 1 ? 5 : 8); }
// One tile per step for the launches that write records: the step's queue is a third smaller, and what it gives back goes
// to the front table (2 432 -> 3 136 entries for 17-byte rows) — the table's size is worth more than the second tile (32 M
// noisy rows 0.320 -> 0.312 ms, clean 0.245 -> 0.231; with 1 024 entries 0.34-0.41, with 512 0.53; tools/ab/census_env_ab.py).
// SK_CENSUS_TILES in the environment, with whatever value, switches the rule off.
inline int tiles_for_launch(const Knobs &k, int R, bool spill, int nw_class) { return (spill && nw_class >= 1 && !k.tiles_set) ? 1 : R; }
// the index into census_variant: R tiles per step x row width x spill
constexpr int kVariants = kCensusMaxSub * 3 * 2;
inline int variant(int Rk, int nw_class, bool spill) { return ((Rk - 1) * 3 + nw_class) * 2 + (spill ? 1 : 0); }

// ---- the workgroup's LDS -----------------------------------------------------------------------------------------------------------
// [front table][kCensusWaves wave slots][tail]; the kernel finds the slots and the tail from tile_slot and front_entries.
// A front-table entry: chunks B and A (and C for strings of more than 20 bytes) of 16 bytes and the u32 count (FrontShape<NW>::kEntryBytes)
constexpr int front_entry_bytes(int nw_class) { return (nw_class == 2 ? 3 : 2) * 16 + 4; }
// a wave's queue of rows that take the long way: 64 left over + the step's R x 64 (census_kernel's kQueueCap)
constexpr int queue_cap(int R) { return 64 + R * 64; }
// ... each entry its NW dwords and its row's index
constexpr int queue_bytes(int R, int nw) { return queue_cap(R) * (4 * nw + 4); }
// the flush queue of the launches that insert by themselves lies behind the row indices and the first 64 queue entries (dead once the
// passes ran): kCensusQueue keys of 16 bytes, then their rows; where it ends
constexpr int flush_end(int R, int nw) { return ((queue_cap(R) * 4 + 64 * 4 * nw + 15) & ~15) + kCensusQueue * (16 + 4); }
constexpr int tile_slot_bytes(int R, int nw, bool spill)
{
	return ((!spill && queue_bytes(R, nw) < flush_end(R, nw) ? flush_end(R, nw) : queue_bytes(R, nw)) + 15) & ~15;
}
// behind the slots: 64 bytes kept free, then the workgroup's kSpillBuckets + 1 cursors into the bucket regions and its step counter
constexpr int kTailBytes = 64 + (kSpillBuckets + 4) * 4;

struct Layout {
	int tile_slot;       // bytes per wave
	int front_entries;   // a multiple of 64
	int bytes;           // the launch's dynamic LDS
};
// the front table takes what is left of the CU's LDS (less 16 bytes: its arrays end on a 16-byte boundary), in whole 64 entries
inline Layout lds_layout(const Knobs &k, int Rk, int nw_class, bool spill)
{
	Layout l;
	l.tile_slot = tile_slot_bytes(Rk, class_dwords(nw_class), spill);
	const int rest = kCensusWaves * l.tile_slot + kTailBytes;
	const int eb = front_entry_bytes(nw_class);
	l.front_entries = ((kLdsPerCu - 16 - rest) / eb) & ~63;
	if (k.front_entries >= 64 && k.front_entries <= l.front_entries) l.front_entries = k.front_entries;
	l.bytes = rest + ((l.front_entries * eb + 15) & ~15);
	return l;
}

// ---- bites of the input ------------------------------------------------------------------------------------------------------------
// most rows per launch: a launch's matrix stays below 2 GiB (less 16 MiB), the front kernel addresses it through one descriptor with
// 32-bit offsets; and a record's row index has kRecRowBits bits (the knob's range)
inline int64_t chunk_rows(const Knobs &k, int bc_stride)
{
	const int64_t max_rows = ((((int64_t)1 << 31) - (1 << 24)) / bc_stride) & ~(int64_t)63;
	return k.chunk > max_rows ? max_rows : k.chunk;
}
// the least rows worth a launch of their own (launches have a fixed cost)
inline int64_t min_chunk_rows(const Knobs &k, int64_t chunk) { return k.min_chunk > chunk ? chunk : k.min_chunk; }

// The launch must not be able to fill the table beyond one half even if every row is a new key.  When the bound on the key count
// says it could, the exact count is fetched (census_stats) ...
inline bool bite_needs_count(uint64_t distinct_bound, int64_t nr, uint64_t slots, const Knobs &k)
{
	return 2 * (distinct_bound + (uint64_t)nr) > slots && !k.trust_slots;
}
// ... then either a smaller bite fits the table as it is — at least min_chunk rows, or all that was asked for — or there is no room
// worth a launch: the table grows for the whole bite (census_reserve).  is_last: the bite asked for reaches the end of the input.  A
// bite that does not (a smaller one never does) is whole 64 rows from 64 on: later launches start on a 16-byte boundary of the matrix.
struct Bite { int64_t nr; bool grow; };
inline Bite bite_after_count(uint64_t distinct, uint64_t slots, int64_t nr, int64_t min_chunk, bool is_last)
{
	Bite b{nr, false};
	const int64_t room = (int64_t)(slots / 2) - (int64_t)distinct;
	const int64_t least = nr < min_chunk ? nr : min_chunk;
	if (room >= least) b.nr = nr < room ? nr : room;
	else b.grow = true;
	if ((!is_last || b.nr < nr) && b.nr >= 64) b.nr &= ~(int64_t)63;
	return b;
}
// the table's size once it holds `need` slots: doubled until it does.  0: refused — the hash is 32 bits wide (and this would be a
// 128 GiB table)
inline uint64_t grown_slots(uint64_t slots, uint64_t need)
{
	while (slots < need) slots <<= 1;
	return slots > (1ull << 32) ? 0 : slots;
}

// ---- the launch --------------------------------------------------------------------------------------------------------------------
// does the launch write records (the partition path)?  Their three key dwords hold kSpillMaxLen characters
inline bool wants_spill(const Knobs &k, int L, int64_t nr) { return L <= kSpillMaxLen && (k.spill_mode < 0 ? nr >= k.spill_min_rows : k.spill_mode != 0); }
// one workgroup per CU, and no more than have a step of all their waves
inline int grid(int64_t nr, int Rk, int n_cu, const Knobs &k)
{
	const int64_t groups = (nr + (int64_t)64 * Rk * kCensusWaves - 1) / ((int64_t)64 * Rk * kCensusWaves);
	const int g = n_cu * k.wgs_per_cu;
	return g > groups ? (int)groups : g;
}
// a (workgroup, bucket) region: twice the workgroup's share of a launch in which EVERY row is spilled and spreads evenly, and
// room for its front table's records; a piece that finds its region full is inserted by the front kernel itself.  !ok: the combine
// pass cannot address that many workgroups, or a workgroup's regions are beyond its record descriptor (2^27 records = 2 GiB)
struct Region { uint32_t cap; bool ok; };
inline Region spill_region(int64_t nr, int Rk, int grid)
{
	const int64_t nsteps = (nr + (int64_t)64 * Rk - 1) / ((int64_t)64 * Rk);
	const int64_t per_wave = (nsteps + (int64_t)grid * kCensusWaves - 1) / ((int64_t)grid * kCensusWaves);
	const int64_t wg_rows = per_wave * kCensusWaves * Rk * 64;
	const int64_t cap = (((wg_rows + kSpillBuckets - 1) / kSpillBuckets) * 2 + 256 + 7) & ~(int64_t)7;
	return Region{(uint32_t)cap, grid <= kSpillMaxGrid && cap * kSpillBuckets < ((int64_t)1 << 27)};
}
// more records than this in the launch: they are inserted as they lie (census_direct_kernel), not combined
inline uint32_t direct_above(int64_t nr, const Knobs &k) { return (uint32_t)((uint64_t)nr * (uint64_t)k.direct_pct / 100); }
inline int combine_grid(int n_cu) { return 2 * n_cu; }
inline int direct_grid(int grid, const Knobs &k) { return grid * k.direct_split; }

}  // namespace censusplan
}  // namespace sk
