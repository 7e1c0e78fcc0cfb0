// censusplan_test.cpp — sk_censusplan.h (the launch decisions of the barcode census) on the host, built with the address and
// undefined-behaviour sanitizers (tests/test_censusplan_cpu.py).  Every expectation below is written out by hand from the rules as
// census_add and census_create applied them before the header existed, and from the LDS layout as census_kernel reads it: tiles, slot
// bytes, front-table entries, grids and capacities are literal numbers here, never the header asked a second time.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <initializer_list>
#include <utility>

#include "sk_censusplan.h"

using namespace sk;
using namespace sk::censusplan;

static long g_checks = 0, g_cases = 0;
static char g_what[256] = "";                    // the case at hand, for a failing CHECK ...
static long g_rows = 0, g_cus = 0, g_refused = 0;  // ... and where the launch sweep is within it
#define CHECK(cond)                                                                                                     \
	do {                                                                                                                \
		g_checks++;                                                                                                     \
		if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed [%s] (rows %ld cus %ld refused %ld)\n", __FILE__, __LINE__, #cond, g_what, g_rows, g_cus, g_refused); exit(1); }   \
	} while (0)
#define CASE(...) do { g_cases++; snprintf(g_what, sizeof g_what, __VA_ARGS__); } while (0)

// the knobs of an environment that holds SK_CENSUS_<name>=<value> for each pair
typedef std::pair<const char *, const char *> Var;
static Knobs knobs(std::initializer_list<Var> env)
{
	Knobs k;
	for (const Var &v : env) set_knob(k, v.first, strlen(v.first), v.second);
	return k;
}
static Knobs knob(const char *name, const char *value) { return knobs({{name, value}}); }

// ---- the variables and their ranges ------------------------------------------------------------------------------------------------
static void test_knobs()
{
	CASE("defaults");
	const Knobs d;
	CHECK(!d.tiles_set && d.tiles == 0 && d.front_entries == 0 && d.wgs_per_cu == 1 && d.direct_pct == 50 && d.spill_min_rows == 524288);
	CHECK(d.direct_split == 8 && d.merge_records && d.spill_mode == -1 && d.chunk == 33554432 && d.min_chunk == 4194304);
	CHECK(!d.trust_slots && !d.long_way_only && d.initial_slots == 67108864ull && d.log_cap == 65536u);

	CASE("TILES");
	CHECK(knob("TILES", "1").tiles_set && knob("TILES", "1").tiles == 1);
	CHECK(knob("TILES", "2").tiles == 2 && knob("TILES", "7").tiles == 7);      // (held to R where R is known: tiles_per_step)
	CHECK(knob("TILES", "0").tiles_set && knob("TILES", "0").tiles == 0);
	CHECK(knob("TILES", "-1").tiles_set && knob("TILES", "-1").tiles == 0);
	CHECK(knob("TILES", "").tiles_set && knob("TILES", "two").tiles_set && knob("TILES", "two").tiles == 0);
	CHECK(!knob("TILESX", "1").tiles_set && !knob("TILE", "1").tiles_set);      // whole names only

	CASE("FRONT_ENTRIES");
	CHECK(knob("FRONT_ENTRIES", "63").front_entries == 0 && knob("FRONT_ENTRIES", "64").front_entries == 64);
	CHECK(knob("FRONT_ENTRIES", "127").front_entries == 64 && knob("FRONT_ENTRIES", "128").front_entries == 128);
	CHECK(knob("FRONT_ENTRIES", "-1").front_entries == 0 && knob("FRONT_ENTRIES", "0").front_entries == 0);
	CHECK(knob("FRONT_ENTRIES", "100000").front_entries == 99968);               // (too many for any layout: lds_layout)

	CASE("WGS");
	CHECK(knob("WGS", "0").wgs_per_cu == 1 && knob("WGS", "1").wgs_per_cu == 1 && knob("WGS", "2").wgs_per_cu == 2);
	CHECK(knob("WGS", "4").wgs_per_cu == 4 && knob("WGS", "5").wgs_per_cu == 1);

	CASE("SPILL_MAX_PCT");
	CHECK(knob("SPILL_MAX_PCT", "-1").direct_pct == 50 && knob("SPILL_MAX_PCT", "0").direct_pct == 0);
	CHECK(knob("SPILL_MAX_PCT", "100").direct_pct == 100 && knob("SPILL_MAX_PCT", "101").direct_pct == 50);

	CASE("SPILL_MIN_ROWS_LOG2");
	CHECK(knob("SPILL_MIN_ROWS_LOG2", "5").spill_min_rows == 524288 && knob("SPILL_MIN_ROWS_LOG2", "6").spill_min_rows == 64);
	CHECK(knob("SPILL_MIN_ROWS_LOG2", "30").spill_min_rows == 1073741824 && knob("SPILL_MIN_ROWS_LOG2", "31").spill_min_rows == 524288);

	CASE("DIRECT_SPLIT");
	CHECK(knob("DIRECT_SPLIT", "0").direct_split == 8 && knob("DIRECT_SPLIT", "1").direct_split == 1);
	CHECK(knob("DIRECT_SPLIT", "64").direct_split == 64 && knob("DIRECT_SPLIT", "65").direct_split == 8);

	CASE("MERGE_RECORDS, SPILL, LONG_WAY_ONLY, TRUST_SLOTS");
	CHECK(!knob("MERGE_RECORDS", "0").merge_records && knob("MERGE_RECORDS", "1").merge_records && !knob("MERGE_RECORDS", "").merge_records);
	CHECK(knob("SPILL", "0").spill_mode == 0 && knob("SPILL", "1").spill_mode == 1 && knob("SPILL", "5").spill_mode == 1 && knob("SPILL", "").spill_mode == 0);
	CHECK(knob("SPILL_MAX", "1").spill_mode == -1 && knob("SPILL_MAX_PCT", "1").spill_mode == -1);
	CHECK(!knob("LONG_WAY_ONLY", "0").long_way_only && knob("LONG_WAY_ONLY", "1").long_way_only && !knob("LONG_WAY_ONLY", "yes").long_way_only);
	CHECK(knob("TRUST_SLOTS", "").trust_slots && knob("TRUST_SLOTS", "0").trust_slots);

	CASE("CHUNK_LOG2, MIN_CHUNK_LOG2");
	CHECK(knob("CHUNK_LOG2", "5").chunk == 33554432 && knob("CHUNK_LOG2", "6").chunk == 64);
	CHECK(knob("CHUNK_LOG2", "25").chunk == 33554432 && knob("CHUNK_LOG2", "24").chunk == 16777216 && knob("CHUNK_LOG2", "26").chunk == 33554432);
	CHECK(knob("MIN_CHUNK_LOG2", "5").min_chunk == 4194304 && knob("MIN_CHUNK_LOG2", "6").min_chunk == 64);
	CHECK(knob("MIN_CHUNK_LOG2", "30").min_chunk == 1073741824 && knob("MIN_CHUNK_LOG2", "31").min_chunk == 4194304);
	CHECK(knob("CHUNK_LOG2", "6").min_chunk == 4194304 && knob("MIN_CHUNK_LOG2", "6").chunk == 33554432);

	CASE("SLOTS_LOG2, LOG_CAP_LOG2");
	CHECK(knob("SLOTS_LOG2", "9").initial_slots == 67108864ull && knob("SLOTS_LOG2", "10").initial_slots == 1024ull);
	CHECK(knob("SLOTS_LOG2", "32").initial_slots == 4294967296ull && knob("SLOTS_LOG2", "33").initial_slots == 67108864ull);
	CHECK(knob("LOG_CAP_LOG2", "-2").log_cap == 65536u && knob("LOG_CAP_LOG2", "-1").log_cap == 0u && knob("LOG_CAP_LOG2", "0").log_cap == 1u);
	CHECK(knob("LOG_CAP_LOG2", "20").log_cap == 1048576u && knob("LOG_CAP_LOG2", "21").log_cap == 65536u);

	CASE("several variables, any order");
	const Knobs k = knobs({{"SPILL_MAX_PCT", "0"}, {"SPILL", "1"}, {"FRONT_ENTRIES", "64"}, {"MERGE_RECORDS", "0"}});
	CHECK(k.direct_pct == 0 && k.spill_mode == 1 && k.front_entries == 64 && !k.merge_records && k.direct_split == 8);
}

// ---- tiles, row widths, the instantiation -----------------------------------------------------------------------------------------
static void test_kernel_choice()
{
	const Knobs d;
	CASE("tiles per step: 5120 bytes per wave and step, two tiles at most");
	CHECK(tiles_per_step(d, 1) == 2 && tiles_per_step(d, 8) == 2 && tiles_per_step(d, 17) == 2);
	CHECK(tiles_per_step(d, 40) == 2 && tiles_per_step(d, 41) == 1);             // 2 x 64 x 40 = 5120; 2 x 64 x 41 = 5248
	CHECK(tiles_per_step(d, 64) == 1 && tiles_per_step(d, 65) == 0 && tiles_per_step(d, 0) == 0);
	CASE("SK_CENSUS_TILES: 1..R");
	CHECK(tiles_per_step(knob("TILES", "1"), 8) == 1 && tiles_per_step(knob("TILES", "2"), 8) == 2 && tiles_per_step(knob("TILES", "3"), 8) == 2);
	CHECK(tiles_per_step(knob("TILES", "2"), 41) == 1 && tiles_per_step(knob("TILES", "1"), 41) == 1 && tiles_per_step(knob("TILES", "0"), 8) == 2);
	CHECK(tiles_per_step(knob("TILES", "1"), 65) == 0);

	CASE("one tile per step for launches that write records of rows wider than 8 bytes");
	CHECK(tiles_for_launch(d, 2, true, 0) == 2 && tiles_for_launch(d, 2, true, 1) == 1 && tiles_for_launch(d, 2, true, 2) == 1);
	CHECK(tiles_for_launch(d, 2, false, 1) == 2 && tiles_for_launch(d, 2, false, 2) == 2 && tiles_for_launch(d, 1, true, 1) == 1 && tiles_for_launch(d, 1, false, 0) == 1);
	CASE("... unless SK_CENSUS_TILES is in the environment, usable or not");
	CHECK(tiles_for_launch(knob("TILES", "2"), 2, true, 1) == 2 && tiles_for_launch(knob("TILES", "0"), 2, true, 1) == 2);
	CHECK(tiles_for_launch(knob("TILES", ""), 2, true, 2) == 2 && tiles_for_launch(knob("TILES", "9"), 2, true, 1) == 2);
	CHECK(tiles_for_launch(knob("TILES", "1"), tiles_per_step(knob("TILES", "1"), 17), true, 1) == 1);

	CASE("row widths: 8 / 20 / 31 characters in 2 / 5 / 8 dwords");
	CHECK(nw_class(1) == 0 && nw_class(8) == 0 && nw_class(9) == 1 && nw_class(20) == 1 && nw_class(21) == 2 && nw_class(24) == 2 && nw_class(25) == 2 && nw_class(31) == 2);
	CHECK(nw_dwords(1) == 2 && nw_dwords(8) == 2 && nw_dwords(9) == 5 && nw_dwords(20) == 5 && nw_dwords(21) == 8 && nw_dwords(31) == 8);
	CHECK(class_dwords(0) == 2 && class_dwords(1) == 5 && class_dwords(2) == 8);
	CHECK(front_entry_bytes(0) == 36 && front_entry_bytes(1) == 36 && front_entry_bytes(2) == 52);

	CASE("census_variant's order: <1,2,f> <1,2,t> <1,5,f> <1,5,t> <1,8,f> <1,8,t> <2,2,f> ... <2,8,t>");
	CHECK(kVariants == 12);
	CHECK(variant(1, 0, false) == 0 && variant(1, 0, true) == 1 && variant(1, 1, false) == 2 && variant(1, 1, true) == 3 && variant(1, 2, false) == 4 && variant(1, 2, true) == 5);
	CHECK(variant(2, 0, false) == 6 && variant(2, 0, true) == 7 && variant(2, 1, false) == 8 && variant(2, 1, true) == 9 && variant(2, 2, false) == 10 && variant(2, 2, true) == 11);
}

// ---- one launch from end to end: the anchors ---------------------------------------------------------------------------------------
struct Launch { int R, Rk, tile_slot, front_entries, lds, grid, variant; bool spill; uint32_t cap; bool region_ok; };
// what census_add asks of the plan for a launch of nr rows, in its order
static Launch launch_of(const Knobs &k, int L, int bc_stride, int64_t nr, int n_cu, bool allocator_refuses = false)
{
	Launch x{};
	x.R = tiles_per_step(k, bc_stride);
	const int nwc = nw_class(L);
	x.spill = wants_spill(k, L, nr);
	x.Rk = tiles_for_launch(k, x.R, x.spill, nwc);
	x.grid = grid(nr, x.Rk, n_cu, k);
	if (x.spill) {
		const Region rg = spill_region(nr, x.Rk, x.grid);
		x.cap = rg.cap; x.region_ok = rg.ok;
		if (!rg.ok || allocator_refuses) x.spill = false;
	}
	const Layout l = lds_layout(k, x.Rk, nwc, x.spill);
	x.tile_slot = l.tile_slot; x.front_entries = l.front_entries; x.lds = l.bytes;
	x.variant = variant(x.Rk, nwc, x.spill);
	return x;
}
static bool launch_is(const Launch &x, int R, int Rk, int tile_slot, int front_entries, int lds, int grid, int variant)
{
	return x.R == R && x.Rk == Rk && x.tile_slot == tile_slot && x.front_entries == front_entries && x.lds == lds && x.grid == grid && x.variant == variant;
}

static void test_anchors()
{
	const Knobs d;
	// tail = 64 + 260 x 4 = 1 104 bytes; front entries = ((163 840 - 16 - 16 slots - 1 104) / entry bytes) & ~63
	CASE("L 8 / 8, 1 000 rows: slot = flush queue's end (192 x 4 + 64 x 8 = 1 280) + 128 x 20 = 3 840; (163 824 - 62 544) / 36 = 2 813");
	Launch x = launch_of(d, 8, 8, 1000, 256);
	CHECK(!x.spill && launch_is(x, 2, 2, 3840, 2752, 161616, 1, 6));
	CASE("L 8 / 8, 2^25 rows, records: slot = 192 x 12 = 2 304; (163 824 - 37 968) / 36 = 3 496; 64 steps per wave: cap = 2 x 512 + 256");
	x = launch_of(d, 8, 8, 1 << 25, 256);
	CHECK(x.spill && launch_is(x, 2, 2, 2304, 3456, 162384, 256, 7) && x.cap == 1280 && x.region_ok);
	CASE("L 17 / 17, 70 000 rows: slot = 192 x 24 = 4 608 = the flush queue's end (768 + 1 280 + 2 560); 88 992 / 36 = 2 472; 70 000 / 2 048 = 34.2");
	x = launch_of(d, 17, 17, 70000, 256);
	CHECK(!x.spill && launch_is(x, 2, 2, 4608, 2432, 162384, 35, 8));
	CASE("L 17 / 17, 2^25 rows, records: one tile: slot = 128 x 24 = 3 072; 113 568 / 36 = 3 154; 128 steps per wave");
	x = launch_of(d, 17, 17, 1 << 25, 256);
	CHECK(x.spill && launch_is(x, 2, 1, 3072, 3136, 163152, 256, 3) && x.cap == 1280 && x.region_ok);
	CASE("... with two tiles it was 2 432 entries (the figure beside tiles_for_launch)");
	CHECK(lds_layout(d, 2, 1, true).front_entries == 2432 && lds_layout(d, 2, 1, true).tile_slot == 4608 && lds_layout(d, 2, 1, true).bytes == 162384);
	CASE("L 17 / 24, 2^19 rows, records: 2 steps per wave, 2 048 rows per workgroup: cap = 2 x 8 + 256");
	x = launch_of(d, 17, 24, 1 << 19, 256);
	CHECK(x.spill && launch_is(x, 2, 1, 3072, 3136, 163152, 256, 3) && x.cap == 272 && x.region_ok);
	CASE("L 24 / 24, 2^25 rows, records: slot = 128 x 36 = 4 608; 88 992 / 52 = 1 711");
	x = launch_of(d, 24, 24, 1 << 25, 256);
	CHECK(x.spill && launch_is(x, 2, 1, 4608, 1664, 161360, 256, 5) && x.cap == 1280 && x.region_ok);
	CASE("L 31 / 32, 2^25 rows: too long for records; slot = 192 x 36 = 6 912 (> 2 816 + 2 560); 52 128 / 52 = 1 002");
	x = launch_of(d, 31, 32, 1 << 25, 256);
	CHECK(!x.spill && launch_is(x, 2, 2, 6912, 960, 161616, 256, 10));
	CASE("L 31 / 64, 100 rows: one tile; slot = flush queue's end 512 + 2 048 + 2 560 = 5 120 (> 128 x 36); 80 800 / 52 = 1 553");
	x = launch_of(d, 31, 64, 100, 256);
	CHECK(!x.spill && launch_is(x, 1, 1, 5120, 1536, 162896, 1, 4));
	CASE("L 20 / 41, 5 000 rows: one tile; slot = 512 + 1 280 + 2 560 = 4 352 (> 128 x 24); 93 088 / 36 = 2 585; 5 000 / 1 024 = 4.9");
	x = launch_of(d, 20, 41, 5000, 256);
	CHECK(!x.spill && launch_is(x, 1, 1, 4352, 2560, 162896, 5, 2));
	CASE("L 16 / 16, 32 000 000 rows, records: 500 000 steps / 4 096 waves = 123 each: cap = 2 x 492 + 256");
	x = launch_of(d, 16, 16, 32000000, 256);
	CHECK(x.spill && launch_is(x, 2, 1, 3072, 3136, 163152, 256, 3) && x.cap == 1240 && x.region_ok);

	CASE("records refused by the allocator: the direct kernel of the same tiles per step, and its layout");
	x = launch_of(d, 17, 17, 1 << 25, 256, true);
	CHECK(!x.spill && launch_is(x, 2, 1, 4352, 2560, 162896, 256, 2));
	CASE("SK_CENSUS_FRONT_ENTRIES: v & ~63 in [64, what the layout leaves]");
	CHECK(lds_layout(knob("FRONT_ENTRIES", "64"), 1, 1, true).front_entries == 64 && lds_layout(knob("FRONT_ENTRIES", "64"), 1, 1, true).bytes == 50256 + 2304);
	CHECK(lds_layout(knob("FRONT_ENTRIES", "63"), 1, 1, true).front_entries == 3136 && lds_layout(knob("FRONT_ENTRIES", "100"), 1, 1, true).front_entries == 64);
	CHECK(lds_layout(knob("FRONT_ENTRIES", "3136"), 1, 1, true).front_entries == 3136 && lds_layout(knob("FRONT_ENTRIES", "3199"), 1, 1, true).front_entries == 3136);
	CHECK(lds_layout(knob("FRONT_ENTRIES", "3072"), 1, 1, true).front_entries == 3072 && lds_layout(knob("FRONT_ENTRIES", "3200"), 1, 1, true).front_entries == 3136);
	CHECK(lds_layout(knob("FRONT_ENTRIES", "1024"), 2, 2, false).front_entries == 960 && lds_layout(knob("FRONT_ENTRIES", "960"), 2, 2, false).front_entries == 960);
	CHECK(lds_layout(knob("FRONT_ENTRIES", "896"), 2, 2, false).front_entries == 896 && lds_layout(knob("FRONT_ENTRIES", "896"), 2, 2, false).bytes == 111696 + 896 * 52);
	CASE("SK_CENSUS_TILES=1, 8-byte rows: 128 x 12 = 1 536 < 512 + 512 + 2 560 = 3 584; (163 824 - 58 448) / 36 = 2 927");
	x = launch_of(knob("TILES", "1"), 8, 8, 1000, 256);
	CHECK(launch_is(x, 1, 1, 3584, 2880, 162128, 1, 0));
}

// ---- records or not, grid, regions --------------------------------------------------------------------------------------------------
static void test_launch_rules()
{
	const Knobs d;
	CASE("records: barcodes of at most 24 characters, launches from 2^19 rows");
	CHECK(wants_spill(d, 24, 524288) && !wants_spill(d, 25, 524288) && !wants_spill(d, 24, 524287) && wants_spill(d, 1, 1 << 25) && !wants_spill(d, 31, 1 << 25));
	CHECK(wants_spill(knob("SPILL", "1"), 24, 1) && !wants_spill(knob("SPILL", "1"), 25, 1 << 25) && !wants_spill(knob("SPILL", "0"), 8, 1 << 25));
	CHECK(wants_spill(knob("SPILL_MIN_ROWS_LOG2", "6"), 17, 64) && !wants_spill(knob("SPILL_MIN_ROWS_LOG2", "6"), 17, 63));

	CASE("grid: a workgroup per CU, at most one per 16 waves' step");
	CHECK(grid(1, 2, 256, d) == 1 && grid(2048, 2, 256, d) == 1 && grid(2049, 2, 256, d) == 2 && grid(1024, 1, 256, d) == 1 && grid(1025, 1, 256, d) == 2);
	CHECK(grid(1 << 25, 2, 256, d) == 256 && grid(1 << 25, 1, 3, d) == 3 && grid(1 << 25, 1, 1, d) == 1 && grid(256 * 1024, 1, 256, d) == 256 && grid(255 * 1024, 1, 256, d) == 255);
	CHECK(grid(1 << 25, 1, 256, knob("WGS", "4")) == 1024 && grid(1 << 25, 1, 256, knob("WGS", "5")) == 256 && grid(3000, 1, 256, knob("WGS", "4")) == 3);

	CASE("regions: the combine pass addresses 1 024 workgroups");
	// 2^25 rows, one tile: 524 288 steps over 16 384 waves = 32 each: 32 768 rows per workgroup: cap = 2 x 128 + 256
	CHECK(spill_region(1 << 25, 1, 1024).ok && spill_region(1 << 25, 1, 1024).cap == 512);
	CHECK(!spill_region(1 << 25, 1, 1025).ok && spill_region(1 << 25, 1, 1025).cap == 512);
	CASE("regions: a workgroup's 256 regions stay below 2^27 records");
	// one workgroup, two tiles: w steps per wave are 2 048 w rows: cap = 16 w + 256 < 2^19 while w <= 32 751 = 524 016 steps of 128 rows
	CHECK(spill_region(67074048, 2, 1).ok && spill_region(67074048, 2, 1).cap == 524272);
	CHECK(!spill_region(67074049, 2, 1).ok && spill_region(67074049, 2, 1).cap == 524288);
	CASE("regions: small launches (tests): one step per wave at most");
	CHECK(spill_region(1, 1, 1).cap == 264 && spill_region(1, 1, 1).ok);         // 1 024 rows per workgroup: 2 x 4 + 256
	CHECK(spill_region(64, 2, 1).cap == 272 && spill_region(70000, 1, 3).cap == 440);      // 2 048 rows: 16 + 256; 1 094 steps / 48 waves = 23: 23 552 rows: 2 x 92 + 256

	CASE("direct above, combine grid, direct grid");
	CHECK(direct_above(1000, d) == 500 && direct_above(3, d) == 1 && direct_above(1 << 25, d) == 16777216u);
	CHECK(direct_above(1000, knob("SPILL_MAX_PCT", "0")) == 0 && direct_above(1000, knob("SPILL_MAX_PCT", "100")) == 1000 && direct_above(1 << 25, knob("SPILL_MAX_PCT", "100")) == 33554432u);
	CHECK(combine_grid(256) == 512 && combine_grid(3) == 6 && combine_grid(1) == 2);
	CHECK(direct_grid(256, d) == 2048 && direct_grid(256, knob("DIRECT_SPLIT", "1")) == 256 && direct_grid(256, knob("DIRECT_SPLIT", "64")) == 16384 && direct_grid(3, knob("DIRECT_SPLIT", "65")) == 24);
}

// ---- bites and growth ----------------------------------------------------------------------------------------------------------------
static bool bite_is(const Bite &b, int64_t nr, bool grow) { return b.nr == nr && b.grow == grow; }
static void test_bites()
{
	const Knobs d;
	CASE("rows per launch: 2^25, and a matrix below 2^31 - 2^24 bytes");
	CHECK(chunk_rows(d, 1) == 33554432 && chunk_rows(d, 17) == 33554432 && chunk_rows(d, 63) == 33554432);      // 2 130 706 432 / 63 = 33 820 737
	CHECK(chunk_rows(d, 64) == 33292288);                                         // 2 130 706 432 / 64, a multiple of 64 as it is
	CHECK(chunk_rows(knob("CHUNK_LOG2", "24"), 64) == 16777216 && chunk_rows(knob("CHUNK_LOG2", "6"), 64) == 64 && chunk_rows(knob("CHUNK_LOG2", "26"), 17) == 33554432);
	CASE("the least rows worth a launch: 2^22, at most the chunk");
	CHECK(min_chunk_rows(d, 33554432) == 4194304 && min_chunk_rows(d, 64) == 64 && min_chunk_rows(d, 4194304) == 4194304 && min_chunk_rows(d, 4194303) == 4194303);
	CHECK(min_chunk_rows(knob("MIN_CHUNK_LOG2", "30"), 33292288) == 33292288 && min_chunk_rows(knob("MIN_CHUNK_LOG2", "6"), 33554432) == 64);

	CASE("the count is fetched when the bound says the bite could fill the table beyond one half");
	CHECK(!bite_needs_count(0, 512, 1024, d) && bite_needs_count(0, 513, 1024, d) && bite_needs_count(1, 512, 1024, d) && !bite_needs_count(100, 412, 1024, d));
	CHECK(!bite_needs_count(0, 1 << 25, 1ull << 26, d) && bite_needs_count(1, 1 << 25, 1ull << 26, d));
	CHECK(!bite_needs_count(1000, 1000, 1024, knob("TRUST_SLOTS", "")));

	CASE("a table of 1 024 slots with 312 keys has room for 200: a smaller bite when that is worth a launch, in whole 64 rows");
	CHECK(bite_is(bite_after_count(312, 1024, 1024, 200, false), 192, false));
	CHECK(bite_is(bite_after_count(312, 1024, 1024, 199, false), 192, false));
	CHECK(bite_is(bite_after_count(312, 1024, 1024, 201, false), 1024, true));
	CHECK(bite_is(bite_after_count(312, 1024, 1000, 200, true), 192, false));    // (no longer the last bite)
	CHECK(bite_is(bite_after_count(312, 1024, 1000, 201, true), 1000, true));    // the last bite grows the table for all of its rows
	CASE("the bite as asked for is the least when it is smaller than min_chunk");
	CHECK(bite_is(bite_after_count(312, 1024, 200, 4194304, true), 200, false));
	CHECK(bite_is(bite_after_count(313, 1024, 200, 4194304, true), 200, true));
	CHECK(bite_is(bite_after_count(462, 1024, 50, 64, true), 50, false) && bite_is(bite_after_count(463, 1024, 50, 64, true), 50, true));
	CHECK(bite_is(bite_after_count(448, 1024, 100, 64, true), 64, false) && bite_is(bite_after_count(449, 1024, 100, 64, true), 100, true));
	CASE("room for all of it after the count (the bound was too high)");
	CHECK(bite_is(bite_after_count(0, 1024, 100, 64, true), 100, false) && bite_is(bite_after_count(0, 1024, 512, 64, false), 512, false));
	CHECK(bite_is(bite_after_count(0, 1024, 500, 64, false), 448, false));       // (census_add asks for whole chunks but for the last)
	CASE("a table beyond one half (a caller's own inserts): grow");
	CHECK(bite_is(bite_after_count(600, 1024, 64, 64, false), 64, true) && bite_is(bite_after_count(512, 1024, 1, 64, true), 1, true));
	CASE("the product's sizes: 2^26 slots, 2^25 rows asked for, 2^22 the least");
	CHECK(bite_is(bite_after_count(29360128, 1ull << 26, 1 << 25, 1 << 22, false), 4194304, false));
	CHECK(bite_is(bite_after_count(29360129, 1ull << 26, 1 << 25, 1 << 22, false), 1 << 25, true));
	CHECK(bite_is(bite_after_count(29360000, 1ull << 26, 1 << 25, 1 << 22, false), 4194432, false));      // room 4 194 432 = 65 538 x 64

	CASE("growth: doubled until `need` fits; no table beyond 2^32 slots");
	CHECK(grown_slots(1024, 1024) == 1024 && grown_slots(1024, 1025) == 2048 && grown_slots(1024, 2048) == 2048 && grown_slots(1024, 2049) == 4096);
	CHECK(grown_slots(1ull << 26, 2 * ((1ull << 25) + 1)) == 1ull << 27 && grown_slots(1024, 1) == 1024);
	CHECK(grown_slots(1024, 1ull << 32) == 1ull << 32 && grown_slots(1024, (1ull << 32) + 1) == 0 && grown_slots(1ull << 32, (1ull << 32) + 2) == 0);
	CHECK(grown_slots(1ull << 32, 1ull << 32) == 1ull << 32 && grown_slots(1ull << 31, (1ull << 31) + 1) == 1ull << 32);
}

// ---- the sweep ----------------------------------------------------------------------------------------------------------------------
// What the kernels lean on, restated from census_kernel's side: the front table's arrays from byte 0 (entries x (2 or 3 chunks of 16 bytes
// + a count), rounded to 16), then a slot per wave, then 64 bytes, 257 cursors and the step counter.
static const char *const kTiles[] = {nullptr, "1", "2", "0"}, *const kFront[] = {nullptr, "64", "100000"}, *const kWgs[] = {nullptr, "1", "4"};
static const char *const kChunk[] = {nullptr, "6", "25"}, *const kMinChunk[] = {nullptr, "6", "30"};
static const int64_t kRows[] = {1, 63, 64, 65, (1 << 19) - 1, (1 << 19) + 1, 1 << 25};
static const int kCus[] = {1, 3, 256};

static void sweep_launches()
{
	CASE("sweep: launches");
	for (int L = 1; L <= 31; L++)
	for (int stride = L; stride <= 64; stride++)
	for (const char *tiles : kTiles)
	for (const char *front : kFront)
	for (const char *wgs : kWgs)
	for (int spill_mode = -1; spill_mode <= 1; spill_mode++) {
		Knobs k;
		if (tiles) set_knob(k, "TILES", 5, tiles);
		if (front) set_knob(k, "FRONT_ENTRIES", 13, front);
		if (wgs) set_knob(k, "WGS", 3, wgs);
		if (spill_mode >= 0) set_knob(k, "SPILL", 5, spill_mode ? "1" : "0");
		snprintf(g_what, sizeof g_what, "sweep: L %d stride %d TILES %s FRONT %s WGS %s SPILL %d", L, stride, tiles ? tiles : "-", front ? front : "-", wgs ? wgs : "-", spill_mode);
		for (int64_t nr : kRows)
		for (int n_cu : kCus)
		for (int refused = 0; refused < 2; refused++) {
			g_rows = (long)nr; g_cus = n_cu; g_refused = refused;
			const Launch x = launch_of(k, L, stride, nr, n_cu, refused != 0);
			const int nw = L <= 8 ? 2 : L <= 20 ? 5 : 8, eb = nw == 8 ? 52 : 36;
			CHECK(x.R >= 1 && x.R <= 2 && x.Rk >= 1 && x.Rk <= x.R && (x.R == 1 || 2 * 64 * stride <= 5120));
			CHECK(!x.spill || L <= 24);
			// the layout
			CHECK(x.lds <= 160 * 1024);
			CHECK(x.front_entries >= 64 && x.front_entries % 64 == 0);
			const int front_bytes = (x.front_entries * eb + 15) & ~15, tail = front_bytes + 16 * x.tile_slot;
			CHECK(x.tile_slot % 16 == 0 && tail + 64 + (256 + 1 + 1) * 4 <= x.lds);
			const int queue = 64 + x.Rk * 64;
			CHECK(queue * 4 + queue * 4 * nw <= x.tile_slot);
			if (!x.spill) CHECK(((queue * 4 + 64 * 4 * nw + 15) & ~15) + 128 * 16 + 128 * 4 <= x.tile_slot);
			// the instantiation
			CHECK(x.variant >= 0 && x.variant < 12 && (x.variant & 1) == (x.spill ? 1 : 0) && (x.variant >> 1) % 3 == (nw == 2 ? 0 : nw == 5 ? 1 : 2) && (x.variant >> 1) / 3 + 1 == x.Rk);
			// the grid, and every row in some workgroup's share
			CHECK(x.grid >= 1 && x.grid <= n_cu * 4);
			if (x.spill) {
				CHECK(x.region_ok && x.grid <= 1024 && x.cap % 8 == 0 && (int64_t)x.cap * 256 < ((int64_t)1 << 27));
				const int64_t nsteps = (nr + 64 * x.Rk - 1) / (64 * x.Rk), per_wave = (nsteps + x.grid * 16 - 1) / (x.grid * 16);
				CHECK((int64_t)x.cap * 256 >= 2 * per_wave * 16 * x.Rk * 64 + 256 * 256);
			}
			g_cases++;
		}
	}
}

// the loop of census_add over an input of n rows, every row a new key (all_new) or none, on a table of `slots` slots that holds d0 keys
static void bites_of(int64_t chunk, int64_t min_chunk, int64_t n, uint64_t slots, uint64_t d0, bool all_new, int stride)
{
	const Knobs d;
	uint64_t bound = d0, exact = d0;
	int64_t nr = 0, covered = 0;
	for (int64_t o = 0; o < n; o += nr) {
		CHECK(o % 64 == 0);                                                       // every bite but the last is whole 64 rows
		nr = n - o < chunk ? n - o : chunk;
		if (bite_needs_count(bound, nr, slots, d)) {
			bound = exact;
			const Bite b = bite_after_count(bound, slots, nr, min_chunk, nr == n - o);
			if (b.grow) {
				slots = grown_slots(slots, 2 * (bound + (uint64_t)nr));
				CHECK(slots != 0 && (slots & (slots - 1)) == 0);
			}
			CHECK(b.nr >= 1 && b.nr <= nr);
			nr = b.nr;
		}
		CHECK(2 * (bound + (uint64_t)nr) <= slots);
		CHECK(nr <= ((int64_t)1 << 25) && nr * stride <= ((int64_t)1 << 31) - (1 << 24));
		bound += (uint64_t)nr;
		if (all_new) exact += (uint64_t)nr;
		covered += nr;
	}
	CHECK(covered == n);
}
static void sweep_bites()
{
	// (the bites depend on the pitch through chunk_rows alone: a pitch whose chunk another had is not walked again)
	int64_t seen[64][2];
	int n_seen = 0;
	for (int stride = 1; stride <= 64; stride++)
	for (const char *ck : kChunk)
	for (const char *mk : kMinChunk) {
		Knobs k;
		if (ck) set_knob(k, "CHUNK_LOG2", 10, ck);
		if (mk) set_knob(k, "MIN_CHUNK_LOG2", 14, mk);
		const int64_t chunk = chunk_rows(k, stride), min_chunk = min_chunk_rows(k, chunk);
		snprintf(g_what, sizeof g_what, "sweep: bites, stride %d CHUNK %s MIN_CHUNK %s", stride, ck ? ck : "-", mk ? mk : "-");
		CHECK(chunk >= 64 && chunk % 64 == 0 && chunk <= ((int64_t)1 << 25) && chunk * stride <= ((int64_t)1 << 31) - (1 << 24) && min_chunk >= 64 && min_chunk <= chunk);
		bool known = false;
		for (int i = 0; i < n_seen; i++) known = known || (seen[i][0] == chunk && seen[i][1] == min_chunk);
		if (known) continue;
		CHECK(n_seen < 64);
		seen[n_seen][0] = chunk; seen[n_seen][1] = min_chunk; n_seen++;
		for (int64_t n : kRows)
		for (int slots_lg : {10, 20, 26})
		for (int fill = 0; fill < 3; fill++)
		for (int all_new = 0; all_new < 2; all_new++) {
			const uint64_t slots = 1ull << slots_lg, d0 = fill == 0 ? 0 : fill == 1 ? slots / 2 - 100 : slots / 2;
			snprintf(g_what, sizeof g_what, "sweep: bites, stride %d chunk %ld min %ld rows %ld slots 2^%d holding %lu, %s", stride, (long)chunk, (long)min_chunk, (long)n, slots_lg,
			         (unsigned long)d0, all_new ? "all new" : "no new");
			bites_of(chunk, min_chunk, n, slots, d0, all_new != 0, stride);
			g_cases++;
		}
	}
}

int main()
{
	test_knobs();
	test_kernel_choice();
	test_anchors();
	test_launch_rules();
	test_bites();
	sweep_launches();
	sweep_bites();
	printf("ok: %ld cases, %ld checks\n", g_cases, g_checks);
	return 0;
}
