// tileplan_test.cpp — sk_tileplan.h (the launch decisions of the fused tile pass and the demultiplex kernels) on the host, built with
// the address and undefined-behaviour sanitizers (tests/test_tileplan_cpu.py).  Every expectation below is written out by hand from
// the rules as launch_tile_pass, plan_shape and launch_tile_blocked applied them before the header existed: kernel, waves, LDS bytes
// and caps are literal numbers here, never the header asked a second time.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <set>

#include "sk_tileplan.h"

using namespace sk;
using namespace sk::tileplan;

static long g_checks = 0, g_cases = 0;
static char g_what[256] = "";                    // the case at hand, for a failing CHECK
#define CHECK(cond)                                                                                                     \
	do {                                                                                                                \
		g_checks++;                                                                                                     \
		if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed [%s]\n", __FILE__, __LINE__, #cond, g_what); exit(1); }   \
	} while (0)
#define CASE(...) do { g_cases++; snprintf(g_what, sizeof g_what, __VA_ARGS__); } while (0)

// ---- shapes ------------------------------------------------------------------------------------------------------------------------
// a sheet of 96 samples that every matcher serves (3 groups of 32; a 1 000-byte bit-sliced blob), no table yet
static Shape sheet96()
{
	Shape s;
	s.n_cu = 256;
	s.S = 96; s.G = 3; s.bitsliced = true; s.matcher_bytes = 1000;
	return s;
}
// demultiplex alone, the decision only, by a full-key table of (mask_slots + 1) * 16 bytes
static Shape demux_alone(int64_t n, int bc_stride, int W1, int W2, int mask_slots)
{
	Shape s = sheet96();
	s.n = n; s.has_bc = true; s.bc_stride = bc_stride;
	s.full_key = true; s.W1 = W1; s.W2 = W2; s.mask_slots = mask_slots;
	return s;
}
static Shape factored(int64_t n, int bc_stride, int W, int pair_bytes)
{
	Shape s = demux_alone(n, bc_stride, W, W, 0);
	s.full_key = false; s.factored = true; s.pair_bytes = pair_bytes;
	return s;
}
static Shape with_detail(Shape s, bool matched) { s.lowest_diff = s.first_idx = s.last_idx = true; s.detail_matched = matched; return s; }
static Shape as_many(Shape s) { s.many = true; s.many_quads = (int)((s.n + 255) / 256); return s; }
// two mates, mask and trim, 150-byte rows, 8-byte barcodes of the 96-sample sheet: the fused pass
static Shape fused_pass(int64_t n)
{
	Shape s = sheet96();
	s.n = n; s.stride = 150;
	s.mask[0] = s.trim[0] = s.mask[1] = s.trim[1] = true;
	s.has_bc = true; s.bc_stride = 8;
	return s;
}

static bool is(const KernelId &id, Family f, int W1, int W2, bool direct, bool ldstab, bool detail, bool pair, bool many)
{
	return id.family == f && id.W1 == W1 && id.W2 == W2 && id.direct == direct && id.ldstab == ldstab && id.detail == detail && id.pair == pair && id.many == many;
}
static bool lookup(const KernelId &id, int W1, int W2, bool direct, bool ldstab, bool detail, bool pair = false, bool many = false) { return is(id, kLookup, W1, W2, direct, ldstab, detail, pair, many); }
static bool x8x2(const KernelId &id, bool ldstab, bool detail, bool many = false) { return is(id, kLookup8x2, 0, 0, false, ldstab, detail, false, many); }
static bool lds_is(const LdsPlan &lp, int table_bytes, int hist_off, int tiles_off, int tile_slot, int use_lds_hist)
{
	return lp.table_bytes == table_bytes && lp.hist_off == hist_off && lp.tiles_off == tiles_off && lp.tile_slot == tile_slot && lp.use_lds_hist == use_lds_hist;
}

// ---- which lookup kernel -------------------------------------------------------------------------------------------------------------
static void test_lookup_choice()
{
	const Knobs k0;
	// 96 samples: the histogram is 99 * 4 = 396 -> 400 bytes; a table of 1 024 * 16 = 16 384 bytes; a wave's slot is 1 KiB
	CASE("8-byte pitch, W1 = 2, n = 1 499 999");
	{
		const DemuxPlan p = demux_plan(k0, demux_alone(1499999, 8, 2, 0, 1023));
		CHECK(lookup(p.id, 2, 0, true, true, false));
		CHECK(p.nw == 16 && p.lds == 400 + 16384 + 16 * 1024 && p.lds == 33168);
		CHECK(lds_is(p.lp, 16384, 0, 16784, 1024, 1));
		CHECK(p.max_wg == 1 && p.force_wg == 0 && p.wg(5) == 1 && p.wg(1) == 1);      // LDSTAB: one workgroup per CU
		CHECK(!p.many_ok);
	}
	CASE("8-byte pitch, W1 = 2, n = 1 500 000");
	{
		const DemuxPlan p = demux_plan(k0, demux_alone(1500000, 8, 2, 0, 1023));
		CHECK(x8x2(p.id, true, false) && p.nw == 16 && p.lds == 33168 && p.many_ok);
	}
	CASE("8-byte pitch, detail of matched rows: 8x2 at every n");
	for (int64_t n : {(int64_t)1, (int64_t)70001, (int64_t)1499999, (int64_t)1500000, (int64_t)100000000})
		CHECK(x8x2(demux_plan(k0, with_detail(demux_alone(n, 8, 2, 0, 1023), true)).id, true, true));
	CASE("SK_DEMUX_ROWS2 = 0 / 1");
	{
		Knobs k; k.demux_rows2 = 0;
		CHECK(lookup(demux_plan(k, demux_alone(2000000, 8, 2, 0, 1023)).id, 2, 0, true, true, false));
		CHECK(lookup(demux_plan(k, with_detail(demux_alone(70001, 8, 2, 0, 1023), true)).id, 2, 0, true, true, true));
		k.demux_rows2 = 1;
		CHECK(x8x2(demux_plan(k, demux_alone(100, 8, 2, 0, 1023)).id, true, false));
	}
	CASE("SK_DEMUX_DIRECT = 0: the gather form, which rules rows2 out");
	{
		Knobs k; k.demux_direct = 0;
		CHECK(lookup(demux_plan(k, demux_alone(2000000, 8, 2, 0, 1023)).id, 2, 0, false, true, false));
		k.demux_rows2 = 1;
		CHECK(lookup(demux_plan(k, demux_alone(2000000, 8, 2, 0, 1023)).id, 2, 0, false, true, false));
		CHECK(lookup(demux_plan(k, demux_alone(100, 4, 1, 0, 511)).id, 1, 0, false, true, false));
		k = Knobs(); k.demux_direct = 1;
		CHECK(lookup(demux_plan(k, demux_alone(100, 4, 1, 0, 511)).id, 1, 0, true, true, false));
	}
	CASE("other pitches and keys");
	CHECK(lookup(demux_plan(k0, demux_alone(70001, 12, 3, 0, 1023)).id, 3, 0, false, true, false));      // three key dwords: gathered
	CHECK(lookup(demux_plan(k0, demux_alone(70001, 17, 2, 2, 1023)).id, 2, 2, false, true, false));      // 8 + 8 beside a separator
	CHECK(lookup(demux_plan(k0, demux_alone(70001, 9, 1, 1, 1023)).id, 1, 1, false, true, false));
	CHECK(lookup(demux_plan(k0, demux_alone(70001, 16, 4, 0, 1023)).id, 4, 0, false, true, false));
	CHECK(lookup(demux_plan(k0, demux_alone(70001, 20, 5, 0, 1023)).id, 5, 0, false, true, false));
	CHECK(lookup(demux_plan(k0, demux_alone(70001, 12, 2, 0, 1023)).id, 2, 0, true, true, false));       // 8 key bytes on a 12-byte pitch: direct, one row per lane
	CHECK(lookup(demux_plan(k0, demux_alone(9000000, 12, 2, 0, 1023)).id, 2, 0, true, true, false));     // ... at any n: 8x2 wants the 8-byte pitch
	CHECK(lookup(demux_plan(k0, demux_alone(70001, 4, 2, 0, 1023)).id, 2, 0, false, true, false));       // the key's dwords reach past the pitch: gathered
	CASE("a pitch that is no multiple of 4 is never direct");
	for (int pitch : {5, 6, 7, 9, 10, 11, 13, 30})
		for (int W1 : {1, 2}) {
			Knobs k; k.demux_direct = 1; k.demux_rows2 = 1;
			const KernelId id = demux_plan(k, demux_alone(2000000, pitch, W1, 0, 1023)).id;
			CHECK(lookup(id, W1, 0, false, true, false));
		}
	CASE("the factored form: PAIR, always LDSTAB");
	for (int ldstab : {-1, 0, 1})
		for (int detail = 0; detail < 2; detail++) {
			Knobs k; k.demux_ldstab = ldstab;
			Shape s1 = factored(70001, 9, 1, 40000), s2 = factored(70001, 17, 2, 40000);
			if (detail) { s1 = with_detail(s1, true); s2 = with_detail(s2, true); }
			CHECK(lookup(demux_plan(k, s1).id, 1, 1, false, true, detail, true));
			CHECK(lookup(demux_plan(k, s2).id, 2, 2, false, true, detail, true));
		}
	{
		const DemuxPlan p = demux_plan(k0, factored(70001, 17, 2, 40000));
		CHECK(p.nw == 16 && p.lds == 400 + 40000 + 16384 && p.lds == 56784 && lds_is(p.lp, 40000, 0, 40400, 1024, 1) && p.max_wg == 1);
	}
	CASE("the table's 128 KiB: at it in LDS, just above it in the vector cache with 4 waves at most");
	{
		DemuxPlan p = demux_plan(k0, demux_alone(70001, 17, 2, 2, 8191));           // 8 192 * 16 = 131 072
		CHECK(lookup(p.id, 2, 2, false, true, false) && p.nw == 16 && p.lds == 400 + 131072 + 16384);
		p = demux_plan(k0, demux_alone(70001, 17, 2, 2, 8192));                     // 8 193 * 16 = 131 088
		CHECK(lookup(p.id, 2, 2, false, false, false) && p.nw == 4 && p.lds == 400 + 4096 && p.lds == 4496);
		CHECK(lds_is(p.lp, 0, 0, 400, 1024, 1));
		CHECK(p.max_wg == 0 && p.wg(8) == 8 && p.wg(3) == 3);                      // whatever is resident
		CHECK(!p.many_ok);
		p = demux_plan(k0, demux_alone(70001, 17, 2, 2, 16383));                    // 256 KiB
		CHECK(lookup(p.id, 2, 2, false, false, false) && p.nw == 4);
	}
	CASE("SK_DEMUX_LDSTAB = 0");
	{
		Knobs k; k.demux_ldstab = 0;
		DemuxPlan p = demux_plan(k, demux_alone(2000000, 8, 2, 0, 1023));
		CHECK(x8x2(p.id, false, false) && p.nw == 4 && p.lds == 4496 && p.max_wg == 0 && !p.many_ok);
		p = demux_plan(k, demux_alone(70001, 8, 2, 0, 1023));
		CHECK(lookup(p.id, 2, 0, true, false, false) && p.nw == 4);
		k.lut_nw = 16;                                                               // above the 256 threads these are compiled for: not applied
		CHECK(demux_plan(k, demux_alone(70001, 8, 2, 0, 1023)).nw == 4);
		k.lut_nw = 5;
		CHECK(demux_plan(k, demux_alone(70001, 8, 2, 0, 1023)).nw == 4);
		k.lut_nw = 2;
		CHECK(demux_plan(k, demux_alone(70001, 8, 2, 0, 1023)).nw == 2);
	}
	CASE("a table above 64 KiB: sixteen waves below 4 M rows, eight from there");
	{
		DemuxPlan p = demux_plan(k0, demux_alone(3999999, 17, 2, 2, 8191));
		CHECK(p.nw == 16 && p.lds == 400 + 131072 + 16 * 1024 && p.lds == 147856);
		p = demux_plan(k0, demux_alone(4000000, 17, 2, 2, 8191));
		CHECK(p.nw == 8 && p.lds == 400 + 131072 + 8 * 1024 && p.lds == 139664);
		p = demux_plan(k0, demux_alone(4000000, 17, 2, 2, 4095));                   // 65 536 bytes: not above
		CHECK(p.nw == 16);
		p = demux_plan(k0, demux_alone(4000000, 17, 2, 2, 4096));                   // 65 552
		CHECK(p.nw == 8);
	}
	CASE("an LDS total over 160 KiB halves the waves, never below 4");
	{
		DemuxPlan p = demux_plan(k0, factored(70001, 17, 2, 150000));               // 150 400 + 16 384 = 166 784 > 163 840; + 8 192 = 158 592
		CHECK(p.nw == 8 && p.lds == 158592);
		p = demux_plan(k0, factored(70001, 17, 2, 157008));                         // + 8 192 = 165 600 > 163 840; + 4 096 = 161 504
		CHECK(p.nw == 4 && p.lds == 161504);
		p = demux_plan(k0, factored(70001, 17, 2, 162000));                         // + 4 096 = 166 496: stays at 4 (the occupancy query refuses it)
		CHECK(p.nw == 4 && p.lds == 166496);
		p = demux_plan(k0, factored(70001, 17, 2, 147040));                         // 147 440 + 16 384 = 163 824 <= 163 840
		CHECK(p.nw == 16 && p.lds == 163824);
	}
	CASE("SK_LUT_NW / SK_LUT_WG within their bounds");
	{
		Knobs k;
		for (int v : {1, 3, 8, 16}) { k.lut_nw = v; CHECK(demux_plan(k, demux_alone(70001, 8, 2, 0, 1023)).nw == v); }
		for (int v : {-1, 0, 17, 64}) { k.lut_nw = v; CHECK(demux_plan(k, demux_alone(70001, 8, 2, 0, 1023)).nw == 16); }
		k = Knobs();
		k.lut_wg = 2;
		DemuxPlan p = demux_plan(k, demux_alone(70001, 8, 2, 0, 1023));
		CHECK(p.force_wg == 2 && p.wg(1) == 2 && p.wg(7) == 2);                     // instead of the answer, LDSTAB or not
		k.demux_ldstab = 0;
		p = demux_plan(k, demux_alone(70001, 8, 2, 0, 1023));
		CHECK(p.wg(8) == 2);
		k.lut_wg = 0;
		CHECK(demux_plan(k, demux_alone(70001, 8, 2, 0, 1023)).wg(8) == 8);
		k.lut_wg = -3;
		CHECK(demux_plan(k, demux_alone(70001, 8, 2, 0, 1023)).wg(8) == 8);
	}
}

// ---- many batches in one launch ------------------------------------------------------------------------------------------------------
static void test_many()
{
	const Knobs k0;
	Knobs kg; kg.lut_many_gather = true;
	CASE("many_ok: the 8x2 LDSTAB kernels");
	{
		DemuxPlan p = demux_plan(k0, as_many(demux_alone(1500000, 8, 2, 0, 1023)));
		CHECK(p.many_ok && x8x2(p.id, true, false, true));
		p = demux_plan(k0, as_many(with_detail(demux_alone(512, 8, 2, 0, 1023), true)));
		CHECK(p.many_ok && x8x2(p.id, true, true, true));
		p = demux_plan(k0, demux_alone(1500000, 8, 2, 0, 1023));                    // the answer does not wait for the many-batch call
		CHECK(p.many_ok && x8x2(p.id, true, false, false));
		p = demux_plan(k0, as_many(demux_alone(1499999, 8, 2, 0, 1023)));           // one row per lane below 1.5 M rows: no one-launch form
		CHECK(!p.many_ok && lookup(p.id, 2, 0, true, true, false));
	}
	CASE("many_ok with SK_LUT_MANY_GATHER=1: gathered W1 = W2 = 2, full-key or factored");
	{
		DemuxPlan p = demux_plan(kg, as_many(demux_alone(70001, 17, 2, 2, 1023)));
		CHECK(p.many_ok && lookup(p.id, 2, 2, false, true, false, false, true));
		p = demux_plan(kg, as_many(with_detail(factored(70001, 17, 2, 40000), true)));
		CHECK(p.many_ok && lookup(p.id, 2, 2, false, true, true, true, true));
		CHECK(!demux_plan(k0, as_many(demux_alone(70001, 17, 2, 2, 1023))).many_ok);
		CHECK(!demux_plan(k0, as_many(factored(70001, 17, 2, 40000))).many_ok);
	}
	CASE("many_ok is false for every other shape");
	CHECK(!demux_plan(kg, as_many(demux_alone(70001, 12, 3, 0, 1023))).many_ok);
	CHECK(!demux_plan(kg, as_many(demux_alone(70001, 9, 1, 1, 1023))).many_ok);
	CHECK(!demux_plan(kg, as_many(factored(70001, 9, 1, 40000))).many_ok);
	CHECK(!demux_plan(kg, as_many(demux_alone(70001, 8, 2, 0, 1023))).many_ok);
	CHECK(!demux_plan(kg, as_many(demux_alone(2000000, 12, 2, 0, 1023))).many_ok);
	CHECK(!demux_plan(kg, as_many(demux_alone(2000000, 4, 1, 0, 1023))).many_ok);
	{
		Knobs k = kg; k.demux_ldstab = 0;                                           // !LDSTAB
		CHECK(!demux_plan(k, as_many(demux_alone(2000000, 8, 2, 0, 1023))).many_ok);
		CHECK(!demux_plan(k, as_many(demux_alone(70001, 17, 2, 2, 1023))).many_ok);
		CHECK(!demux_plan(kg, as_many(demux_alone(2000000, 17, 2, 2, 8192))).many_ok);
		k = kg; k.demux_direct = 0;                                                 // the gathered <2, 0>
		CHECK(!demux_plan(k, as_many(demux_alone(2000000, 8, 2, 0, 1023))).many_ok);
	}
	{
		const DemuxPlan p = demux_plan(kg, as_many(with_detail(demux_alone(2000000, 8, 2, 0, 1023), false)));      // not by the table
		CHECK(!p.many_ok && p.id.family == kMatcherTile && !p.id.many);
		Knobs k = kg; k.no_hash_demux = true;
		CHECK(!demux_plan(k, as_many(demux_alone(2000000, 8, 2, 0, 1023))).many_ok);
	}
}

// ---- by the table or not; fusing -----------------------------------------------------------------------------------------------------
static void test_by_table_and_fusing()
{
	const Knobs k0;
	CASE("by the table or not");
	{
		const Shape s = demux_alone(70001, 8, 2, 0, 1023);
		CHECK(demux_by_table(k0, s) && demux_plan(k0, s).id.family == kLookup);
		CHECK(demux_by_table(k0, with_detail(s, true)));
		CHECK(!demux_by_table(k0, with_detail(s, false)) && demux_plan(k0, with_detail(s, false)).id.family == kMatcherTile);
		Shape one = s; one.first_idx = true;                                        // any one detail column
		CHECK(!demux_by_table(k0, one));
		CHECK(demux_by_table(k0, demux_alone(70001, 32, 2, 0, 1023)));              // 64 rows x 32 = 2 048
		CHECK(!demux_by_table(k0, demux_alone(70001, 33, 2, 0, 1023)) && demux_plan(k0, demux_alone(70001, 33, 2, 0, 1023)).id.family == kMatcherTile);
		Knobs k; k.no_hash_demux = true;
		CHECK(!demux_by_table(k, s) && demux_plan(k, s).id.family == kMatcherTile);
		Shape none = s; none.full_key = false;
		CHECK(!demux_by_table(k0, none) && demux_plan(k0, none).id.family == kMatcherTile);
		CHECK(demux_by_table(k0, factored(70001, 17, 2, 40000)));
		const DemuxPlan p = demux_plan(k0, none);                                   // the matchers' launch: no lookup shape, no one-launch form
		CHECK(is(p.id, kMatcherTile, 0, 0, false, false, false, false, false) && !p.many_ok && p.nw == 0 && p.lds == 0);
		Shape nobc = s; nobc.has_bc = false;
		CHECK(demux_plan(k0, nobc).id.family == kNoLaunch);
	}
	CASE("fusing: every factor in turn");
	{
		Shape s = sheet96();
		s.n = 70001; s.stride = 150; s.mask[0] = true; s.has_bc = true; s.bc_stride = 32; s.G = 4; s.S = 128;
		CHECK(fuses_demux(k0, s) && demux_plan(k0, s).id.family == kNoLaunch && !wants_neighbour_table(k0, s));
		Shape t = s; t.has_bc = false; CHECK(!fuses_demux(k0, t));
		t = s; t.mask[0] = false; CHECK(!fuses_demux(k0, t));
		t = s; t.mask[0] = false; t.trim[1] = true; CHECK(fuses_demux(k0, t));     // any mate's work will do
		t = s; t.stride = 960; CHECK(fuses_demux(k0, t));
		t = s; t.stride = 961; CHECK(!fuses_demux(k0, t));
		t = s; t.bitsliced = false; CHECK(!fuses_demux(k0, t));
		t = s; t.G = 5; CHECK(!fuses_demux(k0, t));
		t = s; t.S = 0; CHECK(!fuses_demux(k0, t));
		t = s; t.bc_stride = 33; CHECK(!fuses_demux(k0, t));
		Knobs k; k.no_fused_demux = true;
		CHECK(!fuses_demux(k, s) && demux_plan(k, s).id.family == kMatcherTile && wants_neighbour_table(k, s));
		// a call that does not fuse wants the table: for the decision alone, or for the detail of matched rows
		t = s; t.G = 5;
		CHECK(wants_neighbour_table(k0, t) && wants_neighbour_table(k0, with_detail(t, true)) && !wants_neighbour_table(k0, with_detail(t, false)));
		t.has_bc = false;
		CHECK(!wants_neighbour_table(k0, t));
	}
	CASE("fusing: row_bytes = max(stride if a mate trims else 0, bc_stride)");
	{
		Shape s = fused_pass(70001);                                                // trims: 150 against 8
		MatePlan p = mate_plan(k0, s);
		CHECK(p.tiles && p.demux && !p.fallback && p.row_bytes == 150 && p.slots == 2);
		s.trim[0] = s.trim[1] = false;                                              // the mask alone: the barcodes' 8
		CHECK(mate_plan(k0, s).row_bytes == 8);
		s.bc_stride = 32; s.stride = 20; s.trim[1] = true;                          // 20 against 32
		CHECK(mate_plan(k0, s).row_bytes == 32);
		s.mask[0] = s.mask[1] = false;                                              // one mate, trim alone, but fused: the two-mate kernel and rule
		p = mate_plan(k0, s);
		CHECK(p.demux && p.slots == 2 && p.max_wg == 3);
	}
}

// ---- the mate pass ---------------------------------------------------------------------------------------------------------------------
static void test_mate_pass()
{
	const Knobs k0;
	Shape s;
	s.n = 70001; s.stride = 150; s.n_cu = 256;
	CASE("trim alone");
	{
		s.trim[0] = true;
		const MatePlan p = mate_plan(k0, s);
		CHECK(p.tiles && !p.demux && !p.fallback && p.slots == 10 && p.max_wg == 4 && p.row_bytes == 150);
		Shape t = s; t.trim[0] = false; t.trim[1] = true;                           // the second mate's alone
		CHECK(mate_plan(k0, t).slots == 10 && mate_plan(k0, t).max_wg == 4);
	}
	CASE("one mate with the mask");
	{
		s.trim[0] = false; s.mask[0] = true;
		MatePlan p = mate_plan(k0, s);
		CHECK(p.tiles && !p.demux && p.slots == 4 && p.max_wg == 3 && p.row_bytes == 0);
		s.trim[0] = true;
		p = mate_plan(k0, s);
		CHECK(p.slots == 4 && p.max_wg == 3 && p.row_bytes == 150);
	}
	CASE("two mates: three workgroups below n_cu * 128 tiles, two from there on");
	{
		s.mask[1] = true;
		// 256 CUs: 32 768 tiles of 64 rows
		s.n = 2097088;                                                              // 32 767 tiles
		MatePlan p = mate_plan(k0, s);
		CHECK(p.tiles && !p.demux && p.slots == 2 && p.max_wg == 3 && p.row_bytes == 150);
		s.n = 2097089;                                                              // 32 768
		CHECK(mate_plan(k0, s).max_wg == 2 && mate_plan(k0, s).slots == 2);
		s.n_cu = 3;                                                                 // 384 tiles
		s.n = 24512; CHECK(mate_plan(k0, s).max_wg == 3);                           // 383
		s.n = 24513; CHECK(mate_plan(k0, s).max_wg == 2);                           // 384
		s.n_cu = 1;
		s.n = 8128; CHECK(mate_plan(k0, s).max_wg == 3);                            // 127
		s.n = 8129; CHECK(mate_plan(k0, s).max_wg == 2);                            // 128
		CHECK(two_mate_wg(2097088, 256) == 3 && two_mate_wg(2097089, 256) == 2);
		// the fused pass takes the same rule
		Shape f = fused_pass(2097088);
		CHECK(mate_plan(k0, f).demux && mate_plan(k0, f).max_wg == 3);
		f.n = 2097089;
		CHECK(mate_plan(k0, f).max_wg == 2);
	}
	CASE("the blocked pass: its cap, slots and image");
	CHECK(blocked_max_wg(1, 70001, 256) == 3 && blocked_max_wg(1, 100000000, 256) == 3);
	CHECK(blocked_max_wg(2, 2097088, 256) == 3 && blocked_max_wg(2, 2097089, 256) == 2 && blocked_max_wg(2, 24512, 3) == 3 && blocked_max_wg(2, 24513, 3) == 2);
	CHECK(blocked_slots(1) == 4 && blocked_slots(2) == 2);
	CHECK(blocked_image(150, 2, false) == 10240);                                   // 9 600 bytes: ten chunks
	CHECK(blocked_image(150, 4, true) == 12288);                                    // ... in whole rounds of four
	CHECK(blocked_image(8, 2, true) == 2048 && blocked_image(8, 4, false) == 4096 && blocked_image(960, 2, false) == 61440 && blocked_image(151, 2, false) == 10240);
	CASE("rows of 960 bytes tile, of 961 fall back and nothing fuses");
	{
		Shape f = fused_pass(70001);
		f.stride = 960;
		MatePlan p = mate_plan(k0, f);
		CHECK(p.tiles && p.demux && !p.fallback && p.row_bytes == 960 && !long_rows(f));
		f.stride = 961;
		p = mate_plan(k0, f);
		CHECK(p.fallback && !p.tiles && !p.demux && long_rows(f) && !fuses_demux(k0, f));
		CHECK(demux_plan(k0, f).id.family == kMatcherTile && wants_neighbour_table(k0, f));      // the barcodes get a launch of their own
		f.full_key = true; f.W1 = 2; f.mask_slots = 1023;
		CHECK(lookup(demux_plan(k0, f).id, 2, 0, true, true, false));
		f.has_bc = false;
		CHECK(mate_plan(k0, f).fallback && demux_plan(k0, f).id.family == kNoLaunch);
		Shape none = fused_pass(70001);                                             // no mate has work: long rows do not matter
		none.mask[0] = none.trim[0] = none.mask[1] = none.trim[1] = false; none.stride = 5000;
		p = mate_plan(k0, none);
		CHECK(!p.fallback && !p.tiles && !long_rows(none));
	}
}

// ---- LDS layout, shape search, grid -------------------------------------------------------------------------------------------------
static void test_layout_search_grid()
{
	CASE("tile kernels' LDS layout");
	CHECK(lds_is(tile_lds(false, 0, 0, 64 * 150), 0, 0, 0, 16 + 9600 + 16, 0));                    // trim alone: the image and its pads
	CHECK(lds_is(tile_lds(false, 1000, 96, 0), 0, 0, 0, 32, 0));                                   // the mask alone: no image, no tables
	CHECK(lds_is(tile_lds(true, 1000, 96, 64 * 150), 1008, 1008, 1408, 9632, 1));                  // the fused pass: 1 008 + 396 = 1 404 -> 1 408
	CHECK(lds_is(tile_lds(true, 1000, 96, 64 * 33), 1008, 1008, 1408, 16 + 2112 + 16, 1));         // the matchers' launch on a 33-byte pitch
	CHECK(lds_is(tile_lds(true, 1000, 96, 64 * 17), 1008, 1008, 1408, 16 + 1088 + 16, 1));
	CHECK(lds_is(tile_lds(true, 1000, 96, 100), 1008, 1008, 1408, 16 + 112 + 16, 1));              // an image rounds up to 16
	CHECK(lds_is(tile_lds(true, 20440, 1021, 512), 20448, 20448, 20448 + 4096, 544, 1));           // S + 3 = 1 024: the last histogram in LDS
	CHECK(lds_is(tile_lds(true, 20460, 1022, 512), 20464, 20464, 20464, 544, 0));                  // 1 025: global atomics
	CASE("shape search: the candidates");
	{
		const LdsPlan lp = tile_lds(true, 1000, 96, 64 * 150);
		Knobs k;
		Candidates c = tile_candidates(k, lp, 4);
		CHECK(c.n == 3 && c.nw[0] == 4 && c.nw[1] == 2 && c.nw[2] == 1 && c.lds[0] == 1408 + 4 * 9632 && c.lds[0] == 39936 && c.lds[1] == 20672 && c.lds[2] == 11040);
		k.tile_waves = 2;
		c = tile_candidates(k, lp, 4);
		CHECK(c.n == 2 && c.nw[0] == 2 && c.nw[1] == 1);
		k.tile_waves = 8;
		c = tile_candidates(k, lp, 4);
		CHECK(c.n == 4 && c.nw[0] == 8 && c.nw[3] == 1 && c.lds[0] == 1408 + 8 * 9632);
		k.tile_waves = 3;
		c = tile_candidates(k, lp, 4);
		CHECK(c.n == 2 && c.nw[0] == 3 && c.nw[1] == 1);
		for (int v : {-1, 0, 9, 64}) { k.tile_waves = v; c = tile_candidates(k, lp, 4); CHECK(c.n == 3 && c.nw[0] == 4); }
		// 960-byte rows: four waves are 4 * 61 472 = 245 888 bytes, above the 163 840
		const LdsPlan big = tile_lds(false, 0, 0, 64 * 960);
		c = tile_candidates(Knobs(), big, 4);
		CHECK(c.n == 2 && c.nw[0] == 2 && c.lds[0] == 122944 && c.nw[1] == 1 && c.lds[1] == 61472);
		const LdsPlan huge = {0, 0, 0, 200000, 0};
		CHECK(tile_candidates(Knobs(), huge, 4).n == 0);
	}
	CASE("shape search: the choice among occupancy answers");
	{
		const Candidates c = tile_candidates(Knobs(), tile_lds(true, 1000, 96, 64 * 150), 4);      // 4, 2, 1 waves
		Knobs k;
		auto pick = [&](int a, int b, int d, int max_wg) { const int occ[3] = {a, b, d}; return tile_pick(k, c, occ, max_wg); };
		Pick p = pick(2, 4, 8, 0);                                                  // 8 waves each: the first wins
		CHECK(p.nw == 4 && p.wg == 2 && p.lds == 39936);
		p = pick(1, 3, 8, 0);                                                       // 4, 6, 8
		CHECK(p.nw == 1 && p.wg == 8 && p.lds == 11040);
		p = pick(1, 3, 5, 0);                                                       // 4, 6, 5
		CHECK(p.nw == 2 && p.wg == 3 && p.lds == 20672);
		p = pick(8, 8, 8, 3);                                                       // capped: 12, 6, 3
		CHECK(p.nw == 4 && p.wg == 3);
		p = pick(1, 8, 8, 2);                                                       // 4, 4, 2: a tie again
		CHECK(p.nw == 4 && p.wg == 1);
		p = pick(0, 1, 8, 4);                                                       // 0, 2, 4
		CHECK(p.nw == 1 && p.wg == 4);
		p = pick(0, 0, 0, 4);                                                       // nothing is resident
		CHECK(p.nw == 0 && p.wg == 0);
		k.tile_wgs = 1;                                                             // SK_TILE_WGS instead of the cap
		p = pick(8, 8, 8, 3);
		CHECK(p.nw == 4 && p.wg == 1);
		k.tile_wgs = 5;
		p = pick(8, 8, 8, 2);
		CHECK(p.nw == 4 && p.wg == 5);
		p = pick(3, 8, 8, 2);                                                       // never above the answer: 12, 10, 5
		CHECK(p.nw == 4 && p.wg == 3);
	}
	CASE("grid = min(ceil(units / waves), n_cu * wg)");
	CHECK(grid_for(1000, 4, 1, 2) == 2 && grid_for(1000, 4, 3, 3) == 9 && grid_for(1000, 4, 256, 2) == 250 && grid_for(1001, 4, 256, 2) == 251);
	CHECK(grid_for(1, 4, 1, 2) == 1 && grid_for(1, 16, 256, 1) == 1 && grid_for(5, 4, 1, 1) == 1 && grid_for(5, 4, 3, 1) == 2);
	CHECK(grid_for(100000, 16, 256, 1) == 256 && grid_for(100000, 16, 3, 1) == 3 && grid_for(100000, 16, 1, 1) == 1 && grid_for(4095, 16, 256, 1) == 256 && grid_for(4080, 16, 256, 1) == 255);
	CHECK(grid_for((int64_t)1 << 30, 1, 256, 8) == 2048);
	CHECK(units(70001, 64) == 1094 && units(64, 64) == 1 && units(65, 64) == 2);
	{
		Shape s = demux_alone(70001, 8, 2, 0, 1023);
		CHECK(lookup_units(s) == 274);                                              // steps of 256 rows
		s.many = true; s.many_quads = 5000;                                         // a many-batch launch: its own count of steps
		CHECK(lookup_units(s) == 5000);
		s.many = false;
		CHECK(drops_count_rep(512, s) && !drops_count_rep(513, s) && drops_count_rep(1, s));
		s.counts_wide = true;
		CHECK(drops_count_rep(513, s) && drops_count_rep(100000, s));
	}
}

// ---- sweep ----------------------------------------------------------------------------------------------------------------------------
// the instantiations of the lookup kernels that exist (sk_kernels.hip: demux_fn), written out
static std::set<uint32_t> existing()
{
	std::set<uint32_t> e;
	auto add = [&](Family f, int W1, int W2, bool direct, bool ldstab, bool detail, bool pair, bool many) {
		KernelId id; id.family = f; id.W1 = W1; id.W2 = W2; id.direct = direct; id.ldstab = ldstab; id.detail = detail; id.pair = pair; id.many = many;
		if (!e.insert(id.key()).second) { fprintf(stderr, "two kernels share a key\n"); exit(1); }
	};
	add(kNoLaunch, 0, 0, false, false, false, false, false);
	add(kMatcherTile, 0, 0, false, false, false, false, false);
	for (int ldstab = 0; ldstab < 2; ldstab++)
		for (int detail = 0; detail < 2; detail++) {
			add(kLookup, 1, 0, true, ldstab, detail, false, false);
			add(kLookup, 2, 0, true, ldstab, detail, false, false);
			add(kLookup, 1, 1, false, ldstab, detail, false, false);
			add(kLookup, 2, 2, false, ldstab, detail, false, false);
			for (int W1 = 1; W1 <= 5; W1++) add(kLookup, W1, 0, false, ldstab, detail, false, false);
			add(kLookup8x2, 0, 0, false, ldstab, detail, false, false);
		}
	for (int detail = 0; detail < 2; detail++) {
		add(kLookup, 1, 1, false, true, detail, true, false);
		add(kLookup, 2, 2, false, true, detail, true, false);
		add(kLookup, 2, 2, false, true, detail, true, true);
		add(kLookup, 2, 2, false, true, detail, false, true);
		add(kLookup8x2, 0, 0, false, true, detail, false, true);
	}
	return e;      // 2 + 4 * 10 + 2 * 5 = 52 keys, 50 of them kernels
}

static void test_sweep()
{
	CASE("sweep");
	const std::set<uint32_t> exist = existing();
	CHECK(exist.size() == 52);
	struct Sheet { int S, G; bool bitsliced; int matcher_bytes; };
	const Sheet sheets[] = {{96, 3, true, 1000}, {160, 5, true, 9000}, {96, 3, false, 96 * 8}, {1021, 32, false, 1021 * 17}};
	struct Table { bool full, pair; int W1, W2, mask_slots, pair_bytes; };
	const Table tables[] = {{false, false, 0, 0, 0, 0}, {true, false, 1, 0, 511, 0}, {true, false, 2, 0, 1023, 0}, {true, false, 3, 0, 4095, 0},
	                        {true, false, 2, 2, 8191, 0}, {true, false, 5, 0, 16383, 0}, {false, true, 1, 1, 0, 30000}, {false, true, 2, 2, 0, 120000}};
	const bool mates[][4] = {{false, false, false, false}, {false, true, false, false}, {true, true, false, false}, {true, true, true, true}};      // mask0, trim0, mask1, trim1
	long plans = 0;
	for (int64_t n : {(int64_t)1, (int64_t)1499999, (int64_t)1500000, (int64_t)4000000})
	for (const auto &mt : mates)
	for (int stride : {150, 961})
	for (int bc_stride : {0, 8, 12, 17, 32, 33})                                    // 0: no barcodes
	for (int detail = 0; detail < 2; detail++)
	for (int matched = 0; matched < 2; matched++)
	for (int many = 0; many < 2; many++)
	for (int n_cu : {3, 256})
	for (const Sheet &sh : sheets)
	for (const Table &tb : tables) {
		if (bc_stride == 0 && (detail || matched || many || tb.full || tb.pair || sh.S != 96)) continue;      // one call without barcodes will do
		if (matched && !detail) continue;                                           // (the mode says nothing without a detail column)
		if (n_cu == 3 && (n != 1500000 || sh.S != 96)) continue;                    // (the CU count enters the mate pass's cap alone)
		Shape s;
		s.n = n; s.stride = stride; s.n_cu = n_cu;
		s.mask[0] = mt[0]; s.trim[0] = mt[1]; s.mask[1] = mt[2]; s.trim[1] = mt[3];
		s.has_bc = bc_stride != 0; s.bc_stride = bc_stride;
		s.lowest_diff = s.first_idx = s.last_idx = detail != 0; s.detail_matched = matched != 0;
		s.many = many != 0; s.many_quads = many ? (int)((n + 255) / 256) : 0;
		s.S = sh.S; s.G = sh.G; s.bitsliced = sh.bitsliced; s.matcher_bytes = sh.matcher_bytes;
		s.full_key = tb.full; s.factored = tb.pair; s.W1 = tb.W1; s.W2 = tb.W2; s.mask_slots = tb.mask_slots; s.pair_bytes = tb.pair_bytes;
		for (int direct : {-1, 0})
		for (int ldstab : {-1, 0})
		for (int rows2 : {-1, 0, 1})
		for (int bits = 0; bits < 16; bits++)
		for (int lut_nw : {0, 8}) {
			Knobs k;
			k.demux_direct = direct; k.demux_ldstab = ldstab; k.demux_rows2 = rows2; k.lut_nw = lut_nw;
			k.no_hash_demux = bits & 1; k.no_fused_demux = bits & 2; k.lut_many_gather = bits & 4; k.tile_waves = (bits & 8) ? 2 : 0;
			const DemuxPlan p = demux_plan(k, s);
			const MatePlan m = mate_plan(k, s);
			plans++;
			CHECK(exist.count(p.id.key()) == 1);
			const bool lut = p.id.family == kLookup || p.id.family == kLookup8x2;
			if (lut) {
				CHECK(p.lds <= 160 * 1024 && p.lds == p.lp.tiles_off + p.nw * p.lp.tile_slot);
				CHECK(p.nw >= 1 && 64 * p.nw <= (p.id.ldstab ? 1024 : 256));
				CHECK(p.wg(1) >= 1);
			}
			CHECK(!p.many_ok || (lut && p.id.ldstab));
			CHECK(p.id.many == (s.many && p.many_ok));
			// the barcodes are matched exactly once: in the tile pass or by a launch of their own
			CHECK((p.id.family != kNoLaunch) == (s.has_bc && !(m.tiles && m.demux)));
			CHECK(m.demux == fuses_demux(k, s) && (!m.demux || m.tiles));
			CHECK(m.fallback == (any_mate(s) && stride == 961) && m.tiles == (any_mate(s) && stride != 961));
			// wants_neighbour_table against demux_by_table, for a launch of the barcodes' own when a table exists: a call that goes by the
			// table has asked for it; and one that asked goes by it unless the pitch (64 rows above 2 048 bytes) or SK_NO_HASH_DEMUX
			// keeps the launch from the table (ensure_neighbour_table builds none under that knob)
			if ((tb.full || tb.pair) && p.id.family != kNoLaunch) {
				CHECK(!demux_by_table(k, s) || wants_neighbour_table(k, s));
				CHECK(demux_by_table(k, s) == (wants_neighbour_table(k, s) && bc_stride <= 32 && !k.no_hash_demux));
				CHECK(lut == demux_by_table(k, s));
			}
			if (p.id.family == kNoLaunch) CHECK(!wants_neighbour_table(k, s));
			if (m.tiles || p.id.family == kMatcherTile) {
				// the tile kernels are compiled for 256 threads: every candidate of the search fits them and the LDS
				const LdsPlan lp = m.tiles ? tile_lds(m.demux, s.matcher_bytes, s.S, 64 * m.row_bytes) : tile_lds(true, s.matcher_bytes, s.S, 64 * s.bc_stride);
				const Candidates c = tile_candidates(k, lp, 4);
				CHECK(c.n >= 1);
				for (int i = 0; i < c.n; i++) CHECK(c.lds[i] <= 160 * 1024 && 64 * c.nw[i] <= 256 && c.lds[i] == lp.tiles_off + c.nw[i] * lp.tile_slot);
				if (m.tiles) CHECK(m.max_wg >= 2 && m.max_wg <= 4 && (m.slots == 2 || m.slots == 4 || m.slots == 10));
			}
		}
	}
	CHECK(plans > 5000000);
}

int main()
{
	test_lookup_choice();
	test_many();
	test_by_table_and_fusing();
	test_mate_pass();
	test_layout_search_grid();
	test_sweep();
	printf("ok: %ld cases, %ld checks\n", g_cases, g_checks);
	return 0;
}
