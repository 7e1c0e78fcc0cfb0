// sk_tileplan.h — the launch decisions of the fused tile pass and the demultiplex kernels, each stated once: does the barcode phase
// ride in the tile pass, does the sheet's lookup table serve a launch of its own, which kernel runs, with how many waves, what LDS
// layout and what grid, and the slots and workgroup cap of the mate pass.  Pure arithmetic on plain facts (Knobs: the SK_* tuning
// variables as read; Shape: the call): no HIP, no heap, no getenv — it runs on every launch of the command-line hosts' small batches.
// sk_kernels.hip reads the environment, builds the Shape, asks here, maps the kernel id to a function and makes the occupancy query;
// sk_capi_fused.cpp asks the same functions what a call needs.  tests/cpp/tileplan_test.cpp holds every rule to expectations written out
// by hand, on the CPU.
#pragma once
#include <stdint.h>

namespace sk {

constexpr int kWave = 64;             // gfx950 wavefront; one read tile = 64 reads = one wave
constexpr int kTileRows = 64;
constexpr int kLdsPad = 16;           // bytes kept free before and after the LDS tile image
constexpr int kMaxTileStride = 960;   // 64 rows x 960 B + pads + histogram <= 64 KiB of LDS
constexpr int kMaxLdsHist = 1024;     // per-wave LDS histogram entries (S+3) before falling back to global atomics
constexpr int kLdsPerCu = 160 * 1024; // what one workgroup may be given of a gfx950 CU's LDS
#ifndef SK_SLOTS
#define SK_SLOTS 2
#endif
#ifndef SK_SLOTS1
#define SK_SLOTS1 4
#endif
constexpr int kSlots = SK_SLOTS;      // 1 KiB chunk loads in flight per wave and stream
constexpr int kSlotsTrim = 10;        // ... of the trim-alone pass

// where a tile kernel finds its pieces in the workgroup's LDS (a kernel argument)
struct LdsPlan {
	int table_bytes;     // matcher tables (bit-sliced blob, one-hot codes or raw sheet bytes), rounded to 16
	int hist_off;        // u32[S+3]
	int tiles_off;       // first wave's tile slot (includes the front pad)
	int tile_slot;       // bytes per wave: front pad + 64*row_bytes rounded to 16 + back pad
	int use_lds_hist;
};

namespace tileplan {

// The SK_* variables the decisions read, as sk_kernels.hip: tile_knobs() found them.  0 / false / -1 = unset.
struct Knobs {
	int tile_waves = 0, tile_wgs = 0;        // SK_TILE_WAVES, SK_TILE_WGS (tools/ablate.py, tools/waves_exp.py)
	bool no_fused_demux = false;             // SK_NO_FUSED_DEMUX (tests, tools)
	bool no_hash_demux = false;              // SK_NO_HASH_DEMUX
	int demux_direct = -1, demux_ldstab = -1, demux_rows2 = -1;      // SK_DEMUX_DIRECT / _LDSTAB / _ROWS2: 0 / 1 force the form (the tests run every kernel on the same inputs)
	bool lut_many_gather = false;            // SK_LUT_MANY_GATHER=1
	int lut_nw = 0, lut_wg = 0;              // SK_LUT_NW, SK_LUT_WG (tools/lut_cold_ab.py)
};

// One call, as plain facts.
struct Shape {
	int64_t n = 0;                           // rows; of a many-batch launch the rows of all batches, each rounded up to 256
	bool mask[2] = {false, false}, trim[2] = {false, false};      // per mate: out_seq / lowest_k asked for
	int stride = 0;
	bool has_bc = false;
	int bc_stride = 0;
	bool lowest_diff = false, first_idx = false, last_idx = false;      // the detail columns asked for
	bool detail_matched = false;             // SK_DETAIL_MATCHED: the detail columns of unmatched rows are unspecified
	bool counts_wide = false;                // the lookup kernels add to the ctx's wide counters
	bool many = false;                       // many batches in one launch ...
	int many_quads = 0;                      // ... and its steps of 256 rows
	int n_cu = 0;
	// the sheet
	int S = 0, G = 0;
	bool bitsliced = false;                  // the bit-sliced blob serves the matchers (else the one-hot codes, else the raw bytes) ...
	int matcher_bytes = 0;                   // ... and the bytes of whichever does
	bool full_key = false;                   // a full-key lookup table exists ...
	int W1 = 0, W2 = 0, mask_slots = 0;      // ... its key dwords (also of the factored form) and slots per table - 1
	bool factored = false;                   // or the factored form ...
	int pair_bytes = 0;                      // ... and the bytes of its blob
};

inline bool any_mate(const Shape &s) { return s.mask[0] || s.trim[0] || s.mask[1] || s.trim[1]; }
inline bool want_detail(const Shape &s) { return s.lowest_diff || s.first_idx || s.last_idx; }
inline int64_t units(int64_t n, int rows) { return (n + rows - 1) / rows; }

// rows that do not fit an LDS tile: trim falls back to the row-per-thread kernel, mask to the flat one; they fuse nothing
inline bool long_rows(const Shape &s) { return any_mate(s) && s.stride > kMaxTileStride; }

// ONE statement of when the barcode phase rides in the tile pass: the launcher decides with it, and the C-ABI layer asks it (through
// wants_neighbour_table) whether a call needs the neighbourhood table built.  The bit-sliced matcher applies (S <= 128) and the
// tile's barcodes fit two 1 KiB register chunks; otherwise the phase is a launch of its own beside the mate pass.
inline bool fuses_demux(const Knobs &k, const Shape &s)
{
	return s.has_bc && any_mate(s) && s.stride <= kMaxTileStride && s.bitsliced && s.G <= 4 && s.S > 0 && kTileRows * s.bc_stride <= 2048 && !k.no_fused_demux;
}

// does a barcode-phase launch take the sheet's lookup table (one lookup per read)?  The sheet has one and the call wants the decision
// alone, or the detail columns of matched rows only.
inline bool demux_by_table(const Knobs &k, const Shape &s)
{
	return (s.full_key || s.factored) && (!want_detail(s) || s.detail_matched) && kTileRows * s.bc_stride <= 2048 && !k.no_hash_demux;
}

// must the neighbourhood table be built before this call is launched?  A call that does not fuse takes the table for its barcode
// launch; were this and demux_by_table to disagree, no table would be there and the S x L matchers would run instead: correct,
// 10-50 x slower.
inline bool wants_neighbour_table(const Knobs &k, const Shape &s)
{
	return s.has_bc && !fuses_demux(k, s) && (!want_detail(s) || s.detail_matched);
}

// ---- the barcode phase as a launch of its own -------------------------------------------------------------------------------------
enum Family : uint8_t {
	kNoLaunch,       // no barcodes, or the phase rides in the tile pass
	kMatcherTile,    // demux_tile_kernel: the matchers (bit-sliced, one-hot, byte compare), a tile of rows in LDS
	kLookup,         // demux_lut_kernel<W1, W2, DIRECT, LDSTAB, DETAIL, PAIR, MANY>
	kLookup8x2,      // demux_lut8x2_kernel<LDSTAB, DETAIL, MANY>
};
struct KernelId {
	Family family = kNoLaunch;
	int W1 = 0, W2 = 0;                      // the template's key dwords (kLookup)
	bool direct = false, ldstab = false, detail = false, pair = false, many = false;
	constexpr uint32_t key() const
	{
		return (uint32_t)family | (uint32_t)W1 << 2 | (uint32_t)W2 << 5 | (uint32_t)direct << 8 | (uint32_t)ldstab << 9 | (uint32_t)detail << 10 | (uint32_t)pair << 11 | (uint32_t)many << 12;
	}
};

struct DemuxPlan {
	KernelId id;
	bool many_ok = false;                    // one launch serves a many-batch call of this shape
	// the lookup kernels' launch (kMatcherTile goes through the shape search below)
	int nw = 0;
	LdsPlan lp{};
	int lds = 0;
	int max_wg = 0, force_wg = 0;            // workgroups per CU: a cap on the occupancy answer (0: none), or SK_LUT_WG's value instead of it
	int wg(int occupancy) const { return force_wg >= 1 ? force_wg : (max_wg > 0 && occupancy > max_wg) ? max_wg : occupancy; }
};

inline DemuxPlan demux_plan(const Knobs &k, const Shape &s)
{
	DemuxPlan p;
	if (!s.has_bc || fuses_demux(k, s)) return p;
	// the sheet has a neighbourhood table and the call wants the decision alone, or the detail columns of matched rows
	// only (detail_matched): one lookup per read
	if (!demux_by_table(k, s)) { p.id.family = kMatcherTile; return p; }      // (many batches in one launch: the table's kernels only)
	const bool detail = want_detail(s);
	// rows on dword boundaries whose key is one or two dwords: lane r loads row r as it lies (one 8 B/lane load for 8-byte
	// rows); every other shape gathers (demux_lut_kernel).  (SK_DEMUX_DIRECT=0 / SK_DEMUX_LDSTAB=0 force the other forms:
	// the tests run every kernel on the same inputs)
	const bool pair = s.factored;                                 // the factored form (sk_lut.h): its three tables always in LDS
	const bool direct = !pair && (s.bc_stride & 3) == 0 && s.W2 == 0 && s.W1 <= 2 && 4 * s.W1 <= s.bc_stride && k.demux_direct != 0;
	const int table_bytes = pair ? s.pair_bytes : (s.mask_slots + 1) * 2 * 8;
	const bool ldstab = pair || (table_bytes <= (128 << 10) && k.demux_ldstab != 0);
	// rows of exactly 8 key bytes on an 8-byte pitch: two rows per lane (demux_lut8x2_kernel) — always when the detail columns
	// are written too, and for the decision alone from 1.5 M rows (after round 4's instruction diet: 10 M rows 20.4 us
	// against 23.6 with one row per lane, 2 M 8.3 / 9.5, 6 M 14.6 / 16.9, 100 M the same; 1 M 7.8 / 7.3: a workgroup's
	// first tile is its whole share there).  SK_DEMUX_ROWS2=0 / 1 force the choice (tools/demux_ab.py, tests).
	const bool rows2 = direct && s.W1 == 2 && s.bc_stride == 8 && (k.demux_rows2 >= 0 ? k.demux_rows2 != 0 : (detail || s.n >= 1500000));
	KernelId &id = p.id;
	id.ldstab = ldstab; id.detail = detail;
	if (pair) { id.family = kLookup; id.W1 = id.W2 = s.W1 == 1 ? 1 : 2; id.pair = true; }
	else if (rows2) id.family = kLookup8x2;
	else if (direct) { id.family = kLookup; id.W1 = s.W1 == 1 ? 1 : 2; id.direct = true; }
	else if (s.W2 > 0) { id.family = kLookup; id.W1 = id.W2 = s.W1 == 1 ? 1 : 2; }
	else { id.family = kLookup; id.W1 = s.W1 >= 1 && s.W1 <= 4 ? s.W1 : 5; }
	// many batches in one launch: the two kernels that serve the benchmark's sheets have the form; any other shape is the caller's loop
	// (the gathered-row kernel has the form too and keeps it for A/B — SK_LUT_MANY_GATHER=1 — but its many-batch launch is SLOWER than its
	// launches back to back, which is what the caller's loop does: 96 dual-index, 4 x 10 M rows from HBM, 0.51 of the HBM peak against 0.56)
	p.many_ok = ldstab && (rows2 || (k.lut_many_gather && !direct && s.W1 == 2 && s.W2 == 2));
	id.many = s.many && p.many_ok;
	LdsPlan &lp = p.lp;
	lp.use_lds_hist = 1;                                          // S + 3 <= kMaxLdsHist
	lp.hist_off = 0;
	lp.table_bytes = ldstab ? table_bytes : 0;
	lp.tiles_off = (((s.S + 3) * 4 + 15) & ~15) + lp.table_bytes;
	lp.tile_slot = 4 * kTileRows * 4;                             // rows come straight from memory: no image; 1 KiB per wave in which a quad's codes change lanes
	// sixteen waves share a table copy; eight once the call is long and the table leaves room for one workgroup per CU only
	// (rows from HBM, 100 M pairs of the 96 dual-index sheet: 381 us against 398; shorter calls want the waves)
	int nw = ldstab ? ((lp.table_bytes > (64 << 10) && s.n >= 4000000) ? 8 : 16) : 4;
	// tuning knobs (tools/lut_cold_ab.py); the kernels that keep their table in the vector cache are compiled for 256 threads, so
	// they take 4 waves at most
	if (k.lut_nw >= 1 && k.lut_nw <= (ldstab ? 16 : 4)) nw = k.lut_nw;
	while (nw > 4 && lp.tiles_off + nw * lp.tile_slot > kLdsPerCu) nw >>= 1;
	p.nw = nw;
	p.lds = lp.tiles_off + nw * lp.tile_slot;
	// sixteen waves per CU whatever the table leaves room for: with its rows coming from HBM a 10 M-row call of the cfg 3 sheet
	// took 25.3 us on sixteen and 26.7 on thirty-two (each wave's first load is a full HBM round trip before anything
	// moves, and twice the waves end in twice the stragglers); 100 M rows the same (tools/lut_cold_ab.py)
	p.max_wg = ldstab ? 1 : 0;
	p.force_wg = k.lut_wg >= 1 ? k.lut_wg : 0;
	return p;
}

// a persistent grid: a workgroup of nw waves takes nw units at a time, and no more workgroups than are resident (wg per CU)
inline int64_t grid_for(int64_t n_units, int nw, int n_cu, int wg)
{
	const int64_t want = (n_units + nw - 1) / nw, cap = (int64_t)n_cu * wg;
	return want < cap ? want : cap;
}
// a lookup wave's unit: 256 rows in either kernel
inline int64_t lookup_units(const Shape &s) { return s.many ? (int64_t)s.many_quads : units(s.n, 4 * kTileRows); }
// a few hundred workgroups add to the counters directly; thousands go through the spread copies and the fold
inline bool drops_count_rep(int64_t grid, const Shape &s) { return grid <= 512 || s.counts_wide; }

// ---- the mate pass ---------------------------------------------------------------------------------------------------------------
// Shape of the phase kernel: workgroups of four waves, and how many of them a CU holds depends on what the pass is
// bound by (tools/waves_exp.py, tools/small_n.py; same buffers, one process):
//  * two mates, streaming-bound: TWO per CU (eight resident waves).  More waves keep more requests in flight than
//    HBM serves well: 62.5 M clusters 9.52 ms with 16 waves, 9.31 ms with 8; at 16 M clusters +5 % for the fused
//    pass, +14 % for mask + trim of two mates.  Short inputs (fewer than 16 tiles per wave) take three, to shorten
//    the tail: 1 M clusters 176 -> 160 us;
//  * one mate with the mask: three (1 M reads 101 -> 89 us, no difference at 16 M);
//  * trim alone, bound by the scan's VALU work: four (16 M reads of full-length scans 1.19 -> 0.80 ms).
inline int two_mate_wg(int64_t n, int n_cu) { return units(n, kTileRows) < (int64_t)n_cu * 4 * 2 * 16 ? 3 : 2; }

struct MatePlan {
	bool fallback = false;   // long_rows: the flat mask and the row-per-thread trim, mate by mate
	bool tiles = false;      // tile_pass_kernel<MODE, demux, slots> runs
	bool demux = false;      // ... with the barcode phase in it (the matcher tables staged in LDS)
	int slots = 0;           // chunks in flight per stream
	int row_bytes = 0;       // of the wave's LDS image
	int max_wg = 0;          // workgroups per CU at most
};

inline MatePlan mate_plan(const Knobs &k, const Shape &s)
{
	MatePlan p;
	if (!any_mate(s)) return p;
	if (long_rows(s)) { p.fallback = true; return p; }
	p.tiles = true;
	p.demux = fuses_demux(k, s);
	if (s.trim[0] || s.trim[1]) p.row_bytes = s.stride;           // only the trim scan needs the LDS image
	if (p.demux && s.bc_stride > p.row_bytes) p.row_bytes = s.bc_stride;      // the barcode phase puts the tile's barcodes into the wave's LDS slot
	// One mate = two read streams at most: keep four chunks per stream in flight instead of two (mask + trim of one
	// mate 4.9 -> 5.1 TB/s at 16 M x 150; no gain with two mates or the barcode phase).  Trim alone reads ONE stream and
	// spends most of its time in the scan: there the whole next tile (ten chunks at 150 bp) is kept in flight
	// (3.6 -> 3.9 -> 4.3 TB/s with 2 / 4 / 10 slots on read-like qualities).
	const int active = ((s.mask[0] || s.trim[0]) ? 1 : 0) + ((s.mask[1] || s.trim[1]) ? 1 : 0);
	const bool any_mask = s.mask[0] || s.mask[1];
	if (p.demux || active == 2) { p.slots = kSlots; p.max_wg = two_mate_wg(s.n, s.n_cu); }
	else if (!any_mask) { p.slots = kSlotsTrim; p.max_wg = 4; }
	else { p.slots = SK_SLOTS1; p.max_wg = 3; }
	return p;
}

// the tile-blocked pass (launch_tile_blocked): chunks in flight per stream — 2 / 3 / 4 measure the same on the two-mate pass
// (10.56-10.64 ms), 5 is slower —, the LDS image and the workgroup cap
inline int blocked_slots(int n_mates) { return n_mates == 1 ? SK_SLOTS1 : kSlots; }
inline int blocked_image(int stride, int slots, bool demux)
{
	const int nchunkp = (((kTileRows * stride + 1023) >> 10) + slots - 1) / slots * slots;
	const int image = nchunkp * 1024;                             // the LDS image takes whole chunks, trim or not
	return demux && image < 2048 ? 2048 : image;
}
inline int blocked_max_wg(int n_mates, int64_t n, int n_cu) { return n_mates == 1 ? 3 : two_mate_wg(n, n_cu); }

// ---- LDS layout + workgroup shape of a tile kernel (tile_pass_kernel, tile_blocked_kernel, demux_tile_kernel) ---------------------
// the grid comes from the occupancy API so that every workgroup of the persistent grid is resident (a queued workgroup would run
// its whole share of tiles late)
inline LdsPlan tile_lds(bool with_tables, int matcher_bytes, int S, int image_bytes /* per wave */)
{
	LdsPlan lp{};
	lp.table_bytes = with_tables ? (matcher_bytes + 15) & ~15 : 0;
	lp.use_lds_hist = (with_tables && S + 3 <= kMaxLdsHist) ? 1 : 0;
	lp.hist_off = lp.table_bytes;
	lp.tiles_off = (lp.hist_off + (lp.use_lds_hist ? (S + 3) * 4 : 0) + 15) & ~15;
	lp.tile_slot = kLdsPad + ((image_bytes + 15) & ~15) + kLdsPad;
	return lp;
}

// the workgroup sizes the search asks the occupancy API about: max_nw waves (or SK_TILE_WAVES's), halved down to one, those that fit
struct Candidates {
	int n = 0;
	int nw[4] = {0, 0, 0, 0}, lds[4] = {0, 0, 0, 0};
};
inline Candidates tile_candidates(const Knobs &k, const LdsPlan &lp, int max_nw)
{
	Candidates c;
	for (int nw = (k.tile_waves > 0 && k.tile_waves <= 8) ? k.tile_waves : max_nw; nw >= 1; nw >>= 1) {
		const int lds = lp.tiles_off + nw * lp.tile_slot;
		if (lds > kLdsPerCu) continue;
		c.nw[c.n] = nw; c.lds[c.n] = lds; c.n++;
	}
	return c;
}
// the choice among the occupancy answers (workgroups per CU, one per candidate): each capped by max_wg (0: none) or by SK_TILE_WGS's
// value instead, then the most resident waves; the first wins a tie.  nw == 0: nothing fits.
struct Pick { int nw = 0, wg = 0, lds = 0; };
inline Pick tile_pick(const Knobs &k, const Candidates &c, const int *occupancy, int max_wg)
{
	Pick best;
	for (int i = 0; i < c.n; i++) {
		int wg = occupancy[i];
		if (k.tile_wgs > 0) { if (wg > k.tile_wgs) wg = k.tile_wgs; }
		else if (max_wg > 0 && wg > max_wg) wg = max_wg;
		if (wg * c.nw[i] > best.wg * best.nw) { best.nw = c.nw[i]; best.wg = wg; best.lds = c.lds[i]; }
	}
	return best;
}

}  // namespace tileplan
}  // namespace sk
