// sk_capi_fused.cpp — the C-ABI of include/seqkit_hip.h, the fused pass: device and host forms, many batches in one call, placement
// tuning, tile-blocked batches, and the single-operation views of it.
#include "sk_ctx.h"

// ---- fused pass ------------------------------------------------------------------------------------
static int check_fused(sk_ctx *c, const sk_fused_args *a, bool dev)
{
	if (!a) return fail(c, SK_ERR_INVALID, "args is NULL");
	if (a->n < 0) return fail(c, SK_ERR_INVALID, "n = %lld is negative", (long long)a->n);
	if (a->n_mates < 0 || a->n_mates > 2) return fail(c, SK_ERR_INVALID, "n_mates = %d outside 0..2", a->n_mates);
	bool any = false;
	for (int m = 0; m < a->n_mates; m++) {
		const sk_mate &mt = a->mate[m];
		if (!mt.out_seq && !mt.lowest_k) continue;
		any = true;
		if (a->stride <= 0 || a->stride > 65535) return fail(c, SK_ERR_INVALID, "stride = %d outside 1..65535", a->stride);
		if (!mt.qual) return fail(c, SK_ERR_INVALID, "mate %d: qual is NULL", m);
		if (mt.out_seq && !mt.seq) return fail(c, SK_ERR_INVALID, "mate %d: out_seq given without seq", m);
		if (dev && (!aligned16(mt.qual) || (mt.out_seq && (!aligned16(mt.seq) || !aligned16(mt.out_seq)))))
			return fail(c, SK_ERR_INVALID, "mate %d: device byte matrices must be 16-byte aligned", m);
	}
	if (a->bc) {
		if (!c->bar.have_table) return fail(c, SK_ERR_STATE, "sk_set_barcodes has not been called");
		if (a->bc_stride < c->bar.L || a->bc_stride <= 0) return fail(c, SK_ERR_INVALID, "bc_stride = %d is below the barcode length %d", a->bc_stride, c->bar.L);
		if (a->bc_stride > sk::kMaxTileStride) return fail(c, SK_ERR_INVALID, "bc_stride = %d above %d", a->bc_stride, sk::kMaxTileStride);
		if (!a->assign) return fail(c, SK_ERR_INVALID, "assign is NULL");
		if (dev && !aligned16(a->bc)) return fail(c, SK_ERR_INVALID, "bc must be 16-byte aligned");
		// the lookup kernels write a wave's 256 rows of every output column with ONE wide store per lane (16 bytes of assign, 4 of
		// lowest_diff, 8 of first_idx / last_idx): the columns' natural alignment is not enough for a device pointer
		if (dev && (!aligned16(a->assign) || ((uintptr_t)a->lowest_diff & 3u) || ((uintptr_t)a->first_idx & 7u) || ((uintptr_t)a->last_idx & 7u)))
			return fail(c, SK_ERR_INVALID, "device output columns: assign must be 16-byte, lowest_diff 4-byte, first_idx / last_idx 8-byte aligned");
	} else if (!any) {
		return fail(c, SK_ERR_INVALID, "nothing to do: no bc, no out_seq, no lowest_k");
	}
	return SK_OK;
}

static sk::TileArgs tile_args_of(const sk_ctx *c, const sk_fused_args *a)
{
	sk::TileArgs t;
	memset(&t, 0, sizeof t);
	t.n = a->n; t.n_mates = a->n_mates; t.stride = a->stride;
	t.qc = sk::make_qual_consts(a->min_baseq);
	for (int m = 0; m < a->n_mates; m++) {
		t.mate[m].seq = a->mate[m].seq; t.mate[m].qual = a->mate[m].qual; t.mate[m].len = a->mate[m].len;
		t.mate[m].out_seq = a->mate[m].out_seq; t.mate[m].lowest_k = a->mate[m].lowest_k;
	}
	t.bc = a->bc; t.bc_stride = a->bc_stride;
	if (a->bc) t.table = sk::table_of(c);
	t.assign = a->assign; t.lowest_diff = a->lowest_diff; t.first_idx = a->first_idx; t.last_idx = a->last_idx;
	t.detail_matched = c->detail_mode == SK_DETAIL_MATCHED ? 1 : 0;
	t.counts = a->counts ? (unsigned long long *)a->counts : c->bar.d_counts.get();
	t.counts_wide = a->counts ? nullptr : c->bar.d_counts_wide.get();
	t.counts_wide_rows = (t.counts_wide && c->bar.S + 3 > sk::kCountDenseFrom) ? sk::kCountDenseRows : 0;
	return t;
}

// demultiplex alone, with the decision only or the detail columns of matched rows only: the neighbourhood table's case — unless the
// pass matches in the tile pass itself (sk_tileplan.h: wants_neighbour_table states both).  Called with the ctx's device bound (the
// table is uploaded to the current device).
static int prepare_demux(sk_ctx *c, const sk::tileplan::Knobs &kn, sk::TileArgs &t)
{
	if (!t.bc || c->bar.nbr_tried) return SK_OK;       // (tried: the table is there, or the sheet has none)
	if (!sk::tileplan::wants_neighbour_table(kn, sk::tile_shape(t, c->n_cu))) return SK_OK;
	if (int r = sk::ensure_neighbour_table(c)) return r;
	t.table.nbr = c->bar.nbr;
	return SK_OK;
}
static int prepare_demux(sk_ctx *c, const sk::tileplan::Knobs &kn, const sk_fused_args *a)
{
	sk::TileArgs t = tile_args_of(c, a);
	return prepare_demux(c, kn, t);
}

static void one_mate(sk_fused_args &a, const uint8_t *seq, const uint8_t *qual, const uint16_t *len, int stride, int64_t n,
                     uint8_t min_baseq, uint8_t *out_seq, uint16_t *lowest_k)
{
	memset(&a, 0, sizeof a);
	a.n = n; a.n_mates = 1; a.stride = stride; a.min_baseq = min_baseq;
	a.mate[0].seq = seq; a.mate[0].qual = qual; a.mate[0].len = len; a.mate[0].out_seq = out_seq; a.mate[0].lowest_k = lowest_k;
}

static void demux_alone(sk_fused_args &a, const uint8_t *bc, int bc_stride, int64_t n, int32_t *assign, uint8_t *lowest_diff,
                        int16_t *first_idx, int16_t *last_idx, uint64_t *counts)
{
	memset(&a, 0, sizeof a);
	a.n = n; a.n_mates = 0; a.bc = bc; a.bc_stride = bc_stride; a.assign = assign;
	a.lowest_diff = lowest_diff; a.first_idx = first_idx; a.last_idx = last_idx; a.counts = counts;
}

extern "C" {

int sk_fused_pass_dev(sk_ctx *c, const sk_fused_args *a)
{
	if (!c) return SK_ERR_INVALID;
	if (int r = bind(c)) return r;          // first: what follows may upload the sheet's table to the current device
	if (int r = check_fused(c, a, true)) return r;
	if (a->n == 0) return SK_OK;
	const sk::tileplan::Knobs kn = sk::tile_knobs();
	sk::TileArgs t = tile_args_of(c, a);
	if (int r = prepare_demux(c, kn, t)) return r;
	if (t.bc && t.counts_wide) c->bar.wide_dirty = true;
	SK_HIP(c, sk::launch_tile_pass(t, kn, c->n_cu, c->stream));
	return SK_OK;
}

// Many independent batches in one call: every batch is checked, the sheet's table goes up once, and the launches
// follow each other on the ctx stream with nothing between them — what a host that has its batches at hand gets without a call,
// an argument check and an event per batch (bench.py: `frac_many` against `frac`, one event pair per call).
// Lookups of one shape (demultiplex alone, a table in LDS) run as ONE launch: the steps of all batches are dealt to the launch's
// waves, the table is staged once, the next batch's rows are fetched while the last of this one are looked up (ManyBatch,
// demux_lut8x2_kernel).  Measured before that (round 6, gpurun_out/r06_l): the batches dealt to four streams behind one fork event
// — SLOWER than one stream (10 M x 8 bp: 0.47 of the HBM peak against 0.58 per call and 0.62 back to back): two lookup kernels
// on a CU are thirty-two waves where sixteen stream best, and every batch pays two more events.
int sk_fused_pass_many_dev(sk_ctx *c, const sk_fused_args *batches, int n_batches)
{
	if (!c) return SK_ERR_INVALID;
	if (n_batches < 0 || (n_batches > 0 && !batches)) return fail(c, SK_ERR_INVALID, "n_batches = %d", n_batches);
	if (n_batches == 0) return SK_OK;
	if (int r = bind(c)) return r;
	for (int i = 0; i < n_batches; i++) if (int r = check_fused(c, &batches[i], true)) return r;
	const sk::tileplan::Knobs kn = sk::tile_knobs();
	// ONE launch for all of them when they are lookups of one shape: demultiplex alone into the ctx's counters, the same pitch and the
	// same set of output columns, served by a table in LDS (the plan says no for any other shape — sk_tileplan.h: many_ok —: the loop below)
	{
		bool same = n_batches >= 2;
		int64_t rows = 0;
		const sk_fused_args *first = nullptr;                            // the first batch that has rows
		for (int i = 0; i < n_batches && same; i++) {
			const sk_fused_args &a = batches[i], &f = batches[0];
			bool mates = false;
			for (int m = 0; m < a.n_mates; m++) mates = mates || a.mate[m].out_seq || a.mate[m].lowest_k;
			same = !mates && a.bc && !a.counts && a.bc_stride == f.bc_stride && !a.lowest_diff == !f.lowest_diff && !a.first_idx == !f.first_idx && !a.last_idx == !f.last_idx;
			rows += ((a.n + 255) / 256) * 256;
			if (!first && a.n > 0) first = &a;
		}
		if (const char *ev = getenv("SK_MANY_ONE_LAUNCH")) same = same && atoi(ev) != 0;      // (A/B: the batches' own launches instead)
		sk::TileArgs t;
		if (same && first && rows < ((int64_t)1 << 31) && n_batches <= kManyMax) {
			t = tile_args_of(c, first);
			if (int r = prepare_demux(c, kn, t)) return r;
			t.n = rows;
			sk::tileplan::Shape s = sk::tile_shape(t, c->n_cu);
			s.many = true; s.many_quads = (int)(rows / 256);
			same = sk::tileplan::demux_plan(kn, s).many_ok;
		} else same = false;
		if (same) {
			if (!c->many.pin) {
				SK_HIP(c, c->many.pin.alloc(kManySlots * kManyMax * sizeof(sk::ManyBatch), true));
				for (int k = 0; k < kManySlots; k++) SK_HIP(c, hipEventCreateWithFlags(&c->many.ev[k], hipEventDisableTiming));
			}
			const int slot = c->many.next++ % kManySlots;
			SK_HIP(c, hipEventSynchronize(c->many.ev[slot]));                // (the launch that read this slot eight calls ago: long done)
			sk::ManyBatch *hb = c->many.pin.get() + (size_t)slot * kManyMax;
			int64_t q0 = 0;
			int nb = 0;
			for (int i = 0; i < n_batches; i++) {
				const sk_fused_args &a = batches[i];
				if (a.n == 0) continue;
				const int64_t r0 = q0 * 256;
				sk::ManyBatch &m = hb[nb++];
				m.bc = a.bc - r0 * a.bc_stride;
				m.assign = a.assign - r0;
				m.lowest_diff = a.lowest_diff ? a.lowest_diff - r0 : nullptr;
				m.first_idx = a.first_idx ? a.first_idx - r0 : nullptr;
				m.last_idx = a.last_idx ? a.last_idx - r0 : nullptr;
				m.row_end = (uint32_t)(r0 + a.n);
				q0 += (a.n + 255) / 256;
				m.q_end = (int32_t)q0;
			}
			// (the kernel reads the descriptors where they lie, in pinned host memory: a wave reads one when its cursor moves to the next
			// batch — a copy of 200 bytes in front of the launch was 10 us on the stream, a tenth of what four batches take)
			t.many = hb; t.n_many = nb; t.many_quads = (int)q0;      // (t.n = q0 * 256, as the plan was asked)
			if (t.counts_wide) c->bar.wide_dirty = true;
			const hipError_t e = sk::launch_tile_pass(t, kn, c->n_cu, c->stream);
			SK_HIP(c, hipEventRecord(c->many.ev[slot], c->stream));
			if (e != hipSuccess) return fail(c, SK_ERR_HIP, "launch_tile_pass (many batches): %s", hipGetErrorString(e));
			return SK_OK;
		}
	}
	// batches without a barcode phase (trim / mask alone: nothing but their own outputs is written, no counters) alternate between the
	// ctx's two streams, so that one batch's last tiles and the next one's first share the chip: cfg 2's 1 M-read batches from HBM 39.0 ->
	// 31.5 us each = 0.49 -> 0.60 of the HBM peak (SK_MANY_TWO_STREAMS=0: one stream).  (Batches with a barcode phase stay on one stream:
	// their launches fold per-workgroup counter copies that the next launch is already adding to.)
	bool two = n_batches >= 2;
	int two_mode = 1;
	if (const char *ev = getenv("SK_MANY_TWO_STREAMS")) { two_mode = atoi(ev); two = two && two_mode != 0; }
	for (int i = 0; i < n_batches && two; i++) {
		if (batches[i].bc == nullptr) continue;
		// (A/B, SK_MANY_TWO_STREAMS=2: barcode-only batches whose launches take the lookup table and add to the ctx's wide counters)
		bool mates = false;
		for (int m = 0; m < batches[i].n_mates; m++) mates = mates || batches[i].mate[m].out_seq || batches[i].mate[m].lowest_k;
		if (two_mode < 2 || mates || batches[i].counts) { two = false; break; }
		sk::TileArgs t = tile_args_of(c, &batches[i]);
		if (int r = prepare_demux(c, kn, t)) return r;
		two = t.counts_wide != nullptr && sk::tileplan::demux_by_table(kn, sk::tile_shape(t, c->n_cu));
	}
	if (two) {
		SK_HIP(c, hipEventRecord(c->ev_pipe, c->stream));
		SK_HIP(c, hipStreamWaitEvent(c->stream2, c->ev_pipe, 0));
	}
	int k = 0;
	for (int i = 0; i < n_batches; i++) {
		const sk_fused_args *a = &batches[i];
		if (a->n == 0) continue;
		sk::TileArgs t = tile_args_of(c, a);
		if (int r = prepare_demux(c, kn, t)) return r;
		if (t.bc && t.counts_wide) c->bar.wide_dirty = true;
		SK_HIP(c, sk::launch_tile_pass(t, kn, c->n_cu, (two && (k & 1)) ? c->stream2 : c->stream));
		k++;
	}
	if (two) {
		SK_HIP(c, hipEventRecord(c->ev_pipe, c->stream2));
		SK_HIP(c, hipStreamWaitEvent(c->stream, c->ev_pipe, 0));
	}
	return SK_OK;
}

int sk_demux_assign_many_dev(sk_ctx *c, const sk_demux_batch *b, int n_batches, int bc_stride)
{
	if (!c) return SK_ERR_INVALID;
	if (n_batches < 0 || (n_batches > 0 && !b)) return fail(c, SK_ERR_INVALID, "n_batches = %d", n_batches);
	std::vector<sk_fused_args> v((size_t)n_batches);
	for (int i = 0; i < n_batches; i++) {
		if (!b[i].bc && b[i].n > 0) return fail(c, SK_ERR_INVALID, "batch %d: bc is NULL", i);
		demux_alone(v[(size_t)i], b[i].bc, bc_stride, b[i].n, b[i].assign, b[i].lowest_diff, b[i].first_idx, b[i].last_idx, nullptr);
	}
	return sk_fused_pass_many_dev(c, v.data(), n_batches);
}

int sk_trim_by_quality_many_dev(sk_ctx *c, const sk_trim_batch *b, int n_batches, int stride, uint8_t min_baseq)
{
	if (!c) return SK_ERR_INVALID;
	if (n_batches < 0 || (n_batches > 0 && !b)) return fail(c, SK_ERR_INVALID, "n_batches = %d", n_batches);
	std::vector<sk_fused_args> v((size_t)n_batches);
	for (int i = 0; i < n_batches; i++) {
		if (b[i].n > 0 && !b[i].lowest_k) return fail(c, SK_ERR_INVALID, "batch %d: lowest_k is NULL", i);
		one_mate(v[(size_t)i], nullptr, b[i].qual, b[i].len, stride, b[i].n, min_baseq, nullptr, b[i].lowest_k);
	}
	return sk_fused_pass_many_dev(c, v.data(), n_batches);
}

// Host-pointer form: chunks of rows are staged through the device workspace.
int sk_fused_pass(sk_ctx *c, const sk_fused_args *a)
{
	if (!c) return SK_ERR_INVALID;
	if (int r = bind(c)) return r;
	if (int r = check_fused(c, a, false)) return r;
	if (a->n == 0) return SK_OK;
	const sk::tileplan::Knobs kn = sk::tile_knobs();
	if (int r = prepare_demux(c, kn, a)) return r;
	const int64_t stride = a->stride;
	sk_fused_args d = *a;                                      // the chunk on the device: every pointer below is set by stage_in()
	d.counts = nullptr;
	Stage cols;
	for (int m = 0; m < a->n_mates; m++) {
		const sk_mate &mt = a->mate[m];
		sk_mate &dm = d.mate[m];
		dm = sk_mate{nullptr, nullptr, nullptr, nullptr, nullptr};
		if (!mt.out_seq && !mt.lowest_k) continue;
		cols.add(dm.qual, stride, kIn, mt.qual);
		if (mt.out_seq) { cols.add(dm.seq, stride, kIn, mt.seq); cols.add(dm.out_seq, stride, kOut, mt.out_seq); }
		if (mt.len) cols.add(dm.len, 2, kIn, mt.len);
		if (mt.lowest_k) cols.add(dm.lowest_k, 2, kOut, mt.lowest_k);
	}
	if (a->bc) {                                               // (the budget counts the three detail columns whether they are asked for or not)
		cols.add(d.bc, a->bc_stride, kIn, a->bc);
		cols.add(d.assign, 4, kOut, a->assign);
		cols.add(d.lowest_diff, 1, kOut, a->lowest_diff);
		cols.add(d.first_idx, 2, kOut, a->first_idx);
		cols.add(d.last_idx, 2, kOut, a->last_idx);
	}
	ChunkPipe pipe(c, cols);
	if (int r = pipe.begin(a->n, cols.rows_for_bytes(pipe_chunk(kPipeChunkBytes), 64, a->n))) return r;
	for (; pipe.more(); pipe.next()) {
		d.n = pipe.nr;
		if (int r = pipe.stage_in()) return r;
		sk::TileArgs t = tile_args_of(c, &d);
		if (t.table.count_rep && (pipe.k & 1)) t.table.count_rep += c->bar.count_rep_set;     // the second lane's set of counter copies
		if (t.bc && t.counts_wide) c->bar.wide_dirty = true;
		SK_HIP(c, sk::launch_tile_pass(t, kn, c->n_cu, pipe.st()));
		if (int r = pipe.stage_out()) return r;
	}
	return pipe.end();
}

// ---- placement tuning -------------------------------------------------------------------------------------------
int sk_fused_tune_placement_dev(sk_ctx *c, sk_fused_args *a, const sk_fused_candidates *cd, int sweeps, float *ms_before, float *ms_after, int *n_probes)
{
	if (!c) return SK_ERR_INVALID;
	if (!a || !cd) return fail(c, SK_ERR_INVALID, "args or candidates is NULL");
	if (cd->k < 1 || cd->k > SK_MAX_CANDIDATES || sweeps < 0) return fail(c, SK_ERR_INVALID, "k = %d (1..%d), sweeps = %d", cd->k, SK_MAX_CANDIDATES, sweeps);
	if (int r = bind(c)) return r;
	if (int r = check_fused(c, a, true)) return r;
	const sk::tileplan::Knobs kn = sk::tile_knobs();
	if (int r = prepare_demux(c, kn, a)) return r;
	// the matrices that take part: those the pass uses and that have candidates
	struct Slot { int mate, what; };                       // what: 0 seq, 1 qual, 2 out_seq
	std::vector<Slot> slots;
	for (int m = 0; m < a->n_mates; m++) {
		const sk_mate &mt = a->mate[m];
		if (!mt.out_seq && !mt.lowest_k) continue;
		if (mt.out_seq && cd->seq[m][0]) slots.push_back({m, 0});
		if (cd->qual[m][0]) slots.push_back({m, 1});
		if (mt.out_seq && cd->out_seq[m][0]) slots.push_back({m, 2});
	}
	for (const Slot &sl : slots)
		for (int k = 0; k < cd->k; k++) {
			const void *p = sl.what == 0 ? (const void *)cd->seq[sl.mate][k] : sl.what == 1 ? (const void *)cd->qual[sl.mate][k] : (const void *)cd->out_seq[sl.mate][k];
			if (!p || !aligned16(p)) return fail(c, SK_ERR_INVALID, "candidate %d of mate %d is NULL or not 16-byte aligned", k, sl.mate);
		}
	unsigned long long *scratch = nullptr;                  // the probes count here, not into the caller's counters
	SK_HIP(c, hipMalloc((void **)&scratch, (size_t)(c->bar.S + 3) * 8 + 8));
	sk_fused_args t = *a;
	t.counts = (uint64_t *)scratch;
	std::vector<int> choice(slots.size(), 0);
	auto apply = [&](sk_fused_args &x, const std::vector<int> &ch) {
		for (size_t i = 0; i < slots.size(); i++) {
			sk_mate &mt = x.mate[slots[i].mate];
			if (slots[i].what == 0) mt.seq = cd->seq[slots[i].mate][ch[i]];
			else if (slots[i].what == 1) mt.qual = cd->qual[slots[i].mate][ch[i]];
			else mt.out_seq = cd->out_seq[slots[i].mate][ch[i]];
		}
	};
	int probes = 0;
	int rc = SK_OK;
	auto time_choice = [&](const std::vector<int> &ch, float &ms) -> int {
		apply(t, ch);
		sk::TileArgs ta = tile_args_of(c, &t);
		probes++;
		hipError_t e = sk::launch_tile_pass(ta, kn, c->n_cu, c->stream);             // warm
		if (e == hipSuccess) e = hipEventRecord(c->ev0, c->stream);
		for (int i = 0; i < 2 && e == hipSuccess; i++) e = sk::launch_tile_pass(ta, kn, c->n_cu, c->stream);
		if (e == hipSuccess) e = hipEventRecord(c->ev1, c->stream);
		if (e == hipSuccess) e = hipEventSynchronize(c->ev1);
		if (e == hipSuccess) e = hipEventElapsedTime(&ms, c->ev0, c->ev1);
		if (e != hipSuccess) return fail(c, SK_ERR_HIP, "placement probe: %s", hipGetErrorString(e));
		ms *= 0.5f;
		return SK_OK;
	};
	float best = 0.f;
	rc = time_choice(choice, best);
	const float first = best;
	for (int sw = 0; sw < sweeps && rc == SK_OK; sw++) {
		bool moved = false;
		for (size_t i = 0; i < slots.size() && rc == SK_OK; i++)
			for (int k = 0; k < cd->k && rc == SK_OK; k++) {
				if (k == choice[i]) continue;
				std::vector<int> trial = choice;
				trial[i] = k;
				float ms = 0.f;
				rc = time_choice(trial, ms);
				if (rc == SK_OK && ms < best * 0.998f) { best = ms; choice = trial; moved = true; }
			}
		if (!moved) break;
	}
	(void)hipStreamSynchronize(c->stream);
	(void)hipFree(scratch);
	if (rc != SK_OK) return rc;
	apply(*a, choice);
	if (ms_before) *ms_before = first;
	if (ms_after) *ms_after = best;
	if (n_probes) *n_probes = probes;
	return SK_OK;
}

// ---- tile-blocked batches ---------------------------------------------------------------------------------------
int sk_blocked_layout_init(sk_blocked_layout *lay, int n_mates, int stride, int bc_stride, int flags)
{
	if (!lay) return SK_ERR_INVALID;
	if (n_mates < 1 || n_mates > 2 || bc_stride < 0 || stride <= 0 || stride > 65535) return SK_ERR_INVALID;
	if (!(flags & (SK_BLK_MASK | SK_BLK_TRIM))) return SK_ERR_INVALID;      // barcodes alone: sk_demux_assign(_dev)
	memset(lay, 0, sizeof *lay);
	lay->n_mates = n_mates; lay->stride = stride; lay->bc_stride = bc_stride; lay->flags = flags;
	for (int m = 0; m < 2; m++) lay->in_qual[m] = lay->in_seq[m] = lay->in_len[m] = lay->out_seq[m] = lay->out_lowest_k[m] = -1;
	lay->in_bc = lay->out_assign = lay->out_lowest_diff = lay->out_first_idx = lay->out_last_idx = -1;
	int64_t in = 0, out = 0;
	auto seg = [](int64_t &at, int64_t bytes) { int64_t o = at; at += (bytes + 63) & ~(int64_t)63; return (int32_t)o; };
	for (int m = 0; m < n_mates; m++) {                       // streams first, in the order the kernel walks them
		lay->in_qual[m] = seg(in, 64 * (int64_t)stride);
		if (flags & SK_BLK_MASK) lay->in_seq[m] = seg(in, 64 * (int64_t)stride);
	}
	if (bc_stride > 0) lay->in_bc = seg(in, 64 * (int64_t)bc_stride);
	if (flags & SK_BLK_LEN) for (int m = 0; m < n_mates; m++) lay->in_len[m] = seg(in, 128);
	if (flags & ~(SK_BLK_MASK | SK_BLK_TRIM | SK_BLK_LEN | SK_BLK_DETAIL)) return SK_ERR_INVALID;
	if (flags & SK_BLK_MASK) for (int m = 0; m < n_mates; m++) lay->out_seq[m] = seg(out, 64 * (int64_t)stride);
	if (flags & SK_BLK_TRIM) for (int m = 0; m < n_mates; m++) lay->out_lowest_k[m] = seg(out, 128);
	if (bc_stride > 0) {
		lay->out_assign = seg(out, 256);
		if (flags & SK_BLK_DETAIL) { lay->out_lowest_diff = seg(out, 64); lay->out_first_idx = seg(out, 128); lay->out_last_idx = seg(out, 128); }
	}
	in = (in + 127) & ~(int64_t)127;                            // whole 128-byte lines: no line is shared by two tiles (two waves would fetch it)
	out = (out + 127) & ~(int64_t)127;
	if (in > 0x3fffffff || out > 0x3fffffff) return SK_ERR_INVALID;
	lay->in_block = (int32_t)in; lay->out_block = (int32_t)out;
	return SK_OK;
}

int sk_fused_pass_blocked_dev(sk_ctx *c, const sk_blocked_layout *lay, const uint8_t *in, uint8_t *out, int64_t n, uint8_t min_baseq, uint64_t *counts)
{
	if (!c) return SK_ERR_INVALID;
	if (!lay) return fail(c, SK_ERR_INVALID, "layout is NULL");
	if (n < 0) return fail(c, SK_ERR_INVALID, "n = %lld is negative", (long long)n);
	if (n == 0) return SK_OK;
	sk_blocked_layout want;
	if (sk_blocked_layout_init(&want, lay->n_mates, lay->stride, lay->bc_stride, lay->flags) != SK_OK || memcmp(&want, lay, sizeof want) != 0)
		return fail(c, SK_ERR_INVALID, "layout was not made by sk_blocked_layout_init");
	if (!in || !out || !aligned16(in) || !aligned16(out)) return fail(c, SK_ERR_INVALID, "in/out must be 16-byte aligned device buffers");
	if (lay->bc_stride > 0) {
		if (!c->bar.have_table) return fail(c, SK_ERR_STATE, "sk_set_barcodes has not been called");
		if (lay->bc_stride < c->bar.L) return fail(c, SK_ERR_INVALID, "bc_stride = %d is below the barcode length %d", lay->bc_stride, c->bar.L);
	}
	if (int r = bind(c)) return r;
	sk::BlockedArgs a;
	memset(&a, 0, sizeof a);
	a.in = in; a.out = out; a.n = n;
	a.n_mates = lay->n_mates; a.stride = lay->stride; a.bc_stride = lay->bc_stride;
	a.in_block = lay->in_block; a.out_block = lay->out_block;
	for (int m = 0; m < 2; m++) {
		a.in_qual[m] = lay->in_qual[m]; a.in_seq[m] = lay->in_seq[m]; a.in_len[m] = lay->in_len[m];
		a.out_seq[m] = lay->out_seq[m]; a.out_lowest_k[m] = lay->out_lowest_k[m];
	}
	a.in_bc = lay->in_bc; a.out_assign = lay->out_assign; a.out_lowest_diff = lay->out_lowest_diff;
	a.out_first_idx = lay->out_first_idx; a.out_last_idx = lay->out_last_idx;
	a.qc = sk::make_qual_consts(min_baseq);
	if (lay->bc_stride > 0) a.table = sk::table_of(c);
	a.counts = counts ? (unsigned long long *)counts : c->bar.d_counts.get();
	if (!sk::blocked_shape_ok(a)) return fail(c, SK_ERR_INVALID, "shape not served by the tile-blocked pass (stride %d, bc_stride %d, S %d): use sk_fused_pass_dev", lay->stride, lay->bc_stride, c->bar.S);
	SK_HIP(c, sk::launch_tile_blocked(a, c->n_cu, c->stream));
	return SK_OK;
}

// ---- single-operation entry points are thin views of the fused pass ----------------------------------
int sk_demux_assign_dev(sk_ctx *c, const uint8_t *bc, int bc_stride, int64_t n, int32_t *assign, uint8_t *lowest_diff,
                        int16_t *first_idx, int16_t *last_idx, uint64_t *counts)
{
	if (!c) return SK_ERR_INVALID;
	if (!bc && n > 0) return fail(c, SK_ERR_INVALID, "bc is NULL");
	sk_fused_args a;
	demux_alone(a, bc, bc_stride, n, assign, lowest_diff, first_idx, last_idx, counts);
	if (n == 0) return SK_OK;
	return sk_fused_pass_dev(c, &a);
}

int sk_demux_assign(sk_ctx *c, const uint8_t *bc, int bc_stride, int64_t n, int32_t *assign, uint8_t *lowest_diff,
                    int16_t *first_idx, int16_t *last_idx)
{
	if (!c) return SK_ERR_INVALID;
	if (!bc && n > 0) return fail(c, SK_ERR_INVALID, "bc is NULL");
	sk_fused_args a;
	demux_alone(a, bc, bc_stride, n, assign, lowest_diff, first_idx, last_idx, nullptr);
	if (n == 0) return SK_OK;
	return sk_fused_pass(c, &a);
}

int sk_trim_by_quality_dev(sk_ctx *c, const uint8_t *qual, const uint16_t *len, int stride, int64_t n, uint8_t min_baseq, uint16_t *lowest_k)
{
	if (!c) return SK_ERR_INVALID;
	if (n == 0) return SK_OK;
	if (!lowest_k) return fail(c, SK_ERR_INVALID, "lowest_k is NULL");
	sk_fused_args a;
	one_mate(a, nullptr, qual, len, stride, n, min_baseq, nullptr, lowest_k);
	return sk_fused_pass_dev(c, &a);
}

int sk_trim_by_quality(sk_ctx *c, const uint8_t *qual, const uint16_t *len, int stride, int64_t n, uint8_t min_baseq, uint16_t *lowest_k)
{
	if (!c) return SK_ERR_INVALID;
	if (n == 0) return SK_OK;
	if (!lowest_k) return fail(c, SK_ERR_INVALID, "lowest_k is NULL");
	sk_fused_args a;
	one_mate(a, nullptr, qual, len, stride, n, min_baseq, nullptr, lowest_k);
	return sk_fused_pass(c, &a);
}

int sk_mask_by_quality_dev(sk_ctx *c, const uint8_t *seq, const uint8_t *qual, int stride, int64_t n, uint8_t min_baseq, uint8_t *out_seq)
{
	if (!c) return SK_ERR_INVALID;
	if (n < 0 || stride <= 0) return fail(c, SK_ERR_INVALID, "n = %lld, stride = %d", (long long)n, stride);
	if (n == 0) return SK_OK;
	if (!seq || !qual || !out_seq) return fail(c, SK_ERR_INVALID, "seq, qual or out_seq is NULL");
	if (!aligned16(seq) || !aligned16(qual) || !aligned16(out_seq)) return fail(c, SK_ERR_INVALID, "device byte matrices must be 16-byte aligned");
	if (int r = bind(c)) return r;
	SK_HIP(c, sk::launch_mask_flat(seq, qual, out_seq, n * (int64_t)stride, sk::make_qual_consts(min_baseq), c->n_cu, c->stream));
	return SK_OK;
}

int sk_mask_by_quality(sk_ctx *c, uint8_t *seq, const uint8_t *qual, const uint16_t *len, int stride, int64_t n, uint8_t min_baseq)
{
	if (!c) return SK_ERR_INVALID;
	if (n < 0 || stride <= 0) return fail(c, SK_ERR_INVALID, "n = %lld, stride = %d", (long long)n, stride);
	if (n == 0) return SK_OK;
	if (!seq || !qual) return fail(c, SK_ERR_INVALID, "seq or qual is NULL");
	(void)len;   // pad bytes of the output are unspecified: the whole matrix is one byte stream
	if (int r = bind(c)) return r;
	const int64_t total = n * (int64_t)stride;
	uint8_t *ds, *dq, *dout;
	Stage cols;
	cols.add(ds, 1, kIn, seq); cols.add(dq, 1, kIn, qual); cols.add(dout, 1, kOut, seq);
	ChunkPipe pipe(c, cols);
	if (int r = pipe.begin(total, rows_per_chunk(pipe_chunk((size_t)16 << 20), 16, total))) return r;
	sk::QualConsts qc = sk::make_qual_consts(min_baseq);
	for (; pipe.more(); pipe.next()) {
		if (int r = pipe.stage_in()) return r;
		SK_HIP(c, sk::launch_mask_flat(ds, dq, dout, pipe.nr, qc, c->n_cu, pipe.st()));
		if (int r = pipe.stage_out()) return r;
	}
	return pipe.end();
}

}  // extern "C"
