// sk_capi_barcodes.cpp — the C-ABI of include/seqkit_hip.h, the barcode table and the counters: sk_set_barcodes and the tables it
// builds, the neighbourhood table built on first use, the detail mode, and the ctx's counters (sk_ctx.h: sk_ctx::Barcodes).
#include "sk_ctx.h"

extern "C" {

// ---- barcode table ---------------------------------------------------------------------------------
int sk_set_barcodes(sk_ctx *c, const uint8_t *table, int S, int L, int max_diff)
{
	if (!c) return SK_ERR_INVALID;
	if (S < 0 || S > SK_MAX_SAMPLES) return fail(c, SK_ERR_INVALID, "S = %d outside 0..%d", S, SK_MAX_SAMPLES);
	if (L < 0 || L > SK_MAX_BARCODE_LEN || (S > 0 && L == 0)) return fail(c, SK_ERR_INVALID, "L = %d outside 1..%d", L, SK_MAX_BARCODE_LEN);
	if (S > 0 && !table) return fail(c, SK_ERR_INVALID, "table is NULL");
	if (max_diff < 0 || max_diff > 255) return fail(c, SK_ERR_INVALID, "max_diff = %d outside 0..255", max_diff);
	if (int r = bind(c)) return r;
	SK_HIP(c, hipStreamSynchronize(c->stream));
	c->bar = sk_ctx::Barcodes{};           // (have_table is false until the last upload below is done)
	c->bar.S = S; c->bar.L = L; c->bar.max_diff = max_diff;
	c->bar.W = (L + 3) / 4;

	SK_HIP(c, c->bar.d_raw.alloc((size_t)S * L + 16));
	if (S > 0) SK_HIP(c, hipMemcpy(c->bar.d_raw.get(), table, (size_t)S * L, hipMemcpyHostToDevice));

	// one-hot re-coding: possible when every position uses <= 7 distinct non-wildcard bytes
	bool onehot_ok = S > 0 && L <= sk::kMaxOneHotLen && !getenv("SK_NO_ONEHOT");
	std::vector<uint8_t> lut((size_t)(L ? L : 1) * 256, 0x80);
	std::vector<uint32_t> codes((size_t)(S ? S : 1) * (c->bar.W ? c->bar.W : 1), 0u);
	for (int k = 0; k < L && onehot_ok; k++) {
		int cls[256];
		for (int b = 0; b < 256; b++) cls[b] = -1;
		int ncls = 0;
		for (int s = 0; s < S; s++) {
			uint8_t b = table[(size_t)s * L + k];
			if (b == 'N' || b == 'U') continue;                 // wildcards: src/fasta_demultiplex.rs:273
			if (cls[b] < 0) { if (ncls == 7) { onehot_ok = false; break; } cls[b] = ncls++; }
		}
		if (!onehot_ok) break;
		for (int b = 0; b < 256; b++) lut[(size_t)k * 256 + b] = (uint8_t)(0x80 | (cls[b] >= 0 ? (1 << cls[b]) : 0));
		for (int s = 0; s < S; s++) {
			uint8_t b = table[(size_t)s * L + k];
			uint32_t code = (b == 'N' || b == 'U') ? 0x80u : (1u << cls[b]);
			codes[(size_t)s * c->bar.W + (k >> 2)] |= code << (8 * (k & 3));
		}
	}
	if (onehot_ok) {
		SK_HIP(c, c->bar.d_lut.alloc(lut.size()));
		SK_HIP(c, hipMemcpy(c->bar.d_lut.get(), lut.data(), lut.size(), hipMemcpyHostToDevice));
		SK_HIP(c, c->bar.d_onehot.alloc(codes.size() * 4 + 64));
		SK_HIP(c, hipMemcpy(c->bar.d_onehot.get(), codes.data(), codes.size() * 4, hipMemcpyHostToDevice));
	}
	// bit-sliced matcher: possible when the whole sheet uses <= 7 distinct non-wildcard bytes and L <= 31
	{
		int cls[256];
		for (int b = 0; b < 256; b++) cls[b] = -1;
		int ncls = 0;
		bool ok = S > 0 && L <= sk::kMaxBitSlicedLen && !getenv("SK_NO_BITSLICE");
		for (int s = 0; s < S && ok; s++)
			for (int k = 0; k < L; k++) {
				uint8_t b = table[(size_t)s * L + k];
				if (b == 'N' || b == 'U') continue;
				if (cls[b] < 0) { if (ncls == 7) { ok = false; break; } cls[b] = ncls++; }
			}
		const int G = (S + 31) / 32;
		const int mm_off = 256 + ((G * 4 + 15) & ~15);
		const size_t bytes = (size_t)mm_off + (size_t)L * 8 * G * 4;
		if (ok && bytes <= (size_t)sk::kMaxBitSlicedBytes) {
			std::vector<uint8_t> blob(bytes, 0);
			for (int b = 0; b < 256; b++) blob[b] = (uint8_t)(cls[b] >= 0 ? cls[b] : 7);
			uint32_t *valid = (uint32_t *)(blob.data() + 256);
			uint32_t *mm = (uint32_t *)(blob.data() + mm_off);
			for (int s = 0; s < S; s++) {
				valid[s >> 5] |= 1u << (s & 31);
				for (int k = 0; k < L; k++) {
					uint8_t b = table[(size_t)s * L + k];
					if (b == 'N' || b == 'U') continue;                  // wildcard: never a mismatch
					for (int cc = 0; cc < 8; cc++)
						if (cc != cls[b]) mm[((size_t)k * 8 + cc) * G + (s >> 5)] |= 1u << (s & 31);
				}
			}
			SK_HIP(c, c->bar.d_bs.alloc(bytes));
			SK_HIP(c, hipMemcpy(c->bar.d_bs.get(), blob.data(), bytes, hipMemcpyHostToDevice));
			c->bar.bs_bytes = (int)bytes; c->bar.bs_mm_off = mm_off; c->bar.G = G;
		}
	}
	// (the neighbourhood table of the sheet is built on the first demultiplex-alone call it can serve: ensure_neighbour_table)
	c->bar.sheet.assign(table, table + (size_t)S * L);
	c->bar.nbr_tried = false;
	SK_HIP(c, c->bar.d_counts.alloc((size_t)(S + 3) * 8));
	SK_HIP(c, hipMemset(c->bar.d_counts.get(), 0, (size_t)(S + 3) * 8));
	if (S <= sk::kLutMaxSamples) {
		const size_t wide_bytes = S + 3 > sk::kCountDenseFrom ? (size_t)sk::kCountDenseRows * (S + 3) * 8
		                                                        : (((size_t)sk::kCountReplicas * (S + 3)) << sk::kCountWideShift) * 8;
		SK_HIP(c, c->bar.d_counts_wide.alloc(wide_bytes));
		SK_HIP(c, hipMemset(c->bar.d_counts_wide.get(), 0, wide_bytes));
	}
	if (S + 3 <= sk::kMaxLdsHist) {
		// two sets: the chunk pipeline of the host entry points has launches of its two lanes in flight together, and a
		// set serves one launch (the kernel and the fold behind it) at a time
		c->bar.count_rep_pitch = (S + 3 + 31) & ~31;                 // whole 256-byte pieces: no line is shared by two copies
		c->bar.count_rep_set = (size_t)sk::kCountReplicas * c->bar.count_rep_pitch;
		SK_HIP(c, c->bar.d_count_rep.alloc(2 * c->bar.count_rep_set * 8));
		SK_HIP(c, hipMemset(c->bar.d_count_rep.get(), 0, 2 * c->bar.count_rep_set * 8));
	}
	SK_HIP(c, hipDeviceSynchronize());     // the ctx stream is non-blocking: make the uploads visible to it
	c->bar.have_table = true;
	return SK_OK;
}

}  // extern "C"

// The neighbourhood table costs some host work per sheet (enumerate, decide, place): it is built when a call first
// asks for the decision alone or for the detail columns of matched rows only — a caller that always wants every row's
// detail (SK_DETAIL_FULL) never pays for it.  The caller has bound the ctx's device.
int sk::ensure_neighbour_table(sk_ctx *c)
{
	if (c->bar.nbr_tried || !c->bar.have_table) return SK_OK;
	c->bar.nbr_tried = true;
	sk::LutHost h;
	// (SK_DEMUX_PAIR=0: never the factored form — a table too large for the LDS is then probed through the vector cache; tests)
	const char *env_pair = getenv("SK_DEMUX_PAIR");
	const int lds_budget = (env_pair && atoi(env_pair) == 0) ? 0 : (128 << 10);
	if (getenv("SK_NO_HASH_DEMUX") || !sk::lut_build(c->bar.sheet.data(), c->bar.S, c->bar.L, c->bar.max_diff, h, lds_budget)) return SK_OK;
	const size_t slot_bytes = h.slots.size() * 4, amb_bytes = h.amb.size() * 2;
	SK_HIP(c, c->bar.d_nbr.alloc(slot_bytes + amb_bytes + 16));
	SK_HIP(c, hipMemcpy(c->bar.d_nbr.get(), h.slots.data(), slot_bytes, hipMemcpyHostToDevice));
	if (amb_bytes) SK_HIP(c, hipMemcpy(c->bar.d_nbr.get() + slot_bytes, h.amb.data(), amb_bytes, hipMemcpyHostToDevice));
	SK_HIP(c, hipDeviceSynchronize());     // the ctx streams are non-blocking: make the upload visible to them
	c->bar.nbr = h.dev;
	c->bar.nbr_keys = (int64_t)h.n_keys; c->bar.nbr_bytes = (int64_t)(slot_bytes + amb_bytes);
	if (h.dev.pair.bytes != 0) c->bar.nbr.pair.tab = reinterpret_cast<const uint32_t *>(c->bar.d_nbr.get());      // the factored form: three tables in one blob
	else c->bar.nbr.tab = reinterpret_cast<const uint32_t *>(c->bar.d_nbr.get());
	c->bar.nbr.amb = reinterpret_cast<const int16_t *>(c->bar.d_nbr.get() + slot_bytes);
	return SK_OK;
}

sk::BarcodeDev sk::table_of(const sk_ctx *c)
{
	sk::BarcodeDev t;
	t.raw = c->bar.d_raw.get(); t.onehot = c->bar.d_onehot.get(); t.lut = c->bar.d_lut.get();
	t.bs = c->bar.d_bs.get(); t.bs_bytes = c->bar.bs_bytes; t.bs_mm_off = c->bar.bs_mm_off; t.G = c->bar.G;
	t.S = c->bar.S; t.L = c->bar.L; t.W = c->bar.W; t.max_diff = c->bar.max_diff;
	t.nbr = c->bar.nbr;
	t.count_rep = c->bar.d_count_rep.get(); t.count_rep_pitch = c->bar.count_rep_pitch;
	return t;
}

// The lookup kernel adds the ctx's counters into one line each (d_counts_wide); everything that reads or hands out
// d_counts first moves them over, on the ctx stream (the device is bound, and the second lane has been waited for).
int sk::fold_counts(sk_ctx *c)
{
	if (!c->bar.wide_dirty) return SK_OK;
	SK_HIP(c, sk::launch_counts_fold_wide(c->bar.d_counts_wide.get(), c->bar.S + 3, c->bar.S + 3 > sk::kCountDenseFrom ? sk::kCountDenseRows : 0, c->bar.d_counts.get(), c->stream));
	c->bar.wide_dirty = false;
	return SK_OK;
}

extern "C" {

int sk_barcode_table_info(sk_ctx *c, int *kind, int64_t *keys, int64_t *bytes)
{
	if (!c) return SK_ERR_INVALID;
	if (!c->bar.have_table) return fail(c, SK_ERR_STATE, "sk_set_barcodes has not been called");
	if (int r = bind(c)) return r;
	if (int r = sk::ensure_neighbour_table(c)) return r;
	const sk::LutDev &nbr = c->bar.nbr;
	const bool full = nbr.tab != nullptr, pair = nbr.pair.tab != nullptr;
	if (kind) *kind = (full ? SK_TABLE_FULL_KEY : pair ? SK_TABLE_FACTORED : SK_TABLE_NONE) | ((full || pair) && nbr.wide ? SK_TABLE_WIDE_CLASSES : 0);
	if (keys) *keys = (full || pair) ? c->bar.nbr_keys : 0;
	if (bytes) *bytes = (full || pair) ? c->bar.nbr_bytes : 0;
	return SK_OK;
}

int sk_set_detail_mode(sk_ctx *c, int mode)
{
	if (!c) return SK_ERR_INVALID;
	if (mode != SK_DETAIL_FULL && mode != SK_DETAIL_MATCHED) return fail(c, SK_ERR_INVALID, "detail mode %d is neither SK_DETAIL_FULL nor SK_DETAIL_MATCHED", mode);
	c->detail_mode = mode;
	return SK_OK;
}

int sk_counts_reset(sk_ctx *c)
{
	if (!c) return SK_ERR_INVALID;
	if (!c->bar.have_table) return fail(c, SK_ERR_STATE, "sk_set_barcodes has not been called");
	if (int r = bind(c)) return r;
	if (int r = sk::fold_counts(c)) return r;
	SK_HIP(c, hipMemsetAsync(c->bar.d_counts.get(), 0, (size_t)(c->bar.S + 3) * 8, c->stream));
	return SK_OK;
}

int sk_counts_get(sk_ctx *c, uint64_t *counts)
{
	if (!c || !counts) return SK_ERR_INVALID;
	if (!c->bar.have_table) return fail(c, SK_ERR_STATE, "sk_set_barcodes has not been called");
	if (int r = bind(c)) return r;
	if (int r = sk::fold_counts(c)) return r;
	SK_HIP(c, hipMemcpyAsync(counts, c->bar.d_counts.get(), (size_t)(c->bar.S + 3) * 8, hipMemcpyDeviceToHost, c->stream));
	SK_HIP(c, hipStreamSynchronize(c->stream));
	return SK_OK;
}

void *sk_counts_device_ptr(sk_ctx *c)
{
	if (!c || !c->bar.have_table) return nullptr;
	if (bind(c) != SK_OK || sk::fold_counts(c) != SK_OK) return nullptr;      // what was enqueued before this call is in the vector once the stream gets there
	return (void *)c->bar.d_counts.get();
}

}  // extern "C"
