// sk_bamfile_reads.cpp — sk_bam_file_reads / sk_bam_file_reads_next, sk_bam_file_pairs / sk_bam_file_pairs_next and sk_bam_file_pairs_gz /
// sk_bam_file_pairs_gz_next (include/seqkit_hip.h) behind the front half of sk_bamfile.cpp.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "sk_bamfile.h"

using namespace bamfile;

// ---- sam to raw|fasta|fastq (include/seqkit_hip.h: sk_bam_file_reads, sk_bam_file_reads_next) ----------------------------------
// The front half, then the sizing pass and the kept records' columns (kept_columns), the windows, and the first window's text on its
// way.  Every allocation that fails leaves the file to the caller's reader (info[5] = -21).

// window w of the plan (the next non-empty one) into buffer b: the text kernel, then the copies back; false: no window left
static bool reads_issue(sk_ctx *c, ReadsState &s, int b, int *rc)
{
	*rc = SK_OK;
	size_t w;
	if (!s.next_window(w)) return false;
	const int64_t first = (int64_t)s.ws[w], n = (int64_t)(s.ws[w + 1] - s.ws[w]);
	const uint64_t t0 = s.wt[w], tb = s.wt[w + 1] - t0, n0 = s.wn[w], nbytes = s.wn[w + 1] - n0;
	hipStream_t st = sk::ctx_stream(c);
	uint8_t *d = s.d_win[b], *h = s.h_win[b];
	hipError_t e = sk::launch_bam_reads_text(s.d_out, s.krec, s.ktoff, s.knoff, first, n, t0, n0, s.fmt, s.min_baseq, d, (uint64_t *)(d + s.at_toff),
	                                         d + s.at_names, (uint32_t *)(d + s.at_noff), sk::ctx_n_cu(c), st);
	if (e == hipSuccess && tb) e = hipMemcpyAsync(h, d, (size_t)tb, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess) e = hipMemcpyAsync(h + s.at_toff, d + s.at_toff, (size_t)(n + 1) * 8, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess) e = hipMemcpyAsync(h + s.at_noff, d + s.at_noff, (size_t)(n + 1) * 4, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess && nbytes) e = hipMemcpyAsync(h + s.at_names, d + s.at_names, (size_t)nbytes, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess) e = hipMemcpyAsync(h + s.at_kind, s.kkind + first, (size_t)n, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess) e = hipMemcpyAsync(h + s.at_key, s.kkey + first, (size_t)n * 8, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess) e = hipEventRecord(s.ev[b], st);
	if (e != hipSuccess) { *rc = sk::ctx_fail(c, SK_ERR_HIP, "sk_bam_file_reads: window %zu: %s", w, hipGetErrorString(e)); return false; }
	s.first[b] = first; s.n[b] = n;
	return true;
}

// What sk_bam_file_reads and sk_bam_file_pairs do first behind the front half: the sizing pass (per block: kept records, text bytes, name
// bytes, decline bits) and its scans — the decision to serve the file is taken there, before any text exists — then the kept records'
// columns (device, ctx slot kKeepFileCols): stream offset, text offset, name offset, key, kind.  ready = false: the file is left to the
// caller's reader (info[5] says why).
struct KeptCols {
	bool ready = false;
	int64_t K = 0;                               // kept records
	uint64_t T = 0, N = 0;                       // their text and name bytes
	uint64_t *krec = nullptr, *ktoff = nullptr, *knoff = nullptr, *kkey = nullptr;
	uint8_t *kkind = nullptr;
};
static int kept_columns(sk_ctx *c, Cleanup &cl, const Front &fr, int format, int want_unpaired, double info[8], KeptCols &kc)
{
	hipStream_t st = sk::ctx_stream(c);
	const int64_t nb = fr.nb;
	// ---- the sizing pass: per block kept records, text and name bytes (then their exclusive offsets), the decline bits, the longest record
	uint64_t *d_blk = nullptr;
	if (hipMalloc((void **)&d_blk, (size_t)(nb + 1) * 24 + 64) != hipSuccess) { (void)hipGetLastError(); BF_LEAVE(21); }
	cl.dev.push_back(d_blk);
	uint64_t *bk = d_blk, *bt = bk + nb + 1, *bn = bt + nb + 1;
	uint32_t *d_decline = (uint32_t *)(bn + nb + 1);
	BF_HIP(hipMemsetAsync(d_decline, 0, 4, st));
	BF_HIP(sk::launch_bam_reads_size(fr.d_out, fr.d_bend, fr.d_entry, nb, format, want_unpaired ? 1 : 0, bk, bt, bn, d_decline, st));
	uint64_t tot[3] = {0, 0, 0};                                        // kept, text, names
	BF_HIP(hipMemcpyAsync(tot, bk + nb, 8, hipMemcpyDeviceToHost, st));
	BF_HIP(hipMemcpyAsync(tot + 1, bt + nb, 8, hipMemcpyDeviceToHost, st));
	BF_HIP(hipMemcpyAsync(tot + 2, bn + nb, 8, hipMemcpyDeviceToHost, st));
	BF_LEAVE_DECLINED(d_decline, 0);                                    // (1 qname, 2 fastq quality, 4 l_seq, 8 invalid record: info[5] = -31 .. -45)
	kc.K = (int64_t)tot[0]; kc.T = tot[1]; kc.N = tot[2];
	// ---- the kept records' columns: stream offset, text offset, name offset, key, kind
	int krc = SK_OK;
	const size_t kcol = up((uint64_t)kc.K * 8);
	uint8_t *kb = (uint8_t *)sk::ctx_keep(c, sk::kKeepFileCols, kcol * 4 + up((uint64_t)kc.K) + 256, false, &krc);
	if (!kb) BF_LEAVE(21);
	kc.krec = (uint64_t *)kb; kc.ktoff = (uint64_t *)(kb + kcol); kc.knoff = (uint64_t *)(kb + 2 * kcol); kc.kkey = (uint64_t *)(kb + 3 * kcol); kc.kkind = kb + 4 * kcol;
	BF_HIP(sk::launch_bam_reads_index(fr.d_out, fr.d_bend, fr.d_entry, nb, format, want_unpaired ? 1 : 0, bk, bt, bn, kc.krec, kc.ktoff, kc.knoff, kc.kkey, kc.kkind, st));
	kc.ready = true;
	return SK_OK;
}

extern "C" int sk_bam_file_reads(sk_ctx *c, const char *path, int format, uint8_t min_baseq, int want_unpaired, uint64_t window_bytes, int64_t *n_kept,
                                 uint64_t *text_bytes, int *handled, double info[8])
{
	Cleanup cl;
	Front fr;
	if (int r = file_call_open(c, path, "sk_bam_file_reads", handled, info, cl, fr, [&] {
		    if (n_kept) *n_kept = 0;
		    if (text_bytes) *text_bytes = 0;
		    if (format < 0 || format > 2) return sk::ctx_fail(c, SK_ERR_INVALID, "format = %d", format);
		    return (int)SK_OK;
	    }))
		return r;
	if (!fr.ready) return SK_OK;
	const double t_size = now_ms();
	Ranges *R = (Ranges *)sk::ctx_ext(c);
	ReadsState &s = R->reads;
	KeptCols kc;
	if (int r = kept_columns(c, cl, fr, format, want_unpaired, info, kc)) return r;
	if (!kc.ready) return SK_OK;
	const int64_t K = kc.K;
	const uint64_t T = kc.T, N = kc.N;
	int krc = SK_OK;
	s.krec = kc.krec; s.ktoff = kc.ktoff; s.knoff = kc.knoff; s.kkey = kc.kkey; s.kkind = kc.kkind;
	// ---- the windows: at most W text + name bytes each
	uint64_t mx[3];                                                     // records, text bytes, name bytes
	bool room = true;
	if (int r = plan_windows(c, cl, window_bytes, s.ktoff, s.knoff, (uint64_t)K, T, N, s, s.wt, &s.wn, mx, &room)) return r;
	if (!room) BF_LEAVE(21);
	const uint64_t max_n = mx[0], max_t = mx[1], max_nm = mx[2];
	// ---- two window buffers, on the device and page-locked, in one layout
	s.at_toff = up(max_t + 16);
	s.at_noff = s.at_toff + up((max_n + 1) * 8);
	s.at_names = s.at_noff + up((max_n + 1) * 4);
	s.at_kind = s.at_names + up(max_nm + 16);
	s.at_key = s.at_kind + up(max_n + 16);
	const size_t wbytes = s.at_key + up(max_n * 8 + 16);
	uint8_t *dw = (uint8_t *)sk::ctx_keep(c, sk::kKeepFileWin, 2 * wbytes, false, &krc);
	if (!dw) BF_LEAVE(21);
	uint8_t *hw = (uint8_t *)sk::ctx_keep(c, sk::kKeepFilePin, 2 * wbytes, true, &krc);
	if (!hw) BF_LEAVE(21);
	for (int b = 0; b < 2; b++) {
		s.d_win[b] = dw + (size_t)b * wbytes; s.h_win[b] = hw + (size_t)b * wbytes;
		if (!blocking_event(s.ev[b])) BF_LEAVE(21);
	}
	s.fmt = format; s.min_baseq = min_baseq;
	s.begin(fr.d_out, R->gen);
	int rc = SK_OK;
	if (reads_issue(c, s, 0, &rc)) s.cur = 0;
	if (rc) return rc;
	s.live = true;
	if (n_kept) *n_kept = K;
	if (text_bytes) *text_bytes = T;
	*handled = 1;
	char tail[128];
	snprintf(tail, sizeof tail, "; %lld kept, %llu text bytes, %lld windows", (long long)K, (unsigned long long)T, (long long)s.ws.size() - 1);
	file_call_close(fr, "size + index + plan", t_size, tail, info);
	return SK_OK;
}

extern "C" int sk_bam_file_reads_next(sk_ctx *c, sk_bam_reads_window *w)
{
	if (!c || !w) return SK_ERR_INVALID;
	memset(w, 0, sizeof *w);
	Ranges *R = (Ranges *)sk::ctx_ext(c);
	if (!R || !R->reads.current(R->gen)) return sk::ctx_fail(c, SK_ERR_INVALID, "sk_bam_file_reads_next: no sk_bam_file_reads in progress");
	if (int r = sk::ctx_bind(c)) return r;
	ReadsState &s = R->reads;
	const int b = s.cur;
	if (b < 0) return SK_OK;                                            // the end
	int rc = SK_OK;
	s.cur = reads_issue(c, s, b ^ 1, &rc) ? (b ^ 1) : -1;                 // (the buffer of the window returned last time: the caller is done with it)
	if (rc) { s.live = false; return rc; }
	BF_HIP(hipEventSynchronize(s.ev[b]));
	const uint8_t *h = s.h_win[b];
	w->first = s.first[b]; w->n = s.n[b];
	w->text = h; w->text_off = (const uint64_t *)(h + s.at_toff); w->kind = h + s.at_kind; w->key = (const uint64_t *)(h + s.at_key);
	w->names = h + s.at_names; w->name_off = (const uint32_t *)(h + s.at_noff);
	return SK_OK;
}

// ---- sam to, the texts in output order (include/seqkit_hip.h: sk_bam_file_pairs, sk_bam_file_pairs_next) ------------------------
// The front half, the sizing pass and the kept records' columns as above, then the passes of sk_bampair.hip: the mates paired per name
// in sorted order, every written record's stream and rank from scans in file order, and per stream the permutation rank -> record and the
// 64-bit offsets of the texts.  The windows are rank ranges of one stream each; the text kernel takes a window's records from anywhere in
// the resident stream.  Working memory, per kept record: 12 B kept for the windows (permutation and offsets; ctx slot kKeepPassWork) and
// 38 B of scratch until the windows are planned — the sort's two key and two index buffers (24 B, then the ranks), two u32 scan columns,
// fate, class and partner — and the scratch of the sort and the scans; the scratch lies in the device buffer of the COMPRESSED file, idle
// once the stream is verified, where it fits there, else behind the kept head.

//
// sk_bam_file_pairs_gz / sk_bam_file_pairs_gz_next: the same front (pairs_plan), then the window area of the BAM-writing calls
// (sk_bamfile.h: PackArea) in place of the text buffers.  A window's text is written into its raw area, cut into blocks of at most
// SK_DEFLATE_MAX_IN bytes wherever the count falls, deflated where it lies and packed into complete members; only those are copied back,
// on the second stream, while the first runs the following window.  Per window: the text, 31 B and a deflate slot and its tokens per
// block, and twice the packed bytes on each side.

// plan window w into buffer b: the text kernel, then the copy back or, for members, cut, deflate and pack; false: no window left
static bool pairs_issue(sk_ctx *c, PairsState &s, int b, int *rc)
{
	*rc = SK_OK;
	if (s.next_w >= s.plan.size()) return false;
	const PairsState::Window &w = s.plan[s.next_w++];
	hipStream_t st = sk::ctx_stream(c);
	const uint64_t at = s.base[w.stream] + (uint64_t)w.stream;
	uint8_t *text = s.members ? s.pk.d_raw : s.d_win[b];
	hipError_t e = sk::launch_bam_pair_text(s.d_out, s.krec, s.perm + at, s.soff + at, (int64_t)w.first, (int64_t)w.n, s.fmt, s.min_baseq, text,
	                                        sk::ctx_n_cu(c), st);
	if (s.members) {
		if (e == hipSuccess) e = pack_issue(c, s.pk, w.bytes, b, s.ev[b]);
	} else {
		if (e == hipSuccess && w.bytes) e = hipMemcpyAsync(s.h_win[b], s.d_win[b], (size_t)w.bytes, hipMemcpyDeviceToHost, st);
		if (e == hipSuccess) e = hipEventRecord(s.ev[b], st);
	}
	if (e != hipSuccess) { *rc = sk::ctx_fail(c, SK_ERR_HIP, "sk_bam_file_pairs: window %zu: %s", s.next_w - 1, hipGetErrorString(e)); return false; }
	s.in[b] = w;
	return true;
}

// What sk_bam_file_pairs and sk_bam_file_pairs_gz do behind the front half, up to the per-stream window plan: it leaves the kept records'
// stream offsets, perm, soff, base[] and plan in the ctx's PairsState and the counts here.  ready = false: the file is left to the caller's
// reader (info[5] says why).
struct PairsPlan {
	bool ready = false;
	uint64_t K = 0, max_t = 0;                   // kept records; the largest window's text
	uint32_t P = 0;                              // paired records among them
	sk::PairRanks tot{0, 0, 0, 0};
	uint64_t bytes[3] = {0, 0, 0};               // the streams' text
	double t_size = 0;
};
static int pairs_plan(sk_ctx *c, Cleanup &cl, const Front &fr, int format, int interleaved, uint64_t window_bytes, double info[8], PairsPlan &pp)
{
	hipStream_t st = sk::ctx_stream(c);
	pp.t_size = now_ms();
	KeptCols kc;
	if (int r = kept_columns(c, cl, fr, format, interleaved ? 0 : 1, info, kc)) return r;
	if (!kc.ready) return SK_OK;
	const uint64_t K = (uint64_t)kc.K;
	if (K >= ((uint64_t)1 << 32)) BF_LEAVE(21);                         // (ranks and permutations are u32)
	int bits = 64;                                                      // (a test knob: fewer bits make key collisions reachable)
	if (const char *ev = getenv("SK_PAIR_KEY_BITS")) { const int v = atoi(ev); if (v >= 1 && v <= 64) bits = v; }
	// ---- the working memory
	const uint64_t K1 = K ? K : 1;
	passmem::SortBufs sb;
	BF_HIP(pass_temp(sb, K1, bits, st, [&](size_t *b) { return sk::bam_pair_scan_bytes(K1, b, st); }));
	uint32_t *perm = nullptr, *ipos = nullptr, *lz = nullptr, *aux = nullptr, *d_decline = nullptr;
	uint64_t *soff = nullptr;
	uint8_t *fate = nullptr, *cls = nullptr;
	passmem::Layout Lk, Ls;
	Lk.add(perm, (K + 3) * 4); Lk.add(soff, (K + 3) * 8);
	Ls.add(sb.key, K1 * 8); Ls.add(sb.idx, K1 * 4); Ls.add(ipos, K1 * 4); Ls.add(lz, K1 * 4); Ls.add(aux, K1 * 4); Ls.add(fate, K1); Ls.add(cls, K1);
	Ls.add(d_decline, 64); Ls.add(sb.temp, sb.temp_bytes);
	const passmem::Placement pl = passmem::place(Lk.total(), Ls.total(), fr.fsize + 64, getenv("SK_PAIRS_OWN_MEMORY") != nullptr);   // (the knob: for tests of the other placement)
	uint8_t *own = nullptr;
	if (!pass_memory(c, pl, own)) BF_LEAVE(21);
	pl.trace(fr.who, "", "the compressed file's buffer");
	Lk.carve(own);
	Ls.carve(pl.scratch_at(own, fr.d_comp));
	uint32_t *hs = ipos;                                                // (the places of the paired records are read by the compaction alone)
	sk::PairRanks *ranks = (sk::PairRanks *)sb.key[0];                  // (behind the fates the sort's buffers are idle: 16 of their 24 B per record)
	static_assert(sizeof(sk::PairRanks) == 16, "the ranks lie in the two key buffers");
	// ---- the paired records, sorted by key; fates; ranks
	BF_HIP(hipMemsetAsync(d_decline, 0, 4, st));
	uint32_t &P = pp.P;
	if (K) {
		BF_HIP(sk::bam_pair_scan_paired(sb.temp, sb.temp_bytes, kc.kkind, ipos, K, st));
		BF_HIP(hipMemcpyAsync(&P, ipos + (K - 1), 4, hipMemcpyDeviceToHost, st));
		BF_HIP(hipStreamSynchronize(st));                               // (P: the sort's length)
	}
	BF_HIP(sk::launch_bam_pair_compact(kc.kkind, kc.kkey, ipos, K, bits, sb.key[0], sb.idx[0], fate, aux, cls, st));
	int cur = 0;
	if (P) {
		size_t need = 0, tb = sb.temp_bytes;
		BF_HIP(sk::bam_sort_pairs(nullptr, &need, sb.key, sb.idx, P, bits, nullptr, st));
		if (need > sb.temp_bytes) BF_LEAVE(21);                         // (the scratch was sized for K >= P records)
		BF_HIP(sk::bam_sort_pairs(sb.temp, &tb, sb.key, sb.idx, P, bits, &cur, st));
	}
	const uint64_t *skey = sb.key[cur];
	const uint32_t *sidx = sb.idx[cur];
	BF_HIP(sk::launch_bam_pair_heads(fr.d_out, kc.krec, kc.kkind, skey, sidx, P, lz, d_decline, st));
	BF_LEAVE_DECLINED(d_decline, 0);                                    // (64: two names under one key: info[5] = -94)
	BF_HIP(sk::bam_pair_scan_max(sb.temp, sb.temp_bytes, lz, P, st));
	BF_HIP(sk::launch_bam_pair_holds(skey, lz, P, hs, st));
	BF_HIP(sk::bam_pair_scan_max(sb.temp, sb.temp_bytes, hs, P, st));
	BF_HIP(sk::launch_bam_pair_fates(skey, sidx, kc.kkind, lz, hs, P, fate, aux, cls, st));
	sk::PairRanks &tot = pp.tot;
	if (K) {
		BF_HIP(sk::bam_pair_scan_ranks(sb.temp, sb.temp_bytes, cls, ranks, K, st));
		BF_HIP(hipMemcpyAsync(&tot, ranks + (K - 1), sizeof tot, hipMemcpyDeviceToHost, st));
		BF_HIP(hipStreamSynchronize(st));
	}
	// ---- the streams: stream 1 and stream 2 hold a record per pair and the single stream the unpaired records, then the leftover first
	// mates, then the leftover last mates; interleaved: one stream of both mates, the rest is written nowhere
	Ranges *R = (Ranges *)sk::ctx_ext(c);
	PairsState &s = R->pairs;
	uint64_t n[3];
	n[0] = interleaved ? 2ull * tot.pair : tot.pair;
	n[1] = interleaved ? 0 : tot.pair;
	n[2] = interleaved ? 0 : (uint64_t)tot.single + tot.order1 + tot.order2;
	s.base[0] = 0; s.base[1] = n[0]; s.base[2] = n[0] + n[1];
	BF_HIP(sk::launch_bam_pair_place(fate, aux, ranks, kc.ktoff, K, kc.T, n, s.base, tot.single, tot.order1, interleaved ? 1 : 0, perm, soff, st));
	uint64_t (&bytes)[3] = pp.bytes;
	for (int q = 0; q < 3; q++) {
		uint64_t *so = soff + s.base[q] + q;
		BF_HIP(sk::bam_pair_scan_offsets(sb.temp, sb.temp_bytes, so, n[q], st));
		BF_HIP(hipMemcpyAsync(&bytes[q], so + n[q], 8, hipMemcpyDeviceToHost, st));
	}
	BF_HIP(hipStreamSynchronize(st));
	// ---- the windows: at most W text bytes each, stream by stream
	s.plan.clear();
	uint64_t &max_t = pp.max_t;
	for (int q = 0; q < 3; q++) {
		WindowedState ws;
		std::vector<uint64_t> w0;
		uint64_t mx[3];
		bool room = true;
		if (int r = plan_windows(c, cl, window_bytes, soff + s.base[q] + q, nullptr, n[q], bytes[q], 0, ws, w0, nullptr, mx, &room)) return r;
		if (!room) BF_LEAVE(21);
		for (size_t w = 0; w + 1 < ws.ws.size(); w++)
			if (ws.ws[w + 1] > ws.ws[w]) s.plan.push_back(PairsState::Window{q, ws.ws[w], ws.ws[w + 1] - ws.ws[w], w0[w + 1] - w0[w]});
		max_t = std::max(max_t, mx[1]);
	}
	s.fmt = format;
	s.krec = kc.krec; s.perm = perm; s.soff = soff;
	pp.K = K;
	pp.ready = true;
	return SK_OK;
}

// What both calls end with once their window buffers are there: the first window on its way, the counts, the trace line.
static int pairs_start(sk_ctx *c, const Front &fr, PairsState &s, const PairsPlan &pp, uint8_t min_baseq, bool members, uint64_t counts[8], int *handled,
                       double info[8])
{
	for (int b = 0; b < 2; b++)
		if (!blocking_event(s.ev[b])) BF_LEAVE(21);
	s.min_baseq = min_baseq; s.members = members;
	s.begin(fr.d_out, ((Ranges *)sk::ctx_ext(c))->gen);
	int rc = SK_OK;
	if (pairs_issue(c, s, 0, &rc)) s.cur = 0;
	if (rc) return rc;
	s.live = true;
	if (counts) {
		counts[0] = pp.tot.pair; counts[1] = pp.tot.single; counts[2] = pp.tot.order1; counts[3] = pp.tot.order2;
		counts[4] = (uint64_t)pp.P - 2ull * pp.tot.pair - pp.tot.order1 - pp.tot.order2;
		for (int q = 0; q < 3; q++) counts[5 + q] = pp.bytes[q];
	}
	*handled = 1;
	char tail[160];
	snprintf(tail, sizeof tail, "; %llu kept, %u pairs, %llu text bytes, %zu windows", (unsigned long long)pp.K, pp.tot.pair,
	         (unsigned long long)(pp.bytes[0] + pp.bytes[1] + pp.bytes[2]), s.plan.size());
	file_call_close(fr, "size + index + pair + plan", pp.t_size, tail, info);
	return SK_OK;
}

extern "C" int sk_bam_file_pairs(sk_ctx *c, const char *path, int format, uint8_t min_baseq, int interleaved, uint64_t window_bytes, uint64_t counts[8],
                                 int *handled, double info[8])
{
	Cleanup cl;
	Front fr;
	if (int r = file_call_open(c, path, "sk_bam_file_pairs", handled, info, cl, fr, [&] {
		    if (counts) for (int i = 0; i < 8; i++) counts[i] = 0;
		    if (format < 0 || format > 2) return sk::ctx_fail(c, SK_ERR_INVALID, "format = %d", format);
		    return (int)SK_OK;
	    }))
		return r;
	if (!fr.ready) return SK_OK;
	PairsPlan pp;
	if (int r = pairs_plan(c, cl, fr, format, interleaved, window_bytes, info, pp)) return r;
	if (!pp.ready) return SK_OK;
	PairsState &s = ((Ranges *)sk::ctx_ext(c))->pairs;
	// ---- two text buffers, on the device and page-locked
	int krc = SK_OK;
	const size_t wbytes = up(pp.max_t + 16);
	uint8_t *dw = (uint8_t *)sk::ctx_keep(c, sk::kKeepFileWin, 2 * wbytes, false, &krc);
	if (!dw) BF_LEAVE(21);
	uint8_t *hw = (uint8_t *)sk::ctx_keep(c, sk::kKeepFilePin, 2 * wbytes, true, &krc);
	if (!hw) BF_LEAVE(21);
	for (int b = 0; b < 2; b++) { s.d_win[b] = dw + (size_t)b * wbytes; s.h_win[b] = hw + (size_t)b * wbytes; }
	return pairs_start(c, fr, s, pp, min_baseq, false, counts, handled, info);
}

extern "C" int sk_bam_file_pairs_next(sk_ctx *c, sk_bam_pairs_window *w)
{
	if (!c || !w) return SK_ERR_INVALID;
	memset(w, 0, sizeof *w);
	Ranges *R = (Ranges *)sk::ctx_ext(c);
	if (!R || !R->pairs.current(R->gen) || R->pairs.members) return sk::ctx_fail(c, SK_ERR_INVALID, "sk_bam_file_pairs_next: no sk_bam_file_pairs in progress");
	if (int r = sk::ctx_bind(c)) return r;
	PairsState &s = R->pairs;
	const int b = s.cur;
	if (b < 0) return SK_OK;                                            // the end
	int rc = SK_OK;
	s.cur = pairs_issue(c, s, b ^ 1, &rc) ? (b ^ 1) : -1;                 // (the buffer of the window returned last time: the caller is done with it)
	if (rc) { s.live = false; return rc; }
	BF_HIP(hipEventSynchronize(s.ev[b]));
	w->stream = s.in[b].stream; w->first = (int64_t)s.in[b].first; w->n = (int64_t)s.in[b].n;
	w->text = s.h_win[b]; w->bytes = s.in[b].bytes;
	return SK_OK;
}

extern "C" int sk_bam_file_pairs_gz(sk_ctx *c, const char *path, int format, uint8_t min_baseq, int level, uint64_t window_bytes, uint64_t counts[8],
                                    int *handled, double info[8])
{
	Cleanup cl;
	Front fr;
	if (int r = file_call_open(c, path, "sk_bam_file_pairs_gz", handled, info, cl, fr, [&] {
		    if (counts) for (int i = 0; i < 8; i++) counts[i] = 0;
		    if (format < 0 || format > 2) return sk::ctx_fail(c, SK_ERR_INVALID, "format = %d", format);
		    if (level < 0 || level > 1) return sk::ctx_fail(c, SK_ERR_INVALID, "level = %d", level);
		    return (int)SK_OK;
	    }))
		return r;
	if (!fr.ready) return SK_OK;
	PairsPlan pp;
	if (int r = pairs_plan(c, cl, fr, format, 0, window_bytes, info, pp)) return r;
	if (!pp.ready) return SK_OK;
	PairsState &s = ((Ranges *)sk::ctx_ext(c))->pairs;
	if (!pack_area(c, s.pk, pp.max_t, level)) BF_LEAVE(21);
	return pairs_start(c, fr, s, pp, min_baseq, true, counts, handled, info);
}

extern "C" int sk_bam_file_pairs_gz_next(sk_ctx *c, sk_bam_pairs_gz_window *w)
{
	if (!c || !w) return SK_ERR_INVALID;
	memset(w, 0, sizeof *w);
	Ranges *R = (Ranges *)sk::ctx_ext(c);
	if (!R || !R->pairs.current(R->gen) || !R->pairs.members) return sk::ctx_fail(c, SK_ERR_INVALID, "sk_bam_file_pairs_gz_next: no sk_bam_file_pairs_gz in progress");
	if (int r = sk::ctx_bind(c)) return r;
	PairsState &s = R->pairs;
	const int b = s.cur;
	if (b < 0) return SK_OK;                                            // the end
	BF_HIP(hipEventSynchronize(s.ev[b]));
	const uint64_t bytes = s.pk.h_size[b];
	const PairsState::Window in = s.in[b];
	int rc = SK_OK;
	s.cur = pairs_issue(c, s, b ^ 1, &rc) ? (b ^ 1) : -1;                 // (the buffer of the window returned last time: the caller is done with it)
	if (rc) { s.live = false; return rc; }
	BF_HIP(pack_fetch(c, s.pk, b, bytes));
	w->stream = in.stream; w->first = (int64_t)in.first; w->n = (int64_t)in.n;
	w->bgzf = s.pk.h_pin[b]; w->bytes = bytes; w->raw_bytes = in.bytes;
	return SK_OK;
}
