// sk_bamfile_out.cpp — the BAM-writing file calls (include/seqkit_hip.h: sk_bam_file_rewrite, _minimize, _markdup, _subsample, _recalc_tlen,
// _merge, _concatenate, _discard_tails and sk_bam_file_rewrite_next) behind the front half of sk_bamfile.cpp: one spine (rw_open, the call's own passes, rw_begin, rw_issue).
#include <fcntl.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "sk_bamfile.h"

using namespace bamfile;

// ---- BAM out (include/seqkit_hip.h: sk_bam_file_rewrite, sk_bam_file_minimize, sk_bam_file_markdup, sk_bam_file_subsample; sk_bam_file_rewrite_next) ---
// The front half above, then the call's own passes, among them a sizing pass (per block: output bytes, decline bits) and its scan; the
// decision to serve the file is taken there, before any window exists.  Then every record's stream and output offsets, the windows, and
// the header's members on their way.  A window is rewritten into one device buffer, cut into blocks of at most 0xff00 bytes, deflated where it lies and packed into
// complete members; only the members' bytes are copied back.  Every allocation that fails leaves the file to the caller's reader
// (info[5] = -21).

// ---- the window area and what runs in it (sk_bamfile.h: PackArea), for the calls here and for sk_bam_file_pairs_gz -------------------
// the window area: raw bytes, blocks, deflate scratch and slots, member sizes, two packed buffers (device); two page-locked ones
bool bamfile::pack_area(sk_ctx *c, PackArea &a, uint64_t max_raw, int level)
{
	int krc = SK_OK;
	const uint64_t nblk = std::max<uint64_t>(1, (max_raw + SK_DEFLATE_MAX_IN - 1) / SK_DEFLATE_MAX_IN);
	const uint64_t pack = max_raw + nblk * 31 + 64;
	const size_t a_raw = up(max_raw + 64), a_blk = up(nblk * 16), a_res = up(nblk * 8), a_crc = up(nblk * 4), a_msz = up((nblk + 1) * 8), a_pack = up(pack);
	const size_t a_slots = level ? up(nblk * (uint64_t)SK_DEFLATE_SLOT) : 0, a_tok = level ? up(nblk * sk::deflate_tokens_per_block() * 4) : 0;
	uint8_t *dw = (uint8_t *)sk::ctx_keep(c, sk::kKeepFileWin, a_raw + a_blk + a_res + a_crc + a_msz + 2 * a_pack + a_slots + a_tok, false, &krc);
	if (!dw) return false;
	const size_t p_pack = up(pack + 28);
	uint8_t *hw = (uint8_t *)sk::ctx_keep(c, sk::kKeepFilePin, 2 * p_pack + 64, true, &krc);
	if (!hw) return false;
	a.d_raw = dw; a.d_blocks = dw + a_raw; a.d_result = (uint32_t *)(dw + a_raw + a_blk); a.d_crc = (uint32_t *)(dw + a_raw + a_blk + a_res);
	a.d_msz = (uint64_t *)(dw + a_raw + a_blk + a_res + a_crc);
	uint8_t *dp = dw + a_raw + a_blk + a_res + a_crc + a_msz;
	a.d_pack[0] = dp; a.d_pack[1] = dp + a_pack;
	a.d_slots = level ? dp + 2 * a_pack : nullptr;
	a.d_tokens = level ? (uint32_t *)(dp + 2 * a_pack + a_slots) : nullptr;
	a.h_pin[0] = hw; a.h_pin[1] = hw + p_pack; a.h_size = (uint64_t *)(hw + 2 * p_pack);
	a.level = level;
	for (int b = 0; b < 2; b++) {
		if (!blocking_event(a.ev_copy[b])) return false;
		if (hipEventRecord(a.ev_copy[b], sk::ctx_stream2(c)) != hipSuccess) { (void)hipGetLastError(); return false; }   // (nothing to wait for before the first copy)
	}
	return true;
}

// a window's raw_len bytes lie in d_raw: cut, deflate or crc, pack into packed buffer b, and the packed size back; then `done`
hipError_t bamfile::pack_issue(sk_ctx *c, PackArea &a, uint64_t raw_len, int b, hipEvent_t done)
{
	hipStream_t st = sk::ctx_stream(c);
	const int64_t nblk = (int64_t)((raw_len + SK_DEFLATE_MAX_IN - 1) / SK_DEFLATE_MAX_IN);
	hipError_t e = hipMemsetAsync(a.d_raw + raw_len, 0, 8, st);                          // (the deflate reads whole dwords)
	if (e == hipSuccess) e = hipStreamWaitEvent(st, a.ev_copy[b], 0);                   // (the copy out of this packed buffer)
	if (e == hipSuccess) e = sk::launch_bgzf_cut(raw_len, a.d_blocks, nblk, st);
	if (e == hipSuccess) e = a.level ? sk::launch_bgzf_deflate(a.d_raw, a.d_blocks, nblk, a.d_slots, SK_DEFLATE_SLOT, a.d_tokens, a.d_result, a.d_crc, sk::ctx_n_cu(c), st)
	                                 : sk::launch_bgzf_crc(a.d_raw, a.d_blocks, nblk, a.d_crc, sk::ctx_n_cu(c), st);
	if (e == hipSuccess) e = sk::launch_bgzf_pack(a.d_raw, a.d_blocks, nblk, a.d_slots, SK_DEFLATE_SLOT, a.d_result, a.d_crc, a.level ? 0 : 1, a.d_msz,
	                                              a.d_pack[b], sk::ctx_n_cu(c), st);
	if (e == hipSuccess) e = hipMemcpyAsync(a.h_size + b, a.d_msz + nblk, 8, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess) e = hipEventRecord(done, st);
	return e;
}

// packed buffer b's bytes into its page-locked twin, on the second stream (the first one runs the next window meanwhile), and waited for
hipError_t bamfile::pack_fetch(sk_ctx *c, PackArea &a, int b, uint64_t bytes)
{
	hipStream_t st2 = sk::ctx_stream2(c);
	hipError_t e = bytes ? hipMemcpyAsync(a.h_pin[b], a.d_pack[b], (size_t)bytes, hipMemcpyDeviceToHost, st2) : hipSuccess;
	if (e == hipSuccess) e = hipEventRecord(a.ev_copy[b], st2);
	if (e == hipSuccess) e = hipEventSynchronize(a.ev_copy[b]);
	return e;
}

// the header (first) or window w of the plan (the next non-empty one) into packed buffer b: rewrite, then pack_issue; false: nothing left
static bool rw_issue(sk_ctx *c, RewriteState &s, int b, int *rc)
{
	*rc = SK_OK;
	hipStream_t st = sk::ctx_stream(c);
	int64_t first = 0, n = 0;
	uint64_t raw_len = 0;
	hipError_t e = hipSuccess;
	if (!s.header_done) {
		s.header_done = true;
		raw_len = s.header.size();
		e = hipMemcpyAsync(s.d_raw, s.header.data(), (size_t)raw_len, hipMemcpyHostToDevice, st);
	} else {
		size_t w;
		if (!s.next_window(w)) return false;
		first = (int64_t)s.ws[w]; n = (int64_t)(s.ws[w + 1] - s.ws[w]);
		raw_len = s.wo[w + 1] - s.wo[w];
		e = s.write(sk::WriteWindow{s.d_out, s.krec, s.kout, first, n, s.wo[w], s.d_raw}, sk::ctx_n_cu(c), st);
	}
	if (e == hipSuccess) e = pack_issue(c, s, raw_len, b, s.ev[b]);
	if (e != hipSuccess) { *rc = sk::ctx_fail(c, SK_ERR_HIP, "sk_bam_file_rewrite: window at record %lld: %s", (long long)first, hipGetErrorString(e)); return false; }
	s.first[b] = first; s.n[b] = n; s.raw[b] = raw_len;
	return true;
}

// What sk_bam_file_rewrite, sk_bam_file_minimize, sk_bam_file_markdup and sk_bam_file_subsample open with once the stream is verified: the per-block scratch of
// their passes with the decline word behind it, the blocks' first record indices on the device, and the rewrite state with room for
// every record's stream and output offsets (ctx slot kKeepFileCols).  s == nullptr afterwards: that memory cannot be had, and the file
// is left to the caller's reader (info[5] = -21).
struct RwOpen {
	RewriteState *s = nullptr;
	uint64_t *d_blk = nullptr;                   // blk_cols columns of nb + 1 u64 each
	uint64_t *d_rb = nullptr;                    // block b's first record: nb entries, and one word more that is the caller's
	uint32_t *d_decline = nullptr;               // zeroed
	std::vector<uint64_t> rb;                    // (what d_rb is copied from: it lives until the caller has waited for the stream)
	double t_size = 0;
};
static int rw_open(sk_ctx *c, Cleanup &cl, const Front &fr, int blk_cols, RwOpen &o, double info[8])
{
	o.t_size = now_ms();
	hipStream_t st = sk::ctx_stream(c);
	const int64_t nb = fr.nb;
	if (hipMalloc((void **)&o.d_blk, (size_t)(nb + 1) * 8 * (size_t)(blk_cols + 1) + 64) != hipSuccess) { (void)hipGetLastError(); BF_LEAVE(21); }
	cl.dev.push_back(o.d_blk);
	o.d_rb = o.d_blk + (size_t)(nb + 1) * (size_t)blk_cols;
	o.d_decline = (uint32_t *)(o.d_rb + nb + 1);
	BF_HIP(hipMemsetAsync(o.d_decline, 0, 4, st));
	if (int r = block_first_records(c, fr, o.rb)) return r;
	if (nb) BF_HIP(hipMemcpyAsync(o.d_rb, o.rb.data(), (size_t)nb * 8, hipMemcpyHostToDevice, st));
	int krc = SK_OK;
	const size_t a_col = up(fr.n_records * 8 + 8);
	uint8_t *kb = (uint8_t *)sk::ctx_keep(c, sk::kKeepFileCols, 2 * a_col, false, &krc);
	if (!kb) BF_LEAVE(21);
	Ranges *R = (Ranges *)sk::ctx_ext(c);
	R->rw.krec = (uint64_t *)kb; R->rw.kout = (uint64_t *)(kb + a_col);
	o.s = &R->rw;
	return SK_OK;
}

// What they share once the stream and output offsets (s.krec, s.kout) of the N records that go out are there — every record of the file,
// or for sk_bam_file_subsample the kept ones —: the window plan, the window area, and the header's members on their way.  `write`:
// what writes a window; `total`: the records' output bytes; `ends`: SK_CONCAT_HEADER | SK_CONCAT_EOF, both for every call but
// sk_bam_file_concatenate; `more`: whole lines behind the header's text (sk_bam_file_discard_tails: its @CO line).
static int rw_begin(sk_ctx *c, Cleanup &cl, const Front &fr, const RwOpen &o, const WindowWriter &write, int level, uint64_t window_bytes, uint64_t N,
                    uint64_t total, int64_t *n_records, uint64_t *raw_bytes, int *handled, double info[8], int ends = SK_CONCAT_HEADER | SK_CONCAT_EOF,
                    const std::vector<uint8_t> *more = nullptr)
{
	RewriteState &s = *o.s;
	// ---- the windows: at most W rewritten bytes each
	uint64_t mx[3];                                                     // records, rewritten bytes
	bool room = true;
	if (int r = plan_windows(c, cl, window_bytes, s.kout, nullptr, N, total, 0, s, s.wo, nullptr, mx, &room)) return r;
	if (!room) BF_LEAVE(21);
	s.header.clear();
	if (ends & SK_CONCAT_HEADER) s.header = bamfmt::rewrite_header(fr.header, more ? more->data() : nullptr, more ? more->size() : 0);
	const uint64_t max_raw = std::max<uint64_t>(s.header.size(), mx[1]);
	if (!pack_area(c, s, max_raw, level)) BF_LEAVE(21);
	for (int b = 0; b < 2; b++)
		if (!blocking_event(s.ev[b])) BF_LEAVE(21);
	s.write = write;
	s.header_done = !(ends & SK_CONCAT_HEADER); s.eof_due = (ends & SK_CONCAT_EOF) != 0;
	s.begin(fr.d_out, ((Ranges *)sk::ctx_ext(c))->gen);
	int rc = SK_OK;
	if (rw_issue(c, s, 0, &rc)) s.cur = 0;
	if (rc) return rc;
	s.live = true;
	if (n_records) *n_records = (int64_t)N;
	if (raw_bytes) *raw_bytes = s.header.size() + total;
	*handled = 1;
	char tail[128];
	snprintf(tail, sizeof tail, "; %llu records, %llu rewritten bytes, %lld windows", (unsigned long long)N, (unsigned long long)total, (long long)s.ws.size() - 1);
	file_call_close(fr, "size + index + plan", o.t_size, tail, info);
	return SK_OK;
}

extern "C" int sk_bam_file_rewrite(sk_ctx *c, const char *path, int op, int level, uint64_t window_bytes, int64_t *n_records, uint64_t *raw_bytes,
                                   int *handled, double info[8])
{
	Cleanup cl;
	Front fr;
	if (int r = file_call_open(c, path, "sk_bam_file_rewrite", handled, info, cl, fr, [&] {
		    if (n_records) *n_records = 0;
		    if (raw_bytes) *raw_bytes = 0;
		    if (op < SK_REWRITE_TRIM_QNAMES || op > SK_REWRITE_TAGS_FROM_QNAME) return sk::ctx_fail(c, SK_ERR_INVALID, "op = %d", op);
		    if (level < 0 || level > 1) return sk::ctx_fail(c, SK_ERR_INVALID, "level = %d", level);
		    return (int)SK_OK;
	    }))
		return r;
	if (!fr.ready) return SK_OK;
	RwOpen o;
	if (int r = rw_open(c, cl, fr, 1, o, info)) return r;
	if (!o.s) return SK_OK;
	hipStream_t st = sk::ctx_stream(c);
	const int64_t nb = fr.nb;
	// ---- the sizing pass: per block the rewritten bytes (then their exclusive offsets), the decline bits
	uint64_t *bo = o.d_blk;
	BF_HIP(sk::launch_bam_rw_size(fr.d_out, fr.d_bend, fr.d_entry, nb, op, bo, o.d_decline, st));
	uint64_t total = 0;
	BF_HIP(hipMemcpyAsync(&total, bo + nb, 8, hipMemcpyDeviceToHost, st));
	BF_LEAVE_DECLINED(o.d_decline, 0);                                  // (1 trim panic, 2 unsupported tag, 4 long name, 8 invalid record, 16 aux: info[5] = -31 .. -61)
	// ---- every record's stream and output offsets
	BF_HIP(sk::launch_bam_rw_index(fr.d_out, fr.d_bend, fr.d_entry, nb, op, bo, o.d_rb, o.s->krec, o.s->kout, st));
	const WindowWriter write = [op](const sk::WriteWindow &w, int n_cu, hipStream_t s) { return sk::launch_bam_rw_write(w, op, n_cu, s); };
	return rw_begin(c, cl, fr, o, write, level, window_bytes, fr.n_records, total, n_records, raw_bytes, handled, info);
}

// ---- sam minimize (include/seqkit_hip.h: sk_bam_file_minimize; the windows come from sk_bam_file_rewrite_next) ---
// The front half, then with SK_MINIMIZE_READ_IDS the id passes (sk_bamminimize.hip: keys, sort, runs, ids) in the working memory of ctx
// slot kKeepPassWork — two key and two index buffers for the sort (24 B per record and the sort's own scratch); behind the sort the idle
// key buffer holds src and the opener counts and the idle index buffer the ids — then the sizing pass with the ids' digits, and from
// there on what sk_bam_file_rewrite does.  The file is left to the caller's reader (info[5] = -21) when that memory cannot be had or
// the file has 2^32 records or more (the ids are u32), and with info[5] = -(30 + bits) on an invalid record (8), a CIGAR operation
// code above 8 (32) or two keys with one hash (64).
extern "C" int sk_bam_file_minimize(sk_ctx *c, const char *path, int flags, uint8_t baseq_fill, int level, uint64_t window_bytes, int64_t *n_records,
                                    uint64_t *raw_bytes, int *handled, double info[8])
{
	Cleanup cl;
	Front fr;
	if (int r = file_call_open(c, path, "sk_bam_file_minimize", handled, info, cl, fr, [&] {
		    if (n_records) *n_records = 0;
		    if (raw_bytes) *raw_bytes = 0;
		    const int all = SK_MINIMIZE_READ_IDS | SK_MINIMIZE_BASE_QUALITIES | SK_MINIMIZE_TAGS;
		    if (!flags || (flags & ~all) || ((flags & SK_MINIMIZE_BASE_QUALITIES) && !(flags & SK_MINIMIZE_TAGS)))
			    return sk::ctx_fail(c, SK_ERR_INVALID, "flags = %d", flags);
		    if (level < 0 || level > 1) return sk::ctx_fail(c, SK_ERR_INVALID, "level = %d", level);
		    return (int)SK_OK;
	    }))
		return r;
	if (!fr.ready) return SK_OK;
	const int64_t nb = fr.nb;
	const uint64_t N = fr.n_records;
	if (N >= ((uint64_t)1 << 32)) BF_LEAVE(21);
	RwOpen o;
	if (int r = rw_open(c, cl, fr, 1, o, info)) return r;
	if (!o.s) return SK_OK;
	hipStream_t st = sk::ctx_stream(c);
	uint64_t *bo = o.d_blk, *krec = o.s->krec, *kout = o.s->kout;
	// ---- the read ids
	const uint32_t *ids = nullptr;
	if ((flags & SK_MINIMIZE_READ_IDS) && N) {
		int bits = 64;                                                  // (a test knob: fewer bits make hash collisions reachable)
		if (const char *ev = getenv("SK_MINIMIZE_KEY_BITS")) { const int v = atoi(ev); if (v >= 1 && v <= 64) bits = v; }
		passmem::SortBufs sb;
		BF_HIP(pass_temp(sb, N, bits, st, [](size_t *) { return hipSuccess; }));
		uint32_t *agg = nullptr;
		passmem::Layout L;
		L.add(sb.key, N * 8); L.add(sb.idx, N * 4); L.add(agg, (N / 1024 + 2) * 4); L.add(sb.temp, sb.temp_bytes);
		uint8_t *own = nullptr;
		if (!pass_memory(c, passmem::place(L.total(), 0, 0, true), own)) BF_LEAVE(21);     // (all of it kept: the windows read the ids)
		L.carve(own);
		BF_HIP(sk::launch_bam_min_keys(fr.d_out, fr.d_bend, fr.d_entry, nb, o.d_rb, bits, sk::IdRule{0, 0u}, krec, sb.key[0], sb.idx[0], o.d_decline, st));
		BF_LEAVE_DECLINED(o.d_decline, 0);                              // (the passes below read the names of valid records only)
		int cur = 0;
		size_t tb = sb.temp_bytes;
		BF_HIP(sk::bam_sort_pairs(sb.temp, &tb, sb.key, sb.idx, N, bits, &cur, st));
		uint32_t *src = (uint32_t *)sb.key[cur ^ 1], *cnt = src + N;
		BF_HIP(sk::launch_bam_min_ids(fr.d_out, krec, sb.key[cur], sb.idx[cur], N, bits, sk::IdRule{0, 0u}, agg, src, cnt, sb.idx[cur ^ 1], o.d_decline, st));
		ids = sb.idx[cur ^ 1];
	}
	// ---- the sizing pass: per block the output bytes (then their exclusive offsets), the decline bits
	BF_HIP(sk::launch_bam_min_size(fr.d_out, fr.d_bend, fr.d_entry, nb, o.d_rb, flags, ids, bo, o.d_decline, st));
	uint64_t total = 0;
	BF_HIP(hipMemcpyAsync(&total, bo + nb, 8, hipMemcpyDeviceToHost, st));
	BF_LEAVE_DECLINED(o.d_decline, 0);
	BF_HIP(sk::launch_bam_min_index(fr.d_out, fr.d_bend, fr.d_entry, nb, o.d_rb, flags, ids, bo, krec, kout, st));
	// (ids: ctx slot kKeepPassWork; nullptr without SK_MINIMIZE_READ_IDS)
	const WindowWriter write = [=](const sk::WriteWindow &w, int n_cu, hipStream_t s) { return sk::launch_bam_min_write(w, ids, flags, baseq_fill, n_cu, s); };
	return rw_begin(c, cl, fr, o, write, level, window_bytes, N, total, n_records, raw_bytes, handled, info);
}

// ---- sam mark duplicates (include/seqkit_hip.h: sk_bam_file_markdup; the windows come from sk_bam_file_rewrite_next) ---
// The front half, then the passes of sk_bammarkdup.hip.  Their working memory — two key and two index buffers for the sort (before the
// sort the second of each holds (tid, pos) and the run flags, and the first index buffer the run indices), five u32 signature columns
// and the scratch of the sort and the scan: 44 B per record — is needed only until the clusters are found, and lies in the device
// buffer of the COMPRESSED file, which is idle once the stream is verified (a BAM record takes more compressed bytes than that; where
// it does not, ctx slot kKeepPassWork serves).  Only the u16 flag column, which the windows read, is kept in that slot: a gigabyte
// taken and given back for a 20 M-record file cost the command 0.1 s.  The records' bytes and sizes do not change: a record's output
// offset is its stream offset less the header's, the windows are planned over those, and the write kernel patches the flag.  Declined
// files: the list in include/seqkit_hip.h.
extern "C" int sk_bam_file_markdup(sk_ctx *c, const char *path, int ignore_umi, int level, uint64_t window_bytes, int64_t *n_records,
                                   int64_t *n_duplicates, uint64_t *raw_bytes, int *handled, double info[8])
{
	Cleanup cl;
	Front fr;
	if (int r = file_call_open(c, path, "sk_bam_file_markdup", handled, info, cl, fr, [&] {
		    if (n_records) *n_records = 0;
		    if (n_duplicates) *n_duplicates = 0;
		    if (raw_bytes) *raw_bytes = 0;
		    if (level < 0 || level > 1) return sk::ctx_fail(c, SK_ERR_INVALID, "level = %d", level);
		    return (int)SK_OK;
	    }))
		return r;
	if (!fr.ready) return SK_OK;
	const int64_t nb = fr.nb;
	const uint64_t N = fr.n_records;
	if (N >= ((uint64_t)1 << 32)) BF_LEAVE(21);
	RwOpen o;
	if (int r = rw_open(c, cl, fr, 0, o, info)) return r;
	if (!o.s) return SK_OK;
	hipStream_t st = sk::ctx_stream(c);
	uint64_t *d_count = o.d_rb + nb;                                    // (no per-block column, one word: the duplicates)
	passmem::SortBufs sb;
	BF_HIP(pass_temp(sb, N ? N : 1, 64, st, [&](size_t *b) { return sk::bam_md_run_scan(nullptr, b, nullptr, nullptr, N ? N : 1, st); }));
	sk::MdCols cols;
	cols.krec = o.s->krec; cols.kout = o.s->kout;
	const uint64_t sig = N * 4 + 4;                                     // (a signature column)
	passmem::Layout L;
	L.add(sb.key, N * 8 + 8); L.add(sb.idx, N * 4 + 4);
	L.add(cols.start, sig); L.add(cols.fl, sig); L.add(cols.lseq, sig); L.add(cols.uoff, sig); L.add(cols.ulen, sig);
	L.add(sb.temp, sb.temp_bytes);
	const passmem::Placement pl = passmem::place(N * 2 + 2, L.total(), fr.fsize + 64, getenv("SK_MARKDUP_OWN_MEMORY") != nullptr);   // (the knob: for tests of the other placement)
	uint8_t *own = nullptr;
	if (!pass_memory(c, pl, own)) BF_LEAVE(21);
	pl.trace(fr.who, "", "the compressed file's buffer");
	L.carve(pl.scratch_at(own, fr.d_comp));
	cols.tidpos = sb.key[1]; cols.nflag = (uint16_t *)own;
	// ---- signatures, order, runs: the decision to serve the file
	BF_HIP(sk::launch_bam_md_sig(fr.d_out, fr.d_bend, fr.d_entry, nb, o.d_rb, ignore_umi ? 1 : 0, fr.first, cols, o.d_decline, st));
	BF_HIP(sk::launch_bam_md_order(cols.tidpos, N, sb.idx[1], o.d_decline, st));
	uint32_t runs = 0;
	if (N) {
		size_t tb = sb.temp_bytes;
		BF_HIP(sk::bam_md_run_scan(sb.temp, &tb, sb.idx[1], sb.idx[0], N, st));
		BF_HIP(hipMemcpyAsync(&runs, sb.idx[0] + (N - 1), 4, hipMemcpyDeviceToHost, st));
	}
	BF_HIP(hipStreamSynchronize(st));                                  // (runs)
	BF_LEAVE_DECLINED(o.d_decline, runs >= 0x7fffffffu ? 64u : 0u);
	// ---- keys, the sort (only the bits the keys use: the all-ones key of the unmapped reads stays the largest), clusters, count
	int bits = 34;
	while (bits < 64 && ((uint64_t)1 << (bits - 33)) <= (uint64_t)runs) bits++;
	uint64_t dups = 0;
	if (N) {
		BF_HIP(sk::launch_bam_md_keys(sb.idx[0], cols, N, sb.key[0], sb.idx[0], st));
		int cur = 0;
		size_t tb = sb.temp_bytes;
		BF_HIP(sk::bam_sort_pairs(sb.temp, &tb, sb.key, sb.idx, N, bits, &cur, st));
		BF_HIP(sk::launch_bam_md_cluster(fr.d_out, cols, sb.key[cur], sb.idx[cur], N, d_count, sk::ctx_n_cu(c), st));
		BF_HIP(hipMemcpyAsync(&dups, d_count, 8, hipMemcpyDeviceToHost, st));
		BF_HIP(hipStreamSynchronize(st));
	}
	const uint16_t *nflag = cols.nflag;
	const WindowWriter write = [nflag](const sk::WriteWindow &w, int n_cu, hipStream_t s) { return sk::launch_bam_md_write(w, nflag, n_cu, s); };
	const int rc = rw_begin(c, cl, fr, o, write, level, window_bytes, N, fr.stream_len - fr.first, n_records, raw_bytes, handled, info);
	if (rc == SK_OK && *handled && n_duplicates) *n_duplicates = (int64_t)dups;
	return rc;
}

// ---- sam subsample (include/seqkit_hip.h: sk_bam_file_subsample; the windows come from sk_bam_file_rewrite_next) ---
// The front half, then sk_bamminimize.hip's id passes under the rule {the whole name is the key, 0x800 takes no part} — they number the
// fragments — and the passes of sk_bamsubsample.hip: the keep pass, two scans and the compaction, which leaves the KEPT records' stream
// and output offsets where sk_bam_file_rewrite leaves every record's.  The working memory (the compressed file's device buffer, idle by
// then, or where that is too small ctx slot kKeepPassWork): two key and two
// index buffers for the sort and every record's stream offset, 32 B per record, and the scratch of the sort and the scans; behind the
// sort the idle key buffer holds src and the opener counts and then the kept lengths and places, the idle index buffer the fragment
// numbers, and the sorted keys' buffer the output offsets.  Declined files: the list in include/seqkit_hip.h.
extern "C" int sk_bam_file_subsample(sk_ctx *c, const char *path, float fraction, uint64_t seed, int level, uint64_t window_bytes, int64_t *n_records,
                                     int64_t *n_total, uint64_t *raw_bytes, int *handled, double info[8])
{
	Cleanup cl;
	Front fr;
	if (int r = file_call_open(c, path, "sk_bam_file_subsample", handled, info, cl, fr, [&] {
		    if (n_records) *n_records = 0;
		    if (n_total) *n_total = 0;
		    if (raw_bytes) *raw_bytes = 0;
		    if (!(fraction >= 0.0f && fraction <= 1.0f)) return sk::ctx_fail(c, SK_ERR_INVALID, "fraction = %g", (double)fraction);
		    if (level < 0 || level > 1) return sk::ctx_fail(c, SK_ERR_INVALID, "level = %d", level);
		    return (int)SK_OK;
	    }))
		return r;
	if (!fr.ready) return SK_OK;
	const int64_t nb = fr.nb;
	const uint64_t N = fr.n_records;
	if (N >= ((uint64_t)1 << 32)) BF_LEAVE(21);
	RwOpen o;
	if (int r = rw_open(c, cl, fr, 3, o, info)) return r;
	if (!o.s) return SK_OK;
	hipStream_t st = sk::ctx_stream(c);
	uint64_t *d_counts = o.d_blk;                                       // (no per-block column, three words: counted, kept, kept bytes)
	uint64_t counts[3] = {0, 0, 0};
	if (N) {
		const sk::IdRule rule{1, 0x800u};
		int bits = 63;                                                  // (a test knob: fewer bits make hash collisions reachable; bit `bits` marks a record with 0x800)
		if (const char *ev = getenv("SK_SUBSAMPLE_KEY_BITS")) { const int v = atoi(ev); if (v >= 1 && v <= 64) bits = std::min(v, 63); }
		passmem::SortBufs sb;
		BF_HIP(pass_temp(sb, N, bits + 1, st, [&](size_t *b) { return sk::bam_sub_scans(nullptr, b, nullptr, nullptr, nullptr, N, st); }));
		uint64_t *krec = nullptr;
		uint32_t *agg = nullptr;
		passmem::Layout L;
		L.add(sb.key, N * 8); L.add(krec, N * 8); L.add(sb.idx, N * 4); L.add(agg, (N / 1024 + 2) * 4); L.add(sb.temp, sb.temp_bytes);
		// (all of it is idle once the kept records are compacted: as sk_bam_file_markdup's scratch it lies in the device buffer of the
		// compressed file where that is large enough, and a gigabyte is not taken and given back for a 20 M-record file)
		const passmem::Placement pl = passmem::place(0, L.total(), fr.fsize + 64, false);
		uint8_t *own = nullptr;
		if (!pass_memory(c, pl, own)) BF_LEAVE(21);
		pl.trace(fr.who, "", "the compressed file's buffer");
		L.carve(pl.scratch_at(own, fr.d_comp));
		// ---- the fragment numbers
		BF_HIP(sk::launch_bam_min_keys(fr.d_out, fr.d_bend, fr.d_entry, nb, o.d_rb, bits, rule, krec, sb.key[0], sb.idx[0], o.d_decline, st));
		BF_LEAVE_DECLINED(o.d_decline, 0);                              // (8: the passes below read the names and flags of valid records only)
		int cur = 0;
		size_t tb = sb.temp_bytes;
		BF_HIP(sk::bam_sort_pairs(sb.temp, &tb, sb.key, sb.idx, N, bits + 1, &cur, st));
		uint32_t *src = (uint32_t *)sb.key[cur ^ 1], *cnt = src + N, *ids = sb.idx[cur ^ 1];
		BF_HIP(sk::launch_bam_min_ids(fr.d_out, krec, sb.key[cur], sb.idx[cur], N, bits, rule, agg, src, cnt, ids, o.d_decline, st));
		// ---- the decisions: the file is served or left here
		uint32_t *len = src, *pos = cnt;
		uint64_t *off = sb.key[cur];
		BF_HIP(sk::launch_bam_sub_keep(fr.d_out, krec, ids, N, seed, sk::subsample_threshold(fraction), len, d_counts, o.d_decline, sk::ctx_n_cu(c), st));
		BF_HIP(hipMemcpyAsync(counts, d_counts, 24, hipMemcpyDeviceToHost, st));
		BF_LEAVE_DECLINED(o.d_decline, 0);                              // (1 a counted record without 0x1, 64 two names with one hash)
		// ---- the kept records' stream and output offsets
		tb = sb.temp_bytes;
		BF_HIP(sk::bam_sub_scans(sb.temp, &tb, len, pos, off, N, st));
		BF_HIP(sk::launch_bam_sub_compact(krec, len, pos, off, N, o.s->krec, o.s->kout, st));
	}
	const int rc = rw_begin(c, cl, fr, o, sk::launch_bam_copy_write, level, window_bytes, counts[1], counts[2], n_records, raw_bytes, handled, info);
	if (rc == SK_OK && *handled && n_total) *n_total = (int64_t)counts[0];
	return rc;
}

// ---- sam recalculate tlen (include/seqkit_hip.h: sk_bam_file_recalc_tlen, _discarded; the windows come from sk_bam_file_rewrite_next) ---
// The front half, then the passes of sk_bamtlen.hip around sk_bamminimize.hip's sort and run pass, which link the mates, and
// sk_bamsubsample.hip's scans and compaction, which leave the WRITTEN records' stream and output offsets where sk_bam_file_rewrite
// leaves every record's.  The working memory is sk_bam_file_subsample's, 32 B per record and the scratch of the sort and the scans, placed
// as there: behind the sort the idle key buffer holds src and the record lengths, the idle index buffer the TLENs in file order, the
// sorted indices' buffer the places and the sorted keys' buffer the output offsets.  What the windows and
// sk_bam_file_recalc_tlen_discarded read is kept in ctx slot kKeepPassWork: one region of 8 B per record with the written records'
// TLENs (4 B each) from its start and the discarded records' stream offsets (8 B each) up to its end — every record is one or the
// other — and the name slots of one chunk of discarded records.  Declined files: the list in include/seqkit_hip.h.
extern "C" int sk_bam_file_recalc_tlen(sk_ctx *c, const char *path, int64_t max_len, int level, uint64_t window_bytes, int64_t *n_records,
                                       int64_t *n_discarded, uint64_t *raw_bytes, int *handled, double info[8])
{
	Cleanup cl;
	Front fr;
	if (int r = file_call_open(c, path, "sk_bam_file_recalc_tlen", handled, info, cl, fr, [&] {
		    if (n_records) *n_records = 0;
		    if (n_discarded) *n_discarded = 0;
		    if (raw_bytes) *raw_bytes = 0;
		    if (max_len <= 0) return sk::ctx_fail(c, SK_ERR_INVALID, "max_len = %lld", (long long)max_len);
		    if (level < 0 || level > 1) return sk::ctx_fail(c, SK_ERR_INVALID, "level = %d", level);
		    return (int)SK_OK;
	    }))
		return r;
	if (!fr.ready) return SK_OK;
	const int64_t nb = fr.nb;
	const uint64_t N = fr.n_records;
	if (N >= ((uint64_t)1 << 32)) BF_LEAVE(21);
	RwOpen o;
	if (int r = rw_open(c, cl, fr, 0, o, info)) return r;
	if (!o.s) return SK_OK;
	hipStream_t st = sk::ctx_stream(c);
	const int n_cu = sk::ctx_n_cu(c);
	int bits = 63;                                                      // (a test knob: fewer bits make hash collisions reachable; bit `bits` marks a record that is no candidate)
	if (const char *ev = getenv("SK_TLEN_KEY_BITS")) { const int v = atoi(ev); if (v >= 1 && v <= 63) bits = v; }
	passmem::SortBufs sb;
	BF_HIP(pass_temp(sb, N ? N : 1, bits + 1, st, [&](size_t *b) { return sk::bam_sub_scans(nullptr, b, nullptr, nullptr, nullptr, N ? N : 1, st); }));
	uint64_t *krec = nullptr;
	uint32_t *agg = nullptr;
	passmem::Layout L;
	L.add(sb.key, N * 8); L.add(krec, N * 8); L.add(sb.idx, N * 4); L.add(agg, (N / 1024 + 2) * 4); L.add(sb.temp, sb.temp_bytes);
	const size_t a_kept = up(N * 8 + 8);
	const passmem::Placement pl = passmem::place(a_kept + (size_t)std::min<uint64_t>(N, RewriteState::kTlenNameSlots) * 256, L.total(), fr.fsize + 64,
	                                             getenv("SK_TLEN_OWN_MEMORY") != nullptr);             // (the knob: for tests of the other placement)
	uint8_t *own = nullptr;
	if (!pass_memory(c, pl, own)) BF_LEAVE(21);
	pl.trace(fr.who, "", "the compressed file's buffer");
	L.carve(pl.scratch_at(own, fr.d_comp));
	int32_t *tlen_out = (int32_t *)own;
	uint64_t written = 0, total = 0;
	if (N) {
		// ---- classes and keys: the passes below read the names, flags and CIGARs of valid records only
		BF_HIP(sk::launch_bam_tlen_keys(fr.d_out, fr.d_bend, fr.d_entry, nb, o.d_rb, max_len, bits, krec, sb.key[0], sb.idx[0], o.d_decline, st));
		BF_LEAVE_DECLINED(o.d_decline, 0);                              // (1 a record the reference stops at, 8 an invalid record, 16 a name byte >= 0x80)
		// ---- the mates' link, the pairs' TLENs: the file is served or left here
		int cur = 0;
		size_t tb = sb.temp_bytes;
		BF_HIP(sk::bam_sort_pairs(sb.temp, &tb, sb.key, sb.idx, N, bits + 1, &cur, st));
		uint32_t *src = (uint32_t *)sb.key[cur ^ 1], *cnt = src + N;
		BF_HIP(sk::launch_bam_min_ids(fr.d_out, krec, sb.key[cur], sb.idx[cur], N, bits, sk::kTlenIdRule, agg, src, cnt, sb.idx[cur ^ 1], o.d_decline, st));
		uint32_t *len = cnt, *pos = sb.idx[cur];                          // (the opener counts, the ids and the sorted pairs are idle from here on)
		int32_t *tlen = (int32_t *)sb.idx[cur ^ 1];
		uint64_t *off = sb.key[cur];
		BF_HIP(sk::launch_bam_tlen_resolve(fr.d_out, krec, src, N, tlen, len, o.d_decline, n_cu, st));
		BF_LEAVE_DECLINED(o.d_decline, 0);                              // (2 mates with equal 0x40 bits, 32 a CIGAR operation code above 8, 64 two names with one hash)
		// ---- the written records' stream and output offsets and TLENs, the discarded records' stream offsets
		tb = sb.temp_bytes;
		BF_HIP(sk::bam_sub_scans(sb.temp, &tb, len, pos, off, N, st));
		uint32_t last[2] = {0, 0};                                       // the last record: its place, its length
		BF_HIP(hipMemcpyAsync(&last[0], pos + (N - 1), 4, hipMemcpyDeviceToHost, st));
		BF_HIP(hipMemcpyAsync(&last[1], len + (N - 1), 4, hipMemcpyDeviceToHost, st));
		BF_HIP(hipMemcpyAsync(&total, off + (N - 1), 8, hipMemcpyDeviceToHost, st));
		BF_HIP(hipStreamSynchronize(st));
		written = (uint64_t)last[0] + (last[1] ? 1 : 0);
		total += last[1];
		BF_HIP(sk::launch_bam_sub_compact(krec, len, pos, off, N, o.s->krec, o.s->kout, st));
		BF_HIP(sk::launch_bam_tlen_gather(krec, len, pos, tlen, N, tlen_out, (uint64_t *)(own + N * 8) - (N - written), n_cu, st));
	}
	const WindowWriter write = [tlen_out](const sk::WriteWindow &w, int n_cu, hipStream_t s) { return sk::launch_bam_tlen_write(w, tlen_out, n_cu, s); };
	const int rc = rw_begin(c, cl, fr, o, write, level, window_bytes, written, total, n_records, raw_bytes, handled, info);
	if (rc == SK_OK && *handled) {
		RewriteState &s = *o.s;
		s.disc_gen = s.gen; s.n_disc = N - written;
		s.disc = (const uint64_t *)(own + N * 8) - s.n_disc;
		s.d_names = own + a_kept;
		if (n_discarded) *n_discarded = (int64_t)s.n_disc;
	}
	return rc;
}

extern "C" int sk_bam_file_recalc_tlen_discarded(sk_ctx *c, int64_t first, int64_t n, uint8_t *names)
{
	if (!c) return SK_ERR_INVALID;
	Ranges *R = (Ranges *)sk::ctx_ext(c);
	if (!R || !R->rw.current(R->gen) || R->rw.disc_gen != R->gen)
		return sk::ctx_fail(c, SK_ERR_INVALID, "sk_bam_file_recalc_tlen_discarded: no sk_bam_file_recalc_tlen to ask");
	const RewriteState &s = R->rw;
	if (first < 0 || n < 0 || (uint64_t)first > s.n_disc || (uint64_t)n > s.n_disc - (uint64_t)first)
		return sk::ctx_fail(c, SK_ERR_INVALID, "sk_bam_file_recalc_tlen_discarded: records %lld .. +%lld of %llu", (long long)first, (long long)n, (unsigned long long)s.n_disc);
	if (n == 0) return SK_OK;
	if (!names) return sk::ctx_fail(c, SK_ERR_INVALID, "sk_bam_file_recalc_tlen_discarded: names is NULL");
	if (int r = sk::ctx_bind(c)) return r;
	hipStream_t st = sk::ctx_stream(c);
	for (int64_t done = 0; done < n;) {                                   // (a chunk of slots at a time through the staging area)
		const int64_t step = std::min<int64_t>(n - done, (int64_t)RewriteState::kTlenNameSlots);
		BF_HIP(sk::launch_bam_tlen_names(s.d_out, s.disc, first + done, step, s.d_names, sk::ctx_n_cu(c), st));
		BF_HIP(hipMemcpyAsync(names + done * 256, s.d_names, (size_t)step * 256, hipMemcpyDeviceToHost, st));
		BF_HIP(hipStreamSynchronize(st));
		done += step;
	}
	return SK_OK;
}

// ---- sam merge (include/seqkit_hip.h: sk_bam_file_merge; the windows come from sk_bam_file_rewrite_next) ---
// K verified streams at once.  The front half serves one file per ctx and keeps its ranges with it, so every input but the first gets a
// helper context of its own on the same device (kept with the caller's ctx in Ranges::helpers, freed with it, invisible in the C-ABI)
// and the unchanged front half runs in each, one after the other: input 1 in the caller's ctx first — that ends an earlier call's windows
// in flight, which may read the helpers' streams — then the others.  When a front returns its stream is verified, which takes the
// host's word: nothing of it is still running, and every record pass and every window of this call runs on the caller's streams.  All
// streams lie in one address space, so a record is addressed by its offset from input 1's stream mod 2^64 and the window writers keep
// their one base pointer.  The reference names are compared on the host as each front returns.  Then the passes of sk_bammerge.hip:
// keys per input, the order check, the shared sort over all records, the gather and the scan.  Their working memory (29 B per record and
// the scratch of the sort and the scan) lies in input 1's compressed file's device buffer, idle by then, where that is large enough,
// else in ctx slot kKeepPassWork, which always holds the one byte per output record that the windows read with a suffix.  Declined
// files: the list in include/seqkit_hip.h.
extern "C" int sk_bam_file_merge(sk_ctx *c, const char *const *paths, int n_paths, int suffix, int level, uint64_t window_bytes, int64_t *n_records,
                                 uint64_t *raw_bytes, int *handled, double info[8])
{
	if (!c || !paths || !handled) return SK_ERR_INVALID;
	*handled = 0;
	if (info) for (int i = 0; i < 8; i++) info[i] = 0.0;
	if (n_records) *n_records = 0;
	if (raw_bytes) *raw_bytes = 0;
	if (n_paths < 2) return sk::ctx_fail(c, SK_ERR_INVALID, "n_paths = %d", n_paths);
	for (int i = 0; i < n_paths; i++) if (!paths[i]) return sk::ctx_fail(c, SK_ERR_INVALID, "paths[%d] is NULL", i);
	if (level < 0 || level > 1) return sk::ctx_fail(c, SK_ERR_INVALID, "level = %d", level);
	if (int r = sk::ctx_bind(c)) return r;
	if (n_paths > 99) BF_LEAVE(21);                                     // (the suffix writer knows one and two digits)
	const size_t K = (size_t)n_paths;
	// (the helpers' Cleanups are declared first and so run last: the caller's streams are waited for before a helper's tables are freed)
	std::unique_ptr<Cleanup[]> cls(new Cleanup[K]);
	Cleanup cl;
	std::vector<Front> fin(K);
	std::vector<std::string> names0;
	int dev = 0;
	BF_HIP(hipGetDevice(&dev));
	for (size_t i = 0; i < K; i++) {
		fin[i].who = "sk_bam_file_merge";
		if (i == 0) {
			if (int r = bam_file_front(c, paths[0], cls[0], fin[0], info)) return r;
		} else {
			Ranges *both = (Ranges *)sk::ctx_ext(c);
			while (both->helpers.size() < i) {
				sk_ctx *h = nullptr;
				if (sk_create(dev, &h) != SK_OK || !h) BF_LEAVE(21);
				both->helpers.push_back(h);
			}
			sk_ctx *h = both->helpers[i - 1];
			if (int r = bam_file_front(h, paths[i], cls[i], fin[i], info)) return sk::ctx_fail(c, r, "input %zu: %s", i + 1, sk_last_error(h));
		}
		if (!fin[i].ready) return SK_OK;                                  // (info[5] says at which check)
		if (i == 0) names0 = fin[0].refs.names(fin[0].header.data());
		else if (fin[i].refs.names(fin[i].header.data()) != names0) {
			if (getenv("SK_BAMFILE_TRACE")) fprintf(stderr, "sk_bam_file_merge: declined (bits 0x4): input %zu's reference names differ\n", i + 1);
			BF_LEAVE(30 + 4);
		}
	}
	// ---- one front over all inputs for the spine: the blocks and records of all of them in a row, input 1's header and stream
	cl.wait_for = {sk::ctx_stream(c), sk::ctx_stream2(c)};
	Front all = fin[0];
	for (size_t i = 1; i < K; i++) {
		all.nb += fin[i].nb; all.n_records += fin[i].n_records; all.fsize += fin[i].fsize; all.stream_len += fin[i].stream_len; all.n_host += fin[i].n_host;
		all.rounds = std::max(all.rounds, fin[i].rounds);
		all.nrec.insert(all.nrec.end(), fin[i].nrec.begin(), fin[i].nrec.end());
	}
	all.t_walk = now_ms();
	const Front &fr = all;
	const uint64_t N = all.n_records;
	if (N >= ((uint64_t)1 << 32)) BF_LEAVE(21);
	RwOpen o;
	if (int r = rw_open(c, cl, all, 0, o, info)) return r;
	if (!o.s) return SK_OK;
	hipStream_t st = sk::ctx_stream(c);
	const uint8_t *kin = nullptr;
	uint64_t total = 0;
	if (N) {
		passmem::SortBufs sb;
		BF_HIP(pass_temp(sb, N, 64, st, [&](size_t *b) { return sk::bam_merge_scan(nullptr, b, nullptr, N, st); }));
		sk::MergeCols cols;
		passmem::Layout L;
		L.add(sb.key, N * 8); L.add(cols.addr, N * 8); L.add(sb.idx, N * 4); L.add(cols.len, N * 4); L.add(cols.in, N); L.add(sb.temp, sb.temp_bytes);
		const passmem::Placement pl = passmem::place(N, L.total(), fin[0].fsize + 64, false);      // (kept: every output record's input number)
		uint8_t *kb = nullptr;
		if (!pass_memory(c, pl, kb)) BF_LEAVE(21);
		char inputs[32];
		snprintf(inputs, sizeof inputs, "%zu inputs", K);
		pl.trace(fr.who, inputs, "the first compressed file's buffer");
		L.carve(pl.scratch_at(kb, fin[0].d_comp));
		cols.key = sb.key[0]; cols.idx = sb.idx[0];
		// ---- keys and checks, input by input: the call is served or left here
		int64_t b0 = 0;
		for (size_t i = 0; i < K; i++) {
			const uint32_t sl = suffix ? (i + 1 >= 10 ? 3u : 2u) : 0u;
			BF_HIP(sk::launch_bam_merge_keys(fin[i].d_out, fin[i].d_bend, fin[i].d_entry, fin[i].nb, o.d_rb + b0, (uint64_t)(uintptr_t)fin[i].d_out - (uint64_t)(uintptr_t)fin[0].d_out,
			                                 (uint32_t)(i + 1), sl, cols, o.d_decline, st));
			b0 += fin[i].nb;
		}
		BF_HIP(sk::launch_bam_merge_order(cols, N, o.d_decline, st));
		BF_LEAVE_DECLINED(o.d_decline, 0);                              // (1 a suffixed name above 254 bytes, 2 an unsorted input, 8 an invalid record)
		// ---- the order: a stable sort of all records by the key, then every output record's address, offset and input number
		int cur = 0;
		size_t tb = sb.temp_bytes;
		BF_HIP(sk::bam_sort_pairs(sb.temp, &tb, sb.key, sb.idx, N, 64, &cur, st));
		BF_HIP(sk::launch_bam_merge_gather(sb.idx[cur], cols, N, o.s->krec, o.s->kout, kb, st));
		tb = sb.temp_bytes;
		BF_HIP(sk::bam_merge_scan(sb.temp, &tb, o.s->kout, N, st));
		BF_HIP(hipMemcpyAsync(&total, o.s->kout + N, 8, hipMemcpyDeviceToHost, st));
		BF_HIP(hipStreamSynchronize(st));
		if (suffix) kin = kb;
	}
	// (krec: offsets from input 1's stream that reach every input's; without a suffix a record is one copied span)
	WindowWriter write = sk::launch_bam_copy_write;
	if (kin) write = [kin](const sk::WriteWindow &w, int n_cu, hipStream_t s) { return sk::launch_bam_merge_write(w, kin, n_cu, s); };
	return rw_begin(c, cl, all, o, write, level, window_bytes, N, total, n_records, raw_bytes, handled, info);
}

// ---- sam concatenate (include/seqkit_hip.h: sk_bam_file_concatenate; the windows come from sk_bam_file_rewrite_next) ---
// ONE input of the command: the front half, then sk_bamconcat.hip's sizing pass, which leaves every record's stream offset and output
// length (its own and the suffix's) in the two columns of ctx slot kKeepFileCols, and sk_bammerge.hip's scan over them.  No key, no
// sort, no gather, nothing kept for the windows but the number itself; the scan's scratch lies in the compressed file's device
// buffer, idle by then, or where that is too small in ctx slot kKeepPassWork.  The header and the EOF block are the caller's to ask
// for (flags): the ctx holds one input's streams at a time, and the caller chains the inputs.
extern "C" int sk_bam_file_concatenate(sk_ctx *c, const char *path, uint32_t number, int flags, int level, uint64_t window_bytes, int64_t *n_records,
                                       uint64_t *raw_bytes, int *handled, double info[8])
{
	Cleanup cl;
	Front fr;
	if (int r = file_call_open(c, path, "sk_bam_file_concatenate", handled, info, cl, fr, [&] {
		    if (n_records) *n_records = 0;
		    if (raw_bytes) *raw_bytes = 0;
		    if (number == 0) return sk::ctx_fail(c, SK_ERR_INVALID, "number = 0");
		    if (flags & ~(SK_CONCAT_HEADER | SK_CONCAT_EOF)) return sk::ctx_fail(c, SK_ERR_INVALID, "flags = %d", flags);
		    if (level < 0 || level > 1) return sk::ctx_fail(c, SK_ERR_INVALID, "level = %d", level);
		    return (int)SK_OK;
	    }))
		return r;
	if (!fr.ready) return SK_OK;
	const uint64_t N = fr.n_records;
	RwOpen o;
	if (int r = rw_open(c, cl, fr, 0, o, info)) return r;
	if (!o.s) return SK_OK;
	hipStream_t st = sk::ctx_stream(c);
	uint32_t sl = 2;                                                    // '.' and the digits
	for (uint32_t v = number; v >= 10u; v /= 10u) sl++;
	uint64_t total = 0;
	if (N) {
		void *temp = nullptr;
		size_t tb = 0;
		BF_HIP(sk::bam_merge_scan(nullptr, &tb, nullptr, N, st));
		passmem::Layout L;
		L.add(temp, tb);
		const passmem::Placement pl = passmem::place(0, L.total(), fr.fsize + 64, false);
		uint8_t *own = nullptr;
		if (!pass_memory(c, pl, own)) BF_LEAVE(21);
		L.carve(pl.scratch_at(own, fr.d_comp));
		// ---- sizes and checks: the input is served or left here
		BF_HIP(sk::launch_bam_concat_size(fr.d_out, fr.d_bend, fr.d_entry, fr.nb, o.d_rb, sl, o.s->krec, o.s->kout, o.d_decline, st));
		BF_LEAVE_DECLINED(o.d_decline, 0);                              // (1 a suffixed name above 254 bytes, 8 an invalid record)
		BF_HIP(sk::bam_merge_scan(temp, &tb, o.s->kout, N, st));
		BF_HIP(hipMemcpyAsync(&total, o.s->kout + N, 8, hipMemcpyDeviceToHost, st));
		BF_HIP(hipStreamSynchronize(st));
	}
	const WindowWriter write = [number, sl](const sk::WriteWindow &w, int n_cu, hipStream_t s) { return sk::launch_bam_concat_write(w, number, sl, n_cu, s); };
	return rw_begin(c, cl, fr, o, write, level, window_bytes, N, total, n_records, raw_bytes, handled, info, flags);
}

// ---- sam discard tail artifacts (include/seqkit_hip.h: sk_bam_file_discard_tails, _loads; the windows come from sk_bam_file_rewrite_next) ---
// The front half, then sk_bamconcat.hip's sizing pass without a suffix for every record's stream offset, the passes of sk_bamtails.hip
// and sk_bamsubsample.hip's scans and compaction, which leave the WRITTEN records' stream and output offsets where sk_bam_file_rewrite
// leaves every record's.  The genome: the .fai's entries are matched to the header's reference names here, a first pass marks the
// refIDs that mapped records name, and only those chromosomes' spans of the FASTA file are read — 64-bit offsets, newlines and all,
// through two page-locked buffers — into one device buffer that is freed when this call returns: the keep pass is the only reader.
// The working memory (the compressed file's device buffer, idle by then, or where that is too small ctx slot kKeepPassWork): 32 B per
// record, the refID tables and the scratch of the scans and the selection.  What sk_bam_file_discard_tails_loads reads is kept in ctx
// slot kKeepPassWork: 4 B per record, of which the loads take the head.  Declined files: the list in include/seqkit_hip.h.
namespace {
struct FdGuard { int fd = -1; ~FdGuard() { if (fd >= 0) close(fd); } };
}

extern "C" int sk_bam_file_discard_tails(sk_ctx *c, const char *path, const char *fasta_path, const char *const *names, const sk_genome_ref *refs, int32_t n_refs,
                                         uint32_t tail_length, uint32_t min_mismatches, const uint8_t *co_line, uint32_t co_bytes, int level, uint64_t window_bytes,
                                         int64_t *n_records, int64_t *n_total, int64_t *n_failed, int64_t *n_passed, int64_t *n_loads, uint64_t *raw_bytes,
                                         int *handled, double info[8])
{
	Cleanup cl;
	Front fr;
	if (int r = file_call_open(c, path, "sk_bam_file_discard_tails", handled, info, cl, fr, [&] {
		    for (int64_t *p : {n_records, n_total, n_failed, n_passed, n_loads}) if (p) *p = 0;
		    if (raw_bytes) *raw_bytes = 0;
		    if (!fasta_path) return sk::ctx_fail(c, SK_ERR_INVALID, "fasta_path is NULL");
		    if (n_refs < 0 || (n_refs > 0 && (!names || !refs))) return sk::ctx_fail(c, SK_ERR_INVALID, "n_refs = %d", (int)n_refs);
		    for (int32_t i = 0; i < n_refs; i++)
			    if (!names[i] || refs[i].line_bases < 1 || refs[i].line_width < refs[i].line_bases) return sk::ctx_fail(c, SK_ERR_INVALID, "refs[%d]", (int)i);
		    if (tail_length == 0) return sk::ctx_fail(c, SK_ERR_INVALID, "tail_length = 0");
		    if (co_bytes && !co_line) return sk::ctx_fail(c, SK_ERR_INVALID, "co_line is NULL");
		    if (level < 0 || level > 1) return sk::ctx_fail(c, SK_ERR_INVALID, "level = %d", level);
		    return (int)SK_OK;
	    }))
		return r;
	if (!fr.ready) return SK_OK;
	const uint64_t N = fr.n_records;
	if (N >= ((uint64_t)1 << 31)) BF_LEAVE(21);                          // (the reference's counters are i32)
	// ---- the header's references against the .fai's entries (of two lines with one name the later counts), spans inside the file
	const std::vector<std::string> bam_names = fr.refs.names(fr.header.data());
	const int32_t n_bam = (int32_t)std::min<size_t>(bam_names.size(), 0x7fffffff);
	auto declined = [&](uint32_t bits, const char *why) {
		if (getenv("SK_BAMFILE_TRACE")) fprintf(stderr, "%s: declined (bits 0x%x): %s\n", fr.who, bits, why);
	};
	if (n_bam == 0) { declined(4, "the header lists no reference"); BF_LEAVE(30 + 4); }
	FdGuard fa;
	fa.fd = open(fasta_path, O_RDONLY);
	uint64_t fa_size = 0;
	if (fa.fd >= 0) {
		const off_t e = lseek(fa.fd, 0, SEEK_END);
		if (e > 0) fa_size = (uint64_t)e;
	}
	std::vector<sk::TailRef> tab((size_t)n_bam, sk::TailRef{0, 0, 0, 0});
	std::vector<uint64_t> file_off((size_t)n_bam, 0), span((size_t)n_bam, 0);
	for (int32_t t = 0; t < n_bam; t++) {
		for (int32_t i = n_refs - 1; i >= 0; i--) {
			if (bam_names[(size_t)t] != names[i]) continue;
			const sk_genome_ref &g = refs[i];
			if (g.length > ((uint64_t)1 << 40) || g.line_width > ((uint64_t)1 << 40)) break;      // (no chromosome is that long: the span's arithmetic stays in 64 bits)
			const uint64_t sp = g.length ? (g.length - 1) / g.line_bases * g.line_width + (g.length - 1) % g.line_bases + 1 : 0;
			if (g.file_offset > fa_size || sp > fa_size - g.file_offset) break;                   // (a span that ends beyond the file: the caller's reader decides)
			tab[(size_t)t] = sk::TailRef{0, g.length, g.line_bases, g.line_width};
			file_off[(size_t)t] = g.file_offset; span[(size_t)t] = sp;
			break;
		}
	}
	if (tab[0].line_bases == 0) { declined(4, "reference 0 has no chromosome in the FASTA index"); BF_LEAVE(30 + 4); }
	RwOpen o;
	if (int r = rw_open(c, cl, fr, 6, o, info)) return r;
	if (!o.s) return SK_OK;
	hipStream_t st = sk::ctx_stream(c);
	const int n_cu = sk::ctx_n_cu(c);
	uint64_t *d_counts = o.d_blk;                                       // (no per-block column, six words: total, failed, passed, written, written bytes; the loads)
	uint64_t counts[6] = {0, 0, 0, 0, 0, 0};
	const std::vector<uint8_t> more(co_line, co_line + co_bytes);
	int32_t *loads = nullptr;
	if (N) {
		size_t tb = 0, tb2 = 0;
		BF_HIP(sk::bam_sub_scans(nullptr, &tb, nullptr, nullptr, nullptr, N, st));
		BF_HIP(sk::bam_tail_loads(nullptr, &tb2, nullptr, nullptr, nullptr, nullptr, N, st));
		tb = std::max(tb, tb2);
		uint64_t *krec = nullptr, *off = nullptr;
		uint32_t *len = nullptr, *pos = nullptr, *used = nullptr;
		int32_t *tidc = nullptr, *last = nullptr;
		sk::TailRef *d_tab = nullptr;
		void *temp = nullptr;
		passmem::Layout L;
		L.add(krec, N * 8); L.add(off, N * 8 + 8); L.add(len, N * 4); L.add(pos, N * 4); L.add(tidc, N * 4); L.add(last, N * 4);
		L.add(used, (uint64_t)n_bam * 4); L.add(d_tab, (uint64_t)n_bam * sizeof(sk::TailRef)); L.add(temp, tb);
		const passmem::Placement pl = passmem::place(N * 4 + 8, L.total(), fr.fsize + 64, getenv("SK_TAILS_OWN_MEMORY") != nullptr);   // (the knob: for tests of the other placement)
		uint8_t *own = nullptr;
		if (!pass_memory(c, pl, own)) BF_LEAVE(21);
		pl.trace(fr.who, "", "the compressed file's buffer");
		L.carve(pl.scratch_at(own, fr.d_comp));
		loads = (int32_t *)own;
		// ---- every record's stream offset (its length goes where the scan will write): the passes below read valid records only
		BF_HIP(sk::launch_bam_concat_size(fr.d_out, fr.d_bend, fr.d_entry, fr.nb, o.d_rb, 0u, krec, off, o.d_decline, st));
		BF_LEAVE_DECLINED(o.d_decline, 0);                              // (8 an invalid record)
		// ---- the genome: the chromosomes that mapped records name
		std::vector<uint32_t> h_used((size_t)n_bam, 0);
		BF_HIP(sk::launch_bam_tail_used(fr.d_out, krec, N, n_bam, used, n_cu, st));
		BF_HIP(hipMemcpyAsync(h_used.data(), used, (size_t)n_bam * 4, hipMemcpyDeviceToHost, st));
		BF_HIP(hipStreamSynchronize(st));
		uint64_t g_bytes = 0;
		for (int32_t t = 0; t < n_bam; t++) {
			if (!h_used[(size_t)t] || tab[(size_t)t].line_bases == 0) { tab[(size_t)t].line_bases = 0; continue; }   // (not read: no record may reach it)
			tab[(size_t)t].base = g_bytes;
			g_bytes += (span[(size_t)t] + 255) & ~(uint64_t)255;
		}
		const double t_genome = now_ms();
		uint8_t *d_genome = nullptr;
		if (hipMalloc((void **)&d_genome, (size_t)g_bytes + 256) != hipSuccess) { (void)hipGetLastError(); BF_LEAVE(21); }
		cl.dev.push_back(d_genome);
		if (g_bytes) {
			const size_t kStage = (size_t)32 << 20;
			uint8_t *stage[2] = {nullptr, nullptr};
			hipEvent_t sev[2] = {nullptr, nullptr};
			for (int b = 0; b < 2; b++) {
				if (hipHostMalloc((void **)&stage[b], kStage, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); BF_LEAVE(21); }
				cl.pinned.push_back(stage[b]);
				if (hipEventCreateWithFlags(&sev[b], hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); BF_LEAVE(21); }
				cl.events.push_back(sev[b]);
			}
			int b = 0;
			bool busy[2] = {false, false};
			for (int32_t t = 0; t < n_bam; t++) {
				if (tab[(size_t)t].line_bases == 0) continue;
				for (uint64_t done = 0; done < span[(size_t)t];) {
					const size_t step = (size_t)std::min<uint64_t>(span[(size_t)t] - done, kStage);
					if (busy[b]) BF_HIP(hipEventSynchronize(sev[b]));
					for (size_t got = 0; got < step;) {
						const ssize_t r = pread(fa.fd, stage[b] + got, step - got, (off_t)(file_off[(size_t)t] + done + got));
						if (r <= 0) BF_LEAVE(21);                                // (the file changed under the call)
						got += (size_t)r;
					}
					BF_HIP(hipMemcpyAsync(d_genome + tab[(size_t)t].base + done, stage[b], step, hipMemcpyHostToDevice, st));
					BF_HIP(hipEventRecord(sev[b], st));
					busy[b] = true;
					b ^= 1;
					done += step;
				}
			}
		}
		BF_HIP(hipMemcpyAsync(d_tab, tab.data(), (size_t)n_bam * sizeof(sk::TailRef), hipMemcpyHostToDevice, st));
		if (getenv("SK_BAMFILE_TRACE")) {
			BF_HIP(hipStreamSynchronize(st));
			fprintf(stderr, "%s: genome: %llu bytes read and copied in %.1f ms\n", fr.who, (unsigned long long)g_bytes, now_ms() - t_genome);
		}
		// ---- the decisions: the file is served or left here
		BF_HIP(sk::launch_bam_tail_keep(fr.d_out, krec, N, d_genome, d_tab, n_bam, tail_length, min_mismatches, len, tidc, d_counts, o.d_decline, n_cu, st));
		BF_HIP(hipMemcpyAsync(counts, d_counts, 40, hipMemcpyDeviceToHost, st));
		BF_LEAVE_DECLINED(o.d_decline, 0);                              // (1 an operation outside M I D = X, 2 an index out of range, 4 a refID without a chromosome, 16 beyond i32)
		// ---- the chromosome loads, the written records' stream and output offsets
		BF_HIP(sk::bam_tail_loads(temp, &tb, tidc, last, loads, d_counts + 5, N, st));
		BF_HIP(hipMemcpyAsync(counts + 5, d_counts + 5, 8, hipMemcpyDeviceToHost, st));
		BF_HIP(sk::bam_sub_scans(temp, &tb, len, pos, off, N, st));
		BF_HIP(sk::launch_bam_sub_compact(krec, len, pos, off, N, o.s->krec, o.s->kout, st));
		BF_HIP(hipStreamSynchronize(st));
	}
	const int rc = rw_begin(c, cl, fr, o, sk::launch_bam_copy_write, level, window_bytes, counts[3], counts[4], n_records, raw_bytes, handled, info,
	                        SK_CONCAT_HEADER | SK_CONCAT_EOF, &more);
	if (rc == SK_OK && *handled) {
		RewriteState &s = *o.s;
		s.loads_gen = s.gen; s.n_loads = counts[5]; s.loads = loads;
		if (n_total) *n_total = (int64_t)counts[0];
		if (n_failed) *n_failed = (int64_t)counts[1];
		if (n_passed) *n_passed = (int64_t)counts[2];
		if (n_loads) *n_loads = (int64_t)counts[5];
	}
	return rc;
}

extern "C" int sk_bam_file_discard_tails_loads(sk_ctx *c, int64_t first, int64_t n, int32_t *tids)
{
	if (!c) return SK_ERR_INVALID;
	Ranges *R = (Ranges *)sk::ctx_ext(c);
	if (!R || !R->rw.current(R->gen) || R->rw.loads_gen != R->gen)
		return sk::ctx_fail(c, SK_ERR_INVALID, "sk_bam_file_discard_tails_loads: no sk_bam_file_discard_tails to ask");
	const RewriteState &s = R->rw;
	if (first < 0 || n < 0 || (uint64_t)first > s.n_loads || (uint64_t)n > s.n_loads - (uint64_t)first)
		return sk::ctx_fail(c, SK_ERR_INVALID, "sk_bam_file_discard_tails_loads: loads %lld .. +%lld of %llu", (long long)first, (long long)n, (unsigned long long)s.n_loads);
	if (n == 0) return SK_OK;
	if (!tids) return sk::ctx_fail(c, SK_ERR_INVALID, "sk_bam_file_discard_tails_loads: tids is NULL");
	if (int r = sk::ctx_bind(c)) return r;
	hipStream_t st = sk::ctx_stream(c);
	BF_HIP(hipMemcpyAsync(tids, s.loads + first, (size_t)n * 4, hipMemcpyDeviceToHost, st));
	BF_HIP(hipStreamSynchronize(st));
	return SK_OK;
}

extern "C" int sk_bam_file_rewrite_next(sk_ctx *c, sk_bam_out_window *w)
{
	if (!c || !w) return SK_ERR_INVALID;
	memset(w, 0, sizeof *w);
	Ranges *R = (Ranges *)sk::ctx_ext(c);
	if (!R || !R->rw.current(R->gen)) return sk::ctx_fail(c, SK_ERR_INVALID, "sk_bam_file_rewrite_next: no sk_bam_file_rewrite in progress");
	if (int r = sk::ctx_bind(c)) return r;
	RewriteState &s = R->rw;
	const int b = s.cur;
	if (b < 0) {                                                        // the end
		if (s.eof_due) {                                                // (no window carried the EOF block: a call without header and records)
			s.eof_due = false;
			memcpy(s.h_pin[0], bamfmt::kBgzfEof, 28);
			w->bgzf = s.h_pin[0]; w->bytes = 28;
		}
		return SK_OK;
	}
	BF_HIP(hipEventSynchronize(s.ev[b]));
	uint64_t bytes = s.h_size[b];
	int rc = SK_OK;
	s.cur = rw_issue(c, s, b ^ 1, &rc) ? (b ^ 1) : -1;                    // (the buffer of the window returned last time: the caller is done with it)
	if (rc) { s.live = false; return rc; }
	BF_HIP(pack_fetch(c, s, b, bytes));
	if (s.cur < 0 && s.eof_due) { s.eof_due = false; memcpy(s.h_pin[b] + bytes, bamfmt::kBgzfEof, 28); bytes += 28; }   // the last window ends with the EOF block
	w->first = s.first[b]; w->n = s.n[b];
	w->bgzf = s.h_pin[b]; w->bytes = bytes; w->raw_bytes = s.raw[b];
	return SK_OK;
}
