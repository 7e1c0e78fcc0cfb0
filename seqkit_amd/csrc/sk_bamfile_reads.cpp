// sk_bamfile_reads.cpp — sk_bam_file_reads and sk_bam_file_reads_next (include/seqkit_hip.h) behind the front half of sk_bamfile.cpp.
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
// The front half above, then the sizing pass (per block: kept records, text bytes, name bytes, decline bits) and its scans; the
// decision to serve the file is taken there, before any text exists.  Then the kept records' columns, the windows, and the first
// window's text on its way.  Every allocation that fails leaves the file to the caller's reader (info[5] = -21).

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
	hipStream_t st = sk::ctx_stream(c);
	const double t_size = now_ms();
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
	const int64_t K = (int64_t)tot[0];
	const uint64_t T = tot[1], N = tot[2];
	// ---- the kept records' columns: stream offset, text offset, name offset, key, kind
	int krc = SK_OK;
	const size_t kcol = up((uint64_t)K * 8);
	uint8_t *kb = (uint8_t *)sk::ctx_keep(c, sk::kKeepFileCols, kcol * 4 + up((uint64_t)K) + 256, false, &krc);
	if (!kb) BF_LEAVE(21);
	Ranges *R = (Ranges *)sk::ctx_ext(c);
	ReadsState &s = R->reads;
	s.krec = (uint64_t *)kb; s.ktoff = (uint64_t *)(kb + kcol); s.knoff = (uint64_t *)(kb + 2 * kcol); s.kkey = (uint64_t *)(kb + 3 * kcol); s.kkind = kb + 4 * kcol;
	BF_HIP(sk::launch_bam_reads_index(fr.d_out, fr.d_bend, fr.d_entry, nb, format, want_unpaired ? 1 : 0, bk, bt, bn, s.krec, s.ktoff, s.knoff, s.kkey, s.kkind, st));
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
