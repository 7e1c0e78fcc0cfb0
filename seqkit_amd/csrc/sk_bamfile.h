// sk_bamfile.h — what the units of the BAM file calls (include/seqkit_hip.h: sk_bam_file_*) share.  sk_bamfile.cpp holds the front half
// (read, ship, inflate, verify, walk: bam_file_front) and the helpers declared here, with the two calls that keep no state (reduce,
// columns); sk_bamfile_reads.cpp the reads and pairs calls and their windows; sk_bamfile_out.cpp the BAM-writing calls and theirs;
// sk_bamfile_coverage.cpp the coverage call.  Internal to the library.
#pragma once
#include <hip/hip_runtime.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <vector>

#include "../../include/seqkit_hip.h"
#include "sk_bamfmt.h"
#include "sk_internal.h"
#include "sk_passmem.h"

namespace bamfile {

using bamfmt::le32;
using passmem::up;

struct Cleanup {                                 // frees what was allocated, whichever way the function is left
	std::vector<void *> dev, pinned;
	std::vector<hipEvent_t> events;
	std::vector<hipStream_t> streams, wait_for;
	int fd = -1;
	~Cleanup()
	{
		// (the big buffers stay with the ctx: nothing of this call may still be running on them when the next one starts)
		for (hipStream_t s : wait_for) (void)hipStreamSynchronize(s);
		for (hipStream_t s : streams) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); }
		for (void *p : dev) if (p) (void)hipFree(p);
		for (void *p : pinned) if (p) (void)hipHostFree(p);
		for (hipEvent_t e : events) (void)hipEventDestroy(e);
		if (fd >= 0) close(fd);
	}
};

inline double now_ms()
{
	return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// not this path's file: say at which check (info[5] = -check) and leave it to the caller's reader
#define BF_LEAVE(code)                                                                                                  \
	do {                                                                                                                \
		if (info) info[5] = -(double)(code);                                                                            \
		return SK_OK;                                                                                                   \
	} while (0)

// The inflated stream's room: its size is known only when the file's last trailer has been read, and six times the file — what a
// well-compressed BAM needs — is 22 GB for a 3.6 GB file of which 5.5 are used.  Memory of that size given back and taken again is
// what the next call, or the next PROCESS, then waits behind (tools/r06/stall_exp.sh).  So the range is only RESERVED (virtual
// addresses), and physical memory is mapped into it piece by piece as the inflater's frontier moves (hipMemCreate / hipMemMap): what a
// file takes is what it inflates to.  The mapping stays with the ctx.  Where the runtime refuses any of this, plain hipMalloc serves.
struct OutRange {
	uint8_t *va = nullptr;
	size_t reserved = 0, mapped = 0, gran = 0, piece = 0;
	int device = 0;
	std::vector<hipMemGenericAllocationHandle_t> handles;
	bool reserve(size_t bytes, int dev)
	{
		hipMemAllocationProp prop{};
		prop.type = hipMemAllocationTypePinned;
		prop.location.type = hipMemLocationTypeDevice;
		prop.location.id = dev;
		size_t g = 0;
		if (hipMemGetAllocationGranularity(&g, &prop, hipMemAllocationGranularityRecommended) != hipSuccess || g == 0) { (void)hipGetLastError(); return false; }
		gran = g;
		piece = (((size_t)512 << 20) + g - 1) / g * g;
		const size_t want = (bytes + piece - 1) / piece * piece;
		void *p = nullptr;
		if (hipMemAddressReserve(&p, want, 0, nullptr, 0) != hipSuccess || !p) { (void)hipGetLastError(); return false; }
		va = (uint8_t *)p; reserved = want; mapped = 0; device = dev;
		return true;
	}
	bool ensure(size_t bytes)                                            // [0, bytes) is backed by memory
	{
		while (mapped < bytes) {
			if (mapped + piece > reserved) return false;
			hipMemAllocationProp prop{};
			prop.type = hipMemAllocationTypePinned;
			prop.location.type = hipMemLocationTypeDevice;
			prop.location.id = device;
			hipMemGenericAllocationHandle_t h;
			if (hipMemCreate(&h, piece, &prop, 0) != hipSuccess) { (void)hipGetLastError(); return false; }
			if (hipMemMap(va + mapped, piece, 0, h, 0) != hipSuccess) { (void)hipGetLastError(); (void)hipMemRelease(h); return false; }
			hipMemAccessDesc acc{};
			acc.location.type = hipMemLocationTypeDevice;
			acc.location.id = device;
			acc.flags = hipMemAccessFlagsProtReadWrite;
			if (hipMemSetAccess(va + mapped, piece, &acc, 1) != hipSuccess) { (void)hipGetLastError(); (void)hipMemUnmap(va + mapped, piece); (void)hipMemRelease(h); return false; }
			handles.push_back(h);
			mapped += piece;
		}
		return true;
	}
	void release()
	{
		for (size_t i = 0; i < handles.size(); i++) { (void)hipMemUnmap(va + i * piece, piece); (void)hipMemRelease(handles[i]); }
		handles.clear();
		if (va) (void)hipMemAddressFree(va, reserved);
		va = nullptr; reserved = mapped = 0;
	}
	static void destroy(void *p) { OutRange *r = (OutRange *)p; r->release(); delete r; }
};

// an event the host sleeps on (created once, kept with the state); false: the runtime refused it
inline bool blocking_event(hipEvent_t &e)
{
	if (!e && hipEventCreateWithFlags(&e, hipEventBlockingSync | hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); e = nullptr; return false; }
	return true;
}

// The double buffer of a windowed file call (sk_bam_file_reads; sk_bam_file_rewrite, _minimize, _markdup and _subsample): the window plan, the next window to issue, and per
// buffer the window in it and the event its work ends with.  One window is in flight while the caller works on the other.
struct WindowedState {
	bool live = false;
	uint64_t gen = 0;                            // Ranges::gen of the file call that set it up
	const uint8_t *d_out = nullptr;              // the verified stream
	std::vector<uint64_t> ws;                    // window w: records ws[w] .. ws[w + 1]
	size_t next_w = 0;                           // the next window to issue
	hipEvent_t ev[2] = {nullptr, nullptr};
	int64_t first[2] = {0, 0}, n[2] = {0, 0};
	int cur = -1;                                // the buffer whose window is in flight, -1: none (the end)
	~WindowedState() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
	bool busy() const { return live || cur >= 0; }
	void stop() { live = false; cur = -1; }
	bool current(uint64_t file_gen) const { return live && gen == file_gen; }     // (a *_next call continues it)
	void begin(const uint8_t *stream, uint64_t file_gen) { d_out = stream; gen = file_gen; next_w = 0; cur = -1; }
	bool next_window(size_t &w)                  // the next non-empty window of the plan; false: none left
	{
		while (next_w + 1 < ws.size() && ws[next_w + 1] == ws[next_w]) next_w++;
		if (next_w + 1 >= ws.size()) return false;
		w = next_w++;
		return true;
	}
};

// The window area of a call whose windows leave as BGZF members (the BAM-writing calls; sk_bam_file_pairs_gz): one device area for the
// window's raw bytes, the block table, the deflate's results, CRCs, member sizes, slots and tokens, and two packed-member buffers on
// each side (ctx slots kKeepFileWin / kKeepFilePin).  pack_area sizes and takes it for windows of at most max_raw bytes (false: it cannot
// be had); pack_issue is what follows once a window's raw_len bytes lie in d_raw: cut, deflate or crc, pack into packed buffer b, the packed
// size back, and `done` recorded; pack_fetch copies buffer b's `bytes` to its page-locked twin on the second stream and waits for them.
struct PackArea {
	int level = 1;
	uint8_t *d_raw = nullptr, *d_slots = nullptr, *d_pack[2] = {nullptr, nullptr}, *h_pin[2] = {nullptr, nullptr};
	uint32_t *d_tokens = nullptr, *d_result = nullptr, *d_crc = nullptr;
	uint64_t *d_msz = nullptr, *h_size = nullptr;   // h_size[b]: window b's packed bytes (page-locked)
	void *d_blocks = nullptr;
	hipEvent_t ev_copy[2] = {nullptr, nullptr};     // the copy of packed buffer b on the second stream
	~PackArea() { for (hipEvent_t e : ev_copy) if (e) (void)hipEventDestroy(e); }
};
bool pack_area(sk_ctx *c, PackArea &a, uint64_t max_raw, int level);
hipError_t pack_issue(sk_ctx *c, PackArea &a, uint64_t raw_len, int b, hipEvent_t done);
hipError_t pack_fetch(sk_ctx *c, PackArea &a, int b, uint64_t bytes);

// sk_bam_file_reads / sk_bam_file_reads_next (`sam to`): the kept records' columns (device, ctx slot kKeepFileCols), the window plan (text and name
// bytes of window w from wt[w] / wn[w] on), and two window buffers on each side (ctx slots kKeepFileWin / kKeepFilePin)
struct ReadsState : WindowedState {
	int fmt = 0;
	uint8_t min_baseq = 10;
	uint64_t *krec = nullptr, *ktoff = nullptr, *knoff = nullptr, *kkey = nullptr;
	uint8_t *kkind = nullptr;
	std::vector<uint64_t> wt, wn;
	uint8_t *d_win[2] = {nullptr, nullptr}, *h_win[2] = {nullptr, nullptr};
	size_t at_toff = 0, at_noff = 0, at_names = 0, at_kind = 0, at_key = 0;   // a window buffer's layout (text at 0)
};

// sk_bam_file_pairs / sk_bam_file_pairs_next (`sam to`, the texts in output order): the kept records' stream offsets (device, ctx slot
// kKeepFileCols), every stream's permutation rank -> record and stream offsets (device, the kept head of ctx slot kKeepPassWork; stream s
// from entry base[s] + s on), the windows of all streams in the order they are returned — stream 1's, stream 2's, the single stream's —
// and two text buffers on each side (ctx slots kKeepFileWin / kKeepFilePin) or, for sk_bam_file_pairs_gz / sk_bam_file_pairs_gz_next, the
// window area of the BAM-writing calls in the same slots.  (ws / next_window of the base are not used: a window here
// is a rank range of ONE stream.)
struct PairsState : WindowedState {
	int fmt = 0;
	uint8_t min_baseq = 10;
	const uint64_t *krec = nullptr, *soff = nullptr;
	const uint32_t *perm = nullptr;
	uint64_t base[3] = {0, 0, 0};
	struct Window { int stream; uint64_t first, n, bytes; };
	std::vector<Window> plan;
	uint8_t *d_win[2] = {nullptr, nullptr}, *h_win[2] = {nullptr, nullptr};
	Window in[2] = {};                           // the window in buffer b
	bool members = false;                        // sk_bam_file_pairs_gz: a window's text goes to pk.d_raw and leaves as members (d_win / h_win idle)
	PackArea pk;
};

// What writes a window's records for the rewrite-window call that is running: that call's launcher (sk_internal.h: launch_bam_*_write)
// with the call's own arguments bound.  (Device columns among them lie in ctx slot kKeepPassWork, which lives as long as the windows.)
typedef std::function<hipError_t(const sk::WriteWindow &w, int n_cu, hipStream_t st)> WindowWriter;

// sk_bam_file_rewrite / sk_bam_file_minimize / sk_bam_file_markdup / sk_bam_file_subsample and sk_bam_file_rewrite_next: every written record's stream and output offsets
// (device, ctx slot kKeepFileCols), the window plan (output bytes of window w from wo[w] on), the write kernel of the call that runs,
// one device area for the window being rewritten and compressed (raw bytes, deflate scratch, blocks) and two packed-member buffers on
// each side (ctx slots kKeepFileWin / kKeepFilePin)
struct RewriteState : WindowedState, PackArea {
	WindowWriter write;
	uint64_t *krec = nullptr, *kout = nullptr;
	std::vector<uint64_t> wo;
	std::vector<uint8_t> header;                 // the output header (the first window); empty: the call writes none (sk_bam_file_concatenate)
	bool header_done = false;
	bool eof_due = true;                         // the 28-byte EOF block is still to come (false from the start: the call writes none)
	uint64_t raw[2] = {0, 0};
	// sk_bam_file_recalc_tlen_discarded: the discarded records' stream offsets in file order and a staging area of kTlenNameSlots name
	// slots (device, the kept head of ctx slot kKeepPassWork), of the file call disc_gen (0: none)
	static constexpr uint64_t kTlenNameSlots = 4096;
	uint64_t disc_gen = 0, n_disc = 0;
	const uint64_t *disc = nullptr;
	uint8_t *d_names = nullptr;
	// sk_bam_file_discard_tails_loads: the refIDs of the chromosome loads after the first, in file order (device, the kept head of ctx
	// slot kKeepPassWork), of the file call loads_gen (0: none)
	uint64_t loads_gen = 0, n_loads = 0;
	const int32_t *loads = nullptr;
};

// what stays with the ctx: the range of the compressed file and the range of the inflated stream
struct Ranges {
	OutRange comp, out;
	std::vector<uint8_t> header;                 // sk_bam_file_columns: the last file's header bytes (cols->header)
	uint64_t gen = 0;                            // file calls so far: a reads state of an earlier call is stale
	ReadsState reads;                            // (only one of the three is live: the next file call, windowed or not, ends each)
	RewriteState rw;
	PairsState pairs;
	std::vector<sk_ctx *> helpers;               // sk_bam_file_merge: one context per further input, whose front half keeps that input's stream
	static void destroy(void *p)
	{
		Ranges *r = (Ranges *)p;
		for (sk_ctx *h : r->helpers) sk_destroy(h);
		r->comp.release(); r->out.release();
		delete r;
	}
};

#define BF_HIP(call)                                                                                                    \
	do {                                                                                                                \
		hipError_t e_ = (call);                                                                                         \
		if (e_ != hipSuccess) return sk::ctx_fail(c, SK_ERR_HIP, "%s: %s", #call, hipGetErrorString(e_));               \
	} while (0)

// What the front half of a file call leaves behind: the verified stream on the device (the inflated blocks back to back, readable
// 64 bytes beyond; block_end and entry of the walk) and, on the host, the per-block record counts and the header bytes.  ready = false
// (info[5] = -check): the file is not one this path serves.  The device buffers of d_bend / d_entry belong to the caller's Cleanup.
struct Front {
	const char *who = nullptr;                   // the file call, in trace lines and messages
	bool ready = false;
	const uint8_t *d_out = nullptr;
	uint8_t *d_comp = nullptr;                   // the compressed file's device buffer (fsize + 64 bytes): idle once the stream is verified
	uint64_t stream_len = 0, first = 0, n_records = 0, fsize = 0, n_host = 0;
	uint64_t *d_bend = nullptr, *d_entry = nullptr;
	int64_t nb = 0;
	int rounds = 0;
	int32_t n_ref = -1;
	std::vector<uint32_t> nrec;                  // records begun in block c
	std::vector<uint8_t> header;                 // "BAM\1" .. the end of the reference list (first bytes)
	bamfmt::RefList refs;                        // the reference list as parsed: offsets into header
	double t0 = 0, t_alloc = 0, t_read = 0, t_inflated = 0, t_header = 0, t_walk = 0;
};

int bam_file_front(sk_ctx *c, const char *path, Cleanup &cl, Front &fr, double info[8]);
void file_call_close(const Front &fr, const char *stage, double t_stage, const char *tail, double info[8]);
int block_first_records(sk_ctx *c, const Front &fr, std::vector<uint64_t> &rb);
int plan_windows(sk_ctx *c, Cleanup &cl, uint64_t window_bytes, const uint64_t *off0, const uint64_t *off1, uint64_t n, uint64_t total0,
                 uint64_t total1, WindowedState &s, std::vector<uint64_t> &w0, std::vector<uint64_t> *w1, uint64_t max[3], bool *room);
int read_decline(sk_ctx *c, const char *who, const uint32_t *d_decline, uint32_t found);

// The opening every file call shares: with c, path and handled given, *handled = 0 and info cleared, then the call's own checks (`check`:
// SK_OK or an error code), the device bound and the front half run.  SK_OK with fr.ready = false: not this path's file (info[5] says why).
template <class Check>
int file_call_open(sk_ctx *c, const char *path, const char *who, int *handled, double info[8], Cleanup &cl, Front &fr, Check check)
{
	if (!c || !path || !handled) return SK_ERR_INVALID;
	*handled = 0;
	if (info) for (int i = 0; i < 8; i++) info[i] = 0.0;
	if (int r = check()) return r;
	if (int r = sk::ctx_bind(c)) return r;
	fr.who = who;
	return bam_file_front(c, path, cl, fr, info);
}

#define BF_LEAVE_DECLINED(d_decline, found)                                                                             \
	do {                                                                                                                \
		const int d_ = read_decline(c, fr.who, d_decline, found);                                                       \
		if (d_) { if (d_ < 0) return SK_ERR_HIP; BF_LEAVE(30 + d_); }                                                   \
	} while (0)

// ---- the record passes' working memory (sk_passmem.h) on the device ----
// what the sort of n pairs by key_bits bits and the call's scan (`scan(&bytes)`) ask for as scratch: the larger into sb.temp_bytes
template <class Scan>
hipError_t pass_temp(passmem::SortBufs &sb, uint64_t n, int key_bits, hipStream_t st, Scan scan)
{
	size_t sort_bytes = 0, scan_bytes = 0;
	hipError_t e = sk::bam_sort_pairs(nullptr, &sort_bytes, sb.key, sb.idx, n, key_bits, nullptr, st);
	if (e == hipSuccess) e = scan(&scan_bytes);
	sb.want(sort_bytes); sb.want(scan_bytes);
	return e;
}
// the call's own buffer as pl sizes it: ctx slot kKeepPassWork (own stays nullptr where pl needs none); false: that memory cannot be had
inline bool pass_memory(sk_ctx *c, const passmem::Placement &pl, uint8_t *&own)
{
	if (!pl.own_bytes()) return true;
	int krc = SK_OK;
	own = (uint8_t *)sk::ctx_keep(c, sk::kKeepPassWork, pl.own_bytes(), false, &krc);
	return own != nullptr;
}

}  // namespace bamfile
