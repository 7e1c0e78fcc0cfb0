// sk_bamfile.cpp — sk_bam_file_reduce (include/seqkit_hip.h): `sam statistics` / `sam fragment lengths` over a BAM FILE with
// the device doing what htslib does for the reference (src/common.rs:121-157): inflate every BGZF block, check its CRC-32, walk
// the records — and then the reduction (src/sam_statistics.rs:63-69, src/sam_fragment_lengths.rs:29-43).
//
// The host's part is what only it can do: read the file (a few threads pread it into pinned buffers, in order), ship the
// COMPRESSED bytes, and follow the chain of BGZF headers — 18 bytes per block that say where the next one begins (BSIZE) —
// reading, next to each, the trailer's CRC32 and ISIZE: that is the block table the inflate kernel takes.  Blocks are inflated
// in batches as their bytes arrive (the copy of the next chunk runs under the kernel of the last), into ONE buffer that holds
// the whole inflated stream: records may straddle blocks as they like, the walk sees a plain byte stream.
//
// Nothing here decides that a file is bad.  Whatever is not a regular, complete BGZF file whose every block inflates (on the
// device, or — the blocks the device gave up — with zlib here) to the size and CRC its trailer states, and whose records
// chain from the end of the header exactly to the end of the stream, is left to the caller's record-at-a-time reader
// (*handled = 0), which produces what the reference would.
#include <fcntl.h>
#include <hip/hip_runtime.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <condition_variable>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/seqkit_hip.h"
#include "sk_bamfmt.h"
#include "sk_internal.h"

using bamfmt::le32;

namespace {

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

double now_ms()
{
	return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

bool pread_full(int fd, uint8_t *dst, size_t n, uint64_t off)
{
	size_t got = 0;
	while (got < n) {
		const ssize_t r = pread(fd, dst + got, n - got, (off_t)(off + got));
		if (r < 0) { if (errno == EINTR) continue; return false; }
		if (r == 0) return false;
		got += (size_t)r;
	}
	return true;
}

}  // namespace

static inline size_t up(uint64_t v) { return (size_t)((v + 255) & ~(uint64_t)255); }   // to the next multiple of 256

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

// (mapping a piece takes ~12 ms — the driver hands out cleared memory —: a thread of its own maps ahead of the frontier while the
// caller's thread reads the file)
struct Mapper {
	OutRange *r = nullptr;
	std::thread th;
	std::mutex m;
	std::condition_variable cv;
	size_t want = 0, have = 0;
	bool stop = false, failed = false;
	void start(OutRange *range)
	{
		r = range; have = r->mapped;
		th = std::thread([this] {
			(void)hipSetDevice(r->device);
			std::unique_lock<std::mutex> lk(m);
			for (;;) {
				cv.wait(lk, [this] { return stop || want > have; });
				if (stop) return;
				const size_t next = have + 1;
				lk.unlock();
				const bool ok = r->ensure(next);                             // one piece
				lk.lock();
				if (!ok) { failed = true; cv.notify_all(); return; }
				have = r->mapped;
				cv.notify_all();
			}
		});
	}
	void ask(size_t bytes) { std::lock_guard<std::mutex> lk(m); if (bytes > want) { want = std::min(bytes, r->reserved); cv.notify_all(); } }
	bool wait_for(size_t bytes) { std::unique_lock<std::mutex> lk(m); if (bytes > want) { want = std::min(bytes, r->reserved); cv.notify_all(); } cv.wait(lk, [&] { return failed || have >= bytes; }); return !failed; }
	~Mapper() { if (th.joinable()) { { std::lock_guard<std::mutex> lk(m); stop = true; cv.notify_all(); } th.join(); } }
};
// an event the host sleeps on (created once, kept with the state); false: the runtime refused it
static bool blocking_event(hipEvent_t &e)
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

// Which of the rewrite-window calls is running — the kernel that writes a window's records — and what that kernel takes
struct WriteOp {
	enum Kind { kRewrite, kMinimize, kMarkdup, kSubsample, kMerge } kind = kRewrite;
	int flags = 0;                               // kRewrite: SK_REWRITE_*; kMinimize: SK_MINIMIZE_*
	uint8_t fill = 255;                          // kMinimize: the qualities' fill byte
	const uint32_t *ids = nullptr;               // kMinimize: the read ids (ctx slot kKeepPassWork; nullptr without SK_MINIMIZE_READ_IDS)
	const uint16_t *md_flags = nullptr;          // kMarkdup: every record's flag (ctx slot kKeepPassWork)
	const uint8_t *merge_in = nullptr;           // kMerge: every output record's input number (ctx slot kKeepPassWork); nullptr without --suffix
};

// sk_bam_file_rewrite / sk_bam_file_minimize / sk_bam_file_markdup / sk_bam_file_subsample and sk_bam_file_rewrite_next: every written record's stream and output offsets
// (device, ctx slot kKeepFileCols), the window plan (output bytes of window w from wo[w] on), the write kernel of the call that runs,
// one device area for the window being rewritten and compressed (raw bytes, deflate scratch, blocks) and two packed-member buffers on
// each side (ctx slots kKeepFileWin / kKeepFilePin)
struct RewriteState : WindowedState {
	WriteOp write;
	int level = 1;
	uint64_t *krec = nullptr, *kout = nullptr;
	std::vector<uint64_t> wo;
	std::vector<uint8_t> header;                 // the output header (the first window)
	bool header_done = false;
	uint8_t *d_raw = nullptr, *d_slots = nullptr, *d_pack[2] = {nullptr, nullptr}, *h_pin[2] = {nullptr, nullptr};
	uint32_t *d_tokens = nullptr, *d_result = nullptr, *d_crc = nullptr;
	uint64_t *d_msz = nullptr, *h_size = nullptr;   // h_size[b]: window b's packed bytes (page-locked)
	void *d_blocks = nullptr;
	hipEvent_t ev_copy[2] = {nullptr, nullptr};     // the copy of packed buffer b on the second stream
	uint64_t raw[2] = {0, 0};
	~RewriteState() { for (hipEvent_t e : ev_copy) if (e) (void)hipEventDestroy(e); }
};

// what stays with the ctx: the range of the compressed file and the range of the inflated stream
struct Ranges {
	OutRange comp, out;
	std::vector<uint8_t> header;                 // sk_bam_file_columns: the last file's header bytes (cols->header)
	uint64_t gen = 0;                            // file calls so far: a reads state of an earlier call is stale
	ReadsState reads;                            // (only one of the two is live: the next file call, windowed or not, ends either)
	RewriteState rw;
	std::vector<sk_ctx *> helpers;               // sk_bam_file_merge: one context per further input, whose front half keeps that input's stream
	static void destroy(void *p)
	{
		Ranges *r = (Ranges *)p;
		for (sk_ctx *h : r->helpers) sk_destroy(h);
		r->comp.release(); r->out.release();
		delete r;
	}
};

// The readers: threads that pread the file's chunks, in order, into a ring of page-locked buffers — chunk k into slot k mod R, once the
// copy of chunk k - R out of that slot has been issued and is done — while the caller's thread takes the chunks in order, issues their
// copies and follows the BGZF headers in them.  (A thread per piece of every chunk, started and joined chunk by chunk, left the file
// unread while the headers of a chunk were followed: 3 600 thread starts for a 3.6 GB file.)
struct Readers {
	int fd = -1;
	uint8_t *ring = nullptr;
	size_t chunk = 0;
	uint64_t fsize = 0, n_chunks = 0;
	int R = 0;
	std::vector<hipEvent_t> ev;                  // slot s: the copy out of it
	std::vector<int64_t> ready, copied;          // slot s: the chunk whose bytes are in it / whose copy has been issued (and its headers followed)
	std::vector<std::thread> th;
	std::mutex m;
	std::condition_variable cv;
	uint64_t next = 0;
	bool stop = false, failed = false;
	int device = 0;
	void start(int threads)
	{
		ready.assign((size_t)R, -1); copied.assign((size_t)R, -1);
		for (int t = 0; t < threads; t++) th.emplace_back([this] {
			(void)hipSetDevice(device);
			for (;;) {
				uint64_t k;
				{
					std::unique_lock<std::mutex> lk(m);
					if (stop || next >= n_chunks) return;
					k = next++;
					const int s = (int)(k % (uint64_t)R);
					if (k >= (uint64_t)R) {
						cv.wait(lk, [&] { return stop || copied[(size_t)s] == (int64_t)(k - (uint64_t)R); });
						if (stop) return;
					}
				}
				const int s = (int)(k % (uint64_t)R);
				if (k >= (uint64_t)R) (void)hipEventSynchronize(ev[(size_t)s]);     // (outside the lock: the copy out of the slot)
				const uint64_t off = k * chunk;
				const size_t len = (size_t)std::min<uint64_t>(chunk, fsize - off);
				const bool ok = pread_full(fd, ring + (size_t)s * chunk, len, off);
				std::lock_guard<std::mutex> lk(m);
				if (!ok) failed = true;
				ready[(size_t)s] = (int64_t)k;
				cv.notify_all();
			}
		});
	}
	bool wait_ready(uint64_t k)                   // chunk k is in its slot (false: a read failed)
	{
		std::unique_lock<std::mutex> lk(m);
		const int s = (int)(k % (uint64_t)R);
		cv.wait(lk, [&] { return failed || ready[(size_t)s] == (int64_t)k; });
		return !failed;
	}
	void done_with(uint64_t k)                    // its copy is issued (and recorded in ev), nobody reads the slot any more
	{
		std::lock_guard<std::mutex> lk(m);
		copied[(size_t)(k % (uint64_t)R)] = (int64_t)k;
		cv.notify_all();
	}
	~Readers()
	{
		{ std::lock_guard<std::mutex> lk(m); stop = true; cv.notify_all(); }
		for (auto &t : th) t.join();
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
	double t0 = 0, t_alloc = 0, t_read = 0, t_inflated = 0, t_header = 0, t_walk = 0;
};

// open and stat, the buffers, the readers, the BGZF headers and the batches of inflate launches, zlib for the blocks the device gave up,
// the BAM header, the walk and its verification: everything the file calls do before they read the records.  fr.who names the caller
// in trace lines.
static int bam_file_front(sk_ctx *c, const char *path, Cleanup &cl, Front &fr, double info[8])
{
	const char *who = fr.who;
	Ranges *both = (Ranges *)sk::ctx_ext(c);
	if (!both) { both = new Ranges; sk::ctx_set_ext(c, both, Ranges::destroy); }
	// an earlier sk_bam_file_reads may have left a window in flight on the ctx stream: its text kernel reads the inflated stream and its
	// copies write the page-locked window buffers.  It ends before this call remaps the ranges or takes the kept buffers again.
	// (the same for an sk_bam_file_rewrite, _minimize or _markdup, whose window copies run on the second stream)
	if (both->reads.busy() || both->rw.busy()) {
		BF_HIP(hipStreamSynchronize(sk::ctx_stream(c)));
		BF_HIP(hipStreamSynchronize(sk::ctx_stream2(c)));
	}
	both->gen++;                                                        // (what an earlier windowed call left is no longer read)
	both->reads.stop();
	both->rw.stop();
	cl.fd = open(path, O_RDONLY);
	if (cl.fd < 0) BF_LEAVE(1);                                        // (the caller's reader says so in the reference's words)
	struct stat sb;
	if (fstat(cl.fd, &sb) != 0 || !S_ISREG(sb.st_mode) || sb.st_size < 28) BF_LEAVE(2);
	const uint64_t fsize = (uint64_t)sb.st_size;
	const double t0 = now_ms();
	hipStream_t st = sk::ctx_stream(c), st2 = sk::ctx_stream2(c);
	cl.wait_for = {st, st2};

	// ---- device buffers: the compressed file, and room for the inflated stream (its size is known only when the last
	// trailer has been read: six times the file — a BAM inflates three- to fourfold — or what the device has left).  They STAY WITH
	// THE CTX from one call to the next (sk::ctx_keep; sk_destroy frees them): a process that gave 20 GB back and asked for them again
	// found one call in three waiting 1.3-2.4 s in its reading loop — the copies queue behind what the driver does with memory
	// that changes hands (with a third of the room: none in nine calls; the first call of a process: never).
	int krc = SK_OK;
	uint64_t out_cap = std::max<uint64_t>(fsize * 6, (uint64_t)256 << 20);
	if (const char *ev = getenv("SK_BAMFILE_OUT_FACTOR")) { const int f = atoi(ev); if (f >= 1 && f <= 1100) out_cap = std::max<uint64_t>(fsize * (uint64_t)f, (uint64_t)1 << 20); }
	uint8_t *d_out = nullptr, *d_comp = nullptr;
	OutRange *range = nullptr, *crange = nullptr;
	if (!getenv("SK_BAMFILE_NO_VMM")) {
		int dev = 0;
		BF_HIP(hipGetDevice(&dev));
		if (both->out.va && both->out.reserved < out_cap + 256) both->out.release();
		if (both->comp.va && both->comp.reserved < fsize + 64) both->comp.release();
		// (the compressed file's range only for big files: mapping costs ~12 ms per 512 MiB whoever asks, a plain allocation of a few GB
		// 6-20 ms — it was an 18 GB one that waited 1.6 s behind another process's exit)
		const bool comp_mapped = fsize > ((uint64_t)8 << 30);
		if (!comp_mapped && both->comp.va) both->comp.release();
		if ((both->out.va || both->out.reserve(out_cap + 256, dev)) && (!comp_mapped || both->comp.va || both->comp.reserve(fsize + 64, dev))) {
			range = &both->out;
			crange = comp_mapped ? &both->comp : nullptr;
		}
	}
	Mapper mapper, cmapper;
	if (range) {
		out_cap = range->reserved - 256;                                 // (a batch asks for its last byte + 128)
		d_out = range->va;
		if (crange) {
			d_comp = crange->va;
			cmapper.start(crange);
			cmapper.ask((size_t)fsize + 64);                              // (all of the file's range, ahead of the readers)
		} else {
			d_comp = (uint8_t *)sk::ctx_keep(c, sk::kKeepComp, fsize + 64, false, &krc);
			if (!d_comp) return krc;
		}
		mapper.start(range);
		mapper.ask(std::min<size_t>((size_t)fsize * 2, range->reserved));   // (a BAM inflates at least that far: on its way before the first byte is read)
	} else if (sk::ctx_kept_bytes(c, sk::kKeepOut) >= out_cap + 64) {
		out_cap = sk::ctx_kept_bytes(c, sk::kKeepOut) - 64;                   // (what an earlier call took: all of it is room)
		d_out = (uint8_t *)sk::ctx_keep(c, sk::kKeepOut, out_cap + 64, false, &krc);
		d_comp = (uint8_t *)sk::ctx_keep(c, sk::kKeepComp, fsize + 64, false, &krc);
		if (!d_comp) return krc;
	} else {
		d_comp = (uint8_t *)sk::ctx_keep(c, sk::kKeepComp, fsize + 64, false, &krc);
		if (!d_comp) return krc;
		size_t free_b = 0, total_b = 0;
		BF_HIP(hipMemGetInfo(&free_b, &total_b));
		out_cap = std::min<uint64_t>(out_cap, (uint64_t)((free_b + sk::ctx_kept_bytes(c, sk::kKeepOut)) * 0.8));
		d_out = (uint8_t *)sk::ctx_keep(c, sk::kKeepOut, out_cap + 64, false, &krc);
		if (!d_out) BF_LEAVE(3);
	}

	// ---- read, ship, follow the headers; inflate batch by batch
	size_t chunk = (size_t)4 << 20;                                      // (a ring of 4 MiB page-locked buffers, one and a half per reader: 48 MiB for 8 readers)
	if (const char *ev = getenv("SK_BAMFILE_CHUNK_LOG2")) { const int lg = atoi(ev); if (lg >= 12 && lg <= 30) chunk = (size_t)1 << lg; }
	int threads = 8;                                                    // (3.6 GB from the page cache: 165-185 ms with 4 readers, 130-155 with 8, the same with 12)
	{ const unsigned hc = std::thread::hardware_concurrency(); if (hc >= 1 && hc < 8) threads = (int)hc; }
	if (const char *ev = getenv("SK_BAMFILE_THREADS")) { const int t = atoi(ev); if (t >= 1 && t <= 64) threads = t; }
	const int kBufs = threads + threads / 2 + 1;
	Readers rd;
	rd.fd = cl.fd; rd.chunk = chunk; rd.fsize = fsize; rd.R = kBufs;
	rd.ring = (uint8_t *)sk::ctx_keep(c, sk::kKeepPin, (size_t)kBufs * chunk, true, &krc);
	if (!rd.ring) return krc;
	BF_HIP(hipGetDevice(&rd.device));
	for (int i = 0; i < kBufs; i++) {
		hipEvent_t e;
		BF_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
		cl.events.push_back(e);
		rd.ev.push_back(e);
	}
	hipEvent_t ev_batch;
	BF_HIP(hipEventCreateWithFlags(&ev_batch, hipEventDisableTiming));
	cl.events.push_back(ev_batch);

	// the block table (pinned: its batches are copied while the next ones are written) and its device copy: room for blocks of
	// 8 KiB on average — a file of smaller ones is not worth this path
	const size_t tab_cap = (size_t)(fsize / 8192) + 1024;
	struct BlockTable {
		sk_bgzf_block *p = nullptr;
		size_t n = 0;
		size_t size() const { return n; }
		sk_bgzf_block *data() const { return p; }
		sk_bgzf_block &operator[](size_t i) const { return p[i]; }
	} blocks;
	blocks.p = (sk_bgzf_block *)sk::ctx_keep(c, sk::kKeepTable, tab_cap * sizeof(sk_bgzf_block), true, &krc);
	if (!blocks.p) return krc;
	std::vector<uint64_t> bend;
	bend.reserve(tab_cap);
	const double t_alloc_pre = now_ms();
	(void)t_alloc_pre;
	sk_bgzf_block *d_blocks = (sk_bgzf_block *)sk::ctx_keep(c, sk::kKeepBlocks, tab_cap * sizeof(sk_bgzf_block), false, &krc);
	if (!d_blocks) return krc;
	uint32_t *d_status = (uint32_t *)sk::ctx_keep(c, sk::kKeepStatus, tab_cap * sizeof(uint32_t), false, &krc);
	if (!d_status) return krc;

	const double t_alloc = now_ms();
	// A launch is a wave per block, and a CU holds 16 of them: a batch is a whole number of such rounds (what is left over of
	// 8 192 + a chunk's blocks would be a last round that fills a fifth of the chip for as long as a full one takes: 16 ms for a
	// block of literals), and batches alternate between two streams, so that one batch's last waves and the next one's first
	// share the chip.
	const size_t slots = (size_t)sk::ctx_n_cu(c) * 16;
	size_t min_batch = 2 * slots;
	if (const char *ev = getenv("SK_BAMFILE_BATCH")) { const int v = atoi(ev); if (v >= 1) min_batch = (size_t)v; }
	bool whole_rounds = true, two_streams = true;
	if (const char *ev = getenv("SK_BAMFILE_ROUNDS")) whole_rounds = atoi(ev) != 0;
	if (const char *ev = getenv("SK_BAMFILE_STREAMS")) two_streams = atoi(ev) >= 2;
	hipStream_t st_b = st;
	hipEvent_t ev_b = nullptr;
	if (two_streams) {
		BF_HIP(hipStreamCreateWithFlags(&st_b, hipStreamNonBlocking));
		cl.streams.push_back(st_b);
		BF_HIP(hipEventCreateWithFlags(&ev_b, hipEventDisableTiming));
		cl.events.push_back(ev_b);
	}
	int n_batches = 0;
	uint64_t scan = 0, out_off = 0;                                     // the next header's file offset; bytes of the stream so far
	size_t launched = 0;                                                // blocks handed to the device
	bool eof_block_last = false;
	const uint64_t n_chunks = (fsize + chunk - 1) / chunk;
	uint8_t carry[65536 + 64];                                          // a header or trailer that straddles two chunks is read again (pread: rare, and cached)
	rd.n_chunks = n_chunks;
	rd.start(threads);
	for (uint64_t k = 0; k < n_chunks; k++) {
		const uint64_t c_off = k * chunk;
		const size_t c_len = (size_t)std::min<uint64_t>(chunk, fsize - c_off);
		uint8_t *buf = rd.ring + (size_t)(k % (uint64_t)kBufs) * chunk;
		if (!rd.wait_ready(k)) BF_LEAVE(4);
		if (crange && !cmapper.wait_for((size_t)(c_off + c_len) + 64)) BF_LEAVE(3);
		BF_HIP(hipMemcpyAsync(d_comp + c_off, buf, c_len, hipMemcpyHostToDevice, st2));
		BF_HIP(hipEventRecord(rd.ev[(size_t)(k % (uint64_t)kBufs)], st2));
		// the blocks that are complete with this chunk
		const uint64_t have = c_off + c_len;
		auto bytes = [&](uint64_t off, size_t n) -> const uint8_t * {   // n bytes of the file at off (off + n <= have)
			if (off >= c_off) return buf + (off - c_off);
			if (n > sizeof carry || !pread_full(cl.fd, carry, n, off)) return nullptr;
			return carry;
		};
		const size_t first_new = blocks.size();
		while (scan + 18 <= have) {
			const uint8_t *h = bytes(scan, 18);
			if (!h) BF_LEAVE(5);
			if (h[0] != 31 || h[1] != 139 || h[2] != 8 || !(h[3] & 4)) BF_LEAVE(6);          // not a BGZF block: the caller's reader sorts it out
			const size_t xlen = (size_t)h[10] | ((size_t)h[11] << 8);
			if (scan + 12 + xlen > have) break;
			const uint8_t *x = bytes(scan, 12 + xlen);
			if (!x) BF_LEAVE(7);
			size_t bsize = 0;
			for (size_t o = 12; o + 4 <= 12 + xlen;) {
				const size_t slen = (size_t)x[o + 2] | ((size_t)x[o + 3] << 8);
				if (x[o] == 'B' && x[o + 1] == 'C' && slen == 2 && o + 6 <= 12 + xlen) { bsize = ((size_t)x[o + 4] | ((size_t)x[o + 5] << 8)) + 1; break; }
				o += 4 + slen;
			}
			if (bsize == 0 || bsize < 12 + xlen + 8) BF_LEAVE(8);
			if (scan + bsize > have) break;                                 // its trailer comes with a later chunk
			const uint8_t *tr = bytes(scan + bsize - 8, 8);
			if (!tr) BF_LEAVE(9);
			sk_bgzf_block b;
			b.in_off = scan + 12 + xlen;
			b.in_len = (uint32_t)(bsize - 12 - xlen - 8);
			b.crc32 = le32(tr);
			b.out_len = le32(tr + 4);
			b.out_off = out_off;
			b.reserved = 0;
			if (b.out_len > 65536u) BF_LEAVE(10);                            // (BGZF: at most 64 KiB per block)
			out_off += b.out_len;
			if (out_off > out_cap) BF_LEAVE(11);                             // inflates further than the room taken: the caller's reader streams it
			if (blocks.n >= tab_cap) BF_LEAVE(12);
			blocks.p[blocks.n++] = b;
			bend.push_back(out_off);
			eof_block_last = b.out_len == 0;
			scan += bsize;
		}
		// a batch of blocks: copied on st2, inflated on st behind the copy.  A launch wants thousands of blocks (a wave per block,
		// 16 waves per CU: 4 096 in flight): the blocks of several chunks go together
		(void)first_new;
		size_t n_new = blocks.size() - launched;
		const bool last = k + 1 == n_chunks;
		if (n_new && (n_new >= min_batch || last)) {
			if (!last && whole_rounds && n_new >= slots) n_new -= n_new % slots;      // (what is left over goes with the next batch)
			const size_t first_new = launched;
			if (range) {
				const size_t upto = (size_t)(blocks[first_new + n_new - 1].out_off + blocks[first_new + n_new - 1].out_len) + 128;
				mapper.ask(upto + ((size_t)3 << 29));                        // (three pieces ahead)
				if (!mapper.wait_for(upto)) BF_LEAVE(3);
			}
			hipStream_t sb = (n_batches & 1) ? st_b : st;
			BF_HIP(hipMemcpyAsync(d_blocks + first_new, blocks.data() + first_new, n_new * sizeof(sk_bgzf_block), hipMemcpyHostToDevice, st2));
			BF_HIP(hipEventRecord(ev_batch, st2));
			BF_HIP(hipStreamWaitEvent(sb, ev_batch, 0));
			BF_HIP(sk::launch_bgzf_inflate(d_comp, d_blocks + first_new, (int64_t)n_new, d_out, d_status + first_new, 1, sk::ctx_n_cu(c), sb));
			launched += n_new;
			n_batches++;
		}
		rd.done_with(k);                                                  // (the chunk's headers have been followed: its slot may be read into again once the copy is through)
	}
	if (two_streams) {                                                   // what follows on st comes behind both streams' batches
		BF_HIP(hipEventRecord(ev_b, st_b));
		BF_HIP(hipStreamWaitEvent(st, ev_b, 0));
	}
	if (scan != fsize) BF_LEAVE(13);                                     // bytes behind the last whole block: a file cut short, or not BGZF to its end
	(void)eof_block_last;                                               // (htslib only warns when the EOF marker is missing; the data are the same)
	if (launched != blocks.size()) BF_LEAVE(13);
	const int64_t nb = (int64_t)blocks.size();
	const uint64_t stream_len = out_off;
	const double t_read = now_ms();
	BF_HIP(hipStreamSynchronize(st2));
	// ---- blocks the device gave up: zlib here
	std::vector<uint32_t> status((size_t)nb);
	BF_HIP(hipMemcpyAsync(status.data(), d_status, (size_t)nb * 4, hipMemcpyDeviceToHost, st));
	{	// (a blocking event: the thread sleeps while the device inflates instead of spinning on the stream)
		hipEvent_t ev_done;
		BF_HIP(hipEventCreateWithFlags(&ev_done, hipEventBlockingSync | hipEventDisableTiming));
		cl.events.push_back(ev_done);
		BF_HIP(hipEventRecord(ev_done, st));
		BF_HIP(hipEventSynchronize(ev_done));
	}
	const double t_inflated = now_ms();
	uint64_t n_host = 0;
	{
		std::vector<uint8_t> cbuf, obuf;
		for (int64_t i = 0; i < nb; i++) {
			if (status[(size_t)i] == 0) continue;
			const sk_bgzf_block &b = blocks[(size_t)i];
			if (getenv("SK_BAMFILE_TRACE")) fprintf(stderr, "%s: block %lld (in %u bytes at %llu, out %u) has status %#x: zlib\n", who, (long long)i, b.in_len, (unsigned long long)b.in_off, b.out_len, status[(size_t)i]);
			cbuf.resize(b.in_len ? b.in_len : 1);
			obuf.resize(b.out_len ? b.out_len : 1);
			if (b.in_len && !pread_full(cl.fd, cbuf.data(), b.in_len, b.in_off)) BF_LEAVE(14);
			z_stream z;
			memset(&z, 0, sizeof z);
			if (inflateInit2(&z, -15) != Z_OK) BF_LEAVE(15);
			z.next_in = cbuf.data(); z.avail_in = b.in_len;
			z.next_out = obuf.data(); z.avail_out = b.out_len;
			const int zr = inflate(&z, Z_FINISH);
			const bool ok = zr == Z_STREAM_END && z.total_out == b.out_len;
			inflateEnd(&z);
			if (!ok) BF_LEAVE(16);                                           // zlib rejects it too: the caller's reader reports it
			if ((uint32_t)crc32(crc32(0L, Z_NULL, 0), obuf.data(), b.out_len) != b.crc32) BF_LEAVE(17);
			if (b.out_len) BF_HIP(hipMemcpy(d_out + b.out_off, obuf.data(), b.out_len, hipMemcpyHostToDevice));
			n_host++;
		}
	}
	// ---- the BAM header: magic, text, references (SAMv1 §4.2) — where the first record begins
	uint64_t first = 0;
	int32_t n_ref_hdr = -1;
	std::vector<uint8_t> hd_keep;
	{
		std::vector<uint8_t> &hd = hd_keep;
		size_t want = (size_t)std::min<uint64_t>(stream_len, (uint64_t)1 << 20);
		for (;;) {
			hd.resize(want);
			if (want) BF_HIP(hipMemcpy(hd.data(), d_out, want, hipMemcpyDeviceToHost));
			bool more = false, bad = false;
			auto need = [&](uint64_t end) { if (end > want) { (end > stream_len ? bad : more) = true; return false; } return true; };
			uint64_t o = 0;
			do {
				if (!need(12)) break;
				if (memcmp(hd.data(), "BAM\1", 4) != 0) { bad = true; break; }
				o = 8 + (uint64_t)le32(hd.data() + 4);
				if (!need(o + 4)) break;
				const uint32_t n_ref = le32(hd.data() + o);
				n_ref_hdr = n_ref <= 0x7fffffffu ? (int32_t)n_ref : -1;
				o += 4;
				for (uint32_t r = 0; r < n_ref && !bad && !more; r++) {
					if (!need(o + 4)) break;
					const uint64_t l_name = le32(hd.data() + o);
					if (l_name > (1u << 20)) { bad = true; break; }              // (the caller's reader refuses such a header)
					o += 4 + l_name + 4;
					if (!need(o)) break;
				}
			} while (false);
			if (bad) BF_LEAVE(18);
			if (!more) { first = o; break; }
			if (want >= stream_len) BF_LEAVE(19);
			want = (size_t)std::min<uint64_t>(stream_len, (uint64_t)want * 4);
		}
	}
	const double t_header = now_ms();
	// ---- the records: walk and verify
	uint64_t *d_bend = nullptr, *d_entry = nullptr, *d_exit = nullptr;
	uint32_t *d_nrec = nullptr;
	BF_HIP(hipMalloc((void **)&d_bend, (size_t)(nb + 1) * 8)); cl.dev.push_back(d_bend);
	BF_HIP(hipMalloc((void **)&d_entry, (size_t)(nb + 1) * 8)); cl.dev.push_back(d_entry);
	BF_HIP(hipMalloc((void **)&d_exit, (size_t)(nb + 1) * 8)); cl.dev.push_back(d_exit);
	BF_HIP(hipMalloc((void **)&d_nrec, (size_t)(nb + 2) * 4)); cl.dev.push_back(d_nrec);
	BF_HIP(hipMemcpyAsync(d_bend, bend.data(), (size_t)nb * 8, hipMemcpyHostToDevice, st));
	BF_HIP(hipMemsetAsync(d_out + stream_len, 0, 64, st));               // (the walk reads whole dwords)
	int verified = 0, rounds = 0;
	uint64_t n_records = 0;
	int max_rounds = 64;
	if (const char *ev = getenv("SK_BAMFILE_MAX_ROUNDS")) { const int v = atoi(ev); if (v >= 1) max_rounds = v; }
	if (int r = sk_bam_walk_dev(c, d_out, stream_len, d_bend, nb, first, n_ref_hdr, d_entry, d_exit, d_nrec, max_rounds, &verified, &n_records, &rounds)) return r;
	if (!verified) BF_LEAVE(20);
	fr.nrec.resize((size_t)nb);
	if (nb) BF_HIP(hipMemcpy(fr.nrec.data(), d_nrec, (size_t)nb * 4, hipMemcpyDeviceToHost));
	fr.header.assign(hd_keep.begin(), hd_keep.begin() + (ptrdiff_t)first);
	fr.ready = true;
	fr.d_out = d_out; fr.d_comp = d_comp; fr.stream_len = stream_len; fr.first = first; fr.n_records = n_records; fr.fsize = fsize; fr.n_host = n_host;
	fr.d_bend = d_bend; fr.d_entry = d_entry; fr.nb = nb; fr.rounds = rounds; fr.n_ref = n_ref_hdr;
	fr.t0 = t0; fr.t_alloc = t_alloc; fr.t_read = t_read; fr.t_inflated = t_inflated; fr.t_header = t_header; fr.t_walk = now_ms();
	return SK_OK;
}

// The opening every file call shares: with c, path and handled given, *handled = 0 and info cleared, then the call's own checks (`check`:
// SK_OK or an error code), the device bound and the front half run.  SK_OK with fr.ready = false: not this path's file (info[5] says why).
template <class Check>
static int file_call_open(sk_ctx *c, const char *path, const char *who, int *handled, double info[8], Cleanup &cl, Front &fr, Check check)
{
	if (!c || !path || !handled) return SK_ERR_INVALID;
	*handled = 0;
	if (info) for (int i = 0; i < 8; i++) info[i] = 0.0;
	if (int r = check()) return r;
	if (int r = sk::ctx_bind(c)) return r;
	fr.who = who;
	return bam_file_front(c, path, cl, fr, info);
}

// The closing every file call shares: the trace line (the front half's stages, the walk up to t_stage, the call's own `stage` from
// there, and `tail`) and info[].
static void file_call_close(const Front &fr, const char *stage, double t_stage, const char *tail, double info[8])
{
	if (getenv("SK_BAMFILE_TRACE"))
		fprintf(stderr, "%s: alloc %.1f ms, read + copy + launches %.1f ms, wait for the inflate %.1f ms, host blocks + header %.1f ms, walk %.1f ms, %s %.1f ms; %lld blocks, %llu by zlib%s\n",
		        fr.who, fr.t_alloc - fr.t0, fr.t_read - fr.t_alloc, fr.t_inflated - fr.t_read, fr.t_header - fr.t_inflated, t_stage - fr.t_header, stage,
		        now_ms() - t_stage, (long long)fr.nb, (unsigned long long)fr.n_host, tail);
	if (!info) return;
	info[0] = (double)fr.fsize; info[1] = (double)fr.stream_len; info[2] = (double)fr.nb; info[3] = (double)fr.n_records;
	info[4] = (double)fr.n_host; info[5] = (double)fr.rounds; info[6] = fr.t_read - fr.t0; info[7] = now_ms() - fr.t_read;
}

// where every block's first record goes: the exclusive prefix of the walk's per-block counts, rb[nb] = the records
static int block_first_records(sk_ctx *c, const Front &fr, std::vector<uint64_t> &rb)
{
	rb.resize((size_t)fr.nb + 1);
	uint64_t run = 0;
	for (int64_t i = 0; i < fr.nb; i++) { rb[(size_t)i] = run; run += fr.nrec[(size_t)i]; }
	rb[(size_t)fr.nb] = run;
	if (run != fr.n_records)
		return sk::ctx_fail(c, SK_ERR_HIP, "%s: %llu records by the blocks' counts, %llu by the walk", fr.who, (unsigned long long)run, (unsigned long long)fr.n_records);
	return SK_OK;
}

// The window plan of a windowed call (sk_internal.h: launch_bam_windows): window w holds the records whose off0 + off1 bytes (off1 ==
// nullptr: off0) lie in [w W, (w + 1) W), W = window_bytes (0: 64 MiB) kept within [256 B, 1 GiB]; one record may go beyond.  s.ws, w0
// and w1 (only with off1) come back with an entry past the last window; max[0 .. 2] = the most records, off0 bytes and off1 bytes of any
// window.  *room = false: no device memory for the plan.
static int plan_windows(sk_ctx *c, Cleanup &cl, uint64_t window_bytes, const uint64_t *off0, const uint64_t *off1, uint64_t n, uint64_t total0,
                        uint64_t total1, WindowedState &s, std::vector<uint64_t> &w0, std::vector<uint64_t> *w1, uint64_t max[3], bool *room)
{
	*room = true;
	uint64_t W = window_bytes ? window_bytes : (uint64_t)64 << 20;
	W = std::min<uint64_t>(std::max<uint64_t>(W, 256), (uint64_t)1 << 30);
	const int64_t nw = n ? (int64_t)((total0 + total1) / W + 2) : 1;
	s.ws.assign((size_t)nw, n); w0.assign((size_t)nw, total0);
	if (w1) w1->assign((size_t)nw, total1);
	if (n) {
		hipStream_t st = sk::ctx_stream(c);
		uint64_t *d_w = nullptr;
		if (hipMalloc((void **)&d_w, (size_t)nw * (w1 ? 24 : 16)) != hipSuccess) { (void)hipGetLastError(); *room = false; return SK_OK; }
		cl.dev.push_back(d_w);
		BF_HIP(sk::launch_bam_windows(off0, off1, (int64_t)n, W, total0, total1, d_w, d_w + nw, w1 ? d_w + 2 * nw : nullptr, nw, st));
		BF_HIP(hipMemcpyAsync(s.ws.data(), d_w, (size_t)nw * 8, hipMemcpyDeviceToHost, st));
		BF_HIP(hipMemcpyAsync(w0.data(), d_w + nw, (size_t)nw * 8, hipMemcpyDeviceToHost, st));
		if (w1) BF_HIP(hipMemcpyAsync(w1->data(), d_w + 2 * nw, (size_t)nw * 8, hipMemcpyDeviceToHost, st));
		BF_HIP(hipStreamSynchronize(st));
	}
	max[0] = max[1] = max[2] = 0;
	for (size_t w = 0; w + 1 < (size_t)nw; w++) {
		max[0] = std::max(max[0], s.ws[w + 1] - s.ws[w]);
		max[1] = std::max(max[1], w0[w + 1] - w0[w]);
		if (w1) max[2] = std::max(max[2], (*w1)[w + 1] - (*w1)[w]);
	}
	return SK_OK;
}

// The decline word of a call's record passes, read back: the copy, the wait for the stream (and so for every copy issued before), and
// under SK_BAMFILE_TRACE the line that names the caller.  The bits, `found` (what the caller has seen itself) among them: the file is
// left to the caller's reader with info[5] = -(30 + bits); < 0: the copy failed, and the message is set.
static int read_decline(sk_ctx *c, const char *who, const uint32_t *d_decline, uint32_t found)
{
	hipStream_t st = sk::ctx_stream(c);
	uint32_t word = 0;
	hipError_t e = hipMemcpyAsync(&word, d_decline, 4, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess) e = hipStreamSynchronize(st);
	if (e != hipSuccess) { sk::ctx_fail(c, SK_ERR_HIP, "%s: the decline word: %s", who, hipGetErrorString(e)); return -1; }
	word |= found;
	if (word && getenv("SK_BAMFILE_TRACE")) fprintf(stderr, "%s: declined (bits %#x)\n", who, word);
	return (int)word;
}
#define BF_LEAVE_DECLINED(d_decline, found)                                                                             \
	do {                                                                                                                \
		const int d_ = read_decline(c, fr.who, d_decline, found);                                                       \
		if (d_) { if (d_ < 0) return SK_ERR_HIP; BF_LEAVE(30 + d_); }                                                   \
	} while (0)

extern "C" int sk_bam_file_reduce(sk_ctx *c, const char *path, int32_t max_frag, uint64_t counters[3], uint64_t *hist, uint64_t *hist_total,
                                  int *handled, double info[8])
{
	Cleanup cl;
	Front fr;
	if (int r = file_call_open(c, path, "sk_bam_file_reduce", handled, info, cl, fr, [&] {
		    if (max_frag < 0) return sk::ctx_fail(c, SK_ERR_INVALID, "max_frag = %d", max_frag);
		    if (!counters && !hist) return sk::ctx_fail(c, SK_ERR_INVALID, "nothing to do");
		    return (int)SK_OK;
	    }))
		return r;
	if (!fr.ready) return SK_OK;
	// ---- the records: reduce
	hipStream_t st = sk::ctx_stream(c);
	uint64_t *d_red = nullptr;
	const size_t nred = 4 + (size_t)max_frag + 1;
	BF_HIP(hipMalloc((void **)&d_red, nred * 8)); cl.dev.push_back(d_red);
	BF_HIP(hipMemsetAsync(d_red, 0, nred * 8, st));
	if (int r = sk_bam_walk_reduce_dev(c, fr.d_out, fr.stream_len, fr.d_bend, fr.d_entry, fr.nb, max_frag, counters ? 1 : 0, hist ? 1 : 0, d_red)) return r;
	std::vector<uint64_t> red(nred);
	BF_HIP(hipMemcpyAsync(red.data(), d_red, nred * 8, hipMemcpyDeviceToHost, st));
	BF_HIP(hipStreamSynchronize(st));
	if (counters) for (int i = 0; i < 3; i++) counters[i] += red[(size_t)i];
	if (hist) {
		if (hist_total) *hist_total += red[3];
		for (size_t i = 0; i <= (size_t)max_frag; i++) hist[i] += red[4 + i];
	}
	*handled = 1;
	file_call_close(fr, "reduce", fr.t_walk, "", info);
	return SK_OK;
}

// The records of the verified stream as SoA columns (include/seqkit_hip.h): the front half above, then one gather launch.  The
// columns stay with the ctx (one allocation, each column 256-byte aligned); what cannot be had — the file, or the memory for the
// columns — leaves *handled = 0 for the caller's reader.
extern "C" int sk_bam_file_columns(sk_ctx *c, const char *path, uint32_t want, sk_bam_columns *cols, int *handled, double info[8])
{
	if (!cols) return SK_ERR_INVALID;
	Cleanup cl;
	Front fr;
	if (int r = file_call_open(c, path, "sk_bam_file_columns", handled, info, cl, fr, [&] {
		    memset(cols, 0, sizeof *cols);
		    if (want & ~(uint32_t)SK_COL_ALL) return sk::ctx_fail(c, SK_ERR_INVALID, "want = %#x", want);
		    return (int)SK_OK;
	    }))
		return r;
	if (!fr.ready) return SK_OK;
	hipStream_t st = sk::ctx_stream(c);
	const double t_gather = now_ms();
	// ---- the columns: one kept allocation
	const uint64_t n = fr.n_records;
	static const size_t width[8] = {2, 1, 4, 4, 4, 4, 4, 4};               // SK_COL_FLAG .. SK_COL_END
	size_t at[8], total = 0;
	for (int k = 0; k < 8; k++) {
		at[k] = total;
		if (want & (1u << k)) total += ((size_t)n * width[k] + 16 + 255) & ~(size_t)255;
	}
	int krc = SK_OK;
	uint8_t *base = (uint8_t *)sk::ctx_keep(c, sk::kKeepCols, total ? total : 256, false, &krc);
	if (!base) BF_LEAVE(21);                                             // (a busy device: the caller's reader serves the file)
	void *col[8];
	for (int k = 0; k < 8; k++) col[k] = (want & (1u << k)) ? (void *)(base + at[k]) : nullptr;
	std::vector<uint64_t> rb;
	if (int r = block_first_records(c, fr, rb)) return r;
	if (want && fr.nb) {
		uint64_t *d_rb = nullptr;
		BF_HIP(hipMalloc((void **)&d_rb, rb.size() * 8)); cl.dev.push_back(d_rb);
		BF_HIP(hipMemcpyAsync(d_rb, rb.data(), rb.size() * 8, hipMemcpyHostToDevice, st));
		BF_HIP(sk::launch_bam_gather(fr.d_out, fr.stream_len, fr.d_bend, fr.d_entry, d_rb, fr.nb, (uint16_t *)col[0], (uint8_t *)col[1], (int32_t *)col[2],
		                             (int32_t *)col[3], (int32_t *)col[4], (int32_t *)col[5], (int32_t *)col[6], (int32_t *)col[7], st));
	}
	BF_HIP(hipStreamSynchronize(st));
	Ranges *keep = (Ranges *)sk::ctx_ext(c);
	keep->header.swap(fr.header);
	cols->n = (int64_t)n;
	cols->flag = (uint16_t *)col[0]; cols->mapq = (uint8_t *)col[1]; cols->tid = (int32_t *)col[2]; cols->mtid = (int32_t *)col[3];
	cols->pos = (int32_t *)col[4]; cols->mpos = (int32_t *)col[5]; cols->tlen = (int32_t *)col[6]; cols->end_pos = (int32_t *)col[7];
	cols->header = keep->header.data();
	cols->header_len = keep->header.size();
	cols->n_ref = fr.n_ref;
	*handled = 1;
	file_call_close(fr, "gather", t_gather, "", info);
	return SK_OK;
}

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
	const size_t kcol = ((size_t)K * 8 + 255) & ~(size_t)255;
	uint8_t *kb = (uint8_t *)sk::ctx_keep(c, sk::kKeepFileCols, kcol * 4 + (((size_t)K + 255) & ~(size_t)255) + 256, false, &krc);
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

// ---- BAM out (include/seqkit_hip.h: sk_bam_file_rewrite, sk_bam_file_minimize, sk_bam_file_markdup, sk_bam_file_subsample; sk_bam_file_rewrite_next) ---
// The front half above, then the call's own passes, among them a sizing pass (per block: output bytes, decline bits) and its scan; the
// decision to serve the file is taken there, before any window exists.  Then every record's stream and output offsets, the windows, and
// the header's members on their way.  A window is rewritten into one device buffer, cut into blocks of at most 0xff00 bytes, deflated where it lies and packed into
// complete members; only the members' bytes are copied back.  Every allocation that fails leaves the file to the caller's reader
// (info[5] = -21).

// the header (first) or window w of the plan (the next non-empty one) into packed buffer b: rewrite, cut, deflate, pack, and the packed
// size back; false: nothing left
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
		const WriteOp &op = s.write;
		switch (op.kind) {
		case WriteOp::kRewrite: e = sk::launch_bam_rw_write(s.d_out, s.krec, s.kout, first, n, s.wo[w], op.flags, s.d_raw, sk::ctx_n_cu(c), st); break;
		case WriteOp::kMinimize: e = sk::launch_bam_min_write(s.d_out, s.krec, s.kout, op.ids, first, n, s.wo[w], op.flags, op.fill, s.d_raw, sk::ctx_n_cu(c), st); break;
		case WriteOp::kMarkdup: e = sk::launch_bam_md_write(s.d_out, s.krec, s.kout, op.md_flags, first, n, s.wo[w], s.d_raw, sk::ctx_n_cu(c), st); break;
		case WriteOp::kSubsample: e = sk::launch_bam_sub_write(s.d_out, s.krec, s.kout, first, n, s.wo[w], s.d_raw, sk::ctx_n_cu(c), st); break;
		case WriteOp::kMerge:                                               // (krec: offsets from input 1's stream that reach every input's; without a suffix a record is one copied span)
			e = op.merge_in ? sk::launch_bam_merge_write(s.d_out, s.krec, s.kout, op.merge_in, first, n, s.wo[w], s.d_raw, sk::ctx_n_cu(c), st)
			                : sk::launch_bam_sub_write(s.d_out, s.krec, s.kout, first, n, s.wo[w], s.d_raw, sk::ctx_n_cu(c), st);
			break;
		}
	}
	const int64_t nblk = (int64_t)((raw_len + SK_DEFLATE_MAX_IN - 1) / SK_DEFLATE_MAX_IN);
	if (e == hipSuccess) e = hipMemsetAsync(s.d_raw + raw_len, 0, 8, st);              // (the deflate reads whole dwords)
	if (e == hipSuccess) e = hipStreamWaitEvent(st, s.ev_copy[b], 0);                   // (the copy out of this packed buffer)
	if (e == hipSuccess) e = sk::launch_bgzf_cut(raw_len, s.d_blocks, nblk, st);
	if (e == hipSuccess) e = s.level ? sk::launch_bgzf_deflate(s.d_raw, s.d_blocks, nblk, s.d_slots, SK_DEFLATE_SLOT, s.d_tokens, s.d_result, s.d_crc, sk::ctx_n_cu(c), st)
	                                 : sk::launch_bgzf_crc(s.d_raw, s.d_blocks, nblk, s.d_crc, sk::ctx_n_cu(c), st);
	if (e == hipSuccess) e = sk::launch_bgzf_pack(s.d_raw, s.d_blocks, nblk, s.d_slots, SK_DEFLATE_SLOT, s.d_result, s.d_crc, s.level ? 0 : 1, s.d_msz,
	                                              s.d_pack[b], sk::ctx_n_cu(c), st);
	if (e == hipSuccess) e = hipMemcpyAsync(s.h_size + b, s.d_msz + nblk, 8, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess) e = hipEventRecord(s.ev[b], st);
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
// or for sk_bam_file_subsample the kept ones —: the window plan, the window area, and the header's members on their way.  `write`: the
// kernel that writes a window; `total`: the records' output bytes.
static int rw_begin(sk_ctx *c, Cleanup &cl, const Front &fr, const RwOpen &o, const WriteOp &write, int level, uint64_t window_bytes, uint64_t N,
                    uint64_t total, int64_t *n_records, uint64_t *raw_bytes, int *handled, double info[8])
{
	RewriteState &s = *o.s;
	int krc = SK_OK;
	// ---- the windows: at most W rewritten bytes each
	uint64_t mx[3];                                                     // records, rewritten bytes
	bool room = true;
	if (int r = plan_windows(c, cl, window_bytes, s.kout, nullptr, N, total, 0, s, s.wo, nullptr, mx, &room)) return r;
	if (!room) BF_LEAVE(21);
	s.header = bamfmt::rewrite_header(fr.header);
	const uint64_t max_raw = std::max<uint64_t>(s.header.size(), mx[1]);
	// ---- the window area: raw bytes, blocks, deflate scratch and slots, member sizes, two packed buffers (device); two page-locked ones
	const uint64_t nblk = std::max<uint64_t>(1, (max_raw + SK_DEFLATE_MAX_IN - 1) / SK_DEFLATE_MAX_IN);
	const uint64_t pack = max_raw + nblk * 31 + 64;
	const size_t a_raw = up(max_raw + 64), a_blk = up(nblk * 16), a_res = up(nblk * 8), a_crc = up(nblk * 4), a_msz = up((nblk + 1) * 8), a_pack = up(pack);
	const size_t a_slots = level ? up(nblk * (uint64_t)SK_DEFLATE_SLOT) : 0, a_tok = level ? up(nblk * sk::deflate_tokens_per_block() * 4) : 0;
	uint8_t *dw = (uint8_t *)sk::ctx_keep(c, sk::kKeepFileWin, a_raw + a_blk + a_res + a_crc + a_msz + 2 * a_pack + a_slots + a_tok, false, &krc);
	if (!dw) BF_LEAVE(21);
	const size_t p_pack = up(pack + 28);
	uint8_t *hw = (uint8_t *)sk::ctx_keep(c, sk::kKeepFilePin, 2 * p_pack + 64, true, &krc);
	if (!hw) BF_LEAVE(21);
	s.d_raw = dw; s.d_blocks = dw + a_raw; s.d_result = (uint32_t *)(dw + a_raw + a_blk); s.d_crc = (uint32_t *)(dw + a_raw + a_blk + a_res);
	s.d_msz = (uint64_t *)(dw + a_raw + a_blk + a_res + a_crc);
	uint8_t *dp = dw + a_raw + a_blk + a_res + a_crc + a_msz;
	s.d_pack[0] = dp; s.d_pack[1] = dp + a_pack;
	s.d_slots = level ? dp + 2 * a_pack : nullptr;
	s.d_tokens = level ? (uint32_t *)(dp + 2 * a_pack + a_slots) : nullptr;
	s.h_pin[0] = hw; s.h_pin[1] = hw + p_pack; s.h_size = (uint64_t *)(hw + 2 * p_pack);
	for (int b = 0; b < 2; b++)
		if (!blocking_event(s.ev[b]) || !blocking_event(s.ev_copy[b])) BF_LEAVE(21);
	for (int b = 0; b < 2; b++) BF_HIP(hipEventRecord(s.ev_copy[b], sk::ctx_stream2(c)));   // (nothing to wait for before the first copy)
	s.write = write; s.level = level; s.header_done = false;
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
	return rw_begin(c, cl, fr, o, WriteOp{WriteOp::kRewrite, op}, level, window_bytes, fr.n_records, total, n_records, raw_bytes, handled, info);
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
		uint64_t *key[2] = {nullptr, nullptr};
		uint32_t *idx[2] = {nullptr, nullptr};
		size_t temp_bytes = 0;
		BF_HIP(sk::bam_sort_pairs(nullptr, &temp_bytes, key, idx, N, bits, nullptr, st));
		const size_t a_key = up(N * 8), a_idx = up(N * 4), a_agg = up((N / 1024 + 2) * 4);
		int krc = SK_OK;
		uint8_t *mb = (uint8_t *)sk::ctx_keep(c, sk::kKeepPassWork, 2 * a_key + 2 * a_idx + a_agg + up(temp_bytes), false, &krc);
		if (!mb) BF_LEAVE(21);
		key[0] = (uint64_t *)mb; key[1] = (uint64_t *)(mb + a_key);
		idx[0] = (uint32_t *)(mb + 2 * a_key); idx[1] = (uint32_t *)(mb + 2 * a_key + a_idx);
		uint32_t *agg = (uint32_t *)(mb + 2 * a_key + 2 * a_idx);
		BF_HIP(sk::launch_bam_min_keys(fr.d_out, fr.d_bend, fr.d_entry, nb, o.d_rb, bits, sk::IdRule{0, 0u}, krec, key[0], idx[0], o.d_decline, st));
		BF_LEAVE_DECLINED(o.d_decline, 0);                              // (the passes below read the names of valid records only)
		int cur = 0;
		BF_HIP(sk::bam_sort_pairs(mb + 2 * a_key + 2 * a_idx + a_agg, &temp_bytes, key, idx, N, bits, &cur, st));
		uint32_t *src = (uint32_t *)key[cur ^ 1], *cnt = src + N;
		BF_HIP(sk::launch_bam_min_ids(fr.d_out, krec, key[cur], idx[cur], N, bits, sk::IdRule{0, 0u}, agg, src, cnt, idx[cur ^ 1], o.d_decline, st));
		ids = idx[cur ^ 1];
	}
	// ---- the sizing pass: per block the output bytes (then their exclusive offsets), the decline bits
	BF_HIP(sk::launch_bam_min_size(fr.d_out, fr.d_bend, fr.d_entry, nb, o.d_rb, flags, ids, bo, o.d_decline, st));
	uint64_t total = 0;
	BF_HIP(hipMemcpyAsync(&total, bo + nb, 8, hipMemcpyDeviceToHost, st));
	BF_LEAVE_DECLINED(o.d_decline, 0);
	BF_HIP(sk::launch_bam_min_index(fr.d_out, fr.d_bend, fr.d_entry, nb, o.d_rb, flags, ids, bo, krec, kout, st));
	return rw_begin(c, cl, fr, o, WriteOp{WriteOp::kMinimize, flags, baseq_fill, ids}, level, window_bytes, N, total, n_records, raw_bytes, handled, info);
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
	int krc = SK_OK;
	uint64_t *key[2] = {nullptr, nullptr};
	uint32_t *idx[2] = {nullptr, nullptr};
	size_t sort_bytes = 0, scan_bytes = 0;
	BF_HIP(sk::bam_sort_pairs(nullptr, &sort_bytes, key, idx, N ? N : 1, 64, nullptr, st));
	BF_HIP(sk::bam_md_run_scan(nullptr, &scan_bytes, nullptr, nullptr, N ? N : 1, st));
	const size_t a_key = up(N * 8 + 8), a_idx = up(N * 4 + 4), a_flag = up(N * 2 + 2), temp_bytes = std::max(sort_bytes, scan_bytes);
	const size_t work = 2 * a_key + 7 * a_idx + up(temp_bytes);
	const bool in_comp = fr.fsize + 64 >= work && !getenv("SK_MARKDUP_OWN_MEMORY");      // (the knob: for tests of the other placement)
	uint8_t *fb = (uint8_t *)sk::ctx_keep(c, sk::kKeepPassWork, a_flag + (in_comp ? 0 : work), false, &krc);
	if (!fb) BF_LEAVE(21);
	uint8_t *mb = in_comp ? fr.d_comp : fb + a_flag;
	if (getenv("SK_BAMFILE_TRACE")) fprintf(stderr, "sk_bam_file_markdup: %zu bytes of scratch in %s\n", work, in_comp ? "the compressed file's buffer" : "its own buffer");
	key[0] = (uint64_t *)mb; key[1] = (uint64_t *)(mb + a_key);
	idx[0] = (uint32_t *)(mb + 2 * a_key); idx[1] = (uint32_t *)(mb + 2 * a_key + a_idx);
	sk::MdCols cols;
	cols.krec = o.s->krec; cols.kout = o.s->kout; cols.tidpos = key[1];
	uint8_t *sig = mb + 2 * a_key + 2 * a_idx;
	cols.start = (uint32_t *)sig; cols.fl = (uint32_t *)(sig + a_idx); cols.lseq = (uint32_t *)(sig + 2 * a_idx);
	cols.uoff = (uint32_t *)(sig + 3 * a_idx); cols.ulen = (uint32_t *)(sig + 4 * a_idx);
	cols.nflag = (uint16_t *)fb;
	void *temp = sig + 5 * a_idx;
	// ---- signatures, order, runs: the decision to serve the file
	BF_HIP(sk::launch_bam_md_sig(fr.d_out, fr.d_bend, fr.d_entry, nb, o.d_rb, ignore_umi ? 1 : 0, fr.first, cols, o.d_decline, st));
	BF_HIP(sk::launch_bam_md_order(cols.tidpos, N, idx[1], o.d_decline, st));
	uint32_t runs = 0;
	if (N) {
		size_t tb = temp_bytes;
		BF_HIP(sk::bam_md_run_scan(temp, &tb, idx[1], idx[0], N, st));
		BF_HIP(hipMemcpyAsync(&runs, idx[0] + (N - 1), 4, hipMemcpyDeviceToHost, st));
	}
	BF_HIP(hipStreamSynchronize(st));                                  // (runs)
	BF_LEAVE_DECLINED(o.d_decline, runs >= 0x7fffffffu ? 64u : 0u);
	// ---- keys, the sort (only the bits the keys use: the all-ones key of the unmapped reads stays the largest), clusters, count
	int bits = 34;
	while (bits < 64 && ((uint64_t)1 << (bits - 33)) <= (uint64_t)runs) bits++;
	uint64_t dups = 0;
	if (N) {
		BF_HIP(sk::launch_bam_md_keys(idx[0], cols, N, key[0], idx[0], st));
		int cur = 0;
		size_t tb = temp_bytes;
		BF_HIP(sk::bam_sort_pairs(temp, &tb, key, idx, N, bits, &cur, st));
		BF_HIP(sk::launch_bam_md_cluster(fr.d_out, cols, key[cur], idx[cur], N, d_count, sk::ctx_n_cu(c), st));
		BF_HIP(hipMemcpyAsync(&dups, d_count, 8, hipMemcpyDeviceToHost, st));
		BF_HIP(hipStreamSynchronize(st));
	}
	const int rc = rw_begin(c, cl, fr, o, WriteOp{WriteOp::kMarkdup, 0, 255, nullptr, cols.nflag}, level, window_bytes, N, fr.stream_len - fr.first, n_records, raw_bytes, handled, info);
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
		uint64_t *key[2] = {nullptr, nullptr};
		uint32_t *idx[2] = {nullptr, nullptr};
		size_t sort_bytes = 0, scan_bytes = 0;
		BF_HIP(sk::bam_sort_pairs(nullptr, &sort_bytes, key, idx, N, bits + 1, nullptr, st));
		BF_HIP(sk::bam_sub_scans(nullptr, &scan_bytes, nullptr, nullptr, nullptr, N, st));
		const size_t a_key = up(N * 8), a_idx = up(N * 4), a_agg = up((N / 1024 + 2) * 4), temp_bytes = std::max(sort_bytes, scan_bytes);
		// (all of it is idle once the kept records are compacted: as sk_bam_file_markdup's scratch it lies in the device buffer of the
		// compressed file where that is large enough, and a gigabyte is not taken and given back for a 20 M-record file)
		const size_t work = 3 * a_key + 2 * a_idx + a_agg + up(temp_bytes);
		const bool in_comp = fr.fsize + 64 >= work;
		int krc = SK_OK;
		uint8_t *mb = in_comp ? fr.d_comp : (uint8_t *)sk::ctx_keep(c, sk::kKeepPassWork, work, false, &krc);
		if (!mb) BF_LEAVE(21);
		if (getenv("SK_BAMFILE_TRACE")) fprintf(stderr, "sk_bam_file_subsample: %zu bytes of scratch in %s\n", work, in_comp ? "the compressed file's buffer" : "its own buffer");
		key[0] = (uint64_t *)mb; key[1] = (uint64_t *)(mb + a_key);
		uint64_t *krec = (uint64_t *)(mb + 2 * a_key);
		idx[0] = (uint32_t *)(mb + 3 * a_key); idx[1] = (uint32_t *)(mb + 3 * a_key + a_idx);
		uint32_t *agg = (uint32_t *)(mb + 3 * a_key + 2 * a_idx);
		void *temp = mb + 3 * a_key + 2 * a_idx + a_agg;
		// ---- the fragment numbers
		BF_HIP(sk::launch_bam_min_keys(fr.d_out, fr.d_bend, fr.d_entry, nb, o.d_rb, bits, rule, krec, key[0], idx[0], o.d_decline, st));
		BF_LEAVE_DECLINED(o.d_decline, 0);                              // (8: the passes below read the names and flags of valid records only)
		int cur = 0;
		size_t tb = temp_bytes;
		BF_HIP(sk::bam_sort_pairs(temp, &tb, key, idx, N, bits + 1, &cur, st));
		uint32_t *src = (uint32_t *)key[cur ^ 1], *cnt = src + N, *ids = idx[cur ^ 1];
		BF_HIP(sk::launch_bam_min_ids(fr.d_out, krec, key[cur], idx[cur], N, bits, rule, agg, src, cnt, ids, o.d_decline, st));
		// ---- the decisions: the file is served or left here
		uint32_t *len = src, *pos = cnt;
		uint64_t *off = key[cur];
		BF_HIP(sk::launch_bam_sub_keep(fr.d_out, krec, ids, N, seed, sk::subsample_threshold(fraction), len, d_counts, o.d_decline, sk::ctx_n_cu(c), st));
		BF_HIP(hipMemcpyAsync(counts, d_counts, 24, hipMemcpyDeviceToHost, st));
		BF_LEAVE_DECLINED(o.d_decline, 0);                              // (1 a counted record without 0x1, 64 two names with one hash)
		// ---- the kept records' stream and output offsets
		tb = temp_bytes;
		BF_HIP(sk::bam_sub_scans(temp, &tb, len, pos, off, N, st));
		BF_HIP(sk::launch_bam_sub_compact(krec, len, pos, off, N, o.s->krec, o.s->kout, st));
	}
	const int rc = rw_begin(c, cl, fr, o, WriteOp{WriteOp::kSubsample}, level, window_bytes, counts[1], counts[2], n_records, raw_bytes, handled, info);
	if (rc == SK_OK && *handled && n_total) *n_total = (int64_t)counts[0];
	return rc;
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
static std::vector<std::string> front_ref_names(const std::vector<uint8_t> &h)     // (the header is checked by the front: it parses)
{
	std::vector<std::string> names;
	uint64_t o = 8 + (uint64_t)le32(h.data() + 4);
	const uint32_t n_ref = le32(h.data() + o);
	o += 4;
	for (uint32_t r = 0; r < n_ref; r++) {
		const uint32_t l_name = le32(h.data() + o);
		std::string name((const char *)h.data() + o + 4, l_name);
		if (!name.empty() && name.back() == '\0') name.pop_back();          // (as the host reader keeps them)
		names.push_back(name);
		o += 4 + (uint64_t)l_name + 4;
	}
	return names;
}

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
		if (i == 0) names0 = front_ref_names(fin[0].header);
		else if (front_ref_names(fin[i].header) != names0) {
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
		uint64_t *key[2] = {nullptr, nullptr};
		uint32_t *idx[2] = {nullptr, nullptr};
		size_t sort_bytes = 0, scan_bytes = 0;
		BF_HIP(sk::bam_sort_pairs(nullptr, &sort_bytes, key, idx, N, 64, nullptr, st));
		BF_HIP(sk::bam_merge_scan(nullptr, &scan_bytes, nullptr, N, st));
		const size_t a_key = up(N * 8), a_idx = up(N * 4), a_in = up(N), temp_bytes = std::max(sort_bytes, scan_bytes);
		const size_t work = 3 * a_key + 3 * a_idx + a_in + up(temp_bytes);
		const bool in_comp = fin[0].fsize + 64 >= work;
		int krc = SK_OK;
		uint8_t *kb = (uint8_t *)sk::ctx_keep(c, sk::kKeepPassWork, a_in + (in_comp ? 0 : work), false, &krc);
		if (!kb) BF_LEAVE(21);
		uint8_t *mb = in_comp ? fin[0].d_comp : kb + a_in;
		if (getenv("SK_BAMFILE_TRACE")) fprintf(stderr, "sk_bam_file_merge: %zu inputs, %zu bytes of scratch in %s\n", K, work, in_comp ? "the first compressed file's buffer" : "its own buffer");
		key[0] = (uint64_t *)mb; key[1] = (uint64_t *)(mb + a_key);
		idx[0] = (uint32_t *)(mb + 3 * a_key); idx[1] = (uint32_t *)(mb + 3 * a_key + a_idx);
		sk::MergeCols cols;
		cols.key = key[0]; cols.addr = (uint64_t *)(mb + 2 * a_key); cols.idx = idx[0];
		cols.len = (uint32_t *)(mb + 3 * a_key + 2 * a_idx); cols.in = mb + 3 * a_key + 3 * a_idx;
		void *temp = mb + 3 * a_key + 3 * a_idx + a_in;
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
		size_t tb = temp_bytes;
		BF_HIP(sk::bam_sort_pairs(temp, &tb, key, idx, N, 64, &cur, st));
		BF_HIP(sk::launch_bam_merge_gather(idx[cur], cols, N, o.s->krec, o.s->kout, kb, st));
		tb = temp_bytes;
		BF_HIP(sk::bam_merge_scan(temp, &tb, o.s->kout, N, st));
		BF_HIP(hipMemcpyAsync(&total, o.s->kout + N, 8, hipMemcpyDeviceToHost, st));
		BF_HIP(hipStreamSynchronize(st));
		if (suffix) kin = kb;
	}
	WriteOp op;
	op.kind = WriteOp::kMerge; op.merge_in = kin;
	return rw_begin(c, cl, all, o, op, level, window_bytes, N, total, n_records, raw_bytes, handled, info);
}

// ---- sam coverage histogram (include/seqkit_hip.h: sk_bam_file_coverage) ---
// The front half, then the passes of sk_bamcoverage.hip.  The host's part: the references' lengths out of the header (base = their
// running sum), the caller's intervals merged per reference for the mark pass, and, from the bits that pass leaves, the target
// intervals as events of their own behind the records'.  The events — two key and two kind buffers for the sort, 24 B per event, the
// idle key buffer taking the running sums behind the sort, and the scratch of the sort and the scan — lie in the device buffer of the
// compressed file where they fit (idle once the stream is verified), else in ctx slot kKeepPassWork.
extern "C" int sk_bam_file_coverage(sk_ctx *c, const char *path, int mode, const int64_t *targets, int64_t n_targets, uint64_t hist[SK_COVERAGE_BINS],
                                    uint64_t *n_positions, uint64_t *n_dropped, int64_t *n_counted, int *handled, double info[8])
{
	Cleanup cl;
	Front fr;
	if (int r = file_call_open(c, path, "sk_bam_file_coverage", handled, info, cl, fr, [&] {
		    if (n_positions) *n_positions = 0;
		    if (n_dropped) *n_dropped = 0;
		    if (n_counted) *n_counted = 0;
		    if (!hist) return sk::ctx_fail(c, SK_ERR_INVALID, "hist = NULL");
		    memset(hist, 0, (size_t)SK_COVERAGE_BINS * 8);
		    if (mode < 0 || mode > 2) return sk::ctx_fail(c, SK_ERR_INVALID, "mode = %d", mode);
		    if (n_targets < 0 || (n_targets > 0 && !targets)) return sk::ctx_fail(c, SK_ERR_INVALID, "n_targets = %lld", (long long)n_targets);
		    return (int)SK_OK;
	    }))
		return r;
	if (!fr.ready) return SK_OK;
	const double t_stage = now_ms();
	hipStream_t st = sk::ctx_stream(c);
	const int64_t nb = fr.nb;
	if (fr.n_ref < 0) BF_LEAVE(21);
	const size_t n_ref = (size_t)fr.n_ref;
	// ---- the references' lengths (the header is checked: every field lies inside it)
	std::vector<uint64_t> base(n_ref + 1, 0);
	{
		const uint8_t *h = fr.header.data();
		uint64_t o = 8 + (uint64_t)le32(h + 4) + 4;
		for (size_t r = 0; r < n_ref; r++) {
			o += 4 + (uint64_t)le32(h + o);
			base[r + 1] = base[r] + le32(h + o);
			o += 4;
		}
	}
	auto l_ref = [&](size_t r) { return (int64_t)(base[r + 1] - base[r]); };
	// ---- the caller's intervals, merged per reference (mode 1: they are the targets as they come)
	struct Iv { int64_t ref, beg, end; };
	std::vector<Iv> iv;
	if (mode != 0)
		for (int64_t k = 0; k < n_targets; k++) {
			const Iv v{targets[3 * k], std::max<int64_t>(targets[3 * k + 1], 0), targets[3 * k + 2]};
			if (v.ref >= 0 && (uint64_t)v.ref < n_ref && v.beg < v.end) iv.push_back(v);
		}
	std::vector<uint32_t> ioff;
	std::vector<int64_t> ibeg, iend;
	if (mode == 2) {
		std::sort(iv.begin(), iv.end(), [](const Iv &a, const Iv &b) { return a.ref != b.ref ? a.ref < b.ref : a.beg < b.beg; });
		std::vector<Iv> merged;
		for (const Iv &v : iv) {
			if (!merged.empty() && merged.back().ref == v.ref && v.beg <= merged.back().end) merged.back().end = std::max(merged.back().end, v.end);
			else merged.push_back(v);
		}
		iv.swap(merged);
		if (iv.size() >= 0xffffffffull) BF_LEAVE(21);
		ioff.assign(n_ref + 1, 0);
		for (const Iv &v : iv) { ioff[(size_t)v.ref + 1]++; ibeg.push_back(v.beg); iend.push_back(v.end); }
		for (size_t r = 0; r < n_ref; r++) ioff[r + 1] += ioff[r];
	}
	// ---- the small device arrays, one allocation: base, the blocks' runs, the intervals, the histogram and its totals, the bits, the words
	const size_t n_words = (n_ref + 31) / 32, n_iv = ibeg.size();
	const size_t a_base = up((n_ref + 1) * 8), a_runs = up((uint64_t)(nb + 1) * 8), a_iv = up(n_iv * 8 + 8), a_ioff = up((n_ref + 1) * 4), a_hist = up((SK_COVERAGE_BINS + 2) * 8);
	const size_t a_bits = up(n_words * 4 + 4);
	uint8_t *sm = nullptr;
	if (hipMalloc((void **)&sm, a_base + a_runs + 2 * a_iv + a_ioff + a_hist + 2 * a_bits + 256) != hipSuccess) { (void)hipGetLastError(); BF_LEAVE(21); }
	cl.dev.push_back(sm);
	uint64_t *d_base = (uint64_t *)sm, *d_runs = (uint64_t *)(sm + a_base);
	int64_t *d_ibeg = (int64_t *)(sm + a_base + a_runs), *d_iend = (int64_t *)(sm + a_base + a_runs + a_iv);
	uint32_t *d_ioff = (uint32_t *)(sm + a_base + a_runs + 2 * a_iv);
	uint64_t *d_hist = (uint64_t *)(sm + a_base + a_runs + 2 * a_iv + a_ioff), *d_tot = d_hist + SK_COVERAGE_BINS;
	uint8_t *zeroed = sm + a_base + a_runs + 2 * a_iv + a_ioff + a_hist;        // has, hit, counted, decline
	uint32_t *d_has = (uint32_t *)zeroed, *d_hit = (uint32_t *)(zeroed + a_bits);
	uint64_t *d_counted = (uint64_t *)(zeroed + 2 * a_bits);
	uint32_t *d_decline = (uint32_t *)(d_counted + 1);
	BF_HIP(hipMemsetAsync(zeroed, 0, 2 * a_bits + 256, st));
	BF_HIP(hipMemcpyAsync(d_base, base.data(), (n_ref + 1) * 8, hipMemcpyHostToDevice, st));
	if (mode == 2) {
		BF_HIP(hipMemcpyAsync(d_ioff, ioff.data(), (n_ref + 1) * 4, hipMemcpyHostToDevice, st));
		if (n_iv) {
			BF_HIP(hipMemcpyAsync(d_ibeg, ibeg.data(), n_iv * 8, hipMemcpyHostToDevice, st));
			BF_HIP(hipMemcpyAsync(d_iend, iend.data(), n_iv * 8, hipMemcpyHostToDevice, st));
		}
	}
	sk::CovArgs a{};
	a.n_ref = fr.n_ref; a.base = d_base; a.ioff = mode == 2 ? d_ioff : nullptr; a.ibeg = d_ibeg; a.iend = d_iend;
	a.bruns = d_runs; a.has = d_has; a.hit = d_hit; a.counted = (unsigned long long *)d_counted; a.decline = d_decline;
	// ---- mark: the runs, the counted records, the references' bits; the file is served or left here
	BF_HIP(sk::launch_bam_cov_mark(fr.d_out, fr.d_bend, fr.d_entry, nb, a, st));
	uint64_t R = 0, counted = 0;
	std::vector<uint32_t> has(n_words + 1, 0), hit(n_words + 1, 0);
	BF_HIP(hipMemcpyAsync(&R, d_runs + nb, 8, hipMemcpyDeviceToHost, st));
	BF_HIP(hipMemcpyAsync(&counted, d_counted, 8, hipMemcpyDeviceToHost, st));
	if (n_words) {
		BF_HIP(hipMemcpyAsync(has.data(), d_has, n_words * 4, hipMemcpyDeviceToHost, st));
		BF_HIP(hipMemcpyAsync(hit.data(), d_hit, n_words * 4, hipMemcpyDeviceToHost, st));
	}
	BF_LEAVE_DECLINED(d_decline, 0);                                    // (8 invalid record: info[5] = -38)
	// ---- the targets, cut to their references
	std::vector<uint64_t> tkey;
	std::vector<uint32_t> tkind;
	auto target = [&](size_t r, int64_t beg, int64_t end) {
		end = std::min(end, l_ref(r));
		if (beg >= end) return;
		tkey.push_back(base[r] + (uint64_t)beg); tkind.push_back(sk::kCovInsideUp);
		tkey.push_back(base[r] + (uint64_t)end); tkind.push_back(sk::kCovInsideDown);
	};
	auto bit = [](const std::vector<uint32_t> &v, size_t r) { return (v[r >> 5] >> (r & 31)) & 1u; };
	if (mode == 0) { for (size_t r = 0; r < n_ref; r++) if (bit(has, r)) target(r, 0, l_ref(r)); }
	else for (const Iv &v : iv) if (mode == 1 || bit(hit, (size_t)v.ref)) target((size_t)v.ref, v.beg, v.end);
	const uint64_t T = tkey.size(), E = 2 * R + T;
	if (E >= ((uint64_t)1 << 32)) BF_LEAVE(21);
	uint64_t tot[2] = {0, 0};
	if (T) {                                                            // (without a target no position is asked for)
		int bits = 1;
		while (bits < 64 && (base[n_ref] >> bits)) bits++;
		uint64_t *key[2] = {nullptr, nullptr};
		uint32_t *kind[2] = {nullptr, nullptr};
		size_t sort_bytes = 0, scan_bytes = 0;
		BF_HIP(sk::bam_sort_pairs(nullptr, &sort_bytes, key, kind, E, bits, nullptr, st));
		BF_HIP(sk::bam_cov_scan(nullptr, &scan_bytes, nullptr, nullptr, E, st));
		const size_t a_key = up(E * 8 + 8), a_kind = up(E * 4 + 4), temp_bytes = std::max(sort_bytes, scan_bytes);
		const size_t work = 2 * a_key + 2 * a_kind + up(temp_bytes);
		const bool in_comp = fr.fsize + 64 >= work;
		int krc = SK_OK;
		uint8_t *mb = in_comp ? fr.d_comp : (uint8_t *)sk::ctx_keep(c, sk::kKeepPassWork, work, false, &krc);
		if (!mb) BF_LEAVE(21);
		if (getenv("SK_BAMFILE_TRACE")) fprintf(stderr, "sk_bam_file_coverage: %llu events, %zu bytes of scratch in %s\n", (unsigned long long)E, work, in_comp ? "the compressed file's buffer" : "its own buffer");
		key[0] = (uint64_t *)mb; key[1] = (uint64_t *)(mb + a_key);
		kind[0] = (uint32_t *)(mb + 2 * a_key); kind[1] = (uint32_t *)(mb + 2 * a_key + a_kind);
		void *temp = mb + 2 * a_key + 2 * a_kind;
		// ---- the events, sorted; the running sums; the histogram
		BF_HIP(sk::launch_bam_cov_emit(fr.d_out, fr.d_bend, fr.d_entry, nb, a, key[0], kind[0], st));
		BF_HIP(hipMemcpyAsync(key[0] + 2 * R, tkey.data(), T * 8, hipMemcpyHostToDevice, st));
		BF_HIP(hipMemcpyAsync(kind[0] + 2 * R, tkind.data(), T * 4, hipMemcpyHostToDevice, st));
		int cur = 0;
		size_t tb = temp_bytes;
		BF_HIP(sk::bam_sort_pairs(temp, &tb, key, kind, E, bits, &cur, st));
		int64_t *sums = (int64_t *)key[cur ^ 1];
		tb = temp_bytes;
		BF_HIP(sk::bam_cov_scan(temp, &tb, kind[cur], sums, E, st));
		BF_HIP(sk::launch_bam_cov_hist(key[cur], sums, E, d_hist, d_tot, sk::ctx_n_cu(c), st));
		BF_HIP(hipMemcpyAsync(hist, d_hist, (size_t)SK_COVERAGE_BINS * 8, hipMemcpyDeviceToHost, st));
		BF_HIP(hipMemcpyAsync(tot, d_tot, 16, hipMemcpyDeviceToHost, st));
		BF_HIP(hipStreamSynchronize(st));
	}
	if (n_positions) *n_positions = tot[0];
	if (n_dropped) *n_dropped = tot[1];
	if (n_counted) *n_counted = (int64_t)counted;
	*handled = 1;
	char tail[160];
	snprintf(tail, sizeof tail, "; %llu counted, %llu runs, %llu target intervals, %llu positions", (unsigned long long)counted, (unsigned long long)R,
	         (unsigned long long)(T / 2), (unsigned long long)tot[0]);
	file_call_close(fr, "mark + emit + sort + scan + histogram", t_stage, tail, info);
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
	if (b < 0) return SK_OK;                                            // the end
	BF_HIP(hipEventSynchronize(s.ev[b]));
	uint64_t bytes = s.h_size[b];
	int rc = SK_OK;
	s.cur = rw_issue(c, s, b ^ 1, &rc) ? (b ^ 1) : -1;                    // (the buffer of the window returned last time: the caller is done with it)
	if (rc) { s.live = false; return rc; }
	hipStream_t st2 = sk::ctx_stream2(c);
	if (bytes) BF_HIP(hipMemcpyAsync(s.h_pin[b], s.d_pack[b], (size_t)bytes, hipMemcpyDeviceToHost, st2));
	BF_HIP(hipEventRecord(s.ev_copy[b], st2));
	BF_HIP(hipEventSynchronize(s.ev_copy[b]));
	if (s.cur < 0) { memcpy(s.h_pin[b] + bytes, bamfmt::kBgzfEof, 28); bytes += 28; }   // the last window ends with the EOF block
	w->first = s.first[b]; w->n = s.n[b];
	w->bgzf = s.h_pin[b]; w->bytes = bytes; w->raw_bytes = s.raw[b];
	return SK_OK;
}
