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

#include "sk_bamfile.h"

using namespace bamfile;

namespace {

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

// open and stat, the buffers, the readers, the BGZF headers and the batches of inflate launches, zlib for the blocks the device gave up,
// the BAM header, the walk and its verification: everything the file calls do before they read the records.  fr.who names the caller
// in trace lines.
int bamfile::bam_file_front(sk_ctx *c, const char *path, Cleanup &cl, Front &fr, double info[8])
{
	const char *who = fr.who;
	Ranges *both = (Ranges *)sk::ctx_ext(c);
	if (!both) { both = new Ranges; sk::ctx_set_ext(c, both, Ranges::destroy); }
	// an earlier sk_bam_file_reads may have left a window in flight on the ctx stream: its text kernel reads the inflated stream and its
	// copies write the page-locked window buffers.  It ends before this call remaps the ranges or takes the kept buffers again.
	// (the same for an sk_bam_file_rewrite, _minimize or _markdup, whose window copies run on the second stream)
	if (both->reads.busy() || both->rw.busy() || both->pairs.busy()) {
		BF_HIP(hipStreamSynchronize(sk::ctx_stream(c)));
		BF_HIP(hipStreamSynchronize(sk::ctx_stream2(c)));
	}
	both->gen++;                                                        // (what an earlier windowed call left is no longer read)
	both->reads.stop();
	both->rw.stop();
	both->pairs.stop();
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
			scan += bsize;
		}
		// a batch of blocks: copied on st2, inflated on st behind the copy.  A launch wants thousands of blocks (a wave per block,
		// 16 waves per CU: 4 096 in flight): the blocks of several chunks go together
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
	// (a last block that is not the empty EOF marker: htslib only warns when the marker is missing; the data are the same)
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
	bamfmt::RefList refs;
	std::vector<uint8_t> hd;
	for (size_t want = (size_t)std::min<uint64_t>(stream_len, (uint64_t)1 << 20);;) {
		hd.resize(want);
		if (want) BF_HIP(hipMemcpy(hd.data(), d_out, want, hipMemcpyDeviceToHost));
		const bamfmt::RefList::Status rs = refs.parse(hd.data(), want, stream_len);
		if (rs == bamfmt::RefList::kBad) BF_LEAVE(18);
		if (rs == bamfmt::RefList::kOk) break;
		if (want >= stream_len) BF_LEAVE(19);
		want = (size_t)std::min<uint64_t>(stream_len, (uint64_t)want * 4);
	}
	const uint64_t first = refs.end;
	const int32_t n_ref_hdr = refs.n_ref;
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
	fr.header.assign(hd.begin(), hd.begin() + (ptrdiff_t)first);
	fr.refs = std::move(refs);
	fr.ready = true;
	fr.d_out = d_out; fr.d_comp = d_comp; fr.stream_len = stream_len; fr.first = first; fr.n_records = n_records; fr.fsize = fsize; fr.n_host = n_host;
	fr.d_bend = d_bend; fr.d_entry = d_entry; fr.nb = nb; fr.rounds = rounds; fr.n_ref = n_ref_hdr;
	fr.t0 = t0; fr.t_alloc = t_alloc; fr.t_read = t_read; fr.t_inflated = t_inflated; fr.t_header = t_header; fr.t_walk = now_ms();
	return SK_OK;
}

// The closing every file call shares: the trace line (the front half's stages, the walk up to t_stage, the call's own `stage` from
// there, and `tail`) and info[].
void bamfile::file_call_close(const Front &fr, const char *stage, double t_stage, const char *tail, double info[8])
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
int bamfile::block_first_records(sk_ctx *c, const Front &fr, std::vector<uint64_t> &rb)
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
int bamfile::plan_windows(sk_ctx *c, Cleanup &cl, uint64_t window_bytes, const uint64_t *off0, const uint64_t *off1, uint64_t n, uint64_t total0,
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
int bamfile::read_decline(sk_ctx *c, const char *who, const uint32_t *d_decline, uint32_t found)
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
		if (want & (1u << k)) total += up(n * width[k] + 16);
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

