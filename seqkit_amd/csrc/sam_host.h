// sam_host.h — what the files of the `sam` host share (sam_main.cpp lists the commands and the file that serves each): the BAM reader
// and writer and the small helpers of sam_bamio.cpp, the gates of the device paths (templates, so they live here), and the commands.
#pragma once
#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "host_common.h"
#include "sk_bamfmt.h"

using bamfmt::le32;
using host::error;
using host::panic;

void check(int rc, const char *what);

// ---- BGZF/BAM container walk ---------------------------------------------------------------------------------
struct BamCore { int32_t tid, pos; uint16_t flag; int32_t mtid, mpos, tlen, end_pos; uint8_t mapq; };

// cigar().end_pos(): pos and the lengths of the operations that consume the reference (M D N = X).  *bad, where given: an operation
// code above 8, at which rust-htslib's cigar() panics.
int64_t cigar_end_pos(const uint8_t *cigar, uint32_t n_cigar, int64_t pos, bool *bad = nullptr);

// the columns of a line, split at tabs
std::vector<std::string> split_tabs(const std::string &t);

class BamStream {
public:
	// keep_header: the header's bytes as read ("BAM\1" .. the end of the reference list) stay in header_raw
	explicit BamStream(const std::string &path, bool keep_header = false);
	// Record errors ("BAM file ended prematurely." / "Invalid BAM record.", src/common.rs:150-154) end the stream: next()
	// returns false and the caller, once it has written what the records before the error produce, calls
	// raise_deferred() — the point the record-at-a-time reference would have reached.
	void raise_deferred() const { if (!err_.empty()) error("%s", err_.c_str()); }
	// the sizes of a record's variable part (qname, cigar, packed bases, qualities, aux), and where in it the aux data begin
	struct Var {
		uint32_t l_read_name, n_cigar, l_seq;
		size_t aux_off() const { return (size_t)l_read_name + 4 * (size_t)n_cigar + (((size_t)l_seq + 1) >> 1) + l_seq; }
	};
	// next record; want_end computes cigar().end_pos() (needed only by the on-target sweep for unpaired reads)
	bool next(BamCore &c, bool want_end);
	// The next records, one call for many: every record that lies wholly inside the current inflated block (walked by the
	// thread that inflated it, host::BgzfStream::bam_records), or — a record that straddles blocks, the end of the data, an
	// invalid record, or want_end — one record by next().  false as next(): the stream has ended or failed.
	bool next_chunk(std::vector<BamCore> &out, bool want_end);
	// next record with its variable part in `body`
	bool next_full(BamCore &c, Var &v, std::vector<uint8_t> &body);
	std::vector<std::string> names;
	std::vector<uint8_t> header_raw;
	uint8_t head[36];                                         // the last record's block_size and core as read
private:
	[[noreturn]] void open_fail() { error("Cannot open BAM file '%s'", path_.c_str()); }
	// block_size and the 32-byte core in one read into head (a short one is sorted out by the rules of the two reads it replaces), and
	// the core's fields; false as next()
	bool next_core(BamCore &c, Var &v);
	bool get(uint8_t *dst, size_t n);
	bool rd_fail(const char *msg) { err_ = msg; return false; }
	bool need(uint8_t *dst, size_t n);
	bool skip(uint32_t n);                                    // need() without a destination
	std::string err_;
	std::string path_;
	std::unique_ptr<host::BgzfStream> bz_;
	std::vector<uint8_t> var_;
	std::vector<host::BgzfStream::BamRec> recs_;
};

const size_t kBatchRecords = 4u << 20;

struct Columns {
	std::vector<uint16_t> flag;
	std::vector<int32_t> tid, mtid, tlen, pos, mpos, end_pos;
	std::vector<BamCore> chunk;                  // fill_batch: the reader's last chunk, and whether the stream goes on
	bool more = true;
	void clear() { flag.clear(); tid.clear(); mtid.clear(); tlen.clear(); pos.clear(); mpos.clear(); end_pos.clear(); }
	void push(const BamCore &c, bool extra)
	{
		flag.push_back(c.flag); tid.push_back(c.tid); mtid.push_back(c.mtid); tlen.push_back(c.tlen);
		if (extra) { pos.push_back(c.pos); mpos.push_back(c.mpos); end_pos.push_back(c.end_pos); }
	}
};

// The next batch of a stream's records as columns: kBatchRecords records, and those that come with the last chunk.  Their number; 0: the
// stream has ended (or failed: raise_deferred() says).
int64_t fill_batch(BamStream &bam, Columns &col, bool want_end, bool extra);

std::string expand_home(const std::string &path);             // PathArgs::get_path, src/common.rs:28-38

// The reference names of a BAM header as BamStream keeps them (one trailing NUL dropped, other bytes kept), from the header bytes
// sk_bam_file_columns returns ("BAM\1" .. the end of the reference list: checked there already).
std::vector<std::string> header_names(const uint8_t *h, uint64_t len);

// device buffers of one command's file path (sk_malloc_device), freed whichever way it is left
struct DevBufs {
	std::vector<void *> p;
	~DevBufs() { for (void *q : p) (void)sk_free_device(host::gpu(), q); }
	void *get(size_t bytes)
	{
		void *q = nullptr;
		if (sk_malloc_device(host::gpu(), bytes ? bytes : 16, &q) != SK_OK) return nullptr;
		p.push_back(q);
		return q;
	}
};

bool file_path_wanted(const std::string &path);

bool bamfile_trace();

// The device-or-host gate of a command: a file the device path is wanted for goes to `from_file` (the number of records, or -1: nothing
// has been written), and SK_BAMFILE_TRACE says which way the command went.  -1: the caller's host reader serves the file.
template <class FromFile>
int64_t device_path(const char *who, const std::string &path, FromFile from_file)
{
	const int64_t n = file_path_wanted(path) ? from_file() : -1;
	if (bamfile_trace()) {
		if (n >= 0) fprintf(stderr, "%s: device path, %lld records\n", who, (long long)n);
		else fprintf(stderr, "%s: host reader\n", who);
	}
	return n;
}

// the window size the windowed file calls are asked for (SK_BAMFILE_WINDOW bytes; 0: the library's default)
uint64_t file_window_bytes();

bool parse_i64(const std::string &s, int64_t &out);          // str::parse::<i64>()

// ---- BAM on stdout -------------------------------------------------------------------------------------------
// A BAM file on stdout: raw BAM bytes are cut into blocks of 0xff00 bytes and written as BGZF members, deflated on the device
// (sk_bgzf_deflate) or, at level 0, stored; finish() writes what is left and the EOF block.  The header goes in members of its own.
class BamOut {
public:
	explicit BamOut(int level) : level_(level) { buf_.reserve(kBatch + 8); }
	void put(const uint8_t *p, size_t n)
	{
		buf_.insert(buf_.end(), p, p + n);
		if (buf_.size() >= kBatch) flush();
	}
	void flush();
	void finish();
	static void write_all(const uint8_t *p, size_t n);
private:
	void deflate_here(const std::vector<sk_deflate_block> &blocks, std::vector<uint64_t> &off);
	static constexpr size_t kBatch = (size_t)256 * SK_DEFLATE_MAX_IN;
	int level_;
	bool done_ = false;
	std::vector<uint8_t> buf_, comp_;
};

// From here on error() and panic() finish `out` (what is left and the EOF block) before the process ends; nullptr: no longer.
void finish_at_exit(BamOut *out);

// The first RX field's value when its type is Z or H (bam_aux_get: the walk stops, not finding it, where the aux data stop parsing)
bool find_rx(const uint8_t *a, size_t n, const uint8_t *&val, size_t &vl);

// The device path of a BAM-writing command: `start` makes the file call that sets the windows up (sk_bam_file_rewrite, _minimize,
// _markdup, _subsample, _recalc_tlen or _merge), and the members go to stdout as they arrive.  -1: nothing has been written, and the caller's reader serves the file (one
// the file path does not take, a device without room, or a record the reference would stop at).  Otherwise the number of records.
template <class Start>
int64_t bam_out_from_file(Start start)
{
	sk_ctx *c = host::gpu();
	int64_t n_rec = 0;
	uint64_t raw = 0;
	int handled = 0;
	if (start(c, file_window_bytes(), &n_rec, &raw, &handled) != SK_OK || !handled) return -1;
	sk_bam_out_window w;
	for (;;) {
		check(sk_bam_file_rewrite_next(c, &w), "sk_bam_file_rewrite_next");
		if (w.n == 0 && w.bytes == 0) break;
		BamOut::write_all(w.bgzf, (size_t)w.bytes);
	}
	return n_rec;
}

// The host path of a BAM-writing command: the reader with the header's bytes kept, the writer on stdout (finished too where the process
// is left through error() or panic()), and the header written in members of its own.  close(): the error the reader met — after the
// records before it have been put —, then what is left and the EOF block.  The reader is the path's, or one the command opened itself
// with its header kept (sam merge: the first input's, once all inputs are open and compared).
struct HostBamRewrite {
	std::unique_ptr<BamStream> own;
	BamStream &bam;
	BamOut out;
	HostBamRewrite(const std::string &path, int level) : own(new BamStream(path, true)), bam(*own), out(level) { start(nullptr, 0); }
	// more: whole header lines behind the text (sam discard tail artifacts: its @CO line)
	HostBamRewrite(BamStream &reader, int level, const uint8_t *more = nullptr, size_t n_more = 0) : bam(reader), out(level) { start(more, n_more); }
	void close();
private:
	void start(const uint8_t *more, size_t n_more);
};

// A record with a new name into rec: the block_size and core as read, the name and its NUL, the `n_tail` bytes kept of what followed the
// old name, and `app` (aux data appended); block_size and l_read_name say so.
void renamed_record(std::vector<uint8_t> &rec, const uint8_t *head, const std::string &name, const uint8_t *tail, size_t n_tail, const std::vector<uint8_t> &app);

// ---- the commands (sam_main.cpp: which file serves which) ------------------------------------------------------------
int statistics_cmd(int argc, char **argv);
int fragment_lengths_cmd(int argc, char **argv);
int fragments_cmd(int argc, char **argv);
int count_cmd(int argc, char **argv);
int to_reads_cmd(int argc, char **argv);
int trim_qnames_cmd(int argc, char **argv);
int tags_from_qname_cmd(int argc, char **argv);
int qname_from_tags_cmd(int argc, char **argv);
int minimize_cmd(int argc, char **argv);
int mark_duplicates_cmd(int argc, char **argv);
int subsample_cmd(int argc, char **argv);
int recalculate_tlen_cmd(int argc, char **argv);
int merge_cmd(int argc, char **argv);
int concatenate_cmd(int argc, char **argv);
int discard_tail_artifacts_cmd(int argc, char **argv);
int coverage_histogram_cmd(int argc, char **argv);
