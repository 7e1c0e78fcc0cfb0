// sam — the `sam` binary of the reference for `sam statistics` and `sam fragment lengths`, with the per-record
// flag / TLEN reduction done by the MI355X library behind include/seqkit_hip.h (dispatch: src/sam_main.rs:50-53).
//
//   sam statistics [--on-target=BED] <bam_file>                         src/sam_statistics.rs:14-116
//   sam fragment lengths [--max-frag-size=F] [--reads=N] <bam_file>     src/sam_fragment_lengths.rs:14-48
//   sam fragments [--min-size=N] [--max-size=N] <bam_file>              src/sam_fragments.rs:14-43   (§8f f2)
//   sam count [--min-mapq=N] [--max-frag-len=N] [--single-end] [--center] <bam_file> <regions.bed>   src/sam_count.rs:20-130 (§8f f2)
//   sam to [interleaved] raw|fasta|fastq <bam_file> [<out_prefix>]      src/sam_to_fastq.rs:61-149   (§8f f4)
//
// The reference reads BAM through rust-htslib; this host walks the BGZF/BAM container itself (SAMv1 §4.2: BGZF is a
// series of gzip members; after the header every record is block_size:u32 + a 32-byte fixed core) and hands the core
// columns flag / refID / next_refID / tlen to the device as SoA batches.  The one order-dependent piece stays here, as
// SURVEY.md §8(e) lists it: the --reads=N early stop.  A regular
// file is first offered to the device whole (sk_bam_file_reduce, sk_bam_file_columns): it inflates and walks it; `sam fragments`
// and `sam count` then run their order checks and their text on the device too, `sam statistics --on-target` its fragment and
// region test (S2: it does not depend on record order), and whatever is irregular falls back to the reader
// here before anything has been written.  `sam to` takes the file the same way: the device writes every record's text, window by
// window, and the mate pairing stays here.  The commands that write BAM to stdout (trim qnames, tags from qname, qname from tags, minimize,
// mark duplicates, subsample, recalculate tlen, merge) share one way through: the gate (device_path), the windows' members to stdout (bam_out_from_file), and for what the
// device does not take the reader and writer of HostBamRewrite around the command's own per-record loop.  `sam coverage histogram` goes
// through the same gate with sk_bam_file_coverage and prints 10 001 lines; its host reader states the rule in one sort and one sweep.
#include <unistd.h>
#include <malloc.h>
#include <sys/random.h>
#include <zlib.h>
#include <fcntl.h>

#include <algorithm>
#include <cstring>
#include <deque>
#include <memory>
#include <new>
#include <string>
#include <unordered_map>
#include <vector>

#include "host_common.h"
#include "sam_pairing.h"
#include "sk_bamfmt.h"

using bamfmt::le32;
using host::error;
using host::panic;

static const char *USAGE_TOP =
	"\nUsage:\n"
	"  sam merge <bam_files>...\n  sam consensus <bam_file>\n  sam count <bam_file> <regions.bed>\n  sam coverage histogram <bam_file>\n"
	"  sam fragments <bam_file>\n  sam fragment lengths <bam_file>\n  sam mark duplicates <bam_file>\n  sam minimize <bam_file>\n"
	"  sam statistics <bam_file>\n  sam subsample <bam_file> <fraction>  \n  sam tags from qname <bam_file>\n  sam qname from tags <bam_file>\n"
	"  sam trim qnames <bam_file>  \n\nExtract reads from BAM files:  \n  sam to fasta <bam_file> <out_prefix>\n  sam to fastq <bam_file> <out_prefix>  \n"
	"  sam to interleaved fasta <bam_file>\n  sam to interleaved fastq <bam_file>\n  sam to interleaved raw <bam_file>\n  sam to raw <bam_file> <out_prefix>\n";
static const char *USAGE_STATS =
	"\nUsage:\n  sam statistics [options] <bam_file>\n\nOptions:\n  --on-target=BED   Count on-target% for regions in BED file [optional]\n";
static const char *USAGE_FRAG =
	"\nUsage:\n  sam fragment lengths [options] <bam_file>\n\nOptions:\n"
	"  --max-frag-size=F     Maximum fragment size [default: 5000]\n"
	"  --reads=N             Finish after analyzing this many reads [default: Inf]\n";

static void check(int rc, const char *what)
{
	if (rc != SK_OK) error("%s failed: %s", what, sk_last_error(host::gpu()));
}

// ---- BGZF/BAM container walk ---------------------------------------------------------------------------------
struct BamCore { int32_t tid, pos; uint16_t flag; int32_t mtid, mpos, tlen, end_pos; uint8_t mapq; };

// cigar().end_pos(): pos and the lengths of the operations that consume the reference (M D N = X).  *bad, where given: an operation
// code above 8, at which rust-htslib's cigar() panics.
static int64_t cigar_end_pos(const uint8_t *cigar, uint32_t n_cigar, int64_t pos, bool *bad = nullptr)
{
	for (uint32_t k = 0; k < n_cigar; k++) {
		const uint32_t op = le32(cigar + 4 * k), code = op & 15;
		if (code > 8 && bad) *bad = true;
		if (code == 0 || code == 2 || code == 3 || code == 7 || code == 8) pos += op >> 4;
	}
	return pos;
}

// the columns of a line, split at tabs
static std::vector<std::string> split_tabs(const std::string &t)
{
	std::vector<std::string> cols;
	for (size_t a = 0;;) {
		const size_t b = t.find('\t', a);
		cols.push_back(t.substr(a, b == std::string::npos ? b : b - a));
		if (b == std::string::npos) return cols;
		a = b + 1;
	}
}

class BamStream {
public:
	// keep_header: the header's bytes as read ("BAM\1" .. the end of the reference list) stay in header_raw
	explicit BamStream(const std::string &path, bool keep_header = false) : path_(path)
	{
		int fd = 0;
		if (path != "-") fd = open(path.c_str(), O_RDONLY);
		if (fd < 0) error("Cannot open BAM file '%s'", path.c_str());
		bz_.reset(new host::BgzfStream(fd, true));
		uint8_t h[8];
		auto keep = [&](const uint8_t *p, size_t n) { if (keep_header) header_raw.insert(header_raw.end(), p, p + n); };
		if (!get(h, 8) || memcmp(h, "BAM\1", 4) != 0) open_fail();
		keep(h, 8);
		if (keep_header) {
			const uint32_t l_text = le32(h + 4);
			for (uint32_t done = 0; done < l_text;) {                 // (in steps: a damaged l_text runs into the end of the data first)
				const uint32_t step = std::min<uint32_t>(l_text - done, 16u << 20);
				header_raw.resize(header_raw.size() + step);
				if (!get(header_raw.data() + header_raw.size() - step, step)) open_fail();
				done += step;
			}
		} else if (!skip(le32(h + 4))) open_fail();
		if (!get(h, 4)) open_fail();
		keep(h, 4);
		const uint32_t n_ref = le32(h);
		for (uint32_t i = 0; i < n_ref; i++) {
			if (!get(h, 4)) open_fail();
			keep(h, 4);
			const uint32_t l_name = le32(h);
			if (l_name > (1u << 20)) open_fail();               // a reference name of megabytes is a damaged header, not an allocation to attempt
			std::string name(l_name, '\0');
			if (l_name && !get(reinterpret_cast<uint8_t *>(&name[0]), l_name)) open_fail();
			keep(reinterpret_cast<const uint8_t *>(name.data()), l_name);
			if (!name.empty() && name.back() == '\0') name.pop_back();
			names.push_back(name);
			if (!get(h, 4)) open_fail();
			keep(h, 4);
		}
	}
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
	bool next(BamCore &c, bool want_end)
	{
		Var v;
		if (!next_core(c, v)) return false;
		const uint32_t l_read_name = v.l_read_name, n_cigar = v.n_cigar;
		uint32_t rest = le32(head) - 32;
		if (want_end && rest >= l_read_name + 4 * n_cigar) {
			var_.resize(l_read_name + 4 * n_cigar);
			if (!need(var_.data(), var_.size())) return false;
			rest -= (uint32_t)var_.size();
			c.end_pos = (int32_t)cigar_end_pos(var_.data() + l_read_name, n_cigar, c.pos);
		}
		return skip(rest);
	}
	// The next records, one call for many: every record that lies wholly inside the current inflated block (walked by the
	// thread that inflated it, host::BgzfStream::bam_records), or — a record that straddles blocks, the end of the data, an
	// invalid record, or want_end — one record by next().  false as next(): the stream has ended or failed.
	bool next_chunk(std::vector<BamCore> &out, bool want_end)
	{
		out.clear();
		if (!err_.empty()) return false;
		if (!want_end) {
			recs_.clear();
			if (bz_->bam_records(recs_) > 0) {
				out.resize(recs_.size());
				for (size_t i = 0; i < recs_.size(); i++) {
					const host::BgzfStream::BamRec &r = recs_[i];
					BamCore &c = out[i];
					c.tid = r.tid; c.pos = r.pos; c.flag = r.flag; c.mtid = r.mtid; c.mpos = r.mpos; c.tlen = r.tlen; c.end_pos = r.pos; c.mapq = r.mapq;
				}
				return true;
			}
		}
		BamCore c;
		if (!next(c, want_end)) return false;
		out.push_back(c);
		return true;
	}
	// next record with its variable part in `body`
	bool next_full(BamCore &c, Var &v, std::vector<uint8_t> &body)
	{
		if (!next_core(c, v)) return false;
		const uint32_t rest = le32(head) - 32;
		// htslib bam_read1: a record whose variable part cannot hold its own fields is invalid
		if (v.l_read_name < 1 || v.l_seq > 0x7fffffffu || v.aux_off() > rest) return rd_fail("Invalid BAM record.");
		// the record's size comes from the file: take it in steps, so that a damaged size field runs into the end of the data
		// ("BAM file ended prematurely.") instead of into one allocation of gigabytes
		body.clear();
		for (uint32_t done = 0; done < rest;) {
			const uint32_t step = std::min<uint32_t>(rest - done, 16u << 20);
			try { body.resize((size_t)done + step); } catch (const std::bad_alloc &) { return rd_fail("Invalid BAM record."); }
			if (!need(body.data() + done, step)) return false;
			done += step;
		}
		return true;
	}
	std::vector<std::string> names;
	std::vector<uint8_t> header_raw;
	uint8_t head[36];                                         // the last record's block_size and core as read
private:
	[[noreturn]] void open_fail() { error("Cannot open BAM file '%s'", path_.c_str()); }
	// block_size and the 32-byte core in one read into head (a short one is sorted out by the rules of the two reads it replaces), and
	// the core's fields; false as next()
	bool next_core(BamCore &c, Var &v)
	{
		if (!err_.empty()) return false;
		const long r = bz_->read(head, 36);
		if (r == 0) return false;
		if (r < 0) return rd_fail("Invalid BAM record.");
		if (r < 4) return rd_fail("BAM file ended prematurely.");
		if (le32(head) < 32) return rd_fail("Invalid BAM record.");
		if (r < 36 && !need(head + r, (size_t)(36 - r))) return false;
		const uint8_t *core = head + 4;
		c.tid = (int32_t)le32(core + 0);
		c.pos = (int32_t)le32(core + 4);
		v.l_read_name = core[8];
		c.mapq = core[9];
		v.n_cigar = (uint32_t)core[12] | ((uint32_t)core[13] << 8);
		c.flag = (uint16_t)(core[14] | (core[15] << 8));
		v.l_seq = le32(core + 16);
		c.mtid = (int32_t)le32(core + 20);
		c.mpos = (int32_t)le32(core + 24);
		c.tlen = (int32_t)le32(core + 28);
		c.end_pos = c.pos;
		return true;
	}
	bool get(uint8_t *dst, size_t n)
	{
		size_t got = 0;
		while (got < n) {
			const long r = bz_->read(dst + got, n - got);
			if (r <= 0) return false;
			got += (size_t)r;
		}
		return true;
	}
	bool rd_fail(const char *msg) { err_ = msg; return false; }
	bool need(uint8_t *dst, size_t n)
	{
		size_t got = 0;
		while (got < n) {
			const long r = bz_->read(dst + got, n - got);
			if (r < 0) return rd_fail("Invalid BAM record.");
			if (r == 0) return rd_fail("BAM file ended prematurely.");
			got += (size_t)r;
		}
		return true;
	}
	bool skip(uint32_t n)                                     // need() without a destination
	{
		size_t got = 0;
		while (got < n) {
			const long r = bz_->skip(n - got);
			if (r < 0) return rd_fail("Invalid BAM record.");
			if (r == 0) return rd_fail("BAM file ended prematurely.");
			got += (size_t)r;
		}
		return true;
	}
	std::string err_;
	std::string path_;
	std::unique_ptr<host::BgzfStream> bz_;
	std::vector<uint8_t> var_;
	std::vector<host::BgzfStream::BamRec> recs_;
};

static const size_t kBatch = 4u << 20;

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

// The next batch of a stream's records as columns: kBatch records, and those that come with the last chunk.  Their number; 0: the stream
// has ended (or failed: raise_deferred() says).
static int64_t fill_batch(BamStream &bam, Columns &col, bool want_end, bool extra)
{
	col.clear();
	while (col.more && col.flag.size() < kBatch && (col.more = bam.next_chunk(col.chunk, want_end)))
		for (const BamCore &c : col.chunk) col.push(c, extra);
	return (int64_t)col.flag.size();
}

static std::string expand_home(const std::string &path)      // PathArgs::get_path, src/common.rs:28-38
{
	if (!path.empty() && path[0] == '~')
		if (const char *home = getenv("HOME")) return std::string(home) + path.substr(1);
	return path;
}

// The reference names of a BAM header as BamStream keeps them (one trailing NUL dropped, other bytes kept), from the header bytes
// sk_bam_file_columns returns ("BAM\1" .. the end of the reference list: checked there already).
static std::vector<std::string> header_names(const uint8_t *h, uint64_t len)
{
	bamfmt::RefList refs;
	(void)refs.parse(h, len, len);
	return refs.names(h);
}

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

static bool file_path_wanted(const std::string &path) { return path != "-" && !getenv("SEQKIT_HOST_INFLATE"); }

static bool bamfile_trace() { static const bool on = getenv("SK_BAMFILE_TRACE") != nullptr; return on; }

// The device-or-host gate of a command: a file the device path is wanted for goes to `from_file` (the number of records, or -1: nothing
// has been written), and SK_BAMFILE_TRACE says which way the command went.  -1: the caller's host reader serves the file.
template <class FromFile>
static int64_t device_path(const char *who, const std::string &path, FromFile from_file)
{
	const int64_t n = file_path_wanted(path) ? from_file() : -1;
	if (bamfile_trace()) {
		if (n >= 0) fprintf(stderr, "%s: device path, %lld records\n", who, (long long)n);
		else fprintf(stderr, "%s: host reader\n", who);
	}
	return n;
}

// the window size the windowed file calls are asked for (SK_BAMFILE_WINDOW bytes; 0: the library's default)
static uint64_t file_window_bytes()
{
	static const uint64_t window = [] { const char *ev = getenv("SK_BAMFILE_WINDOW"); return ev ? (uint64_t)strtoull(ev, nullptr, 10) : (uint64_t)0; }();
	return window;
}

// ---- sam statistics ----------------------------------------------------------------------------------------------
struct Region { int64_t start, end; };

// The target regions of every BAM reference (src/sam_statistics.rs:26-54), 1-based inclusive, sorted by start.  *overflow, where given:
// a BED start of INT64_MAX, whose + 1 (:45) does not fit.
static std::vector<std::vector<Region>> read_targets(const std::string &targets_path, const std::vector<std::string> &names, bool *overflow = nullptr)
{
	std::vector<std::vector<Region>> target_regions(names.size());
	fputs("Reading target regions into memory...\n", stderr);
	host::LineReader bed(targets_path);
	std::string line;
	for (;;) {
		const bool ok = bed.read_line(line);
		if (bed.bad_utf8()) error("I/O error while reading from file.");
		if (!ok) break;
		const size_t off = host::trim_start_off(line), end = host::trim_end_len(line);
		if (end <= off || line[0] == '#') continue;                                                // :37
		const std::vector<std::string> cols = split_tabs(line.substr(off, end - off));
		if (cols.size() < 3) error("Invalid line in BED file %s:\n%s", targets_path.c_str(), line.c_str());
		int tid = -1;
		for (size_t k = 0; k < names.size(); k++) if (names[k] == cols[0]) { tid = (int)k; break; }
		if (tid < 0) error("Chromosome %s is listed in target region BED file, but is not found in BAM file.", cols[0].c_str());
		uint64_t s, e;
		if (!host::parse_uint(cols[1].c_str(), INT64_MAX, s) || !host::parse_uint(cols[2].c_str(), INT64_MAX, e)) panic("called `Result::unwrap()` on an `Err` value: ParseIntError (BED)");
		if (overflow && s == (uint64_t)INT64_MAX) *overflow = true;
		target_regions[tid].push_back({(int64_t)(s + 1), (int64_t)e});                             // :44-47
	}
	for (auto &v : target_regions) std::sort(v.begin(), v.end(), [](const Region &a, const Region &b) { return a.start < b.start; });   // :51-53
	return target_regions;
}

// sam statistics --on-target over the FILE: the device inflates and walks it (sk_bam_file_columns) and counts S1 and S2 of every record
// in one call (sk_on_target_add_dev): whether a fragment overlaps a region does not depend on the records before it.
// -1: nothing has been written to stdout, and the caller's reader serves the file — one the file path does not take, a header without
// references (the reference's target_regions.is_empty()), a BED start whose + 1 overflows, or a fragment whose tid has no reference (the
// reader panics where the reference does).  The regions, once read here, are the caller's too (*have_regions): the BED is read and
// announced once.  Otherwise the number of records; counters = total, aligned, duplicate reads, total and on-target fragments.
static int64_t on_target_from_file(const std::string &path, const std::string &targets_path, int64_t max_frag_len,
                                   std::vector<std::vector<Region>> &target_regions, bool *have_regions, uint64_t counters[5])
{
	sk_ctx *c = host::gpu();
	sk_bam_columns cols;
	int handled = 0;
	const uint32_t want = SK_COL_FLAG | SK_COL_TID | SK_COL_MTID | SK_COL_POS | SK_COL_MPOS | SK_COL_TLEN | SK_COL_END;
	if (sk_bam_file_columns(c, path.c_str(), want, &cols, &handled, nullptr) != SK_OK || !handled) return -1;
	const std::vector<std::string> names = header_names(cols.header, cols.header_len);
	if (names.empty()) return -1;
	bool overflow = false;
	target_regions = read_targets(targets_path, names, &overflow);
	*have_regions = true;
	if (overflow) return -1;
	std::vector<int32_t> chr_off(names.size() + 1, 0);
	std::vector<int64_t> rs, re;
	for (size_t k = 0; k < names.size(); k++) {
		for (const Region &r : target_regions[k]) { rs.push_back(r.start); re.push_back(r.end); }
		if (rs.size() > 0x7fffffffu) return -1;
		chr_off[k + 1] = (int32_t)rs.size();
	}
	if (sk_on_target_set_regions(c, (int)names.size(), chr_off.data(), rs.data(), re.data(), (int64_t)rs.size()) != SK_OK) return -1;
	if (sk_on_target_add_dev(c, cols.flag, cols.tid, cols.mtid, cols.pos, cols.mpos, cols.tlen, cols.end_pos, cols.n, max_frag_len) != SK_OK) return -1;
	uint64_t got[6];
	if (sk_on_target_get(c, got) != SK_OK || got[5] != 0) return -1;
	memcpy(counters, got, 5 * sizeof(uint64_t));
	return cols.n;
}

static int statistics(int argc, char **argv)
{
	std::vector<host::Opt> opts = {{"--on-target", true, false, ""}};
	std::vector<std::string> pos;
	if (!host::parse_args(argc, argv, 2, opts, pos, 1) || pos.size() != 1) error("Invalid arguments.\n%s", USAGE_STATS);
	const std::string bam_path = expand_home(pos[0]), targets_path = expand_home(opts[0].value);     // :17-18
	const int64_t max_frag_len = 5000;                                                                 // :19
	host::gpu_warmup();
	auto print_counters = [](const uint64_t counters[3]) {                                             // :109-112
		char buf[256];
		snprintf(buf, sizeof buf, "Total reads: %llu\n", (unsigned long long)counters[0]);
		host::out().write(buf, strlen(buf));
		snprintf(buf, sizeof buf, "Aligned reads: %llu (%s%% of all reads)\n", (unsigned long long)counters[1],
		         host::fmt_pct((double)counters[1] / (double)counters[0] * 100.0).c_str());
		host::out().write(buf, strlen(buf));
		snprintf(buf, sizeof buf, "Duplicate reads: %llu (%s%% of aligned reads)\n", (unsigned long long)counters[2],
		         host::fmt_pct((double)counters[2] / (double)counters[1] * 100.0).c_str());
		host::out().write(buf, strlen(buf));
	};
	auto print_on_target = [](uint64_t on_target_fragments, uint64_t total_fragments) {                // :114
		char buf[256];
		snprintf(buf, sizeof buf, "On-target: %s%%\n", host::fmt_pct((double)on_target_fragments / (double)total_fragments * 100.0).c_str());
		host::out().write(buf, strlen(buf));
	};
	// S1 over the FILE (round 6): the compressed bytes cross PCIe, the device inflates the BGZF blocks, walks the records and counts
	// (include/seqkit_hip.h: sk_bam_file_reduce).  It serves well-formed regular files only and says so (handled): everything else —
	// stdin, plain gzip, a file cut short, a record chain that does not verify — is read record by record below, which reports it as
	// the reference does.  With --on-target the file goes the same way as columns (on_target_from_file): S2 needs pos and the cigar's
	// end of every record, but not their order.
	if (targets_path.empty() && file_path_wanted(bam_path)) {
		int handled = 0;
		uint64_t fc[3] = {0, 0, 0};
		auto now_ms = [] { timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6; };
		const double t0 = now_ms();
		sk_ctx *c = host::gpu();
		const double t1 = now_ms();
		check(sk_bam_file_reduce(c, bam_path.c_str(), 0, fc, nullptr, nullptr, &handled, nullptr), "sk_bam_file_reduce");
		if (bamfile_trace()) fprintf(stderr, "sam statistics: waited %.1f ms for the device contexts, sk_bam_file_reduce %.1f ms\n", t1 - t0, now_ms() - t1);
		if (handled) { print_counters(fc); return 0; }
	}
	std::vector<std::vector<Region>> target_regions;                                                   // :26-54
	bool have_regions = false;
	if (!targets_path.empty()) {
		uint64_t fc[5] = {0, 0, 0, 0, 0};
		if (device_path("sam statistics", bam_path, [&] { return on_target_from_file(bam_path, targets_path, max_frag_len, target_regions, &have_regions, fc); }) >= 0) {
			print_counters(fc);
			print_on_target(fc[4], fc[3]);
			return 0;
		}
	}
	BamStream bam(bam_path);
	if (!targets_path.empty() && !have_regions) target_regions = read_targets(targets_path, bam.names);
	const bool on_target = !target_regions.empty();

	uint64_t counters[3] = {0, 0, 0};
	uint64_t total_fragments = 0, on_target_fragments = 0;
	Columns col;
	for (int64_t n; (n = fill_batch(bam, col, on_target, on_target)) > 0;) {
		// S1 on the device: src/sam_statistics.rs:63-69
		check(sk_bam_flag_tlen(host::gpu(), col.flag.data(), nullptr, nullptr, nullptr, n, 0, counters, nullptr, nullptr), "sk_bam_flag_tlen");
		if (!on_target) continue;
		// S2 (--on-target) of a file the device path does not take, as the reference states it: src/sam_statistics.rs:72-106
		for (int64_t i = 0; i < n; i++) {
			const uint16_t f = col.flag[i];
			if ((f & 0x100) || (f & 0x800)) continue;
			if (f & 0x4) continue;
			int64_t start, end;
			if (f & 0x1) {
				if (f & 0x8) continue;
				if (col.tid[i] != col.mtid[i]) continue;
				if (col.pos[i] > col.mpos[i] || (col.pos[i] == col.mpos[i] && !(f & 0x40))) continue;
				int64_t tl = col.tlen[i];
				if (tl < 0) tl = -tl;
				if (tl > max_frag_len) continue;
				start = (int64_t)col.pos[i] + 1;
				end = start + tl;
			} else {
				start = (int64_t)col.pos[i] + 1;
				end = (int64_t)col.end_pos[i] + 1;
			}
			total_fragments += 1;
			if (col.tid[i] < 0 || (size_t)col.tid[i] >= target_regions.size()) panic("index out of bounds: target_regions[tid]");
			for (const Region &r : target_regions[col.tid[i]]) {
				if (start <= r.end && end >= r.start) { on_target_fragments += 1; break; }
				if (r.start > end) break;
			}
		}
	}
	bam.raise_deferred();
	print_counters(counters);                                                                          // :109-115
	if (on_target) print_on_target(on_target_fragments, total_fragments);
	return 0;
}

// ---- sam fragment lengths ---------------------------------------------------------------------------------------
static bool frag_keep(uint16_t f, int32_t tid, int32_t mtid, int32_t tlen, uint64_t max_frag, uint64_t &frag)   // :30-38
{
	if ((f & (0x1 | 0x40 | 0x4 | 0x8 | 0x400 | 0x100 | 0x800)) != (0x1 | 0x40)) return false;
	if (tid != mtid) return false;
	const int64_t t = tlen;
	frag = (uint64_t)(t < 0 ? -t : t);
	return frag <= max_frag;
}

static int fragment_lengths(int argc, char **argv)
{
	std::vector<host::Opt> opts = {{"--max-frag-size", true, false, "5000"}, {"--reads", true, false, "Inf"}};
	std::vector<std::string> pos;
	if (!host::parse_args(argc, argv, 3, opts, pos, 1) || pos.size() != 1) error("Invalid arguments.\n%s", USAGE_FRAG);
	uint64_t max_frag = 5000, stop = UINT64_MAX;
	if (!host::parse_uint(opts[0].value.c_str(), UINT64_MAX, max_frag)) panic("called `Result::unwrap()` on an `Err` value: ParseIntError (--max-frag-size)");   // :19-20
	if (opts[1].value != "Inf" && !host::parse_uint(opts[1].value.c_str(), UINT64_MAX, stop)) panic("called `Result::unwrap()` on an `Err` value: ParseIntError (--reads)");   // :21-25
	// |tlen| is at most 2^31, so bins above that can never be hit; the device interface takes an int32 bin count
	if (max_frag > 200000000ull) error("--max-frag-size above 200000000 is not supported by this build.");
	std::vector<uint64_t> hist(max_frag + 1, 0);                                                       // :27
	uint64_t total = 0;
	host::gpu_warmup();
	// H1 over the file on the device (see statistics()); the --reads=N stop depends on record order and keeps the host's path
	bool by_file = false;
	if (stop == UINT64_MAX && file_path_wanted(pos[0])) {
		int handled = 0;
		uint64_t ft = 0;
		std::vector<uint64_t> fh(max_frag + 1, 0);
		check(sk_bam_file_reduce(host::gpu(), pos[0].c_str(), (int32_t)max_frag, nullptr, fh.data(), &ft, &handled, nullptr), "sk_bam_file_reduce");
		if (handled) { hist.swap(fh); total = ft; by_file = true; }
	}
	std::unique_ptr<BamStream> bam_p(by_file ? nullptr : new BamStream(pos[0]));                      // :30
	Columns col;
	bool stopped = false;
	for (int64_t n; !by_file && !stopped && (n = fill_batch(*bam_p, col, false, false)) > 0;) {
		// H1 on the device: src/sam_fragment_lengths.rs:29-43
		std::vector<uint64_t> bh(max_frag + 1, 0);
		uint64_t bt = 0;
		check(sk_bam_flag_tlen(host::gpu(), col.flag.data(), col.tid.data(), col.mtid.data(), col.tlen.data(), n, (int32_t)max_frag, nullptr, bh.data(), &bt), "sk_bam_flag_tlen");
		if (total + bt < stop) {
			for (size_t i = 0; i <= max_frag; i++) hist[i] += bh[i];
			total += bt;
		} else {
			// the --reads=N stop (:42) falls inside this batch: it depends on input order, so the batch is walked here
			for (int64_t i = 0; i < n; i++) {
				uint64_t frag;
				if (!frag_keep(col.flag[i], col.tid[i], col.mtid[i], col.tlen[i], max_frag, frag)) continue;
				total += 1;
				hist[frag] += 1;
				if (total >= stop) { stopped = true; break; }
			}
		}
	}
	if (!stopped && bam_p) bam_p->raise_deferred();
	char buf[64];
	for (uint64_t size = 1; size < max_frag + 1; size++) {                                             // :45-47
		snprintf(buf, sizeof buf, "%llu\t%llu\n", (unsigned long long)size, (unsigned long long)hist[size]);
		host::out().write(buf, strlen(buf));
	}
	return 0;
}

// ---- sam fragments ---------------------------------------------------------------------------
static const char *USAGE_FRAGMENTS =
	"\nUsage:\n  sam fragments [options] <bam_file>\n\nOptions:\n"
	"  --min-size=N     Minimum fragment size [default: 0]\n"
	"  --max-size=N     Maximum fragment size [default: 5000]\n";

static bool parse_i64(const std::string &s, int64_t &out)          // str::parse::<i64>()
{
	const char *p = s.c_str();
	bool neg = false;
	if (*p == '+' || *p == '-') { neg = *p == '-'; p++; }
	uint64_t v;
	if (!host::parse_uint(p, neg ? 9223372036854775808ull : 9223372036854775807ull, v)) return false;
	out = neg ? (int64_t)(0 - v) : (int64_t)v;
	return true;
}

// sam fragments over the FILE: the device inflates and walks it (sk_bam_file_columns), filters the records (sk_bam_fragments_dev) and
// writes the BED text (sk_bam_fragments_bed_dev), which goes out in one write.  -1: nothing has been written, and the caller's reader
// serves the file — one the file path does not take, a device without room, or a kept record whose tid has no name (the reader
// writes the lines before it and panics where the reference does).  Otherwise the number of records.
static int64_t fragments_from_file(const std::string &path, int64_t min_size, int64_t max_size)
{
	sk_ctx *c = host::gpu();
	sk_bam_columns cols;
	int handled = 0;
	if (sk_bam_file_columns(c, path.c_str(), SK_COL_FLAG | SK_COL_TID | SK_COL_MTID | SK_COL_POS | SK_COL_TLEN, &cols, &handled, nullptr) != SK_OK || !handled) return -1;
	const std::vector<std::string> names = header_names(cols.header, cols.header_len);
	const int64_t n = cols.n;
	DevBufs dev;
	uint8_t *bits = (uint8_t *)dev.get((size_t)(n + 7) / 8 + 16);
	uint64_t *kept = (uint64_t *)dev.get(16);
	if (!bits || !kept) return -1;
	const uint64_t zero = 0;
	if (sk_copy_h2d(c, kept, &zero, 8) != SK_OK) return -1;
	if (n && sk_bam_fragments_dev(c, cols.flag, cols.tid, cols.mtid, cols.tlen, n, min_size, max_size, bits, kept) != SK_OK) return -1;   // :27-38
	std::string blob;
	std::vector<uint64_t> off(1, 0);
	for (const std::string &nm : names) { blob += nm; off.push_back(blob.size()); }
	const char *text = nullptr;
	uint64_t text_len = 0;
	int64_t bad = -1;
	if (sk_bam_fragments_bed_dev(c, bits, cols.tid, cols.pos, cols.tlen, n, reinterpret_cast<const uint8_t *>(blob.data()), off.data(), (int32_t)names.size(),
	                             &text, &text_len, &bad) != SK_OK || bad >= 0) return -1;                                        // :41
	if (text_len) host::out().write(text, (size_t)text_len);
	return n;
}

static int fragments(int argc, char **argv)                        // src/sam_fragments.rs:14-43
{
	std::vector<host::Opt> opts = {{"--min-size", true, false, "0"}, {"--max-size", true, false, "5000"}};
	std::vector<std::string> pos;
	if (!host::parse_args(argc, argv, 2, opts, pos, 1) || pos.size() != 1) error("Invalid arguments.\n%s", USAGE_FRAGMENTS);
	int64_t min_size, max_size;
	if (!parse_i64(opts[0].value, min_size)) panic("called `Result::unwrap()` on an `Err` value: ParseIntError (--min-size)");   // :17
	if (!parse_i64(opts[1].value, max_size)) panic("called `Result::unwrap()` on an `Err` value: ParseIntError (--max-size)");   // :18
	host::gpu_warmup();
	if (device_path("sam fragments", pos[0], [&] { return fragments_from_file(pos[0], min_size, max_size); }) >= 0) return 0;
	BamStream bam(pos[0]);
	Columns col;
	std::vector<uint8_t> bits;
	char buf[128];
	for (int64_t n; (n = fill_batch(bam, col, false, true)) > 0;) {
		bits.assign((size_t)(n + 7) / 8, 0);
		uint64_t kept = 0;
		// the record filter on the device: src/sam_fragments.rs:27-38
		check(sk_bam_fragments(host::gpu(), col.flag.data(), col.tid.data(), col.mtid.data(), col.tlen.data(), n, min_size, max_size, bits.data(), &kept), "sk_bam_fragments");
		if (kept == 0) continue;
		for (int64_t i = 0; i < n; i++) {
			if (!(bits[(size_t)i >> 3] >> (i & 7) & 1)) continue;
			if (col.tid[i] < 0 || (size_t)col.tid[i] >= bam.names.size()) panic("index out of bounds: chr_names[tid]");
			int64_t t = col.tlen[i];
			if (t < 0) t = -t;
			snprintf(buf, sizeof buf, "\t%lld\t%lld\n", (long long)col.pos[i], (long long)col.pos[i] + (long long)t);      // :41
			host::out().write(bam.names[col.tid[i]]);
			host::out().write(buf, strlen(buf));
		}
	}
	bam.raise_deferred();
	return 0;
}

// ---- sam count (second half) --------------------------------------------------------------------
static const char *USAGE_COUNT =
	"\nUsage:\n  sam count [options] <bam_file> <regions.bed>\n\nOptions:\n"
	"  --min-mapq=N      Only count reads with MAPQ \xe2\x89\xa5 threshold [default: 0]\n"
	"  --max-frag-len=N  Maximum allowed DNA fragment length [default: 5000]\n"
	"  --single-end      Count individual reads, rather than DNA fragments\n"
	"  --center          Only count fragments whose center is within a region\n"
	"\n"
	"Counts the number of DNA fragments (or single reads) in the input BAM file\n"
	"that overlap each region described in the input BED file. The BAM file must\n"
	"be position-sorted.\n";

// the regions of every BAM reference (src/sam_count.rs:61-63), handed to the device once
struct CountReg { std::string chr; uint32_t start, end; };
static int count_load_regions(const std::vector<std::string> &names, const std::vector<CountReg> &regions)
{
	const int n_chr = (int)names.size();
	std::vector<int32_t> chr_off(n_chr + 1, 0), ridx;
	std::vector<uint32_t> rs, re;
	for (int c = 0; c < n_chr; c++) {
		for (size_t r = 0; r < regions.size(); r++)
			if (regions[r].chr == names[c]) { rs.push_back(regions[r].start); re.push_back(regions[r].end); ridx.push_back((int32_t)r); }
		chr_off[c + 1] = (int32_t)rs.size();
	}
	return sk_count_set_regions(host::gpu(), n_chr, chr_off.data(), rs.data(), re.data(), ridx.data(), (int64_t)rs.size(),
	                            (int64_t)std::max(rs.size(), regions.size()));
}

static void count_print(const std::vector<CountReg> &regions)
{
	std::vector<uint32_t> region_frags(std::max<size_t>(regions.size(), 1));
	check(sk_count_get(host::gpu(), region_frags.data()), "sk_count_get");
	char buf[32];
	for (size_t r = 0; r < regions.size(); r++) {                                                                          // :128-130
		snprintf(buf, sizeof buf, "%u\n", region_frags[r]);
		host::out().write(buf, strlen(buf));
	}
}

// sam count over the FILE: the device inflates and walks it (sk_bam_file_columns), checks the order as :52-73 do
// (sk_count_order_check_dev) and counts every record in one call (sk_count_add_dev).  -1: nothing has been written, and the caller's
// reader serves the file — one the file path does not take, a device without room, a reference name that is not UTF-8 (:37-38), or a
// file where the loop of :52-73 stops (the reader writes what the reference does).  Otherwise the number of records.
static int64_t count_from_file(const std::string &path, const std::vector<CountReg> &regions, uint8_t min_mapq, uint32_t max_frag_len, bool single_end,
                               bool center)
{
	sk_ctx *c = host::gpu();
	sk_bam_columns cols;
	int handled = 0;
	const uint32_t want = SK_COL_FLAG | SK_COL_MAPQ | SK_COL_TID | SK_COL_MTID | SK_COL_POS | SK_COL_MPOS | SK_COL_TLEN | (single_end ? SK_COL_END : 0u);
	if (sk_bam_file_columns(c, path.c_str(), want, &cols, &handled, nullptr) != SK_OK || !handled) return -1;
	const std::vector<std::string> names = header_names(cols.header, cols.header_len);
	for (const std::string &nm : names)
		if (!host::utf8_valid(reinterpret_cast<const uint8_t *>(nm.data()), nm.size())) return -1;
	if (count_load_regions(names, regions) != SK_OK) return -1;
	int64_t stop = -1;
	int code = 0;
	if (sk_count_order_check_dev(c, cols.flag, cols.mapq, cols.tid, cols.pos, cols.n, min_mapq, (int32_t)names.size(), &stop, &code) != SK_OK || stop >= 0) return -1;
	if (sk_count_add_dev(c, cols.flag, cols.mapq, cols.tid, cols.mtid, cols.pos, cols.mpos, cols.tlen, single_end ? cols.end_pos : nullptr, cols.n, min_mapq,
	                     max_frag_len, single_end ? 1 : 0, center ? 1 : 0) != SK_OK || sk_sync(c) != SK_OK) return -1;
	count_print(regions);
	return cols.n;
}

static int count(int argc, char **argv)                            // src/sam_count.rs:20-130
{
	std::vector<host::Opt> opts = {{"--min-mapq", true, false, "0"}, {"--max-frag-len", true, false, "5000"}, {"--single-end", false, false, ""},
	                               {"--center", false, false, ""}};
	std::vector<std::string> pos;
	if (!host::parse_args(argc, argv, 2, opts, pos, 2) || pos.size() != 2) error("Invalid arguments.\n%s", USAGE_COUNT);
	uint64_t v;
	if (!host::parse_uint(opts[0].value.c_str(), 255, v)) error("--min-mapq must be an integer between 0 - 255.");       // :23-24
	const uint8_t min_mapq = (uint8_t)v;
	if (!host::parse_uint(opts[1].value.c_str(), 0xffffffffull, v)) error("--max-frag-len must be an integer.");          // :25
	const uint32_t max_frag_len = (uint32_t)v;
	const bool single_end = opts[2].present, count_centers = opts[3].present;                                              // :26-27

	fputs("Reading target regions from BED file...\n", stderr);                                                            // :30
	std::vector<CountReg> regions;                                                                                              // read_regions, src/common.rs:198-219
	{
		host::LineReader bed(pos[1]);
		std::string line;
		for (;;) {
			const bool ok = bed.read_line(line);
			if (bed.bad_utf8()) error("I/O error while reading from file.");
			if (!ok) break;
			if (!line.empty() && line[0] == '#') continue;
			const size_t off = host::trim_start_off(line), end = host::trim_end_len(line);
			const std::vector<std::string> cols = split_tabs(end > off ? line.substr(off, end - off) : std::string());
			if (cols.size() < 3) error("Invalid region in BED file:\n%s", line.c_str());
			uint64_t s, e;
			if (!host::parse_uint(cols[1].c_str(), 0xffffffffull, s) || !host::parse_uint(cols[2].c_str(), 0xffffffffull, e))
				panic("called `Result::unwrap()` on an `Err` value: ParseIntError (BED)");
			regions.push_back({cols[0], (uint32_t)s, (uint32_t)e});
		}
	}
	fprintf(stderr, "Counting %s...\n", single_end ? "reads" : "DNA fragments");                                            // :34-35
	host::gpu_warmup();
	if (device_path("sam count", pos[0], [&] { return count_from_file(pos[0], regions, min_mapq, max_frag_len, single_end, count_centers); }) >= 0) return 0;
	BamStream bam(pos[0]);                                                                                                 // :36
	for (const std::string &nm : bam.names)                                                                                // :37-38
		if (!host::utf8_valid(reinterpret_cast<const uint8_t *>(nm.data()), nm.size())) panic("called `Result::unwrap()` on an `Err` value: Utf8Error");
	check(count_load_regions(bam.names, regions), "sk_count_set_regions");

	int32_t prev_chr = -1;                                                                                                 // :40-41
	int64_t prev_pos = 0;
	Columns col;
	std::vector<uint8_t> mapq;
	std::vector<BamCore> chunk;
	bool more = true;
	const char *stop = nullptr;                      // an order-dependent error met while reading: raised after the records before it
	int stop_code = 255;
	while (more && !stop) {
		col.clear(); mapq.clear();
		while (col.flag.size() < kBatch && !stop && (more = bam.next_chunk(chunk, single_end))) {
			for (const BamCore &c : chunk) {
				// :46-49 and the order checks :52-73 stay here: they depend on the records before
				if (!((c.flag & 0x4) || (c.flag & 0x400) || (c.flag & 0x100) || (c.flag & 0x800) || c.mapq < min_mapq)) {
					if (c.tid != prev_chr) {
						prev_chr = c.tid;
						if (c.tid < 0 || (size_t)c.tid >= bam.names.size()) { stop = "index out of bounds: chr_names[tid]"; stop_code = 101; break; }
					} else if ((int64_t)c.pos < prev_pos) {
						stop = "Input BAM file is not coordinate sorted."; break;                                              // :70-72
					}
					prev_pos = c.pos;
				}
				col.push(c, true);
				mapq.push_back(c.mapq);
			}
		}
		const int64_t n = (int64_t)col.flag.size();
		if (n == 0) continue;
		check(sk_count_add(host::gpu(), col.flag.data(), mapq.data(), col.tid.data(), col.mtid.data(), col.pos.data(), col.mpos.data(), col.tlen.data(),
		                   single_end ? col.end_pos.data() : nullptr, n, min_mapq, max_frag_len, single_end ? 1 : 0, count_centers ? 1 : 0), "sk_count_add");
	}
	if (stop) { if (stop_code == 101) panic(stop); error("%s", stop); }
	bam.raise_deferred();
	count_print(regions);
	return 0;
}

// ---- sam to raw|fasta|fastq -----------------------------------------------------------------
static const char *USAGE_TO =
	"\nUsage:\n"
	"  sam to raw <bam_file> <out_prefix>\n"
	"  sam to fasta <bam_file> <out_prefix>\n"
	"  sam to fastq <bam_file> <out_prefix>\n"
	"  sam to interleaved raw <bam_file>\n"
	"  sam to interleaved fasta <bam_file>\n"
	"  sam to interleaved fastq <bam_file>\n"
	"\n"
	"These commands convert BAM files into FASTQ, FASTA, or raw sequence-per-line\n"
	"format. Both name-sorted and position-sorted BAM files are supported,\n"
	"but memory usage can reach several GB for position-sorted BAM files.\n"
	"\n"
	"Output is written into files whose name is derived based on output prefix\n"
	"and format. For example, with output format FASTQ and prefix \"sample\",\n"
	"paired end reads are written into files sample_1.fq.gz and sample_2.fq.gz,\n"
	"and orphan reads are written into sample.fq.gz.\n";

enum class OutFmt { RAW, FASTA, FASTQ };

// one of the three destinations of write_reads (:92-93): a gzip file, stdout, or io::sink()
struct ReadSink {
	std::unique_ptr<host::GzWriter> gz;
	bool to_stdout = false;
	void write(const char *p, size_t n)
	{
		if (gz) gz->write(p, n);
		else if (to_stdout) host::out().write(p, n);
	}
	void write(const std::string &s) { write(s.data(), s.size()); }
};

static bool char_boundary(const std::string &s, size_t i) { return i == s.size() || (i < s.size() && ((uint8_t)s[i] & 0xC0) != 0x80); }

static void write_read(ReadSink &out, OutFmt format, const std::string &qname, const std::string &seq)       // :138-149
{
	if (format == OutFmt::FASTQ) {
		const size_t seq_len = (seq.size() - 1) / 2;                                                          // :141
		if (!char_boundary(seq, seq_len) || !char_boundary(seq, seq_len + 1)) panic("byte index is not a char boundary");
		out.write("@", 1); out.write(qname); out.write("\n", 1);
		out.write(seq.data(), seq_len); out.write("\n+\n", 3);
		out.write(seq.data() + seq_len + 1, seq.size() - seq_len - 1); out.write("\n", 1);
	} else if (format == OutFmt::FASTA) {
		out.write(">", 1); out.write(qname); out.write("\n", 1); out.write(seq); out.write("\n", 1);
	} else {
		out.write(seq); out.write("\n", 1);
	}
}

// HashMap<Box<str>, Box<str>> (:98-99) whose leftovers are listed in insertion order (the reference's order is arbitrary)
struct PendingReads {
	struct Val { std::string seq; uint64_t order; };
	std::unordered_map<std::string, Val> map;
	uint64_t next = 0;
	void insert(const std::string &qname, std::string &&seq)
	{
		auto it = map.find(qname);
		if (it != map.end()) it->second.seq = std::move(seq);           // HashMap::insert replaces the value
		else map.emplace(qname, Val{std::move(seq), next++});
	}
	std::vector<const std::pair<const std::string, Val> *> in_order() const
	{
		std::vector<const std::pair<const std::string, Val> *> v;
		v.reserve(map.size());
		for (const auto &kv : map) v.push_back(&kv);
		std::sort(v.begin(), v.end(), [](auto a, auto b) { return a->second.order < b->second.order; });
		return v;
	}
};

static ReadSink g_sinks[3];
static void close_sinks() { for (auto &s : g_sinks) if (s.gz) s.gz->close(); }

// Where the mates of `sam to` are paired when the device serves the file: SEQKIT_HOST_PAIRING=1 on the host, SEQKIT_DEVICE_PAIRING=1 on
// the device, else kDevicePairingDefault (what was measured, and the rule the default follows).
static const bool kDevicePairingDefault = false;
static bool device_pairing_wanted()
{
	if (getenv("SEQKIT_HOST_PAIRING")) return false;
	if (getenv("SEQKIT_DEVICE_PAIRING")) return true;
	return kDevicePairingDefault;
}

// sam to over the FILE.  The device inflates, walks and sizes it, pairs the mates (:113-137) and writes the texts in the order they
// leave (sk_bam_file_pairs): this host writes each window to its sink.  SEQKIT_HOST_PAIRING=1, and every file that call declines (two
// names under one key: info[5] = -94; no room for its working memory: -21), take the path before it: the device writes every kept record's text in file
// order (sk_bam_file_reads) and the pairing runs here over the windows (sam_pairing.h: pair_on_host).  -1: nothing has been written, and
// the caller's reader serves the file (one the file path does not take, a device without room, or a record the reference would panic or
// stop at).  Otherwise the number of records in the file.
static int64_t to_reads_from_file(const std::string &path, OutFmt format, bool interleaved, ReadSink &out_1, ReadSink &out_2, ReadSink &out_single)
{
	sk_ctx *c = host::gpu();
	int handled = 0;
	double info[8];
	const int fmt = format == OutFmt::RAW ? 0 : format == OutFmt::FASTA ? 1 : 2;
	ReadSink *sinks[3] = {&out_1, &out_2, &out_single};
	auto write = [&](int stream, const char *p, size_t n) { sinks[stream]->write(p, n); };
	if (device_pairing_wanted()) {
		uint64_t counts[8];
		if (sk_bam_file_pairs(c, path.c_str(), fmt, 10 /* :103 */, interleaved ? 1 : 0, file_window_bytes(), counts, &handled, info) == SK_OK && handled) {
			if (bamfile_trace()) fprintf(stderr, "sam to pairing: device\n");
			pairing::write_pair_windows([&](sk_bam_pairs_window *w) { check(sk_bam_file_pairs_next(c, w), "sk_bam_file_pairs_next"); }, write);
			return (int64_t)info[3];
		}
		if (info[5] != -94.0 && info[5] != -21.0) return -1;            // (declined as sk_bam_file_reads would: not inflated a second time)
	}
	int64_t n_kept = 0;
	uint64_t text_bytes = 0;
	if (sk_bam_file_reads(c, path.c_str(), fmt, 10 /* :103 */, interleaved ? 0 : 1, file_window_bytes(), &n_kept, &text_bytes, &handled, info) != SK_OK || !handled) return -1;
	if (bamfile_trace()) fprintf(stderr, "sam to pairing: host\n");
	pairing::pair_on_host([&](sk_bam_reads_window *w) { check(sk_bam_file_reads_next(c, w), "sk_bam_file_reads_next"); }, write);
	return (int64_t)info[3];
}

static int to_reads(int argc, char **argv)
{
	const bool interleaved = argc >= 4 && strcmp(argv[2], "interleaved") == 0;
	const char *fmtw = argv[interleaved ? 3 : 2];
	std::vector<host::Opt> opts;
	std::vector<std::string> pos;
	if (!host::parse_args(argc, argv, interleaved ? 4 : 3, opts, pos, 2) || pos.size() != (interleaved ? 1u : 2u)) error("Invalid arguments.\n%s", USAGE_TO);
	const OutFmt format = !strcmp(fmtw, "raw") ? OutFmt::RAW : !strcmp(fmtw, "fasta") ? OutFmt::FASTA : OutFmt::FASTQ;      // :68-71
	ReadSink &out_1 = g_sinks[0], &out_2 = g_sinks[1], &out_single = g_sinks[2];
	if (interleaved) { out_1.to_stdout = true; out_2.to_stdout = true; }                                    // :74-78
	else {                                                                                                   // :79-86
		const char *ext = format == OutFmt::RAW ? "seq" : format == OutFmt::FASTA ? "fa" : "fq";
		out_1.gz.reset(new host::GzWriter(pos[1] + "_1." + ext + ".gz"));
		out_2.gz.reset(new host::GzWriter(pos[1] + "_2." + ext + ".gz"));
		out_single.gz.reset(new host::GzWriter(pos[1] + "." + ext + ".gz"));
		host::at_exit_flush(close_sinks);
	}
	host::gpu_warmup();
	if (device_path("sam to", pos[0], [&] { return to_reads_from_file(pos[0], format, interleaved, out_1, out_2, out_single); }) >= 0) {
		close_sinks();
		return 0;
	}
	BamStream bam(pos[0]);                                                                                   // :96
	PendingReads reads_1, reads_2;

	// a batch of primary records: their bases go through sequence() on the device (:31-59), the rest is text
	struct Rec { std::string qname; uint16_t flag; uint32_t l_seq; size_t off4, offq; };
	std::vector<Rec> recs;
	std::vector<uint8_t> body, raw4, rawq, m4, mq, mout;
	std::vector<uint16_t> lens, flags;
	const size_t kBatchBytes = 48u << 20;
	BamCore c;
	BamStream::Var v;
	bool more = true;
	std::string read_seq;
	while (more) {
		recs.clear(); raw4.clear(); rawq.clear();
		uint32_t max_len = 0;
		while ((more = bam.next_full(c, v, body))) {                                                         // :101
			if ((c.flag & 0x100) || (c.flag & 0x800)) continue;                                              // :102
			if (v.l_seq > 65532) error("Read longer than 65532 bases: not supported by this build.");
			Rec r;
			r.qname.assign(reinterpret_cast<const char *>(body.data()), v.l_read_name - 1);                  // rust-htslib qname(): without the final NUL
			r.flag = c.flag;
			r.l_seq = v.l_seq;
			const uint8_t *seq4 = body.data() + v.l_read_name + 4 * (size_t)v.n_cigar, *qual = seq4 + (v.l_seq + 1) / 2;
			r.off4 = raw4.size(); r.offq = rawq.size();
			raw4.insert(raw4.end(), seq4, seq4 + (v.l_seq + 1) / 2);
			rawq.insert(rawq.end(), qual, qual + v.l_seq);
			recs.push_back(std::move(r));
			max_len = std::max(max_len, v.l_seq);
			if ((recs.size() + 1) * (size_t)(((max_len + 7) & ~7u) + 4) * 3 > kBatchBytes) break;
		}
		const size_t n = recs.size();
		if (n == 0) continue;
		// row pitch: a multiple of 8, so that sequence() runs as its eight-bytes-per-thread kernel whatever the read length
		// (reads within 4 bases of the C-ABI's 65 532 keep the multiple of 4)
		const size_t stride8 = std::max<size_t>(8, (max_len + 7) & ~(size_t)7);
		const size_t stride = stride8 <= 65532 ? stride8 : std::max<size_t>(4, (max_len + 3) & ~(size_t)3), stride4 = std::max<size_t>(4, (stride / 2 + 3) & ~(size_t)3);
		m4.assign(n * stride4, 0); mq.assign(n * stride, 0); mout.resize(n * stride);
		lens.resize(n); flags.resize(n);
		for (size_t i = 0; i < n; i++) {
			memcpy(m4.data() + i * stride4, raw4.data() + recs[i].off4, (recs[i].l_seq + 1) / 2);
			memcpy(mq.data() + i * stride, rawq.data() + recs[i].offq, recs[i].l_seq);
			lens[i] = (uint16_t)recs[i].l_seq;
			flags[i] = recs[i].flag;
		}
		check(sk_bam_sequence(host::gpu(), m4.data(), (int)stride4, mq.data(), (int)stride, lens.data(), flags.data(), (int64_t)n, 10 /* :105 */, mout.data()),
		      "sk_bam_sequence");
		for (size_t i = 0; i < n; i++) {
			const Rec &r = recs[i];
			if (!host::utf8_valid(reinterpret_cast<const uint8_t *>(r.qname.data()), r.qname.size())) {     // :104 str::from_utf8(..).unwrap()
				close_sinks();
				panic("called `Result::unwrap()` on an `Err` value: Utf8Error");
			}
			read_seq.assign(reinterpret_cast<const char *>(mout.data() + i * stride), r.l_seq);
			if (format == OutFmt::FASTQ) {                                                                   // :107-112
				read_seq.push_back('|');
				const uint8_t *q = rawq.data() + r.offq;
				// qualities below 95 (all real ones) are one ASCII byte each: add 33 to the whole row at once; a row with a
				// larger value takes the byte-by-byte form of char::from(u8)
				const size_t at = read_seq.size();
				read_seq.resize(at + r.l_seq);
				uint8_t high = 0;
				for (uint32_t k = 0; k < r.l_seq; k++) {
					const uint8_t ch = (uint8_t)(33 + q[k]);                                                 // u8 arithmetic wraps (release build)
					read_seq[at + k] = (char)ch;
					high |= ch;
				}
				if (high & 0x80) {
					read_seq.resize(at);
					for (uint32_t k = 0; k < r.l_seq; k++) {
						const uint8_t ch = (uint8_t)(33 + q[k]);
						if (ch < 0x80) read_seq.push_back((char)ch);
						else { read_seq.push_back((char)(0xC0 | (ch >> 6))); read_seq.push_back((char)(0x80 | (ch & 0x3F))); }   // char::from(u8) as UTF-8
					}
				}
			}
			if (!(r.flag & 0x1)) {                                                                           // :114-115
				write_read(out_single, format, r.qname, read_seq);
			} else if (r.flag & 0x40) {                                                                      // :116-122
				auto it = reads_2.map.find(r.qname);
				if (it != reads_2.map.end()) {
					write_read(out_1, format, r.qname, read_seq);
					write_read(out_2, format, r.qname, it->second.seq);
					reads_2.map.erase(it);
				} else reads_1.insert(r.qname, std::string(read_seq));
			} else if (r.flag & 0x80) {                                                                      // :123-130
				auto it = reads_1.map.find(r.qname);
				if (it != reads_1.map.end()) {
					write_read(out_1, format, r.qname, it->second.seq);
					write_read(out_2, format, r.qname, read_seq);
					reads_1.map.erase(it);
				} else reads_2.insert(r.qname, std::string(read_seq));
			}
		}
	}
	bam.raise_deferred();
	for (const PendingReads *m : {&reads_1, &reads_2})                                                       // :133-137
		for (const auto *kv : m->in_order()) write_read(out_single, format, kv->first, kv->second.seq);
	close_sinks();
	return 0;
}

// ---- sam trim qnames / tags from qname / qname from tags ------------------------------------------------------------
// src/sam_trim_qnames.rs, src/sam_tags_from_qname.rs, src/sam_qname_from_tags.rs: every record is read, its name (and for tags from
// qname its aux data) rewritten, and written to stdout as BAM (Header::from_template + Writer::from_stdout).  A regular file goes to the
// device whole (sk_bam_file_rewrite): it rewrites and compresses every window, and this host writes the members as they arrive.
// Stdin, SEQKIT_HOST_INFLATE=1 and every file the device declines — among them each one with a record the reference would stop at —
// are read record by record below and written through BamOut, which reproduces the reference's messages, statuses and partial output.
static const char *USAGE_TRIM = "\nUsage:\n  sam trim qnames [options] <bam_file>\n";
static const char *USAGE_TAGS_FROM_QNAME =
	"\nUsage:\n  sam tags from qname [options] <bam_file>\n\nOptions:\n  --uncompressed     Output in uncompressed BAM format\n\n"
	"Finds tags (e.g. \"UMI:xxxx\") in the qname of each BAM record, and turns\nthem into actual SAM format tags.\n";
static const char *USAGE_QNAME_FROM_TAGS =
	"\nUsage:\n  sam qname from tags [options] <bam_file>\n\nOptions:\n  --uncompressed     Output in uncompressed BAM format\n\n"
	"Finds tags (e.g. \"RX:xxxx\") in each BAM record, and appends them to the QNAME.\n";

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
	void flush()
	{
		if (buf_.empty()) return;
		const size_t n = buf_.size(), nblk = (n + SK_DEFLATE_MAX_IN - 1) / SK_DEFLATE_MAX_IN;
		buf_.resize(n + 8, 0);                                       // (the device reads whole dwords)
		std::vector<sk_deflate_block> blocks(nblk);
		for (size_t i = 0; i < nblk; i++) { blocks[i].in_off = i * SK_DEFLATE_MAX_IN; blocks[i].in_len = (uint32_t)std::min<size_t>(SK_DEFLATE_MAX_IN, n - i * SK_DEFLATE_MAX_IN); blocks[i].reserved = 0; }
		std::vector<uint64_t> off(nblk + 1);
		static const bool here = [] { const char *e = getenv("SEQKIT_GPU_DEFLATE"); return e && atoi(e) == 0; }();
		if (level_ && here) deflate_here(blocks, off);
		else if (level_) {
			comp_.resize(nblk * SK_DEFLATE_MAX_MEMBER);
			check(sk_bgzf_deflate(host::gpu(), buf_.data(), n, blocks.data(), (int64_t)nblk, comp_.data(), comp_.size(), off.data()), "sk_bgzf_deflate");
		} else {
			comp_.resize(nblk * (SK_DEFLATE_MAX_IN + 31));
			size_t at = 0;
			static const uint8_t head[16] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0};
			for (size_t i = 0; i < nblk; i++) {
				const uint32_t len = blocks[i].in_len, bsize = len + 31;
				uint8_t *m = comp_.data() + at;
				memcpy(m, head, 16);
				m[16] = (uint8_t)((bsize - 1) & 0xff); m[17] = (uint8_t)((bsize - 1) >> 8);
				m[18] = 1; m[19] = (uint8_t)(len & 0xff); m[20] = (uint8_t)(len >> 8); m[21] = (uint8_t)(~len & 0xff); m[22] = (uint8_t)((~len >> 8) & 0xff);
				memcpy(m + 23, buf_.data() + blocks[i].in_off, len);
				const uint32_t crc = (uint32_t)crc32(crc32(0L, Z_NULL, 0), buf_.data() + blocks[i].in_off, len);
				for (int k = 0; k < 4; k++) { m[23 + len + k] = (uint8_t)(crc >> (8 * k)); m[27 + len + k] = (uint8_t)(len >> (8 * k)); }
				at += bsize;
			}
			off[nblk] = at;
		}
		write_all(comp_.data(), (size_t)off[nblk]);
		buf_.clear();
	}
	void finish()
	{
		if (done_) return;
		done_ = true;
		flush();
		write_all(bamfmt::kBgzfEof, sizeof bamfmt::kBgzfEof);
	}
	static void write_all(const uint8_t *p, size_t n)
	{
		while (n) {
			const ssize_t w = ::write(1, p, n);
			if (w <= 0) error("Output stream closed unexpectedly.");
			p += w; n -= (size_t)w;
		}
	}
private:
	void deflate_here(const std::vector<sk_deflate_block> &blocks, std::vector<uint64_t> &off);
	static constexpr size_t kBatch = (size_t)256 * SK_DEFLATE_MAX_IN;
	int level_;
	bool done_ = false;
	std::vector<uint8_t> buf_, comp_;
};

// (SEQKIT_GPU_DEFLATE=0, the gzip writers' switch: level 1 is deflated here by zlib instead — the inflated stream is the same, and a
// command without --uncompressed can then be run where there is no device)
void BamOut::deflate_here(const std::vector<sk_deflate_block> &blocks, std::vector<uint64_t> &off)
{
	comp_.resize(blocks.size() * SK_DEFLATE_MAX_MEMBER);
	size_t at = 0;
	static const uint8_t head[16] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0};
	for (size_t i = 0; i < blocks.size(); i++) {
		const uint32_t len = blocks[i].in_len;
		const uint8_t *src = buf_.data() + blocks[i].in_off;
		uint8_t *m = comp_.data() + at;
		z_stream z;
		memset(&z, 0, sizeof z);
		if (deflateInit2(&z, 6, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) error("zlib: deflateInit2 failed");
		z.next_in = const_cast<uint8_t *>(src); z.avail_in = len;
		z.next_out = m + 18; z.avail_out = SK_DEFLATE_MAX_MEMBER - 26;
		const int zr = deflate(&z, Z_FINISH);
		uint32_t clen = (uint32_t)z.total_out;
		deflateEnd(&z);
		if (zr != Z_STREAM_END) {                                          // (it does not fit a member: stored)
			m[18] = 1; m[19] = (uint8_t)(len & 0xff); m[20] = (uint8_t)(len >> 8); m[21] = (uint8_t)(~len & 0xff); m[22] = (uint8_t)((~len >> 8) & 0xff);
			memcpy(m + 23, src, len);
			clen = len + 5;
		}
		const uint32_t bsize = clen + 26, crc = (uint32_t)crc32(crc32(0L, Z_NULL, 0), src, len);
		memcpy(m, head, 16);
		m[16] = (uint8_t)((bsize - 1) & 0xff); m[17] = (uint8_t)((bsize - 1) >> 8);
		for (int k = 0; k < 4; k++) { m[18 + clen + k] = (uint8_t)(crc >> (8 * k)); m[22 + clen + k] = (uint8_t)(len >> (8 * k)); }
		at += bsize;
	}
	off[blocks.size()] = at;
}

static BamOut *g_bam_out = nullptr;
static void finish_bam_out() { if (g_bam_out) g_bam_out->finish(); }    // a panic unwinds through the Writer's drop: what was written stays valid BAM

// The first RX field's value when its type is Z or H (bam_aux_get: the walk stops, not finding it, where the aux data stop parsing)
static bool find_rx(const uint8_t *a, size_t n, const uint8_t *&val, size_t &vl)
{
	size_t o = 0;
	while (o + 3 <= n) {
		const uint8_t t0 = a[o], t1 = a[o + 1], ty = a[o + 2];
		size_t v = o + 3, e;
		if (ty == 'A' || ty == 'c' || ty == 'C') e = v + 1;
		else if (ty == 's' || ty == 'S') e = v + 2;
		else if (ty == 'i' || ty == 'I' || ty == 'f') e = v + 4;
		else if (ty == 'Z' || ty == 'H') {
			const void *z = v < n ? memchr(a + v, 0, n - v) : nullptr;
			if (!z) return false;
			e = (size_t)((const uint8_t *)z - a) + 1;
		} else if (ty == 'B') {
			if (v + 5 > n) return false;
			const uint8_t sub = a[v];
			const uint32_t cnt = le32(a + v + 1);
			const size_t es = (sub == 'c' || sub == 'C') ? 1 : (sub == 's' || sub == 'S') ? 2 : (sub == 'i' || sub == 'I' || sub == 'f') ? 4 : 0;
			if (!es) return false;
			e = v + 5 + (size_t)cnt * es;
		} else return false;
		if (e > n) return false;
		if (t0 == 'R' && t1 == 'X') {
			if (ty != 'Z' && ty != 'H') return false;
			val = a + v; vl = e - v - 1;
			return true;
		}
		o = e;
	}
	return false;
}

// The device path of a BAM-writing command: `start` makes the file call that sets the windows up (sk_bam_file_rewrite, _minimize,
// _markdup, _subsample, _recalc_tlen or _merge), and the members go to stdout as they arrive.  -1: nothing has been written, and the caller's reader serves the file (one
// the file path does not take, a device without room, or a record the reference would stop at).  Otherwise the number of records.
template <class Start>
static int64_t bam_out_from_file(Start start)
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
// records before it have been put —, then what is left and the EOF block.
struct HostBamRewrite {
	BamStream bam;
	BamOut out;
	HostBamRewrite(const std::string &path, int level) : bam(path, true), out(level)
	{
		g_bam_out = &out;
		host::at_exit_flush(finish_bam_out);
		const std::vector<uint8_t> hdr = bamfmt::rewrite_header(bam.header_raw);
		out.put(hdr.data(), hdr.size());
		out.flush();
	}
	void close() { bam.raise_deferred(); out.finish(); g_bam_out = nullptr; }
};

// A record with a new name into rec: the block_size and core as read, the name and its NUL, the `n_tail` bytes kept of what followed the
// old name, and `app` (aux data appended); block_size and l_read_name say so.
static void renamed_record(std::vector<uint8_t> &rec, const uint8_t *head, const std::string &name, const uint8_t *tail, size_t n_tail, const std::vector<uint8_t> &app)
{
	const uint32_t bs = (uint32_t)(32 + name.size() + 1 + n_tail + app.size());
	rec.assign(head, head + 36);
	for (int k = 0; k < 4; k++) rec[k] = (uint8_t)(bs >> (8 * k));
	rec[12] = (uint8_t)(name.size() + 1);
	rec.insert(rec.end(), name.begin(), name.end());
	rec.push_back(0);
	rec.insert(rec.end(), tail, tail + n_tail);
	rec.insert(rec.end(), app.begin(), app.end());
}

static int rewrite_cmd(int argc, char **argv, int op, int first, const char *usage, bool has_uncompressed)
{
	std::vector<host::Opt> opts;
	if (has_uncompressed) opts.push_back({"--uncompressed", false, false, ""});
	std::vector<std::string> pos;
	if (!host::parse_args(argc, argv, first, opts, pos, 1) || pos.size() != 1) error("Invalid arguments.\n%s", usage);
	const std::string path = expand_home(pos[0]);
	const int level = has_uncompressed && opts[0].present ? 0 : 1;
	const char *who = op == SK_REWRITE_TRIM_QNAMES ? "sam trim qnames" : op == SK_REWRITE_TAGS_FROM_QNAME ? "sam tags from qname" : "sam qname from tags";
	host::gpu_warmup();
	if (device_path(who, path, [&] { return bam_out_from_file([&](sk_ctx *ctx, uint64_t window, int64_t *n, uint64_t *raw, int *handled) {
		    return sk_bam_file_rewrite(ctx, path.c_str(), op, level, window, n, raw, handled, nullptr); }); }) >= 0) return 0;
	HostBamRewrite io(path, level);
	BamStream &bam = io.bam;
	BamOut &out = io.out;
	BamCore c;
	BamStream::Var v;
	std::vector<uint8_t> body, rec, app;
	std::string name;
	while (bam.next_full(c, v, body)) {
		const size_t L = v.l_read_name - 1;
		const uint8_t *nm = body.data();
		const uint8_t *sp = static_cast<const uint8_t *>(op != SK_REWRITE_QNAME_FROM_TAGS ? memchr(nm, ' ', L) : nullptr);
		bool changed = false;
		app.clear();
		if (op == SK_REWRITE_TRIM_QNAMES && sp) {                                   // src/sam_trim_qnames.rs:20-26
			size_t t = (size_t)(sp - nm);
			if (t < 2) panic("index out of bounds: qname[trim - 2]");
			if (nm[t - 2] == '/' && (nm[t - 1] == '1' || nm[t - 1] == '2')) t -= 2;
			name.assign(reinterpret_cast<const char *>(nm), t);
			changed = true;
		} else if (op == SK_REWRITE_TAGS_FROM_QNAME && sp) {                        // src/sam_tags_from_qname.rs:33-48
			const size_t t = (size_t)(sp - nm);
			name.assign(reinterpret_cast<const char *>(nm), t);
			for (size_t s0 = t + 1;;) {
				size_t e = s0;
				while (e < L && nm[e] != ' ') e++;
				const uint8_t *pt = nm + s0;
				const size_t m = e - s0;
				if (m >= 4 && memcmp(pt, "UMI:", 4) == 0) {
					app.insert(app.end(), {'R', 'X', 'Z'});
					app.insert(app.end(), pt + 4, pt + m);
					app.push_back(0);
				} else if (m >= 3 && pt[2] == ':') {
					app.insert(app.end(), {pt[0], pt[1], 'Z'});
					app.insert(app.end(), pt + 3, pt + m);
					app.push_back(0);
				} else {
					if (!host::utf8_valid(pt, m)) panic("called `Result::unwrap()` on an `Err` value: Utf8Error");
					error("Tag '%.*s' is not supported.", (int)m, reinterpret_cast<const char *>(pt));
				}
				if (e >= L) break;
				s0 = e + 1;
			}
			changed = true;
		} else if (op == SK_REWRITE_QNAME_FROM_TAGS) {                               // src/sam_qname_from_tags.rs:32-38
			const size_t aux = v.aux_off();
			const uint8_t *val = nullptr;
			size_t vl = 0;
			if (find_rx(body.data() + aux, body.size() - aux, val, vl)) {
				name.assign(reinterpret_cast<const char *>(nm), L);
				name += " RX:";
				name.append(reinterpret_cast<const char *>(val), vl);
				if (name.size() > 254) panic("assertion failed: new_qname.len() < 255");
				changed = true;
			}
		}
		if (!changed) {
			out.put(bam.head, 36);
			out.put(body.data(), body.size());
			continue;
		}
		renamed_record(rec, bam.head, name, body.data() + v.l_read_name, body.size() - v.l_read_name, app);
		out.put(rec.data(), rec.size());
	}
	io.close();
	return 0;
}

// ---- sam minimize ------------------------------------------------------------------------------------------------------
// src/sam_minimize.rs: read ids become numbers (--read-ids), the qualities a fill byte (--base-qualities), the aux data go (--tags).
// A regular file goes to the device whole (sk_bam_file_minimize: the ids by a sort of the names' hashes, then the rewrite windows);
// stdin, SEQKIT_HOST_INFLATE=1 and every file the device declines — an invalid record, a CIGAR operation code above 8, where
// rust-htslib's cigar() panics, or two names with one hash — are read record by record below.
static const char *USAGE_MINIMIZE =
	"\nUsage:\n  sam minimize [options] <bam_file>\n\nOptions:\n"
	"  --uncompressed    Output in uncompressed BAM format\n"
	"  --read-ids        Minimize read identifiers (i.e. QNAME fields)\n"
	"  --base-qualities  Remove per-base qualities\n"
	"  --tags            Remove all aux fields (tags)\n"
	"  --baseq-fill=N    Base quality value to fill in as placeholder [default: 255]\n\n"
	"Changes read IDs into simple numeric identifiers, removes per-base qualities,\nand removes all auxiliary fields (tags).\n";

static int minimize_cmd(int argc, char **argv)
{
	std::vector<host::Opt> opts = {{"--uncompressed", false, false, ""}, {"--read-ids", false, false, ""}, {"--base-qualities", false, false, ""},
	                               {"--tags", false, false, ""}, {"--baseq-fill", true, false, "255"}};
	std::vector<std::string> pos;
	if (!host::parse_args(argc, argv, 2, opts, pos, 1) || pos.size() != 1) error("Invalid arguments.\n%s", USAGE_MINIMIZE);
	const std::string path = expand_home(pos[0]);
	const bool read_ids = opts[1].present, baseq = opts[2].present, tags = opts[3].present;
	uint64_t fill64 = 0;
	if (!host::parse_uint(opts[4].value.c_str(), 255, fill64)) error("--baseq-fill must be an integer between 0 and 255.");       // :27-28
	if (!read_ids && !baseq && !tags) error("One of --read-ids, --base-qualities, or --tags must be given.");                    // :30-32
	if (baseq && !tags) error("Running 'sam minimize' with --base-qualities but without the --tags flag is not yet supported.");   // :34-36
	const uint8_t fill = (uint8_t)fill64;
	const int level = opts[0].present ? 0 : 1;
	const int flags = (read_ids ? SK_MINIMIZE_READ_IDS : 0) | (baseq ? SK_MINIMIZE_BASE_QUALITIES : 0) | (tags ? SK_MINIMIZE_TAGS : 0);
	host::gpu_warmup();
	if (device_path("sam minimize", path, [&] { return bam_out_from_file([&](sk_ctx *ctx, uint64_t window, int64_t *n, uint64_t *raw, int *handled) {
		    return sk_bam_file_minimize(ctx, path.c_str(), flags, fill, level, window, n, raw, handled, nullptr); }); }) >= 0) return 0;
	HostBamRewrite io(path, level);
	BamStream &bam = io.bam;
	BamOut &out = io.out;
	BamCore c;
	BamStream::Var v;
	std::vector<uint8_t> body, rec;
	const std::vector<uint8_t> no_aux;
	std::string name;
	std::unordered_map<std::string, uint32_t> qname_to_id;                        // :39-40
	uint32_t highest_id = 0;
	while (bam.next_full(c, v, body)) {
		const size_t L = v.l_read_name - 1;
		const uint8_t *nm = body.data();
		name.assign(reinterpret_cast<const char *>(nm), L);
		if (read_ids) {                                                         // :48-59
			const void *slash = memchr(nm, '/', L);
			if (slash) name.resize((size_t)((const uint8_t *)slash - nm));
			uint32_t id;
			auto it = qname_to_id.find(name);
			if (it != qname_to_id.end()) { id = it->second; qname_to_id.erase(it); }
			else { id = ++highest_id; qname_to_id.emplace(name, id); }
			name = std::to_string(id);
		}
		const uint8_t *cigar = nm + v.l_read_name;                                // :61 read.cigar()
		bool bad_op = false;
		(void)cigar_end_pos(cigar, v.n_cigar, 0, &bad_op);
		if (bad_op) panic("Unexpected cigar operation");
		const size_t cs = 4 * (size_t)v.n_cigar + (((size_t)v.l_seq + 1) >> 1);
		const size_t tail = tags ? cs + v.l_seq : body.size() - v.l_read_name;    // set(): core, name, CIGAR, bases, qualities; set_qname(): all
		renamed_record(rec, bam.head, name, cigar, tail, no_aux);
		const size_t t0 = rec.size() - tail;
		if (tags) {
			if (v.l_seq & 1) rec[t0 + cs - 1] &= 0xf0;                            // (the bases go through as_bytes() and the encoder: the pad nibble is 0)
			if (baseq) memset(rec.data() + t0 + cs, fill, v.l_seq);
		}
		out.put(rec.data(), rec.size());
	}
	io.close();
	return 0;
}

// ---- sam mark duplicates ---------------------------------------------------------------------------------------------------
// src/sam_mark_duplicates.rs: reads that share start position, strand and fragment length or UMI form a cluster; all of a cluster get
// flag 0x400 except its longest read.  A regular file goes to the device whole (sk_bam_file_markdup: signatures, a sort by (tid run,
// start_pos, strand), a greedy per group, the rewrite windows); stdin, SEQKIT_HOST_INFLATE=1 and every file the device declines — one
// with a record the reference stops at among them — go through the reference's own loop below: a FIFO of reads, clustered and flushed
// every 1000 records, at a change of tid and at the end.
static const char *USAGE_MARK_DUPLICATES =
	"\nUsage:\n  sam mark duplicates [options] <bam_file>\n\nOptions:\n"
	"  --uncompressed    Output in uncompressed BAM format\n"
	"  --ignore-umi      Ignore UMI stored in RX tag even if present\n\n"
	"Searches BAM files for DNA fragments that were read multiple times in\nsequencing. When such fragments are found, the highest quality read is\n"
	"kept, and other reads are marked as duplicates.\n\n"
	"The input BAM file must be position-sorted. Output is written to\nthe standard output, preserving the order and content of BAM records,\n"
	"except for the duplicate flag (0x400).\n";

namespace {

struct DupRead {                                                            // :25-32
	uint32_t start_pos, pos, l_seq;
	bool strand, ready;
	uint16_t fraglen;
	std::string umi;
	std::vector<uint8_t> rec;                                               // block_size, core and variable part; the flag at 18
	bool duplicate() const { return rec[19] & 0x04; }
	void set_duplicate(bool on) { rec[19] = (uint8_t)(on ? rec[19] | 0x04 : rec[19] & ~0x04); }
};

// a FIFO that find_clusters indexes: a vector whose front moves
struct DupQueue {
	std::vector<DupRead> v;
	size_t head = 0;
	size_t size() const { return v.size() - head; }
	DupRead &operator[](size_t k) { return v[head + k]; }
	void pop_front() { if (++head == v.size()) { v.clear(); head = 0; } else if (head >= 4096 && head * 2 >= v.size()) { v.erase(v.begin(), v.begin() + (ptrdiff_t)head); head = 0; } }
};

bool umi_matches(const std::string &a, const std::string &b)                 // :169-179
{
	if (a.empty() || b.empty()) return true;
	if (a.size() != b.size()) return false;
	unsigned mismatches = 0;
	for (size_t k = 0; k < a.size(); k++)
		if (!(a[k] == b[k] || a[k] == 'N' || b[k] == 'N')) mismatches++;
	return mismatches <= 1;
}

void find_clusters(DupQueue &reads, uint32_t curr_pos)                       // :131-167
{
	const size_t n = reads.size();
	for (size_t k = 0; k < n; k++) {
		DupRead &rk = reads[k];
		if (rk.ready) continue;
		if (rk.start_pos >= curr_pos) continue;
		size_t best = k;
		uint32_t best_score = rk.l_seq;
		rk.set_duplicate(true);
		rk.ready = true;
		for (size_t j = k + 1; j < n; j++) {
			DupRead &rj = reads[j];
			if (rj.ready) continue;
			if (rj.pos > rk.start_pos) break;
			if (rj.start_pos != rk.start_pos) continue;
			if (rj.strand != rk.strand) continue;
			if (rj.fraglen > 0 && rk.fraglen > 0 && rj.fraglen != rk.fraglen) continue;
			if (!umi_matches(rj.umi, rk.umi)) continue;
			rj.set_duplicate(true);
			rj.ready = true;
			if (rj.l_seq > best_score) { best_score = rj.l_seq; best = j; }
		}
		reads[best].set_duplicate(false);
	}
}

}  // namespace

static void markdup_summary(uint64_t dups, uint64_t total)                    // :112-114
{
	if (total == 0) fprintf(stderr, "%llu / %llu (NaN%%) reads were marked as duplicates.\n", (unsigned long long)dups, (unsigned long long)total);
	else fprintf(stderr, "%llu / %llu (%.1f%%) reads were marked as duplicates.\n", (unsigned long long)dups, (unsigned long long)total,
	             (double)dups / (double)total * 100.0);
}

static int mark_duplicates_cmd(int argc, char **argv)
{
	std::vector<host::Opt> opts = {{"--uncompressed", false, false, ""}, {"--ignore-umi", false, false, ""}};
	std::vector<std::string> pos;
	if (!host::parse_args(argc, argv, 3, opts, pos, 1) || pos.size() != 1) error("Invalid arguments.\n%s", USAGE_MARK_DUPLICATES);
	const std::string path = expand_home(pos[0]);
	const int level = opts[0].present ? 0 : 1;
	const bool ignore_umi = opts[1].present;
	host::gpu_warmup();
	int64_t dups = 0;                                                           // the output records that carry 0x400
	const int64_t n_dev = device_path("sam mark duplicates", path, [&] { return bam_out_from_file([&](sk_ctx *ctx, uint64_t window, int64_t *n, uint64_t *raw, int *handled) {
		    return sk_bam_file_markdup(ctx, path.c_str(), ignore_umi ? 1 : 0, level, window, n, &dups, raw, handled, nullptr); }); });
	if (n_dev >= 0) {
		markdup_summary((uint64_t)dups, (uint64_t)n_dev);
		return 0;
	}
	HostBamRewrite io(path, level);
	BamStream &bam = io.bam;
	BamOut &out = io.out;
	uint64_t total_reads = 0, total_duplicates = 0;
	uint32_t prev_pos = 0;
	int32_t prev_chr = -1;
	DupQueue reads;
	auto flush_reads = [&]() {                                                  // :120-128
		uint64_t flushed = 0;
		while (reads.size() && reads[0].ready) {
			if (reads[0].duplicate()) flushed++;
			out.put(reads[0].rec.data(), reads[0].rec.size());
			reads.pop_front();
		}
		return flushed;
	};
	BamCore c;
	BamStream::Var v;
	std::vector<uint8_t> body;
	while (bam.next_full(c, v, body)) {
		if (c.flag & 0x900) error("BAM file contains secondary or supplementary reads. These are not currently supported.");   // :51-53
		const uint32_t left_pos = (uint32_t)c.pos;
		if (c.tid != prev_chr) {                                                // :58-64
			find_clusters(reads, UINT32_MAX);
			total_duplicates += flush_reads();
			prev_chr = c.tid;
		} else if (left_pos < prev_pos) error("Input BAM file is not coordinate sorted.");
		prev_pos = left_pos;
		const bool unmapped = c.flag & 0x4, reverse = c.flag & 0x10;
		reads.v.emplace_back();
		DupRead &r = reads.v.back();
		r.start_pos = 0;
		if (!unmapped && reverse) {                                             // :73 read.cigar().end_pos()
			bool bad_op = false;
			r.start_pos = (uint32_t)(int32_t)cigar_end_pos(body.data() + v.l_read_name, v.n_cigar, c.pos, &bad_op);
			if (bad_op) { reads.v.pop_back(); panic("Unexpected cigar operation"); }
		} else if (!unmapped) r.start_pos = left_pos;
		r.fraglen = 0;
		if (!unmapped) {                                                        // :79-91
			if (!ignore_umi) {
				const size_t aux = v.aux_off();
				const uint8_t *val = nullptr;
				size_t vl = 0;
				if (find_rx(body.data() + aux, body.size() - aux, val, vl)) r.umi.assign(reinterpret_cast<const char *>(val), vl);
			}
			if (r.umi.empty()) r.fraglen = (uint16_t)std::min<int64_t>(std::llabs((long long)c.tlen), 65535);
		}
		r.pos = left_pos; r.l_seq = v.l_seq; r.strand = !reverse; r.ready = unmapped;
		r.rec.assign(bam.head, bam.head + 36);
		r.rec.insert(r.rec.end(), body.begin(), body.end());
		total_reads++;
		if (total_reads % 1000 == 0) {                                          // :101-104
			total_duplicates += flush_reads();
			find_clusters(reads, left_pos);
		}
	}
	bam.raise_deferred();                                                       // (before the reads still queued would be written)
	find_clusters(reads, UINT32_MAX);                                           // :108-110
	total_duplicates += flush_reads();
	io.close();
	markdup_summary(total_duplicates, total_reads);
	return 0;
}

// ---- sam subsample -----------------------------------------------------------------------------------------------------
// src/sam_subsample.rs: a fraction of the fragments is kept, mates together.  The reference draws from an unseeded generator; here draw
// number d is a pure function of (seed, d) (sk_subsample_keep), the seed --seed=N or 8 bytes from the OS, so that the device, which
// numbers the fragments with a sort, and the loop below write the same bytes.  A regular file goes to the device whole
// (sk_bam_file_subsample: fragment numbers, decisions, the kept records compacted, then the rewrite windows); stdin,
// SEQKIT_HOST_INFLATE=1 and every file the device declines — a counted record without 0x1, an invalid record, or two names with one
// hash — are read record by record below.
static const char *USAGE_SUBSAMPLE =
	"\nUsage:\n  sam subsample [options] <bam_file> <fraction>\n\nOptions:\n"
	"  --seed=N    Seed of the random draws, for a reproducible result [default: from the OS]\n\n"
	"If your BAM file has been duplicate-flagged, remember to re-run duplicate\nflagging after subsampling, otherwise random subsampling can delete the only\n"
	"non-duplicate-flagged DNA fragment in a duplicate cluster.\n";

// str::parse::<f32>(): [+-] then inf | infinity | nan in any case, or digits with at most one '.' and at least one digit, then an
// optional exponent [eE][+-]digits; nothing else, no blanks.  The value is the nearest f32 (strtof rounds correctly).
static bool parse_f32(const std::string &s, float &out)
{
	size_t i = 0;
	if (i < s.size() && (s[i] == '+' || s[i] == '-')) i++;
	std::string low;
	for (size_t k = i; k < s.size(); k++) low.push_back((char)(s[k] >= 'A' && s[k] <= 'Z' ? s[k] + 32 : s[k]));
	if (low != "inf" && low != "infinity" && low != "nan") {
		size_t digits = 0;
		while (i < s.size() && s[i] >= '0' && s[i] <= '9') { i++; digits++; }
		if (i < s.size() && s[i] == '.') i++;
		while (i < s.size() && s[i] >= '0' && s[i] <= '9') { i++; digits++; }
		if (!digits) return false;
		if (i < s.size() && (s[i] == 'e' || s[i] == 'E')) {
			i++;
			if (i < s.size() && (s[i] == '+' || s[i] == '-')) i++;
			size_t ed = 0;
			while (i < s.size() && s[i] >= '0' && s[i] <= '9') { i++; ed++; }
			if (!ed) return false;
		}
		if (i != s.size()) return false;
	}
	out = strtof(s.c_str(), nullptr);
	return true;
}

static void subsample_summary(uint64_t kept, uint64_t total)                  // :61-62
{
	fprintf(stderr, "Total reads: %llu\n", (unsigned long long)total);
	fprintf(stderr, "Kept reads: %llu (%s%% of all reads)\n", (unsigned long long)kept, host::fmt_pct((double)kept / (double)total * 100.0).c_str());
}

static int subsample_cmd(int argc, char **argv)
{
	// (a fraction such as -0.1 is a positional whose value the command itself refuses: it goes behind a "--" of its own)
	std::vector<char *> av(argv, argv + 2), rest;
	bool only_pos = false;
	for (int i = 2; i < argc; i++) {
		char *a = argv[i];
		if (!only_pos && strcmp(a, "--") == 0) { only_pos = true; continue; }
		const bool number = a[0] == '-' && ((a[1] >= '0' && a[1] <= '9') || a[1] == '.');
		(only_pos || number ? rest : av).push_back(a);
	}
	static char dashes[] = "--";
	av.push_back(dashes);
	av.insert(av.end(), rest.begin(), rest.end());
	std::vector<host::Opt> opts = {{"--seed", true, false, ""}};
	std::vector<std::string> pos;
	if (!host::parse_args((int)av.size(), av.data(), 2, opts, pos, 2) || pos.size() != 2) error("Invalid arguments.\n%s", USAGE_SUBSAMPLE);
	const std::string path = expand_home(pos[0]);
	uint64_t seed = 0;
	if (opts[0].present) {
		if (!host::parse_uint(opts[0].value.c_str(), UINT64_MAX, seed)) error("--seed must be an integer between 0 and 18446744073709551615.");
	} else if (getrandom(&seed, sizeof seed, 0) != (ssize_t)sizeof seed) error("Cannot get a seed from the operating system.");
	float frac = -1.0f;
	if (!parse_f32(pos[1], frac) || !(frac >= 0.0f && frac <= 1.0f)) error("Subsampling fraction must be between 0 - 1.");     // :19-22
	host::gpu_warmup();
	int64_t counted = 0;
	const int64_t n_dev = device_path("sam subsample", path, [&] { return bam_out_from_file([&](sk_ctx *ctx, uint64_t window, int64_t *n, uint64_t *raw, int *handled) {
		    return sk_bam_file_subsample(ctx, path.c_str(), frac, seed, 1, window, n, &counted, raw, handled, nullptr); }); });
	if (n_dev >= 0) {
		subsample_summary((uint64_t)n_dev, (uint64_t)counted);
		return 0;
	}
	HostBamRewrite io(path, 1);
	BamStream &bam = io.bam;
	BamOut &out = io.out;
	uint64_t total_reads = 0, kept_reads = 0, draws = 0;
	std::unordered_map<std::string, bool> keep_mate;                              // :33
	BamCore c;
	BamStream::Var v;
	std::vector<uint8_t> body;
	std::string name;
	while (bam.next_full(c, v, body)) {
		if (c.flag & 0x800) continue;                                             // :36
		if (!(c.flag & 0x1)) error("Only paired end sequencing data supported for now.");      // :57
		name.assign(reinterpret_cast<const char *>(body.data()), v.l_read_name - 1);
		bool keep;
		auto it = keep_mate.find(name);
		if (it != keep_mate.end()) { keep = it->second; keep_mate.erase(it); }
		else { keep = sk_subsample_keep(seed, ++draws, frac) == 1; keep_mate.emplace(name, keep); }
		if (keep) {
			out.put(bam.head, 36);
			out.put(body.data(), body.size());
			kept_reads++;
		}
		total_reads++;
	}
	io.close();
	subsample_summary(kept_reads, total_reads);
	return 0;
}

// ---- sam recalculate tlen ----------------------------------------------------------------------------------------------
// src/sam_recalculate_tlen.rs: TLEN becomes the distance between the mates' 5' ends; a candidate whose mate never comes is dropped with
// a line on stderr.  A regular file goes to the device whole (sk_bam_file_recalc_tlen: classes, the mates linked by a sort of the names'
// hashes, the pairs' TLENs, the written records compacted, then the rewrite windows; the dropped records' names afterwards); stdin,
// SEQKIT_HOST_INFLATE=1 and every file the device declines — a record the reference stops at, a name or a CIGAR it might stop at, an
// invalid record, or two names with one hash — go through the reference's own loop below: a FIFO of reads and a map from a name to the
// place of the read that waits for its mate.
static const char *USAGE_RECALCULATE_TLEN =
	"\nUsage:\n  sam recalculate tlen [options] <bam_file>\n\nOptions:\n"
	"  --uncompressed    Output in uncompressed BAM format\n"
	"  --max-len=N       Maximum fragment length [default: 5000]\n\n"
	"Recalculates SAM record TLEN (template length) field based on the distance\nbetween the 5' ends of paired mates. This ensures that the TLEN represents the \n"
	"actual DNA fragment length.\n";

static void discarded_line(const uint8_t *name, size_t n)                    // :103
{
	fputs("Read ", stderr);
	fwrite(name, 1, n, stderr);
	fputs(" discarded due to missing mate.\n", stderr);
}

static int recalculate_tlen_cmd(int argc, char **argv)
{
	std::vector<host::Opt> opts = {{"--uncompressed", false, false, ""}, {"--max-len", true, false, "5000"}};
	std::vector<std::string> pos;
	if (!host::parse_args(argc, argv, 3, opts, pos, 1) || pos.size() != 1) error("Invalid arguments.\n%s", USAGE_RECALCULATE_TLEN);
	const std::string path = expand_home(pos[0]);
	int64_t max_len = 0;
	if (!parse_i64(opts[1].value, max_len)) max_len = 0;                         // :29 parse().unwrap_or(0)
	if (max_len <= 0) error("--max-len must be a positive integer.");            // :30
	const int level = opts[0].present ? 0 : 1;
	host::gpu_warmup();
	int64_t n_disc = 0;
	if (device_path("sam recalculate tlen", path, [&] { return bam_out_from_file([&](sk_ctx *ctx, uint64_t window, int64_t *n, uint64_t *raw, int *handled) {
		    return sk_bam_file_recalc_tlen(ctx, path.c_str(), max_len, level, window, n, &n_disc, raw, handled, nullptr); }); }) >= 0) {
		std::vector<uint8_t> names;
		for (int64_t first = 0; first < n_disc;) {
			const int64_t step = std::min<int64_t>(n_disc - first, 4096);
			names.resize((size_t)step * 256);
			check(sk_bam_file_recalc_tlen_discarded(host::gpu(), first, step, names.data()), "sk_bam_file_recalc_tlen_discarded");
			for (int64_t k = 0; k < step; k++) discarded_line(names.data() + k * 256, strlen(reinterpret_cast<const char *>(names.data() + k * 256)));
			first += step;
		}
		return 0;
	}
	HostBamRewrite io(path, level);
	BamStream &bam = io.bam;
	BamOut &out = io.out;
	struct TlenRead { bool ready; int32_t tlen; std::vector<uint8_t> rec; };   // :20-24 (rec: block_size, core and variable part)
	std::deque<TlenRead> reads;                                                  // :38-40
	std::unordered_map<std::string, size_t> mates;
	size_t reads_written = 0;
	auto write = [&](TlenRead &r) {                                             // :90-92 set_insert_size, write
		for (int k = 0; k < 4; k++) r.rec[32 + k] = (uint8_t)((uint32_t)r.tlen >> (8 * k));
		out.put(r.rec.data(), r.rec.size());
	};
	// the 5' end of a queued or current record (:60-61); cigar() panics at an operation code above 8
	auto start_of = [](const std::vector<uint8_t> &rec) {
		const int64_t p = (int32_t)le32(rec.data() + 8);
		if (!(rec[18] & 0x10)) return p;
		bool bad_op = false;
		const int64_t e = cigar_end_pos(rec.data() + 36 + rec[12], le32(rec.data() + 16) & 0xffff, p, &bad_op);
		if (bad_op) panic("Unexpected cigar operation");
		return e - 1;
	};
	BamCore c;
	BamStream::Var v;
	std::vector<uint8_t> body;
	std::string name;
	while (bam.next_full(c, v, body)) {
		const size_t L = v.l_read_name - 1;
		if (!host::utf8_valid(body.data(), L)) panic("called `Result::unwrap()` on an `Err` value: Utf8Error");   // :43
		TlenRead rd{true, 0, {}};
		rd.rec.assign(bam.head, bam.head + 36);
		rd.rec.insert(rd.rec.end(), body.begin(), body.end());
		const uint16_t f = c.flag;
		if (!(f & 0x1) || (f & 0x4) || (f & 0x8)) reads.push_back(std::move(rd));                        // :44-47
		else if (f & 0x900) error("Secondary and supplementary read alignments are not supported.");   // :48-49
		else if (c.tid != c.mtid || std::llabs((long long)c.pos - (long long)c.mpos) > max_len || !(f & 0x10) == !(f & 0x20))
			reads.push_back(std::move(rd));                                                            // :50-54
		else {
			name.assign(reinterpret_cast<const char *>(body.data()), L);
			auto it = mates.find(name);
			if (it != mates.end()) {                                            // :57-79
				TlenRead &mate = reads[it->second - reads_written];
				mates.erase(it);
				if (!((f ^ mate.rec[18]) & 0x40)) panic("assertion failed: read.is_first_in_template() != mate.is_first_in_template()");
				const int64_t start_pos = start_of(rd.rec), mate_start_pos = start_of(mate.rec);
				int64_t tlen = std::llabs((long long)(start_pos - mate_start_pos)) + 1;
				if (c.pos > (int32_t)le32(mate.rec.data() + 8)) tlen = -tlen;
				if ((start_pos < mate_start_pos && (f & 0x10)) || (start_pos > mate_start_pos && !(f & 0x10))) tlen = 0;
				rd.tlen = (int32_t)(uint32_t)(uint64_t)tlen;                    // `as i32`: the low 32 bits
				mate.tlen = (int32_t)(uint32_t)(uint64_t)(-tlen);
				mate.ready = true;
				reads.push_back(std::move(rd));
			} else {
				mates.emplace(name, reads_written + reads.size());
				rd.ready = false;
				reads.push_back(std::move(rd));
			}
		}
		while (!reads.empty() && reads.front().ready) {                         // :89-95
			write(reads.front());
			reads.pop_front();
			reads_written++;
		}
	}
	bam.raise_deferred();                                                       // (before the reads still queued would be written)
	for (TlenRead &r : reads) {                                                 // :101-111
		if (!r.ready) { discarded_line(r.rec.data() + 36, (size_t)r.rec[12] - 1); continue; }
		write(r);
	}
	io.close();
	return 0;
}

// ---- sam merge -----------------------------------------------------------------------------------------------------------
// src/sam_merge.rs: the inputs' records by (u32 refID, i32 pos), each input's own order kept.  The reference's heap leaves the order of
// records of DIFFERENT inputs with one key to its internals; here they go by the input's place on the command line, so
// that the command is a stable merge and the device, which sorts all records at once (sk_bam_file_merge), and the loop below write the
// same bytes.  Regular files go to the device whole; a "-" among the inputs, SEQKIT_HOST_INFLATE=1 and every call the device declines —
// reference names that differ, an unsorted input, an invalid record, a suffixed name above 254 bytes, more than 99 inputs — are read
// record by record below.
static const char *USAGE_MERGE =
	"\nUsage:\n  sam merge [options] <bam_files>...\n\nOptions:\n"
	"  --suffix          Add a suffix to read identifiers to avoid clashes\n"
	"  --uncompressed    Output in uncompressed BAM format\n\n"
	"Merges two or more position-sorted BAM files together, ensuring that the\nresulting output BAM file is also position-sorted.\n";

struct MergeInput {
	std::unique_ptr<BamStream> bam;
	BamCore c;
	BamStream::Var v;
	uint8_t head[36];
	std::vector<uint8_t> body;
	bool have = false;
	void advance()                                                            // (a reader's error ends the command where the reference's next() would)
	{
		have = bam->next_full(c, v, body);
		if (have) memcpy(head, bam->head, 36);
		else bam->raise_deferred();
	}
};

static int merge_cmd(int argc, char **argv)
{
	std::vector<host::Opt> opts = {{"--suffix", false, false, ""}, {"--uncompressed", false, false, ""}};
	std::vector<std::string> pos;
	if (!host::parse_args(argc, argv, 2, opts, pos, (size_t)-1) || pos.empty()) error("Invalid arguments.\n%s", USAGE_MERGE);
	if (pos.size() < 2) error("At least two BAM files must be provided for concatenation.");      // :62-64
	const bool suffix = opts[0].present;
	const int level = opts[1].present ? 0 : 1;
	std::vector<std::string> paths;
	bool any_stdin = false;
	for (const std::string &p : pos) { paths.push_back(expand_home(p)); any_stdin = any_stdin || paths.back() == "-"; }
	host::gpu_warmup();
	if (device_path("sam merge", any_stdin ? std::string("-") : paths[0], [&] { return bam_out_from_file([&](sk_ctx *ctx, uint64_t window, int64_t *n, uint64_t *raw, int *handled) {
		    std::vector<const char *> cp;
		    for (const std::string &p : paths) cp.push_back(p.c_str());
		    return sk_bam_file_merge(ctx, cp.data(), (int)cp.size(), suffix ? 1 : 0, level, window, n, raw, handled, nullptr); }); }) >= 0) return 0;
	std::vector<MergeInput> in(paths.size());
	for (size_t b = 0; b < paths.size(); b++) in[b].bam.reset(new BamStream(paths[b], b == 0));      // :68
	for (size_t b = 1; b < paths.size(); b++)                                                       // :71-76
		if (in[b].bam->names != in[0].bam->names) error("Input BAM files %s and %s have different SQ fields.", pos[0].c_str(), pos[b].c_str());
	BamOut out(level);
	g_bam_out = &out;
	host::at_exit_flush(finish_bam_out);
	{
		const std::vector<uint8_t> hdr = bamfmt::rewrite_header(in[0].bam->header_raw);
		out.put(hdr.data(), hdr.size());
		out.flush();
	}
	for (MergeInput &m : in) m.advance();                                                           // :83-87
	uint8_t head[36];
	std::vector<uint8_t> body, rec;
	const std::vector<uint8_t> none;
	std::string name;
	for (;;) {
		MergeInput *first = nullptr;                                          // the smallest key; among equal keys the lowest input
		for (MergeInput &m : in) {
			if (!m.have) continue;
			if (!first || (uint32_t)m.c.tid < (uint32_t)first->c.tid || (m.c.tid == first->c.tid && m.c.pos < first->c.pos)) first = &m;
		}
		if (!first) break;
		const uint32_t l_read_name = first->v.l_read_name;
		memcpy(head, first->head, 36);
		body.swap(first->body);
		first->advance();                                                     // :91-93 (before the record is written)
		if (suffix) {                                                         // :94-99
			name.assign(reinterpret_cast<const char *>(body.data()), l_read_name - 1);
			name += "." + std::to_string((size_t)(first - in.data()) + 1);
			if (name.size() > 254) panic("assertion failed: new_qname.len() < 255");
			renamed_record(rec, head, name, body.data() + l_read_name, body.size() - l_read_name, none);
			out.put(rec.data(), rec.size());
		} else {
			out.put(head, 36);
			out.put(body.data(), body.size());
		}
	}
	out.finish();
	g_bam_out = nullptr;
	return 0;
}

// ---- sam coverage histogram (src/sam_coverage_histogram.rs) ----------------------------------------------------
// The reference starts `samtools depth -a`, parses its one line per position back and counts the positions of every depth up to
// 10 000.  No samtools is started here: the rule of include/seqkit_hip.h (sk_bam_file_coverage) is this build's reading of it.  The
// host's part is the options: REGION and the BED file become (refID, beg, end) triples against the header's reference list.  A regular
// file goes to the device whole; "-", SEQKIT_HOST_INFLATE=1 and every file the device declines are read record by record below, where
// the same rule runs sequentially: the events of every counted record's runs and of the targets, sorted, then one sweep.
static const char *USAGE_COVERAGE =
	"\nUsage:\n  sam coverage histogram [options] <bam_file>\n\nOptions:\n"
	"  --region=REGION   Region to calculate coverage in [default: everywhere]\n"
	"  --regions=BED     BED file of regions to calculate coverage in\n"
	"                    [default: everywhere]\n";

namespace {

struct CovRefs { std::vector<std::string> names; std::vector<uint32_t> len; };

// the reference list of complete header bytes ("BAM\1" .. the end of the list); false: they end before the list does, or are no header
bool cov_refs(const uint8_t *h, uint64_t n, CovRefs &out)
{
	out.names.clear(); out.len.clear();
	bamfmt::RefList refs;
	if (refs.parse(h, n, n) != bamfmt::RefList::kOk) return false;
	out.names = refs.names(h);
	for (const bamfmt::RefList::Ref &r : refs.refs) out.len.push_back(r.l_ref);
	return true;
}

// The reference list of a BAM file, for the options of a command whose records the device reads: the file's first BGZF members
// inflated here until the header is complete.  false: anything out of the ordinary, which the host reader then reports in its words.
bool cov_refs_of_file(const std::string &path, CovRefs &out)
{
	FILE *f = fopen(path.c_str(), "rb");
	if (!f) return false;
	std::vector<uint8_t> raw, member, piece(65536);
	bool ok = false;
	for (;;) {
		uint8_t h[18];
		if (fread(h, 1, 18, f) != 18 || h[0] != 31 || h[1] != 139 || h[2] != 8 || !(h[3] & 4)) break;
		const size_t xlen = (size_t)h[10] | ((size_t)h[11] << 8), bsize = ((size_t)h[16] | ((size_t)h[17] << 8)) + 1;
		if (xlen != 6 || h[12] != 'B' || h[13] != 'C' || bsize < 26) break;                 // (a BC field elsewhere: the host reader's)
		member.resize(bsize - 18);
		if (fread(member.data(), 1, member.size(), f) != member.size()) break;
		z_stream z;
		memset(&z, 0, sizeof z);
		if (inflateInit2(&z, -15) != Z_OK) break;
		z.next_in = member.data(); z.avail_in = (uInt)(member.size() - 8);
		z.next_out = piece.data(); z.avail_out = (uInt)piece.size();
		const int zr = inflate(&z, Z_FINISH);
		const size_t got = z.total_out;
		inflateEnd(&z);
		if (zr != Z_STREAM_END) break;
		raw.insert(raw.end(), piece.begin(), piece.begin() + (ptrdiff_t)got);
		if (cov_refs(raw.data(), raw.size(), out)) { ok = true; break; }
		if (raw.size() > ((size_t)1 << 30)) break;
	}
	fclose(f);
	return ok;
}

// 1 to 18 decimal digits
bool cov_digits(const std::string &s, int64_t &v)
{
	if (s.empty() || s.size() > 18) return false;
	v = 0;
	for (char ch : s) { if (ch < '0' || ch > '9') return false; v = v * 10 + (ch - '0'); }
	return true;
}

int64_t cov_ref_index(const CovRefs &refs, const std::string &name)
{
	for (size_t k = 0; k < refs.names.size(); k++) if (refs.names[k] == name) return (int64_t)k;
	return -1;
}

// REGION: name | name:beg | name:beg-end, 1-based inclusive, commas in the numbers ignored; a string that is a reference name as a
// whole wins over the split at its last colon; beg < 1 reads as 1.  false: it names no reference or does not parse.
bool cov_parse_region(const std::string &s, const CovRefs &refs, std::vector<int64_t> &t)
{
	int64_t r = cov_ref_index(refs, s);
	if (r >= 0) { t = {r, 0, (int64_t)refs.len[(size_t)r]}; return true; }
	const size_t colon = s.rfind(':');
	if (colon == std::string::npos || (r = cov_ref_index(refs, s.substr(0, colon))) < 0) return false;
	std::string rest;
	for (size_t k = colon + 1; k < s.size(); k++) if (s[k] != ',') rest.push_back(s[k]);
	const size_t dash = rest.find('-');
	int64_t beg = 0, end = (int64_t)refs.len[(size_t)r];
	if (!cov_digits(rest.substr(0, dash), beg)) return false;
	if (dash != std::string::npos && !cov_digits(rest.substr(dash + 1), end)) return false;
	t = {r, std::max<int64_t>(beg, 1) - 1, end};
	return true;
}

// the BED file's lines: (name, beg, end), 0-based half-open; fields separated by tabs or blanks
struct CovBedLine { std::string name; int64_t beg, end; };
std::vector<CovBedLine> cov_read_bed(const std::string &path)
{
	std::vector<CovBedLine> out;
	host::LineReader bed(path);
	std::string line;
	for (;;) {
		const bool ok = bed.read_line(line);
		if (bed.bad_utf8()) error("I/O error while reading from file.");
		if (!ok) break;
		if (line.compare(0, 1, "#") == 0 || line.compare(0, 5, "track") == 0 || line.compare(0, 7, "browser") == 0) continue;
		std::vector<std::string> f;
		for (size_t a = 0; a < line.size();) {
			while (a < line.size() && (line[a] == ' ' || line[a] == '\t' || line[a] == '\r' || line[a] == '\n')) a++;
			size_t b = a;
			while (b < line.size() && !(line[b] == ' ' || line[b] == '\t' || line[b] == '\r' || line[b] == '\n')) b++;
			if (b > a) f.push_back(line.substr(a, b - a));
			a = b;
		}
		if (f.empty()) continue;
		CovBedLine v;
		if (f.size() < 3 || !cov_digits(f[1], v.beg) || !cov_digits(f[2], v.end)) error("Invalid region in BED file:\n%s", line.c_str());
		v.name = f[0];
		out.push_back(v);
	}
	return out;
}

std::vector<int64_t> cov_bed_targets(const std::vector<CovBedLine> &bed, const CovRefs &refs)
{
	std::vector<int64_t> t;
	for (const CovBedLine &v : bed) {
		const int64_t r = cov_ref_index(refs, v.name);
		if (r >= 0) { t.push_back(r); t.push_back(v.beg); t.push_back(v.end); }
	}
	return t;
}

void cov_print(const uint64_t *hist)                                          // :56-58
{
	char buf[48];
	for (int k = 0; k < SK_COVERAGE_BINS; k++) {
		snprintf(buf, sizeof buf, "%d\t%llu\n", k, (unsigned long long)hist[k]);
		host::out().write(buf, strlen(buf));
	}
}

// The rule on the host: events as (g << 2 | kind), kinds as sk_bamcoverage.hip's.  (62 bits of coordinate: a header whose references
// add up to more is not one this reader serves.)
struct CovHost {
	const CovRefs &refs;
	std::vector<uint64_t> base, ev;
	std::vector<uint8_t> has, hit;
	std::vector<std::vector<std::pair<int64_t, int64_t>>> merged;            // mode 2: per reference, sorted and disjoint
	explicit CovHost(const CovRefs &r) : refs(r), base(r.len.size() + 1, 0), has(r.len.size(), 0), hit(r.len.size(), 0)
	{
		for (size_t k = 0; k < r.len.size(); k++) base[k + 1] = base[k] + r.len[k];
		if (base.back() >> 61) error("The reference list of the BAM file is too long.");
	}
	void set_intervals(const std::vector<int64_t> &t)
	{
		merged.assign(refs.len.size(), {});
		for (size_t k = 0; k + 2 < t.size(); k += 3) if (t[k + 1] < t[k + 2]) merged[(size_t)t[k]].push_back({t[k + 1], t[k + 2]});
		for (auto &v : merged) {
			std::sort(v.begin(), v.end());
			size_t n = 0;
			for (const auto &iv : v) {
				if (n && iv.first <= v[n - 1].second) v[n - 1].second = std::max(v[n - 1].second, iv.second);
				else v[n++] = iv;
			}
			v.resize(n);
		}
	}
	void event(size_t r, int64_t p, unsigned kind) { ev.push_back(((base[r] + (uint64_t)p) << 2) | kind); }
	void target(size_t r, int64_t beg, int64_t end)
	{
		beg = std::max<int64_t>(beg, 0); end = std::min<int64_t>(end, refs.len[r]);
		if (beg < end) { event(r, beg, 2); event(r, end, 3); }
	}
	void record(const BamCore &c, const uint8_t *cigar, uint32_t n_cigar)
	{
		if (c.tid < 0 || (size_t)c.tid >= refs.len.size() || (c.flag & 0x704)) return;
		const size_t r = (size_t)c.tid;
		const int64_t l_ref = refs.len[r];
		has[r] = 1;
		int64_t p = c.pos, rs = 0;
		bool open = false;
		auto close = [&] {
			const int64_t s = std::max<int64_t>(rs, 0), e = std::min(p, l_ref);
			if (s < e) { event(r, s, 0); event(r, e, 1); }
			open = false;
		};
		for (uint32_t q = 0; q < n_cigar; q++) {
			const uint32_t op = le32(cigar + 4 * q), code = op & 15;
			if (code == 0 || code == 7 || code == 8) { if (!open) { rs = p; open = true; } p += op >> 4; }
			else if (code == 2 || code == 3) { if (open) close(); p += op >> 4; }
		}
		if (open) close();
		if (!merged.empty() && !hit[r]) {
			const int64_t end = p > c.pos ? p : (int64_t)c.pos + 1;
			const auto &v = merged[r];
			auto it = std::partition_point(v.begin(), v.end(), [&](const std::pair<int64_t, int64_t> &iv) { return iv.second <= (int64_t)c.pos; });
			if (it != v.end() && it->first < end) hit[r] = 1;
		}
	}
	void histogram(uint64_t *hist)
	{
		std::sort(ev.begin(), ev.end());
		int64_t depth = 0, inside = 0;
		for (size_t i = 0; i + 1 < ev.size(); i++) {
			switch (ev[i] & 3) { case 0: depth++; break; case 1: depth--; break; case 2: inside++; break; default: inside--; }
			const uint64_t w = (ev[i + 1] >> 2) - (ev[i] >> 2);
			if (inside > 0 && w && depth <= SK_COVERAGE_BINS - 1) hist[depth] += w;          // (deeper: `continue`, :52)
		}
	}
};

}  // namespace

static int coverage_histogram_cmd(int argc, char **argv)
{
	std::vector<host::Opt> opts = {{"--region", true, false, "everywhere"}, {"--regions", true, false, "everywhere"}};
	std::vector<std::string> pos;
	if (!host::parse_args(argc, argv, 3, opts, pos, 1) || pos.size() != 1) error("Invalid arguments.\n%s", USAGE_COVERAGE);
	const std::string path = expand_home(pos[0]), region = opts[0].value, bed_path = opts[1].value;
	if (region != "everywhere" && bed_path != "everywhere") error("Only one of --region or --regions can be provided.");     // :24-26
	const int mode = region != "everywhere" ? 1 : bed_path != "everywhere" ? 2 : 0;
	std::vector<CovBedLine> bed;
	if (mode == 2) bed = cov_read_bed(expand_home(bed_path));
	host::gpu_warmup();
	std::vector<uint64_t> hist((size_t)SK_COVERAGE_BINS, 0);
	auto unknown_region = [&] { fprintf(stderr, "Unknown region '%s': no position is counted.\n", region.c_str()); };
	// the targets against a reference list: false for a REGION that names nothing in it
	auto targets_for = [&](const CovRefs &refs, std::vector<int64_t> &t) {
		if (mode == 1) return cov_parse_region(region, refs, t);
		if (mode == 2) t = cov_bed_targets(bed, refs);
		return true;
	};
	if (device_path("sam coverage histogram", path, [&]() -> int64_t {
		    CovRefs refs;
		    std::vector<int64_t> t;
		    if (mode != 0) {
			    if (!cov_refs_of_file(path, refs)) return -1;
			    if (!targets_for(refs, t)) t.clear();                      // (an unknown region: no target, and the file is still read and checked)
		    }
		    int handled = 0;
		    int64_t counted = 0;
		    uint64_t n_pos = 0, n_drop = 0;
		    if (sk_bam_file_coverage(host::gpu(), path.c_str(), mode, t.data(), (int64_t)(t.size() / 3), hist.data(), &n_pos, &n_drop, &counted, &handled,
		                             nullptr) != SK_OK || !handled)
			    return -1;
		    if (mode == 1 && t.empty()) unknown_region();
		    cov_print(hist.data());
		    return counted;
	    }) >= 0)
		return 0;
	std::fill(hist.begin(), hist.end(), 0);
	BamStream bam(path, true);
	CovRefs refs;
	if (!cov_refs(bam.header_raw.data(), bam.header_raw.size(), refs)) error("Cannot open BAM file '%s'", path.c_str());
	std::vector<int64_t> t;
	const bool known = targets_for(refs, t);
	CovHost cov(refs);
	if (mode == 2) cov.set_intervals(t);
	BamCore c;
	BamStream::Var v;
	std::vector<uint8_t> body;
	while (bam.next_full(c, v, body)) cov.record(c, body.data() + v.l_read_name, v.n_cigar);
	bam.raise_deferred();
	if (mode == 0) { for (size_t r = 0; r < refs.len.size(); r++) if (cov.has[r]) cov.target(r, 0, refs.len[r]); }
	else if (mode == 1) { if (known) cov.target((size_t)t[0], t[1], t[2]); }
	else for (size_t r = 0; r < refs.len.size(); r++) if (cov.hit[r]) for (const auto &iv : cov.merged[r]) cov.target(r, iv.first, iv.second);
	cov.histogram(hist.data());
	if (mode == 1 && !known) unknown_region();
	cov_print(hist.data());
	return 0;
}

int main(int argc, char **argv)
{
	// blocks, per-sample strings and gzip jobs are hundreds of KiB each: above glibc's default mmap threshold every one of them was a
	// mapping of its own, faulted in page by page and given back when freed (2.3 s of system time in a demultiplex of 8 M reads).  From
	// the arenas they are recycled.  (SEQKIT_MALLOC_DEFAULT=1: glibc's defaults, for A/B)
	if (!getenv("SEQKIT_MALLOC_DEFAULT")) {
		mallopt(M_MMAP_THRESHOLD, 32 << 20);
		mallopt(M_TRIM_THRESHOLD, 1 << 30);
		mallopt(M_TOP_PAD, 64 << 20);
	}
	int rc = 0;
	auto is = [&](int i, const char *w) { return argc > i && strcmp(argv[i], w) == 0; };
	if (argc >= 2 && is(1, "count")) rc = count(argc, argv);
	else if (argc >= 2 && is(1, "fragments")) rc = fragments(argc, argv);
	else if (argc >= 2 && is(1, "statistics")) rc = statistics(argc, argv);
	else if (argc >= 3 && is(1, "fragment") && is(2, "lengths")) rc = fragment_lengths(argc, argv);
	else if (argc >= 3 && is(1, "to") && (is(2, "raw") || is(2, "fasta") || is(2, "fastq"))) rc = to_reads(argc, argv);
	else if (argc >= 4 && is(1, "to") && is(2, "interleaved") && (is(3, "raw") || is(3, "fasta") || is(3, "fastq"))) rc = to_reads(argc, argv);
	else if (argc >= 4 && is(1, "tags") && is(2, "from") && is(3, "qname")) rc = rewrite_cmd(argc, argv, SK_REWRITE_TAGS_FROM_QNAME, 4, USAGE_TAGS_FROM_QNAME, true);
	else if (argc >= 4 && is(1, "qname") && is(2, "from") && is(3, "tags")) rc = rewrite_cmd(argc, argv, SK_REWRITE_QNAME_FROM_TAGS, 4, USAGE_QNAME_FROM_TAGS, true);
	else if (argc >= 3 && is(1, "trim") && is(2, "qnames")) rc = rewrite_cmd(argc, argv, SK_REWRITE_TRIM_QNAMES, 3, USAGE_TRIM, false);
	else if (argc >= 2 && is(1, "minimize")) rc = minimize_cmd(argc, argv);
	else if (argc >= 3 && is(1, "mark") && is(2, "duplicates")) rc = mark_duplicates_cmd(argc, argv);
	else if (argc >= 2 && is(1, "subsample")) rc = subsample_cmd(argc, argv);
	else if (argc >= 3 && is(1, "recalculate") && is(2, "tlen")) rc = recalculate_tlen_cmd(argc, argv);
	else if (argc >= 2 && is(1, "merge")) rc = merge_cmd(argc, argv);
	else if (argc >= 3 && is(1, "coverage") && is(2, "histogram")) rc = coverage_histogram_cmd(argc, argv);
	else fprintf(stderr, "%s\n", USAGE_TOP);
	host::out().flush();
	// everything is written and closed: what is left is taking the process apart (static destructors, the HIP runtime's exit handlers,
	// gigabytes of heap) — 0.16 s of a demultiplex of 8 M reads.  That is left to the kernel, as on the error path (host::error);
	// SEQKIT_SLOW_EXIT=1 (and SEQKIT_PROF, whose last lines are printed by destructors) returns from main instead.
	if (!getenv("SEQKIT_SLOW_EXIT") && !getenv("SEQKIT_PROF")) { host::flush_for_exit(); fflush(stdout); fflush(stderr); _exit(rc); }
	return rc;
}
