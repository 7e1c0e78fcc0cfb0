// sam_columns.cpp — the `sam` commands that reduce the records' core columns: statistics, fragment lengths, fragments, count.
// A regular file is first offered to the device whole (sk_bam_file_reduce, sk_bam_file_columns); what is irregular falls back, before
// anything has been written, to the reader here, which hands the core columns to the device as SoA batches.  The one order-dependent
// piece stays here, as SURVEY.md §8(e) lists it: the --reads=N early stop.
#include "sam_host.h"

static const char *USAGE_STATS =
	"\nUsage:\n  sam statistics [options] <bam_file>\n\nOptions:\n  --on-target=BED   Count on-target% for regions in BED file [optional]\n";
static const char *USAGE_FRAG =
	"\nUsage:\n  sam fragment lengths [options] <bam_file>\n\nOptions:\n"
	"  --max-frag-size=F     Maximum fragment size [default: 5000]\n"
	"  --reads=N             Finish after analyzing this many reads [default: Inf]\n";

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

int statistics_cmd(int argc, char **argv)
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

int fragment_lengths_cmd(int argc, char **argv)
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

int fragments_cmd(int argc, char **argv)                     // src/sam_fragments.rs:14-43
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

int count_cmd(int argc, char **argv)                         // src/sam_count.rs:20-130
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
		while (col.flag.size() < kBatchRecords && !stop && (more = bam.next_chunk(chunk, single_end))) {
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
