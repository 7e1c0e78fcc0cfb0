// sam_tails.cpp — `sam discard tail artifacts` (src/sam_discard_tail_artifacts.rs with src/genome_reader.rs): a mapped read whose left
// or right tail differs from the reference genome in too many places is dropped; unmapped reads pass.  A regular file goes to the
// device whole (sk_bam_file_discard_tails: the genome's chromosomes raw in device memory, both walks per record, the kept records
// compacted, then the rewrite windows; the chromosome loads afterwards, for the INFO lines); stdin, SEQKIT_HOST_INFLATE=1, --debug and
// every file the device declines — any CIGAR operation outside M I D = X, an index outside the read or the chromosome, a refID
// without a chromosome, an invalid record — go through the reference's own loop below over sam_tails.h.
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <chrono>
#include <cmath>
#include <unordered_map>

#include "sam_host.h"
#include "sam_tails.h"

static const char *USAGE_TAILS =
	"\nUsage:\n  sam discard tail artifacts [options] <ref_genome.fa> <bam_file>\n  sam discard tail artifacts --test\n\nOptions:  \n"
	"  --tail-length=N    The tail length of the read that is examined [default: 20].\n"
	"                     The tail length specifies the number of bases that are \n"
	"                     examined from each end of the read. Indels encountered do\n"
	"                     not affect this number.\n"
	"  --threshold=FLOAT  Threshold ratio (0.0-1.0, inclusive) of variations that\n"
	"                     will cause the read to be discarded [default: 0.15].\n"
	"  --mismatches=N     Number of mismatches (inclusive) in a tail that will cause \n"
	"                     the read to be discarded.\n"
	"                     This number will be converted to a threshold ratio.\n"
	"  --debug            Print information and save discarded reads to a separate \n"
	"                     file.\n"
	"  --test             Run tests and exit.\n\nDescription:\n\n"
	"This script processes all the reads in a bam-file and removes reads that have \n"
	"a number of mismatching bases in the tails (ends) of the reads that is above \n"
	"the specified threshold ratio. Output (new bam file) is written to stdout.\n\n";

namespace {

// "{:.N}" of an f32: the value is exact in a double, and printf rounds the exact value as Rust does
std::string fmt_f32(float v, int digits)
{
	if (std::isnan(v)) return "NaN";
	if (std::isinf(v)) return v < 0 ? "-inf" : "inf";
	char b[64];
	snprintf(b, sizeof b, "%.*f", digits, (double)v);
	return b;
}

// str::parse::<f32>(), as sam_bamout.cpp's subsample reads it
bool parse_f32(const std::string &s, float &out)
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

// the genome as genome_reader.rs holds it: the index, and one chromosome's span of the FASTA file in memory at a time
struct Genome {
	std::string path;
	int fd = -1;
	uint64_t fsize = 0;
	std::vector<tails::FaiEntry> fai;
	std::unordered_map<std::string, size_t> by_name;                            // (the last line of a name counts)
	std::vector<uint8_t> bytes;
	tails::Chrom chr{nullptr, 0, 0, 1, 1};
	bool open(const std::string &p)                                             // IndexedReader::from_file: the FASTA and its .fai
	{
		path = p;
		fd = ::open(p.c_str(), O_RDONLY);
		if (fd < 0) return false;
		struct stat sb;
		if (fstat(fd, &sb) != 0 || !S_ISREG(sb.st_mode)) return false;
		fsize = (uint64_t)sb.st_size;
		const int fi = ::open((p + ".fai").c_str(), O_RDONLY);
		if (fi < 0) return false;
		std::string text;
		char buf[1 << 16];
		for (;;) {
			const ssize_t r = ::read(fi, buf, sizeof buf);
			if (r <= 0) break;
			text.append(buf, (size_t)r);
		}
		::close(fi);
		if (!tails::parse_fai(text.data(), text.size(), fai)) return false;
		for (size_t k = 0; k < fai.size(); k++) by_name[fai[k].name] = k;
		return true;
	}
	const tails::FaiEntry *find(const std::string &name) const
	{
		auto it = by_name.find(name);
		return it == by_name.end() ? nullptr : &fai[it->second];
	}
	void load(const std::string &name)                                         // load_chromosome_seq (src/genome_reader.rs:19-27)
	{
		const tails::FaiEntry *e = find(name);
		if (!e) error("Chromosome %s not found in %s.", name.c_str(), path.c_str());
		const uint64_t span = tails::span_bytes(e->length, e->line_bases, e->line_width);
		const uint64_t have = e->offset >= fsize ? 0 : std::min<uint64_t>(span, fsize - e->offset);
		bytes.resize((size_t)have);
		for (uint64_t done = 0; done < have;) {
			const ssize_t r = pread(fd, bytes.data() + done, (size_t)std::min<uint64_t>(have - done, (uint64_t)1 << 30), (off_t)(e->offset + done));
			if (r <= 0) { bytes.resize((size_t)done); break; }
			done += (uint64_t)r;
		}
		chr = tails::Chrom{bytes.data(), bytes.size(), e->length, e->line_bases, e->line_width};
		loaded_line(name, chr.loaded());
	}
	static void loaded_line(const std::string &name, uint64_t bp) { fprintf(stderr, "INFO: Loaded chromosome %s of length %llu bp\n", name.c_str(), (unsigned long long)bp); }
};

// a BAM file of its own, for --debug: the header, then what put() took, in members deflated here
struct BamFile {
	std::string path;
	int fd = -1;
	std::vector<uint8_t> buf;
	bool create(const std::string &p) { path = p; fd = ::open(p.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644); return fd >= 0; }
	void put(const uint8_t *p, size_t n) { buf.insert(buf.end(), p, p + n); if (buf.size() >= ((size_t)64 << 20)) flush(); }
	void raw(const uint8_t *p, size_t n)
	{
		while (n) {
			const ssize_t w = ::write(fd, p, n);
			if (w <= 0) error("Failed to write debug output");
			p += w; n -= (size_t)w;
		}
	}
	void flush()
	{
		std::vector<uint8_t> m(SK_DEFLATE_MAX_MEMBER);
		for (size_t at = 0; at < buf.size(); at += SK_DEFLATE_MAX_IN) {
			const uint32_t len = (uint32_t)std::min<size_t>(SK_DEFLATE_MAX_IN, buf.size() - at);
			z_stream z;
			memset(&z, 0, sizeof z);
			if (deflateInit2(&z, 6, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) error("zlib: deflateInit2 failed");
			z.next_in = buf.data() + at; z.avail_in = len;
			z.next_out = m.data() + 18; z.avail_out = SK_DEFLATE_MAX_MEMBER - 26;
			const int zr = deflate(&z, Z_FINISH);
			uint32_t clen = (uint32_t)z.total_out;
			deflateEnd(&z);
			if (zr != Z_STREAM_END) clen = (uint32_t)bamfmt::bgzf_stored(m.data() + 18, buf.data() + at, len);
			bamfmt::bgzf_head(m.data(), clen + 26);
			bamfmt::bgzf_trailer(m.data() + 18 + clen, (uint32_t)crc32(crc32(0L, Z_NULL, 0), buf.data() + at, len), len);
			raw(m.data(), clen + 26);
		}
		buf.clear();
	}
	void finish() { if (fd < 0) return; flush(); raw(bamfmt::kBgzfEof, sizeof bamfmt::kBgzfEof); ::close(fd); fd = -1; }
};

BamFile *g_debug_out = nullptr;
BamOut *g_tails_out = nullptr;
void finish_both() { if (g_debug_out) g_debug_out->finish(); if (g_tails_out) g_tails_out->finish(); }

// :229-239
void results(int32_t total, int32_t failed, int32_t passed, float thr, uint64_t seconds, bool debug, const std::string &debug_filename)
{
	const std::string pct = fmt_f32(thr * 100.0f, 1);
	fprintf(stderr, "\nDISCARD TAIL ARTIFACT RESULTS\n");
	fprintf(stderr, "Total number of reads processed: %d\n", total);
	fprintf(stderr, "Number of reads with %s%% or more tail artifacts: %d [FAILED]\n", pct.c_str(), failed);
	fprintf(stderr, "Number of reads with less than %s%% tail artifacts: %d [PASSED]\n", pct.c_str(), passed);
	fprintf(stderr, "\n");
	fprintf(stderr, "Percentage of processed records discarded %s%%\n", fmt_f32(((float)failed / (float)total) * 100.0f, 1).c_str());
	fprintf(stderr, "\n");
	fprintf(stderr, "Processing took %llu seconds.\n", (unsigned long long)seconds);
	if (debug) fprintf(stderr, "Reads with tail artifacts written to file: '%s'\n", debug_filename.c_str());
	fprintf(stderr, "ALL DONE.\n");
}

uint64_t seconds_since(std::chrono::steady_clock::time_point t0)
{
	return (uint64_t)std::chrono::duration_cast<std::chrono::seconds>(std::chrono::steady_clock::now() - t0).count();
}

// :442-563: the reference's cases through sam_tails.h, a line each in ansi_term's green or red, then its performance gate
int self_test()
{
	tails::TestRecord rec;
	std::vector<uint8_t> ref_seq;
	uint64_t offset = 0;
	int failed = 0;
	auto ftr = [&](int32_t expect, int32_t value) -> std::string {
		if (value == expect) return "\x1b[32mPASS\x1b[0m";
		failed++;
		return "\x1b[31mFAIL - " + std::to_string(value) + " vs. " + std::to_string(expect) + "\x1b[0m";
	};
	for (const tails::TestCase &t : tails::self_test_cases(&rec, &ref_seq, &offset)) fprintf(stderr, "[%s] %s\n", ftr(t.expect, t.got).c_str(), t.label);
	const tails::Chrom chr{ref_seq.data(), ref_seq.size(), ref_seq.size(), ref_seq.size(), ref_seq.size()};
	const auto t0 = std::chrono::steady_clock::now();
	int32_t dummy = 0;
	bool timeout = false;
	int stop = 0;
	for (int i = 0; i < 2000000; i++) {
		dummy += tails::count_mismatches(50, rec.cigar.data(), rec.n_cigar, rec.seq4.data(), rec.l_seq, 0, 0, chr, 1, &stop);
		dummy += tails::count_mismatches(50, rec.cigar.data(), rec.n_cigar, rec.seq4.data(), rec.l_seq, 49, offset, chr, -1, &stop);
		if (dummy >= 1000000) {
			dummy = 0;
			if (seconds_since(t0) >= 5) { timeout = true; break; }
		}
	}
	const uint64_t elapsed = seconds_since(t0);
	fprintf(stderr, "[%s] PERFORMANCE (%llu seconds)\n", ftr(1, elapsed < 5 && !timeout ? 1 : 0).c_str(), (unsigned long long)elapsed);
	if (failed == 0) fprintf(stderr, "INFO: All tests passed. [OK]\n");
	else fprintf(stderr, "ERROR: Number of failed tests: %d\n", failed);
	return -failed;
}

}  // namespace

int discard_tail_artifacts_cmd(int argc, char **argv)
{
	std::vector<host::Opt> opts = {{"--tail-length", true, false, "20"}, {"--threshold", true, false, "0.15"}, {"--mismatches", true, false, ""},
	                               {"--debug", false, false, ""}, {"--test", false, false, ""}};
	std::vector<std::string> pos;
	if (!host::parse_args(argc, argv, 4, opts, pos, 2) || !(pos.size() == 2 || (pos.empty() && opts[4].present))) error("Invalid arguments.\n%s", USAGE_TAILS);
	if (opts[4].present) return self_test() & 0xff;                                // :48
	const std::string genome_path = pos[0], bam_path = pos[1];                    // (get_str: no '~' expansion)
	const bool debug = opts[3].present;
	uint64_t tail_length = 0;
	if (!host::parse_uint(opts[0].value.c_str(), UINT64_MAX, tail_length)) error("--tail-length requires a positive integer argument.");       // :53
	float thr = 0.0f;
	if (!parse_f32(opts[1].value, thr)) error("--threshold requires a floating point number argument (default: 0.10).");                       // :54
	if (tail_length < 1) error("--tail-length requires a positive integer argument.");                                                          // :59-61
	if (!opts[2].value.empty()) {                                                 // :63-67
		uint64_t mm = 0;
		if (!host::parse_uint(opts[2].value.c_str(), UINT32_MAX, mm)) error("--mismatches requires a positive integer argument.");
		thr = (float)(uint32_t)mm / (float)tail_length;
		fprintf(stderr, "INFO: Mismatch threshold ratio set to %s\n", fmt_f32(thr, 2).c_str());
	}
	if (thr < 0.0f || thr > 1.0f) error("--threshold requires a floating point number between 0.0 and 1.0.");                                   // :69-71
	const uint64_t min_mm = tails::check_threshold(tail_length, thr);
	fprintf(stderr, "INFO: %llu mismatches in %llu read tail bases will cause read to be discarded.\n", (unsigned long long)min_mm, (unsigned long long)tail_length);
	const std::string co = "@CO\tProcessed with discard tail artifacts (ver 0.5) TAIL_LEN:" + std::to_string(tail_length) + " THRESHOLD:" + fmt_f32(thr, 1) + "\n";   // :82
	host::gpu_warmup();
	std::unique_ptr<BamStream> bam(new BamStream(bam_path, true));                // :77-79
	const std::vector<std::string> names = bam->names;
	Genome genome;
	const bool genome_ok = genome.open(genome_path);
	// ---- the device path: only where the reference reaches its first record, and never with --debug
	const tails::FaiEntry *first = genome_ok && !names.empty() ? genome.find(names[0]) : nullptr;
	{
		int64_t total = 0, failed = 0, passed = 0, loads = 0;
		std::chrono::steady_clock::time_point t0;
		const bool offer = first && !debug && tail_length <= UINT32_MAX;          // (else the gate sees "-": the host reader, and the trace says so)
		const int64_t n_dev = device_path("sam discard tail artifacts", offer ? bam_path : std::string("-"), [&] {
			bam.reset();                                                          // (its header is read; the device reads the file itself)
			std::vector<const char *> fn;
			std::vector<sk_genome_ref> fr;
			for (const tails::FaiEntry &e : genome.fai) { fn.push_back(e.name.c_str()); fr.push_back(sk_genome_ref{e.offset, e.length, e.line_bases, e.line_width}); }
			const uint32_t dev_min = std::isnan(thr) ? UINT32_MAX : (uint32_t)min_mm;   // (a NaN threshold fails no read, whatever its count)
			return bam_out_from_file([&](sk_ctx *ctx, uint64_t window, int64_t *n, uint64_t *raw, int *handled) {
				const int rc = sk_bam_file_discard_tails(ctx, bam_path.c_str(), genome_path.c_str(), fn.data(), fr.data(), (int32_t)fr.size(), (uint32_t)tail_length,
				                                         dev_min, reinterpret_cast<const uint8_t *>(co.data()), (uint32_t)co.size(), 1, window, n, &total, &failed,
				                                         &passed, &loads, raw, handled, nullptr);
				if (rc == SK_OK && *handled) {                                    // (what the reference prints before its first record)
					Genome::loaded_line(names[0], first->length);
					fprintf(stderr, "INFO: Running DISCARD TAIL ARTIFACTS...\n");
					t0 = std::chrono::steady_clock::now();
				}
				return rc;
			});
		});
		if (n_dev >= 0) {
			std::vector<int32_t> tids;
			for (int64_t at = 0; at < loads;) {
				const int64_t step = std::min<int64_t>(loads - at, 1 << 16);
				tids.resize((size_t)step);
				check(sk_bam_file_discard_tails_loads(host::gpu(), at, step, tids.data()), "sk_bam_file_discard_tails_loads");
				for (int32_t t : tids) Genome::loaded_line(names[(size_t)t], genome.find(names[(size_t)t])->length);
				at += step;
			}
			results((int32_t)total, (int32_t)failed, (int32_t)passed, thr, seconds_since(t0), false, "");
			return 0;
		}
		if (!bam) bam.reset(new BamStream(bam_path, true));
	}
	// ---- the reference's loop
	HostBamRewrite io(*bam, 1, reinterpret_cast<const uint8_t *>(co.data()), co.size());      // :81-83
	BamOut &out = io.out;
	std::string debug_filename = bam_path;                                         // :86 replace(".bam", ..): every occurrence
	for (size_t at = 0; (at = debug_filename.find(".bam", at)) != std::string::npos; at += 24) debug_filename.replace(at, 4, "_tail_discards_debug.bam");
	BamFile discarded_out;
	if (debug) {                                                                   // :88-95
		fprintf(stderr, "DEBUG: Writing discarded reads to file '%s'. (debug)\n", debug_filename.c_str());
		// (a path without ".bam" names the input itself, and "-" the standard output: neither is written over here)
		if (debug_filename == bam_path || !discarded_out.create(debug_filename)) error("Cannot create file '%s'", debug_filename.c_str());
		const std::vector<uint8_t> hdr = bamfmt::rewrite_header(bam->header_raw);
		discarded_out.put(hdr.data(), hdr.size());
		g_debug_out = &discarded_out; g_tails_out = &out;
		host::at_exit_flush(finish_both);
	}
	if (!genome_ok) error("Could not open genome FASTA file '%s'.", genome_path.c_str());      // :100, src/genome_reader.rs:15
	if (names.empty()) panic("index out of bounds: the len is 0 but the index is 0");          // :119 chr_names[0]
	size_t chr_index = 0;
	genome.load(names[0]);
	int32_t records_total = 0, records_passed = 0, records_failed = 0, report_progress = 0;
	fprintf(stderr, "INFO: Running DISCARD TAIL ARTIFACTS...\n");                  // :126
	const auto start_time = std::chrono::steady_clock::now();
	BamCore c;
	BamStream::Var v;
	std::vector<uint8_t> body, rec;
	while (bam->next_full(c, v, body)) {                                           // :130-226
		records_total = (int32_t)((uint32_t)records_total + 1u);
		if (c.flag & 0x4) {                                                        // :141-146
			out.put(bam->head, 36);
			out.put(body.data(), body.size());
			continue;
		}
		if (c.tid != (int32_t)(uint32_t)chr_index) {                               // :149-162
			chr_index = (size_t)(int64_t)c.tid;
			if (chr_index >= names.size()) error("Chromosome index error!");
			genome.load(names[chr_index]);
		}
		bool bad_op = false;                                                       // read.cigar(): an operation code above 8
		(void)cigar_end_pos(body.data() + v.l_read_name, v.n_cigar, 0, &bad_op);
		if (bad_op) panic("Unexpected cigar operation");
		rec.assign(bam->head, bam->head + 36);
		rec.insert(rec.end(), body.begin(), body.end());
		int32_t left = 0, right = 0;
		const int stop = tails::record_tails(rec.data(), tail_length, genome.chr, left, right);   // :170-193
		if (stop == tails::kReadIndex) panic("index out of bounds: the read's bases");
		if (stop == tails::kRefIndex) panic("index out of bounds: the chromosome's bases");
		if (stop) { const std::string what = std::string("Unexpected CIGAR type: ") + (char)stop; panic(what.c_str()); }      // :339-343
		const float left_ratio = (float)left / (float)tail_length, right_ratio = (float)right / (float)tail_length;            // :195-196
		if (left_ratio >= thr || right_ratio >= thr) {                             // :198-211
			records_failed++;
			if (debug) discarded_out.put(rec.data(), rec.size());
		} else {
			records_passed++;
			out.put(rec.data(), rec.size());
		}
		if (debug && ++report_progress >= 100000) {                                // :217-225
			report_progress = 0;
			fprintf(stderr, "Records processed: %d/%d (%s%%) [FAILED/TOTAL]\n", records_failed, records_total,
			        fmt_f32(((float)records_failed / (float)records_total) * 100.0f, 1).c_str());
		}
	}
	io.close();
	g_tails_out = nullptr;
	if (debug) { g_debug_out = nullptr; discarded_out.finish(); }
	results(records_total, records_failed, records_passed, thr, seconds_since(start_time), debug, debug_filename);
	return 0;
}
