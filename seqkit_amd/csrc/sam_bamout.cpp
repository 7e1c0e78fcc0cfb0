// sam_bamout.cpp — the `sam` commands that write BAM to stdout: trim qnames, tags from qname, qname from tags, minimize, mark duplicates,
// subsample, recalculate tlen, merge, concatenate.  They share one way through: device_path, bam_out_from_file and HostBamRewrite
// (sam_host.h); concatenate, whose inputs each choose their way, states its own at its end.
#include <sys/random.h>

#include <deque>
#include <unordered_map>

#include "sam_host.h"

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

int trim_qnames_cmd(int argc, char **argv) { return rewrite_cmd(argc, argv, SK_REWRITE_TRIM_QNAMES, 3, USAGE_TRIM, false); }
int tags_from_qname_cmd(int argc, char **argv) { return rewrite_cmd(argc, argv, SK_REWRITE_TAGS_FROM_QNAME, 4, USAGE_TAGS_FROM_QNAME, true); }
int qname_from_tags_cmd(int argc, char **argv) { return rewrite_cmd(argc, argv, SK_REWRITE_QNAME_FROM_TAGS, 4, USAGE_QNAME_FROM_TAGS, true); }

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

int minimize_cmd(int argc, char **argv)
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

int mark_duplicates_cmd(int argc, char **argv)
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

int subsample_cmd(int argc, char **argv)
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

int recalculate_tlen_cmd(int argc, char **argv)
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

int merge_cmd(int argc, char **argv)
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
	HostBamRewrite io(*in[0].bam, level);                                                           // (the header is the first input's)
	BamOut &out = io.out;
	for (MergeInput &m : in) m.advance();                                                        // :83-87
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
	io.close();
	return 0;
}

// ---- sam concatenate -----------------------------------------------------------------------------------------------------
// src/sam_concatenate.rs: the inputs one after the other in command-line order, ".1", ".2", .. behind every read name, under the FIRST
// input's header; the later inputs' headers are read and skipped, not compared.  The inputs are taken one at a time, and each chooses
// its own way: a regular file is offered to the device (sk_bam_file_concatenate, which serves ONE input of a longer output: the header
// only with input 1, the EOF block only with the last); "-", SEQKIT_HOST_INFLATE=1 and every input the device declines — an invalid
// record, a suffixed name above 254 bytes — are read record by record here, that input alone, and the next one is offered to the device
// again.  The order on stdout is this command's business: what the host writer holds is flushed before a device-served input's members
// are written.  From the first byte of output on, every way out through error() or panic() finishes the stream with the EOF block.
static const char *USAGE_CONCATENATE =
	"\nUsage:\n  sam concatenate [options] <bam_files>...\n\nOptions:\n"
	"  --uncompressed    Output in uncompressed BAM format\n\n"
	"Concatenates two or more BAM files together, ensuring that read\nidentifiers do not clash. Currently we simply add a '.1' suffix to all\n"
	"read identifiers found in the first BAM file, a '.2' suffix to all all\nread identifiers found in the second BAM file, and so forth.\n";

int concatenate_cmd(int argc, char **argv)
{
	std::vector<host::Opt> opts = {{"--uncompressed", false, false, ""}};
	std::vector<std::string> pos;
	if (!host::parse_args(argc, argv, 2, opts, pos, (size_t)-1) || pos.empty()) error("Invalid arguments.\n%s", USAGE_CONCATENATE);
	if (pos.size() < 2) error("At least two BAM files must be provided for concatenation.");      // :24-26
	const int level = opts[0].present ? 0 : 1;
	std::vector<std::string> paths;
	for (const std::string &p : pos) paths.push_back(expand_home(p));
	host::gpu_warmup();
	BamOut out(level);
	bool eof_written = false;
	BamCore c;
	BamStream::Var v;
	std::vector<uint8_t> body, rec;
	const std::vector<uint8_t> none;
	std::string name;
	for (size_t b = 0; b < paths.size(); b++) {
		const std::string &path = paths[b];
		const bool first = b == 0, last = b + 1 == paths.size();
		int64_t n_dev = -1;
		if (file_path_wanted(path)) {
			sk_ctx *ctx = host::gpu();
			int64_t n_rec = 0;
			uint64_t raw = 0;
			int handled = 0;
			const int flags = (first ? SK_CONCAT_HEADER : 0) | (last ? SK_CONCAT_EOF : 0);
			if (sk_bam_file_concatenate(ctx, path.c_str(), (uint32_t)(b + 1), flags, level, file_window_bytes(), &n_rec, &raw, &handled, nullptr) == SK_OK && handled) {
				out.flush();                                                    // (what a host-read input before this one left: a short last member is fine)
				finish_at_exit(&out);
				sk_bam_out_window w;
				for (;;) {
					check(sk_bam_file_rewrite_next(ctx, &w), "sk_bam_file_rewrite_next");
					if (w.n == 0 && w.bytes == 0) break;
					BamOut::write_all(w.bgzf, (size_t)w.bytes);
				}
				n_dev = n_rec;
				if (last) { eof_written = true; finish_at_exit(nullptr); }
			}
		}
		if (bamfile_trace()) {
			if (n_dev >= 0) fprintf(stderr, "sam concatenate: input %zu: device path, %lld records\n", b + 1, (long long)n_dev);
			else fprintf(stderr, "sam concatenate: input %zu: host reader\n", b + 1);
		}
		if (n_dev >= 0) continue;
		BamStream bam(path, first);                                             // :28, :37 (a file that cannot be opened ends the command here)
		if (first) {
			const std::vector<uint8_t> hdr = bamfmt::rewrite_header(bam.header_raw);
			out.put(hdr.data(), hdr.size());
			out.flush();                                                        // (the header goes in members of its own)
		}
		finish_at_exit(&out);
		const std::string suffix = "." + std::to_string(b + 1);                 // :41
		while (bam.next_full(c, v, body)) {                                     // :43-48
			name.assign(reinterpret_cast<const char *>(body.data()), v.l_read_name - 1);
			name += suffix;
			if (name.size() > 254) panic("assertion failed: new_qname.len() < 255");
			renamed_record(rec, bam.head, name, body.data() + v.l_read_name, body.size() - v.l_read_name, none);
			out.put(rec.data(), rec.size());
		}
		bam.raise_deferred();
	}
	if (!eof_written) out.finish();
	finish_at_exit(nullptr);
	return 0;
}
