// sam_coverage.cpp — `sam coverage histogram`: through the same gate as the other file commands with sk_bam_file_coverage, 10 001 lines
// out; its host reader states the rule in one sort and one sweep.
#include <zlib.h>

#include "sam_host.h"

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

int coverage_histogram_cmd(int argc, char **argv)
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
