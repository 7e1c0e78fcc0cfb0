// sam_tails.h — what `sam discard tail artifacts` (sam_tails.cpp) computes on the host, apart from the device, the BAM reader and the
// sinks, so that a stand-alone program can run it (tests/cpp/sam_tails_test.cpp): the `.fai` parser and the offset arithmetic of
// bio::io::fasta::IndexedReader as this build reads it (src/genome_reader.rs), and count_mismatches, count_right_end_offset and
// check_threshold of src/sam_discard_tail_artifacts.rs (:243-348, :386-398) over a record's bytes and a chromosome given as the bytes
// of its span in the FASTA file — newlines included, as the device holds it — with its line_bases and line_width.  The casts are the
// release build's: usize arithmetic wraps mod 2^64, `as i32` keeps the low 32 bits and `as usize` sign-extends them.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

namespace tails {

inline uint32_t le32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

// ---- the .fai --------------------------------------------------------------------------------------------------------
// one line: name TAB length TAB offset TAB line_bases TAB line_width, the four numbers plain decimal u64
struct FaiEntry { std::string name; uint64_t length, offset, line_bases, line_width; };

inline bool fai_u64(const char *p, size_t n, uint64_t &out)
{
	if (n == 0 || n > 20) return false;
	uint64_t v = 0;
	for (size_t k = 0; k < n; k++) {
		if (p[k] < '0' || p[k] > '9') return false;
		const uint64_t d = (uint64_t)(p[k] - '0');
		if (v > (UINT64_MAX - d) / 10) return false;
		v = v * 10 + d;
	}
	out = v;
	return true;
}

// false: not five columns, an empty name, a number that does not parse, a line that holds no base or is wider than its bytes allow
inline bool parse_fai_line(const char *line, size_t n, FaiEntry &e)
{
	if (n && line[n - 1] == '\r') n--;
	size_t col[6];
	int nc = 0;
	col[nc++] = 0;
	for (size_t k = 0; k < n; k++)
		if (line[k] == '\t') {
			if (nc == 5) return false;
			col[nc++] = k + 1;
		}
	if (nc != 5) return false;
	col[5] = n + 1;
	if (col[1] - col[0] < 2) return false;
	e.name.assign(line, col[1] - 1);
	uint64_t *dst[4] = {&e.length, &e.offset, &e.line_bases, &e.line_width};
	for (int c = 0; c < 4; c++)
		if (!fai_u64(line + col[c + 1], col[c + 2] - col[c + 1] - 1, *dst[c])) return false;
	return e.line_bases >= 1 && e.line_width >= e.line_bases;
}

// the whole index; false as parse_fai_line, at any line (an empty last line is no line)
inline bool parse_fai(const char *text, size_t n, std::vector<FaiEntry> &out)
{
	out.clear();
	for (size_t a = 0; a < n;) {
		const void *nl = memchr(text + a, '\n', n - a);
		const size_t b = nl ? (size_t)((const char *)nl - text) : n;
		if (b == a && b + 1 >= n) break;
		FaiEntry e;
		if (!parse_fai_line(text + a, b - a, e)) return false;
		out.push_back(e);
		a = b + 1;
	}
	return true;
}

// base p of a chromosome lies this many bytes behind the chromosome's first base
inline uint64_t base_byte(uint64_t p, uint64_t line_bases, uint64_t line_width) { return p / line_bases * line_width + p % line_bases; }
// the bytes from a chromosome's first base to its last
inline uint64_t span_bytes(uint64_t length, uint64_t line_bases, uint64_t line_width) { return length ? base_byte(length - 1, line_bases, line_width) + 1 : 0; }

// a chromosome in memory: the file's bytes from its first base on (n_bytes of them: the span, or what the file holds of it)
struct Chrom {
	const uint8_t *bytes;
	uint64_t n_bytes, length, line_bases, line_width;
	// the bases that lie inside the bytes: what `INFO: Loaded chromosome` prints
	uint64_t loaded() const
	{
		if (n_bytes >= span_bytes(length, line_bases, line_width)) return length;
		const uint64_t full = n_bytes / line_width, rest = n_bytes % line_width;
		return full * line_bases + (rest < line_bases ? rest : line_bases);
	}
};

// ---- the walk --------------------------------------------------------------------------------------------------------
// where a walk ends the command (status 101): an operation N S H P or B (its letter as :339-343 print it), an examined base whose
// read index lies outside [0, l_seq), one whose reference index lies outside the chromosome
enum Stop { kNoStop = 0, kReadIndex = 1, kRefIndex = 2, kOpN = 'N', kOpS = 'S', kOpH = 'H', kOpP = 'P', kOpB = '9' };

inline uint64_t sext32(uint32_t v) { return (uint64_t)(int64_t)(int32_t)v; }

// :243-255, over the record's CIGAR: the deletions' lengths less the insertions', in wrapping i32
inline int32_t count_right_end_offset(const uint8_t *cigar, uint32_t n_cigar)
{
	uint32_t offset = 0;
	for (uint32_t j = 0; j < n_cigar; j++) {
		const uint32_t op = le32(cigar + 4 * (size_t)j);
		if ((op & 15u) == 1u) offset -= op >> 4;
		else if ((op & 15u) == 2u) offset += op >> 4;
	}
	return (int32_t)offset;
}

// :257-348.  step +1: the operations in order; -1: in reverse.  seq4: the packed bases.  *stop is set where the walk ends the command.
inline int32_t count_mismatches(uint64_t tail_length, const uint8_t *cigar, uint32_t n_cigar, const uint8_t *seq4, uint64_t l_seq, uint64_t seq_index,
                                uint64_t ref_offset, const Chrom &chr, int32_t step, int *stop)
{
	uint64_t n_bases_examined = 0;
	uint32_t tail_mismatches = 0;
	for (uint32_t j = 0; j < n_cigar; j++) {
		if (n_bases_examined >= tail_length) break;                                  // :270
		const uint32_t op = le32(cigar + 4 * (size_t)(step > 0 ? j : n_cigar - 1 - j)), code = op & 15u, len = op >> 4;
		const uint32_t ls = len * (uint32_t)step;                                   // l * step, in wrapping i32
		if (code == 0u || code == 7u || code == 8u) {                               // :273-311
			for (uint32_t k = 0; k < len; k++) {
				n_bases_examined++;
				if (seq_index >= l_seq) { *stop = kReadIndex; return (int32_t)tail_mismatches; }
				const uint32_t c4 = (seq4[seq_index >> 1] >> ((seq_index & 1) ? 0 : 4)) & 15u;
				const char read_acgt = c4 == 1 ? 'A' : c4 == 2 ? 'C' : c4 == 4 ? 'G' : c4 == 8 ? 'T' : 'N';
				const uint64_t ri = ref_offset + seq_index;                           // (usize: wraps)
				const uint64_t at = ri < chr.length ? base_byte(ri, chr.line_bases, chr.line_width) : UINT64_MAX;
				if (at >= chr.n_bytes) { *stop = kRefIndex; return (int32_t)tail_mismatches; }
				char ref_acgt = (char)chr.bytes[at];
				if (ref_acgt >= 'a' && ref_acgt <= 'z') ref_acgt = (char)(ref_acgt - 32);
				if (!(read_acgt == ref_acgt || ref_acgt == 'N' || read_acgt == 'N')) tail_mismatches++;
				seq_index = sext32((uint32_t)seq_index + (uint32_t)step);             // :300
				if (n_bases_examined >= tail_length) return (int32_t)tail_mismatches;   // :309
			}
		} else if (code == 1u) {                                                    // :312-324
			tail_mismatches++;
			seq_index = sext32((uint32_t)seq_index + ls);
			ref_offset = sext32((uint32_t)ref_offset - ls);
		} else if (code == 2u) {                                                    // :325-338
			tail_mismatches++;
			ref_offset = sext32((uint32_t)ref_offset + ls);
		} else {
			*stop = code == 3u ? kOpN : code == 4u ? kOpS : code == 5u ? kOpH : code == 6u ? kOpP : kOpB;
			return (int32_t)tail_mismatches;
		}
	}
	return (int32_t)tail_mismatches;
}

// :386-398, f32 throughout
inline uint64_t check_threshold(uint64_t tail_length, float threshold_ratio)
{
	uint64_t n_mismatches = 0;
	while (n_mismatches <= tail_length) {
		const float cur_ratio = (float)n_mismatches / (float)tail_length;
		if (cur_ratio >= threshold_ratio) break;
		n_mismatches++;
	}
	return n_mismatches;
}

// A mapped record's two walks (:170-196): r points at block_size.  left / right: the tails' counts; the stop of the first walk that has
// one (the right walk does not run behind a left walk that stopped).
inline int record_tails(const uint8_t *r, uint64_t tail_length, const Chrom &chr, int32_t &left, int32_t &right)
{
	const uint32_t l_read_name = r[12], n_cigar = le32(r + 16) & 0xffffu, l_seq = le32(r + 20);
	const uint8_t *cigar = r + 36 + l_read_name, *seq4 = cigar + 4 * (size_t)n_cigar;
	int stop = kNoStop;
	left = right = 0;
	uint64_t ref_offset = sext32(le32(r + 8));                                       // read.pos() as usize
	left = count_mismatches(tail_length, cigar, n_cigar, seq4, l_seq, 0, ref_offset, chr, 1, &stop);
	if (stop) return stop;
	ref_offset = sext32((uint32_t)ref_offset + (uint32_t)count_right_end_offset(cigar, n_cigar));
	right = count_mismatches(tail_length, cigar, n_cigar, seq4, l_seq, (uint64_t)l_seq - 1, ref_offset, chr, -1, &stop);
	return stop;
}

// ---- the reference's self-test (:446-531) ---------------------------------------------------------------------------------
struct TestCase { const char *label; int32_t got, expect; };

// a record's CIGAR and packed bases in heap buffers of their exact sizes
struct TestRecord {
	std::vector<uint8_t> cigar, seq4;
	uint32_t n_cigar = 0;
	uint64_t l_seq = 0;
	void set(const std::vector<std::pair<char, uint32_t>> &ops, const std::vector<uint8_t> &seq)
	{
		std::vector<uint8_t> c, s((seq.size() + 1) / 2, 0);
		for (const auto &o : ops) {
			const uint32_t code = o.first == 'M' ? 0u : o.first == 'I' ? 1u : 2u, v = (o.second << 4) | code;
			for (int k = 0; k < 4; k++) c.push_back((uint8_t)(v >> (8 * k)));
		}
		for (size_t i = 0; i < seq.size(); i++) {
			const uint8_t b = seq[i], code = b == 'A' ? 1 : b == 'C' ? 2 : b == 'G' ? 4 : b == 'T' ? 8 : 15;
			s[i >> 1] |= (uint8_t)(i & 1 ? code : code << 4);
		}
		cigar = std::vector<uint8_t>(c.begin(), c.end());
		seq4 = std::vector<uint8_t>(s.begin(), s.end());
		n_cigar = (uint32_t)ops.size(); l_seq = seq.size();
	}
};

// the 31 expectations in the reference's order; the chromosome is one line of exactly its bases
inline std::vector<TestCase> self_test_cases(TestRecord *last_rec = nullptr, std::vector<uint8_t> *last_ref = nullptr, uint64_t *last_offset = nullptr)
{
	std::vector<TestCase> out;
	std::vector<uint8_t> seq_arr(50, 'A'), ref_seq(50, 'A');
	TestRecord rec;
	rec.set({{'M', 50}}, seq_arr);
	auto run = [&](uint64_t T, uint64_t seq_index, uint64_t ref_offset, int32_t step) {
		const std::vector<uint8_t> exact(ref_seq.begin(), ref_seq.end());
		const Chrom chr{exact.data(), exact.size(), exact.size(), exact.size() ? exact.size() : 1, exact.size() ? exact.size() : 1};
		int stop = kNoStop;
		const int32_t v = count_mismatches(T, rec.cigar.data(), rec.n_cigar, rec.seq4.data(), rec.l_seq, seq_index, ref_offset, chr, step, &stop);
		return stop ? -1000 - stop : v;
	};
	auto both = [&](const char *l, const char *r, uint64_t T, int32_t expect) {
		out.push_back({l, run(T, 0, 0, 1), expect});
		out.push_back({r, run(T, 49, 0, -1), expect});
	};
	both("IDENTICAL LEFT: ", "IDENTICAL RIGHT", 20, 0);
	both("LONG TAIL LEFT", "LONG TAIL RIGHT", 100, 0);
	ref_seq[0] = 'N';
	out.push_back({"REF N", run(1, 0, 0, 1), 0});
	seq_arr[1] = 'N'; rec.set({{'M', 50}}, seq_arr);
	out.push_back({"SEQ N", run(1, 0, 0, 1), 0});
	seq_arr[1] = 'A'; rec.set({{'M', 50}}, seq_arr);
	ref_seq[0] = 'a'; ref_seq[49] = 'a';
	both("LOWER CASE LEFT", "LOWER CASE RIGHT", 20, 0);
	ref_seq[0] = 'C'; ref_seq[49] = 'C';
	both("MISMATCH LEFT", "MISMATCH RIGHT", 20, 1);
	ref_seq[19] = 'G'; ref_seq[30] = 'T';
	both("2 MISMATCH LEFT", "2 MISMATCH RIGHT", 20, 2);
	ref_seq[20] = 'G'; ref_seq[29] = 'T';
	both("NON-TAIL MISMATCH LEFT", "NON-TAIL MISMATCH RIGHT", 20, 2);
	ref_seq.assign(50, 'F');
	both("NONSENSE LEFT", "NONSENSE RIGHT", 20, 20);
	both("OVERLAP LEFT", "OVERLAP RIGHT", 50, 50);
	ref_seq.assign(60, 'A');
	for (int i = 20; i < 40; i++) ref_seq[(size_t)i] = 'C';
	uint64_t offset = sext32((uint32_t)count_right_end_offset(rec.cigar.data(), rec.n_cigar));
	out.push_back({"REF OFFSET MATCH", (int32_t)offset, 0});
	rec.set({{'M', 20}, {'D', 10}, {'M', 20}}, seq_arr);
	offset = sext32((uint32_t)count_right_end_offset(rec.cigar.data(), rec.n_cigar));
	out.push_back({"REF OFFSET DEL", (int32_t)offset, 10});
	out.push_back({"DELETION LEFT", run(20, 0, 0, 1), 0});
	out.push_back({"DELETION LEFT (2)", run(21, 0, 0, 1), 2});
	out.push_back({"INDEL RIGHT", run(40, 49, offset, -1), 11});
	rec.set({{'M', 20}, {'I', 10}, {'M', 20}}, seq_arr);
	offset = sext32((uint32_t)count_right_end_offset(rec.cigar.data(), rec.n_cigar));
	out.push_back({"REF OFFSET INS", (int32_t)offset, -10});
	out.push_back({"INSERTION LEFT", run(21, 0, 0, 1), 2});
	out.push_back({"INSERTION RIGHT", run(50, 49, offset, -1), 21});
	rec.set({{'M', 20}, {'I', 5}, {'D', 5}, {'M', 20}}, seq_arr);
	offset = sext32((uint32_t)count_right_end_offset(rec.cigar.data(), rec.n_cigar));
	out.push_back({"REF OFFSET INS-DEL", (int32_t)offset, 0});
	out.push_back({"INS-DEL LEFT", run(23, 0, 0, 1), 5});
	out.push_back({"INS-DEL RIGHT", run(50, 49, offset, -1), 17});
	if (last_rec) *last_rec = rec;
	if (last_ref) *last_ref = ref_seq;
	if (last_offset) *last_offset = offset;
	return out;
}

}  // namespace tails
