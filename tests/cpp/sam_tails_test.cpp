// sam_tails_test.cpp — seqkit_amd/csrc/sam_tails.h in a stand-alone program, for a build under the address and undefined-behaviour
// sanitizers (tests/test_sam_tails_cpu.py): the .fai parser on well-formed and malformed lines, the offset arithmetic at line ends, the
// reference's self-test table, and walks that stop at the edges of a record and of a chromosome — every buffer on the heap, of exactly
// the size its contents take.
#include <stdio.h>
#include <stdlib.h>

#include <memory>
#include <string>
#include <vector>

#include "sam_tails.h"

static int failures = 0;
#define CHECK(cond)                                                                                                      \
	do {                                                                                                                 \
		if (!(cond)) { failures++; fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); }                          \
	} while (0)

// the bytes of s in a heap block of exactly that size
static std::unique_ptr<char[]> exact(const std::string &s)
{
	std::unique_ptr<char[]> p(new char[s.size() ? s.size() : 1]);
	memcpy(p.get(), s.data(), s.size());
	return p;
}

static bool line_ok(const std::string &s, tails::FaiEntry &e)
{
	const auto p = exact(s);
	return tails::parse_fai_line(p.get(), s.size(), e);
}

static void fai_lines()
{
	tails::FaiEntry e;
	CHECK(line_ok("chr1\t5000\t6\t60\t61", e) && e.name == "chr1" && e.length == 5000 && e.offset == 6 && e.line_bases == 60 && e.line_width == 61);
	CHECK(line_ok("c\t0\t0\t1\t1\r", e) && e.name == "c" && e.length == 0);
	CHECK(line_ok("x y\t18446744073709551615\t18446744073709551615\t7\t9", e) && e.length == UINT64_MAX && e.name == "x y");
	for (const char *bad : {"", "chr1", "chr1\t5000\t6\t60", "chr1\t5000\t6\t60\t61\t1", "\t5000\t6\t60\t61", "chr1\t\t6\t60\t61", "chr1\t-5\t6\t60\t61",
	                        "chr1\t5000\t6\t0\t61", "chr1\t5000\t6\t62\t61", "chr1\t18446744073709551616\t6\t60\t61", "chr1\t5000\t6\t60\t6 1",
	                        "chr1\t5000\t6\t60\t", "chr1 5000 6 60 61", "chr1\t123456789012345678901\t6\t60\t61"})
		CHECK(!line_ok(bad, e));
	std::vector<tails::FaiEntry> all;
	const std::string two = "a\t10\t3\t4\t5\nb\t7\t20\t7\t9\r\n";
	CHECK(tails::parse_fai(exact(two).get(), two.size(), all) && all.size() == 2 && all[1].name == "b" && all[1].line_width == 9);
	const std::string no_end = "a\t10\t3\t4\t5";
	CHECK(tails::parse_fai(exact(no_end).get(), no_end.size(), all) && all.size() == 1);
	CHECK(tails::parse_fai(exact("").get(), 0, all) && all.empty());
	const std::string gap = "a\t10\t3\t4\t5\n\nb\t7\t20\t7\t9\n";
	CHECK(!tails::parse_fai(exact(gap).get(), gap.size(), all));
}

static void offsets()
{
	// lines of 4 bases and a newline: base 3 ends line 0, base 4 begins line 1
	CHECK(tails::base_byte(0, 4, 5) == 0 && tails::base_byte(3, 4, 5) == 3 && tails::base_byte(4, 4, 5) == 5 && tails::base_byte(7, 4, 5) == 8 && tails::base_byte(8, 4, 5) == 10);
	CHECK(tails::base_byte(6, 7, 9) == 6 && tails::base_byte(7, 7, 9) == 9);                      // CRLF
	CHECK(tails::base_byte(60, 61, 61) == 60);                                                    // one line, no end
	CHECK(tails::span_bytes(0, 4, 5) == 0 && tails::span_bytes(1, 4, 5) == 1 && tails::span_bytes(4, 4, 5) == 4 && tails::span_bytes(5, 4, 5) == 6 && tails::span_bytes(10, 4, 5) == 12);
	CHECK(tails::base_byte((uint64_t)3 << 32, 60, 61) == ((uint64_t)3 << 32) / 60 * 61 + ((uint64_t)3 << 32) % 60);   // beyond 32 bits
	// a chromosome of 10 bases in lines of 4, held in exactly its span; then cut short inside line 1 and inside a line's end
	const std::string text = "ACGT\nacgt\nNN";
	const auto p = exact(text);
	const tails::Chrom full{(const uint8_t *)p.get(), 12, 10, 4, 5}, cut{(const uint8_t *)p.get(), 7, 10, 4, 5}, at_end{(const uint8_t *)p.get(), 5, 10, 4, 5};
	CHECK(full.loaded() == 10 && cut.loaded() == 6 && at_end.loaded() == 4);
	// a read of 10 As over it: A=A, C G T differ, a matches, c g t differ, N N match
	tails::TestRecord r;
	r.set({{'M', 10}}, std::vector<uint8_t>(10, 'A'));
	int stop = 0;
	CHECK(tails::count_mismatches(10, r.cigar.data(), 1, r.seq4.data(), 10, 0, 0, full, 1, &stop) == 6 && stop == 0);
	CHECK(tails::count_mismatches(10, r.cigar.data(), 1, r.seq4.data(), 10, 9, 0, full, -1, &stop) == 6 && stop == 0);
	CHECK(tails::count_mismatches(3, r.cigar.data(), 1, r.seq4.data(), 10, 9, 0, full, -1, &stop) == 1 && stop == 0);
	CHECK(tails::count_mismatches(10, r.cigar.data(), 1, r.seq4.data(), 10, 0, 0, cut, 1, &stop) == 4 && stop == tails::kRefIndex);   // bases 0 .. 5, then the end
	stop = 0;
	CHECK(tails::count_mismatches(10, r.cigar.data(), 1, r.seq4.data(), 10, 0, 1, full, 1, &stop) == 6 && stop == tails::kRefIndex);  // base 10 of 10
	stop = 0;
	CHECK(tails::count_mismatches(10, r.cigar.data(), 1, r.seq4.data(), 9, 0, 0, full, 1, &stop) == 6 && stop == tails::kReadIndex);  // l_seq 9 under M10
	stop = 0;
	CHECK(tails::count_mismatches(10, r.cigar.data(), 1, r.seq4.data(), 10, 2, 0, full, -1, &stop) == 2 && stop == tails::kReadIndex); // walks below base 0
	stop = 0;
	CHECK(tails::count_mismatches(4, r.cigar.data(), 1, r.seq4.data(), 10, 0, tails::sext32((uint32_t)-1), full, 1, &stop) == 0 && stop == tails::kRefIndex);   // pos -1
}

static void self_test()
{
	const std::vector<tails::TestCase> cases = tails::self_test_cases();
	CHECK(cases.size() == 29);
	for (const tails::TestCase &t : cases) {
		if (t.got != t.expect) { failures++; fprintf(stderr, "%s: %d vs. %d\n", t.label, t.got, t.expect); }
	}
	CHECK(tails::check_threshold(20, 0.15f) == 3 && tails::check_threshold(20, 0.0f) == 0 && tails::check_threshold(20, 1.0f) == 20);
	CHECK(tails::check_threshold(33, 0.15f) == 5 && tails::check_threshold(20, 3.0f / 20.0f) == 3 && tails::check_threshold(1, 1.0f) == 1);
}

static void records()
{
	// a whole record in a block of exactly its bytes: M3 I2 M3 D4 over "ACGTACGTACGT", pos 1; the clipped one stops at its S
	auto make = [](const std::vector<std::pair<uint32_t, uint32_t>> &ops, const std::string &bases, int32_t pos) {
		std::vector<uint8_t> v(36 + 2 + 4 * ops.size() + (bases.size() + 1) / 2 + bases.size(), 0);
		const uint32_t bs = (uint32_t)v.size() - 4, nc = (uint32_t)ops.size(), ls = (uint32_t)bases.size();
		for (int k = 0; k < 4; k++) { v[(size_t)k] = (uint8_t)(bs >> (8 * k)); v[8 + (size_t)k] = (uint8_t)((uint32_t)pos >> (8 * k)); v[20 + (size_t)k] = (uint8_t)(ls >> (8 * k)); }
		v[12] = 2; v[16] = (uint8_t)nc; v[17] = (uint8_t)(nc >> 8); v[36] = 'q';
		for (size_t j = 0; j < ops.size(); j++) { const uint32_t w = (ops[j].second << 4) | ops[j].first; for (int k = 0; k < 4; k++) v[38 + 4 * j + (size_t)k] = (uint8_t)(w >> (8 * k)); }
		for (size_t i = 0; i < bases.size(); i++) {
			const uint8_t c = bases[i] == 'A' ? 1 : bases[i] == 'C' ? 2 : bases[i] == 'G' ? 4 : bases[i] == 'T' ? 8 : 15;
			v[38 + 4 * ops.size() + i / 2] |= (uint8_t)(i & 1 ? c : c << 4);
		}
		return std::vector<uint8_t>(v.begin(), v.end());
	};
	const std::string g = "ACGTACGTACGT";
	const auto gp = exact(g);
	const tails::Chrom chr{(const uint8_t *)gp.get(), 12, 12, 12, 12};
	int32_t left = -1, right = -1;
	const std::vector<uint8_t> a = make({{0, 3}, {1, 2}, {0, 3}, {2, 4}}, "CGTTTACG", 1);       // CGT | TT | ACG, then 4 deleted
	CHECK(tails::record_tails(a.data(), 20, chr, left, right) == 0 && left == 2 && right == 2);
	CHECK(tails::record_tails(a.data(), 3, chr, left, right) == 0 && left == 0 && right == 1);   // the right walk meets the D first
	const std::vector<uint8_t> s = make({{4, 2}, {0, 4}}, "TTACGT", 4);
	CHECK(tails::record_tails(s.data(), 20, chr, left, right) == tails::kOpS);
	const std::vector<uint8_t> n = make({{0, 2}, {3, 5}, {0, 2}}, "ACGT", 0);
	CHECK(tails::record_tails(n.data(), 2, chr, left, right) == 0);                              // neither walk reaches the N
	CHECK(tails::record_tails(n.data(), 3, chr, left, right) == tails::kOpN);
	const std::vector<uint8_t> e = make({}, "", 0);                                              // no CIGAR, no bases: nothing examined
	CHECK(tails::record_tails(e.data(), 20, chr, left, right) == 0 && left == 0 && right == 0);
	const std::vector<uint8_t> far = make({{2, 5}, {0, 2}}, "AC", 2147483647);                   // pos + 5 leaves the i32 range and wraps
	CHECK(tails::record_tails(far.data(), 2, chr, left, right) == tails::kRefIndex);
}

int main()
{
	fai_lines();
	offsets();
	self_test();
	records();
	if (failures) { printf("FAILED: %d checks\n", failures); return 1; }
	printf("ok: sam_tails.h\n");
	return 0;
}
