// passmem_test.cpp — sk_passmem.h (the record passes' working memory) and bamfmt::RefList (sk_bamfmt.h: the BAM header's reference list)
// on the host, built with the address and undefined-behaviour sanitizers (tests/test_passmem_cpu.py).  The five file calls' region
// lists are restated here as sk_bamfile_out.cpp and sk_bamfile_coverage.cpp give them; the expected totals are the sums those calls
// computed by hand before the arena existed.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <functional>
#include <string>
#include <vector>

#include "sk_bamfmt.h"
#include "sk_passmem.h"

using passmem::Layout;
using passmem::Placement;
using passmem::SortBufs;
using passmem::up;

static int g_checks = 0;
#define CHECK(cond)                                                                                                     \
	do {                                                                                                                \
		g_checks++;                                                                                                     \
		if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); exit(1); }               \
	} while (0)

// ---- the arena -------------------------------------------------------------------------------------------------------------------
// one call's layout: its regions (pointer and the bytes the call states for it), the total the parent's code computed, the kept bytes
struct Call {
	const char *name;
	Layout L;
	SortBufs sb;
	uint64_t *c64 = nullptr;                     // krec (subsample), addr (merge)
	uint32_t *c32[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};   // agg; markdup's five signature columns; merge's len
	uint8_t *c8 = nullptr;                       // merge's in
	std::vector<std::pair<std::function<uint8_t *()>, uint64_t>> regions;   // (where carve() put each region, and the bytes stated for it)
	uint64_t expect_total = 0, kept = 0;
	template <class T> void add(T *&p, uint64_t bytes) { L.add(p, bytes); regions.push_back({[&p] { return (uint8_t *)p; }, bytes}); }
	template <class T> void add(T *(&p)[2], uint64_t bytes) { add(p[0], bytes); add(p[1], bytes); }
};

static void build(Call &c, int which, uint64_t N, uint64_t temp)
{
	c.sb.temp_bytes = temp;
	switch (which) {
	case 0:
		c.name = "minimize";
		c.add(c.sb.key, N * 8); c.add(c.sb.idx, N * 4); c.add(c.c32[0], (N / 1024 + 2) * 4); c.add(c.sb.temp, c.sb.temp_bytes);
		c.expect_total = 2 * up(N * 8) + 2 * up(N * 4) + up((N / 1024 + 2) * 4) + up(temp);
		c.kept = c.expect_total;
		break;
	case 1:
		c.name = "markdup";
		c.add(c.sb.key, N * 8 + 8); c.add(c.sb.idx, N * 4 + 4);
		for (int k = 0; k < 5; k++) c.add(c.c32[k], N * 4 + 4);
		c.add(c.sb.temp, c.sb.temp_bytes);
		c.expect_total = 2 * up(N * 8 + 8) + 7 * up(N * 4 + 4) + up(temp);
		c.kept = N * 2 + 2;
		break;
	case 2:
		c.name = "subsample";
		c.add(c.sb.key, N * 8); c.add(c.c64, N * 8); c.add(c.sb.idx, N * 4); c.add(c.c32[0], (N / 1024 + 2) * 4); c.add(c.sb.temp, c.sb.temp_bytes);
		c.expect_total = 3 * up(N * 8) + 2 * up(N * 4) + up((N / 1024 + 2) * 4) + up(temp);
		break;
	case 3:
		c.name = "merge";
		c.add(c.sb.key, N * 8); c.add(c.c64, N * 8); c.add(c.sb.idx, N * 4); c.add(c.c32[0], N * 4); c.add(c.c8, N); c.add(c.sb.temp, c.sb.temp_bytes);
		c.expect_total = 3 * up(N * 8) + 3 * up(N * 4) + up(N) + up(temp);
		c.kept = N;
		break;
	default:
		c.name = "coverage";
		c.add(c.sb.key, N * 8 + 8); c.add(c.sb.idx, N * 4 + 4); c.add(c.sb.temp, c.sb.temp_bytes);
		c.expect_total = 2 * up(N * 8 + 8) + 2 * up(N * 4 + 4) + up(temp);
		break;
	}
}

static void test_layouts()
{
	const uint64_t Ns[] = {0, 1, 63, 64, 65, 1024, 1025, 0xffffffffull};
	const uint64_t temps[] = {0, 1, 255, 256, 257, 4097, 1234567};
	for (int which = 0; which < 5; which++)
		for (uint64_t N : Ns)
			for (uint64_t temp : temps) {
				Call c;
				build(c, which, N, temp);
				CHECK(c.L.total() == c.expect_total);
				CHECK(c.L.total() % 256 == 0);
				const bool small = N <= 1025;
				// (the large N: carved at an address that is never touched, only compared)
				uint8_t *base = small ? (uint8_t *)malloc(c.L.total() ? c.L.total() : 1) : (uint8_t *)(uintptr_t)0x1000000;
				CHECK(base != nullptr);
				c.L.carve(base);
				uint64_t at = 0;
				for (auto &r : c.regions) {                                   // in order, back to back on multiples of 256: disjoint, and inside the total
					const uint8_t *p = r.first();
					CHECK(p == base + at);
					CHECK((uint64_t)(p - base) % 256 == 0);
					CHECK(at + r.second <= c.L.total());
					at += up(r.second);
				}
				CHECK(at == c.L.total());
				if (small) {
					for (size_t k = 0; k < c.regions.size(); k++) memset(c.regions[k].first(), 0x40 + (int)k, c.regions[k].second);   // (ASan: no region overruns the buffer)
					for (size_t k = 0; k < c.regions.size(); k++)
						if (c.regions[k].second) CHECK(*c.regions[k].first() == 0x40 + (int)k);   // (nor the region before it)
					free(base);
				}
			}
}

static void test_placement()
{
	for (int which = 0; which < 5; which++)
		for (uint64_t N : {(uint64_t)0, (uint64_t)1, (uint64_t)65, (uint64_t)1025}) {
			Call c;
			build(c, which, N, 777);
			const size_t scratch = which == 0 ? 0 : c.L.total();
			uint8_t *borrow = (uint8_t *)(uintptr_t)0x7000000;
			// one byte too small: its own buffer, the scratch behind the kept head
			if (scratch) {
				const Placement p = passmem::place(c.kept, scratch, scratch - 1, false);
				CHECK(!p.borrowed && p.own_bytes() == up(c.kept) + scratch);
				std::vector<uint8_t> own(p.own_bytes());
				CHECK(p.scratch_at(own.data(), borrow) == own.data() + up(c.kept));
				c.L.carve(p.scratch_at(own.data(), borrow));
				memset(own.data(), 1, c.kept);                                // the kept head: at the slot's start
				for (auto &r : c.regions) memset(r.first(), 2, r.second);
				for (uint64_t k = 0; k < c.kept; k++) CHECK(own[k] == 1);
			}
			// exactly large enough: borrowed, and the own buffer is the kept head alone (none where nothing is kept)
			{
				const Placement p = passmem::place(c.kept, scratch, scratch, false);
				CHECK(p.borrowed && p.own_bytes() == up(c.kept));
				std::vector<uint8_t> own(p.own_bytes() + 1);
				CHECK(p.scratch_at(own.data(), borrow) == borrow);
			}
			// never borrow: its own buffer however large the other is
			{
				const Placement p = passmem::place(c.kept, scratch, ~(uint64_t)0, true);
				CHECK(!p.borrowed && p.own_bytes() == up(c.kept) + scratch);
				uint8_t *own = (uint8_t *)(uintptr_t)0x3000000;
				CHECK(p.scratch_at(own, borrow) == own + up(c.kept));
			}
		}
	// minimize: everything is kept, nothing is scratch, nothing is borrowed
	const Placement p = passmem::place(5000, 0, 0, true);
	CHECK(!p.borrowed && p.own_bytes() == up(5000));
}

static void test_sort_bufs()
{
	SortBufs sb;
	CHECK(sb.temp_bytes == 0);
	sb.want(100); sb.want(7); sb.want(101); sb.want(0);
	CHECK(sb.temp_bytes == 101);
}

// ---- the reference list ----------------------------------------------------------------------------------------------------------
using bamfmt::RefList;

static void put32(std::vector<uint8_t> &v, uint32_t x) { for (int k = 0; k < 4; k++) v.push_back((uint8_t)(x >> (8 * k))); }
static void set32(std::vector<uint8_t> &v, size_t at, uint32_t x) { for (int k = 0; k < 4; k++) v[at + k] = (uint8_t)(x >> (8 * k)); }

struct TestRef { std::string name; uint32_t len; };           // name: the bytes in the file

static std::vector<uint8_t> header(const std::string &text, const std::vector<TestRef> &refs)
{
	std::vector<uint8_t> h = {'B', 'A', 'M', 1};
	put32(h, (uint32_t)text.size());
	h.insert(h.end(), text.begin(), text.end());
	put32(h, (uint32_t)refs.size());
	for (const TestRef &r : refs) {
		put32(h, (uint32_t)r.name.size());
		h.insert(h.end(), r.name.begin(), r.name.end());
		put32(h, r.len);
	}
	return h;
}

// parse() over a heap copy of exactly `have` bytes: ASan sees a read at or beyond `have`
static RefList::Status parse_copy(RefList &rl, const std::vector<uint8_t> &h, size_t have, uint64_t total)
{
	uint8_t *copy = (uint8_t *)malloc(have ? have : 1);
	if (have) memcpy(copy, h.data(), have);
	const RefList::Status s = rl.parse(have ? copy : copy + 1, have, total);   // (have == 0: a pointer no byte may be read from)
	free(copy);
	return s;
}

static void test_ref_list()
{
	const std::vector<TestRef> refs = {{std::string("chr1\0", 5), 1000}, {"noNUL", 0xfffffff0u}, {"", 7}};
	const std::vector<uint8_t> h = header("@HD\tVN:1.6\n", refs);
	RefList rl;
	for (size_t have = 0; have < h.size(); have++) CHECK(parse_copy(rl, h, have, h.size()) == RefList::kMore);
	CHECK(parse_copy(rl, h, h.size(), h.size()) == RefList::kOk);
	CHECK(rl.end == h.size() && rl.n_ref == 3 && rl.refs.size() == 3);
	CHECK(rl.name(h.data(), 0) == "chr1" && rl.name(h.data(), 1) == "noNUL" && rl.name(h.data(), 2) == "");
	CHECK(rl.refs[0].l_name == 5 && rl.refs[1].l_name == 5 && rl.refs[2].l_name == 0);
	CHECK(rl.refs[0].l_ref == 1000 && rl.refs[1].l_ref == 0xfffffff0u && rl.refs[2].l_ref == 7);
	CHECK(rl.names(h.data()) == (std::vector<std::string>{"chr1", "noNUL", ""}));
	for (size_t r = 0; r < 3; r++) CHECK(memcmp(h.data() + rl.refs[r].name_off, refs[r].name.data(), refs[r].name.size()) == 0);
	// records behind the header: the end is the first record's offset
	std::vector<uint8_t> longer = h;
	longer.resize(h.size() + 100, 0xee);
	CHECK(parse_copy(rl, longer, longer.size(), longer.size()) == RefList::kOk && rl.end == h.size());
	CHECK(parse_copy(rl, longer, h.size(), longer.size()) == RefList::kOk && rl.end == h.size());
	// a name with two trailing NULs loses one
	const std::vector<uint8_t> two = header("", {{std::string("x\0\0", 3), 1}});
	CHECK(parse_copy(rl, two, two.size(), two.size()) == RefList::kOk && rl.name(two.data(), 0) == std::string("x\0", 2));
	// a stream that ends inside a field: bad, whatever is there of it
	for (size_t total = 0; total < h.size(); total++)
		for (size_t have : {(size_t)0, total / 2, total}) CHECK(parse_copy(rl, h, have, total) != RefList::kOk);
	for (size_t total = 0; total < h.size(); total++) CHECK(parse_copy(rl, h, total, total) == RefList::kBad);
	// bad magic
	std::vector<uint8_t> bad = h;
	bad[3] = 2;
	CHECK(parse_copy(rl, bad, bad.size(), bad.size()) == RefList::kBad);
	CHECK(parse_copy(rl, bad, 12, bad.size()) == RefList::kBad);
	CHECK(parse_copy(rl, bad, 11, bad.size()) == RefList::kMore);      // (the magic is judged once 12 bytes are there)
	// a name of 2^20 bytes is read, one of 2^20 + 1 is bad before any of it is there
	const std::vector<uint8_t> big = header("", {{std::string((size_t)1 << 20, 'n'), 5}});
	CHECK(parse_copy(rl, big, big.size(), big.size()) == RefList::kOk && rl.refs[0].l_name == (1u << 20));
	std::vector<uint8_t> toobig = header("", {{"", 5}});
	set32(toobig, 12, (1u << 20) + 1);
	CHECK(parse_copy(rl, toobig, toobig.size(), (uint64_t)1 << 40) == RefList::kBad);
	// no references
	const std::vector<uint8_t> none = header("text", {});
	CHECK(parse_copy(rl, none, none.size(), none.size()) == RefList::kOk && rl.n_ref == 0 && rl.refs.empty() && rl.end == none.size());
	CHECK(rl.names(none.data()).empty());
	// n_ref = 0x80000000 is reported as -1 (and the list then ends beyond the stream, or wants more of it)
	std::vector<uint8_t> neg = header("", {});
	set32(neg, 8, 0x80000000u);
	CHECK(parse_copy(rl, neg, neg.size(), neg.size()) == RefList::kBad && rl.n_ref == -1);
	CHECK(parse_copy(rl, neg, neg.size(), (uint64_t)1 << 40) == RefList::kMore && rl.n_ref == -1);
	set32(neg, 8, 0x7fffffffu);
	CHECK(parse_copy(rl, neg, neg.size(), (uint64_t)1 << 40) == RefList::kMore && rl.n_ref == 0x7fffffff);
}

int main()
{
	test_layouts();
	test_placement();
	test_sort_bufs();
	test_ref_list();
	printf("ok: %d checks\n", g_checks);
	return 0;
}
