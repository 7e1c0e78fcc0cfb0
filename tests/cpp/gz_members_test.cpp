// Unit test of host::GzWriter::write_members (finished gzip members go to the file as they are, behind everything written before) and of
// pairing::write_member_windows (the loop over the windows of sk_bam_file_pairs_gz), without a device.  The files' contents are checked
// by the Python side.  usage: gz_members_test <dir>
#include <zlib.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "host_common.h"
#include "sam_pairing.h"

// one BGZF member that holds `data` (at most 0xff00 bytes) as a stored block
static std::vector<uint8_t> stored_member(const std::string &data)
{
	const uint16_t len = (uint16_t)data.size();
	const uint16_t bsize = (uint16_t)(18 + 5 + data.size() + 8 - 1);
	std::vector<uint8_t> m = {31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 'B', 'C', 2, 0, (uint8_t)(bsize & 255), (uint8_t)(bsize >> 8),
	                          1, (uint8_t)(len & 255), (uint8_t)(len >> 8), (uint8_t)(~len & 255), (uint8_t)((~len >> 8) & 255)};
	m.insert(m.end(), data.begin(), data.end());
	const uint32_t crc = (uint32_t)crc32(0, reinterpret_cast<const Bytef *>(data.data()), (uInt)data.size()), isize = (uint32_t)data.size();
	for (uint32_t v : {crc, isize}) for (int k = 0; k < 4; k++) m.push_back((uint8_t)(v >> (8 * k)));
	return m;
}

static std::string pattern(size_t n, int salt)
{
	std::string s(n, 'x');
	for (size_t k = 0; k < n; k++) s[k] = (char)('A' + (k * (size_t)(salt + 3)) % 23);
	return s;
}

#define CHECK(cond)                                                                          \
	do {                                                                                     \
		if (!(cond)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } \
	} while (0)

int main(int argc, char **argv)
{
	if (argc != 2) return 2;
	const std::string dir = argv[1];
	std::vector<uint8_t> two = stored_member("first member\n");
	const std::vector<uint8_t> second = stored_member(pattern(40000, 1));
	two.insert(two.end(), second.begin(), second.end());
	const std::vector<uint8_t> mid = stored_member("between the texts\n"), last = stored_member(pattern(0xff00, 2));
	{   // a fresh writer: the members, then the EOF block
		host::GzWriter w(dir + "/fresh.gz");
		w.write_members(two.data(), two.size());
		w.close();
	}
	{   // zero bytes (with and without a pointer): the file of a writer that got nothing
		host::GzWriter w(dir + "/zero.gz");
		w.write_members(two.data(), 0);
		w.write_members(nullptr, 0);
		w.close();
	}
	{   // behind buffered text, a few bytes and several pool jobs' worth, and in front of more: the order of the calls is the file's
		host::GzWriter w(dir + "/order.gz");
		w.write("head\n", 5);
		w.write_members(mid.data(), mid.size());
		const std::string big = pattern(1300000, 3);
		for (size_t at = 0; at < big.size(); at += 7001) w.write(big.data() + at, std::min<size_t>(7001, big.size() - at));
		w.write_members(last.data(), last.size());
		w.write(std::string("tail\n"));
		w.write_members(mid.data(), mid.size());
		w.close();
	}
	// write_member_windows: the windows of a stub `next` pass through unchanged and in order; the loop ends at n == 0
	struct Got { int stream; const uint8_t *p; size_t n; };
	std::vector<sk_bam_pairs_gz_window> wins;
	const std::vector<uint8_t> *src[4] = {&two, &mid, &last, &mid};
	const int streams[4] = {0, 0, 1, 2};
	for (int k = 0; k < 4; k++) {
		sk_bam_pairs_gz_window w;
		memset(&w, 0, sizeof w);
		w.stream = streams[k]; w.first = 10 * k; w.n = k + 1; w.bgzf = src[k]->data(); w.bytes = src[k]->size(); w.raw_bytes = 1;
		wins.push_back(w);
	}
	size_t calls = 0;
	std::vector<Got> got;
	pairing::write_member_windows(
		[&](sk_bam_pairs_gz_window *w) {
			if (calls < wins.size()) *w = wins[calls];
			else memset(w, 0, sizeof *w);
			calls++;
		},
		[&](int stream, const uint8_t *p, size_t n) { got.push_back(Got{stream, p, n}); });
	CHECK(calls == 5 && got.size() == 4);
	for (int k = 0; k < 4; k++) CHECK(got[k].stream == streams[k] && got[k].p == src[k]->data() && got[k].n == src[k]->size());
	calls = 0;
	wins.clear();
	pairing::write_member_windows([&](sk_bam_pairs_gz_window *w) { memset(w, 0, sizeof *w); calls++; }, [&](int, const uint8_t *, size_t) { calls += 100; });
	CHECK(calls == 1);
	printf("ok: 3 files, 4 windows\n");
	return 0;
}
