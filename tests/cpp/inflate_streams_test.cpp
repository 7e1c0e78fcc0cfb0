// host::inflate_raw (seqkit_amd/csrc/host_inflate.cpp) on DEFLATE members that zlib's encoder never writes, under ASan + UBSan.
// The members come from tests/deflate_corpus.py (written bit by bit by tests/deflate_writer.py: codes of up to 15 bits in every
// alphabet, headers without run symbols, empty blocks, stored blocks at every bit phase, structured invalid streams ...) in a
// container file:  u32 count;  per member  u32 in_len, out_len, flags (1: the corpus says zlib accepts it; 2: zlib accepts it and
// this decoder reports it, by design), name_len;  name;  payload[in_len];  expected[out_len].
// The rule, against this program's own zlib call, for every member:
//  * inflate_raw accepts  =>  zlib accepts, and the bytes are identical;
//  * zlib accepts  =>  inflate_raw accepts with identical bytes — unless the member is flagged "by design";
//  * the input is an exactly-sized copy (ASan sees a read behind it), the byte behind the output stays.
#include <zlib.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "host_common.h"

static bool zlib_inflate(const uint8_t *in, size_t n, std::vector<uint8_t> &out, size_t want)
{
	z_stream zs;
	memset(&zs, 0, sizeof zs);
	inflateInit2(&zs, -15);
	out.assign(want + 1, 0);
	zs.next_in = const_cast<uint8_t *>(in); zs.avail_in = (uInt)n;
	zs.next_out = out.data(); zs.avail_out = (uInt)want;
	const int rc = inflate(&zs, Z_FINISH);
	const bool ok = rc == Z_STREAM_END && zs.avail_out == 0;
	inflateEnd(&zs);
	out.resize(want);
	return ok;
}

static bool read_u32(FILE *f, uint32_t &v) { return fread(&v, 4, 1, f) == 1; }

int main(int argc, char **argv)
{
	if (argc < 2) { fprintf(stderr, "usage: inflate_streams_test CONTAINER\n"); return 2; }
	FILE *f = fopen(argv[1], "rb");
	if (!f) { perror(argv[1]); return 2; }
	uint32_t count = 0;
	if (!read_u32(f, count)) { fprintf(stderr, "empty container\n"); return 2; }
	size_t accepted = 0, refused = 0, by_design = 0, failures = 0;
	for (uint32_t i = 0; i < count; i++) {
		uint32_t in_len, out_len, flags, name_len;
		if (!read_u32(f, in_len) || !read_u32(f, out_len) || !read_u32(f, flags) || !read_u32(f, name_len)) { fprintf(stderr, "container cut at member %u\n", i); return 2; }
		std::string name(name_len, ' ');
		std::vector<uint8_t> exact(in_len), expected(out_len);
		if ((name_len && fread(&name[0], 1, name_len, f) != name_len) || (in_len && fread(exact.data(), 1, in_len, f) != in_len) ||
		    (out_len && fread(expected.data(), 1, out_len, f) != out_len)) { fprintf(stderr, "container cut at member %u\n", i); return 2; }
		std::vector<uint8_t> out((size_t)out_len + 1, 0xAB), ref;
		const bool mine = host::inflate_raw(exact.data(), exact.size(), out.data(), out_len);
		const bool theirs = zlib_inflate(exact.data(), exact.size(), ref, out_len);
		const char *what = nullptr;
		if (out[out_len] != 0xAB) what = "wrote past the output buffer";
		else if ((flags & 1u) && (!theirs || (out_len && memcmp(ref.data(), expected.data(), out_len) != 0))) what = "the corpus says valid, zlib does not make the expected bytes of it";
		else if (mine && !theirs) what = "accepted a member that zlib refuses";
		else if (mine && out_len && memcmp(out.data(), ref.data(), out_len) != 0) what = "accepted a member and made other bytes of it than zlib";
		else if (theirs && !mine && !(flags & 2u)) what = "refused a member that zlib accepts";
		else if (mine && (flags & 2u)) what = "accepted a member listed as reported by design: the list is stale";
		if (what) { fprintf(stderr, "FAIL member %u (%s): %s\n", i, name.c_str(), what); failures++; continue; }
		if (mine) accepted++;
		else if (theirs) by_design++;
		else refused++;
	}
	fclose(f);
	if (failures) { fprintf(stderr, "%zu of %u members failed\n", failures, count); return 1; }
	printf("ok: %u members, %zu accepted, %zu refused with zlib, %zu reported by design\n", count, accepted, refused, by_design);
	return 0;
}
