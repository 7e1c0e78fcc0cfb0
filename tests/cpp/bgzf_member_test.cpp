// bgzf_member_test.cpp — the BGZF member framer of sk_bamfmt.h (bgzf_head, bgzf_stored, bgzf_trailer) on the host, built with the address
// and undefined-behaviour sanitizers (tests/test_bgzf_member_cpu.py).  Every member is framed in a heap buffer of exactly its size, so a
// byte written past the frame is a sanitizer report; what the frame must hold is restated here from SAMv1 §4.1 and RFC 1951/1952 and
// checked with zlib's own crc32 and inflate, not with the framer.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <zlib.h>

#include <vector>

#include "sk_bamfmt.h"

static long g_checks = 0;
static char g_what[128] = "";                    // the case at hand, for a failing CHECK
#define CHECK(cond)                                                                                                     \
	do {                                                                                                                \
		g_checks++;                                                                                                     \
		if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed [%s]\n", __FILE__, __LINE__, #cond, g_what); exit(1); }   \
	} while (0)

static uint32_t rd16(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
static uint32_t rd32(const uint8_t *p) { return rd16(p) | (rd16(p + 2) << 16); }

// the member as a reader sees it: the head field by field (RFC 1952 §2.3, SAMv1 §4.1), BSIZE, the trailer, and zlib's gzip decoder —
// which checks the head's layout, CRC32 and ISIZE once more on its own — over the whole member
static void check_member(const uint8_t *m, size_t bsize, const uint8_t *src, uint32_t len)
{
	CHECK(bsize >= 26 && bsize <= 65536);
	CHECK(m[0] == 31 && m[1] == 139);                                     // ID1, ID2
	CHECK(m[2] == 8);                                                     // CM = deflate
	CHECK(m[3] == 4);                                                     // FLG = FEXTRA
	CHECK(rd32(m + 4) == 0);                                              // MTIME
	CHECK(m[8] == 0 && m[9] == 255);                                      // XFL, OS = unknown
	CHECK(rd16(m + 10) == 6);                                             // XLEN
	CHECK(m[12] == 'B' && m[13] == 'C' && rd16(m + 14) == 2);             // SI1, SI2, SLEN
	CHECK(rd16(m + 16) == bsize - 1);                                     // BSIZE: the member's size minus one
	CHECK(rd32(m + bsize - 8) == (uint32_t)crc32(crc32(0L, Z_NULL, 0), src, len));
	CHECK(rd32(m + bsize - 4) == len);                                    // ISIZE
	std::vector<uint8_t> back((size_t)len + 1);
	z_stream z;
	memset(&z, 0, sizeof z);
	CHECK(inflateInit2(&z, 15 + 16) == Z_OK);                             // a gzip member, head and trailer included
	z.next_in = const_cast<uint8_t *>(m); z.avail_in = (uInt)bsize;
	z.next_out = back.data(); z.avail_out = (uInt)back.size();
	CHECK(inflate(&z, Z_FINISH) == Z_STREAM_END);
	CHECK(z.total_in == bsize && z.total_out == len);
	inflateEnd(&z);
	CHECK(memcmp(back.data(), src, len) == 0);
}

// `len` bytes that zlib shrinks (text = 1) or cannot (text = 0)
static std::vector<uint8_t> input(uint32_t len, int text)
{
	std::vector<uint8_t> v((size_t)len + 1);                              // (+ 1: a length of 0 still has an address)
	uint32_t s = 0x9e3779b9u ^ len;
	for (uint32_t i = 0; i < len; i++) {
		s = s * 1664525u + 1013904223u;
		v[i] = text ? (uint8_t)("ACGT"[(i / 7 + (s >> 30 == 0)) & 3]) : (uint8_t)(s >> 24);
	}
	return v;
}

int main()
{
	// 65535 - 26 - 5: the largest stored member whose BSIZE - 1 still fits 16 bits ... and 0xff00, the most a writer here puts in a block
	const uint32_t lens[] = {0, 1, 2, 0xfeff, 0xff00, 65535 - 26 - 5};
	for (uint32_t len : lens) {
		for (int text = 0; text < 2; text++) {
			const std::vector<uint8_t> in = input(len, text);
			// stored
			snprintf(g_what, sizeof g_what, "stored, len %u, text %d", len, text);
			{
				const size_t bsize = 18 + ((size_t)len + 5) + 8;
				uint8_t *m = (uint8_t *)malloc(bsize);
				CHECK(m != nullptr);
				memset(m, 0xa5, bsize);
				bamfmt::bgzf_head(m, bsize);
				const size_t clen = bamfmt::bgzf_stored(m + 18, in.data(), len);
				CHECK(clen == (size_t)len + 5);
				bamfmt::bgzf_trailer(m + 18 + clen, (uint32_t)crc32(crc32(0L, Z_NULL, 0), in.data(), len), len);
				// RFC 1951 §3.2.4: BFINAL = 1, BTYPE = 00, the rest of the byte padding; LEN; its one's complement; the bytes
				CHECK(m[18] == 1 && rd16(m + 19) == len && rd16(m + 21) == (~len & 0xffffu));
				CHECK(memcmp(m + 23, in.data(), len) == 0);
				check_member(m, bsize, in.data(), len);
				free(m);
			}
			// deflated by zlib
			snprintf(g_what, sizeof g_what, "deflated, len %u, text %d", len, text);
			{
				std::vector<uint8_t> comp(compressBound(len) + 64);
				z_stream z;
				memset(&z, 0, sizeof z);
				CHECK(deflateInit2(&z, 6, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) == Z_OK);
				z.next_in = const_cast<uint8_t *>(in.data()); z.avail_in = len;
				z.next_out = comp.data(); z.avail_out = (uInt)comp.size();
				CHECK(deflate(&z, Z_FINISH) == Z_STREAM_END);
				const size_t clen = z.total_out;
				deflateEnd(&z);
				CHECK(len < 1000 || (text ? clen < len / 2 : clen > len));    // (the input is what it is meant to be)
				const size_t bsize = 18 + clen + 8;
				// bytes zlib cannot shrink leave it in several stored blocks: at the largest length they do not fit a BSIZE, and a
				// writer stores the block instead (above)
				if (bsize > 65536) { CHECK(!text && len == 65535 - 26 - 5); continue; }
				uint8_t *m = (uint8_t *)malloc(bsize);
				CHECK(m != nullptr);
				memset(m, 0xa5, bsize);
				bamfmt::bgzf_head(m, bsize);
				memcpy(m + 18, comp.data(), clen);
				bamfmt::bgzf_trailer(m + 18 + clen, (uint32_t)crc32(crc32(0L, Z_NULL, 0), in.data(), len), len);
				check_member(m, bsize, in.data(), len);
				free(m);
			}
		}
	}
	// kBgzfHead is the head both constants open with
	CHECK(sizeof bamfmt::kBgzfHead == 16 && memcmp(bamfmt::kBgzfHead, bamfmt::kBgzfEof, 16) == 0);
	// An empty stored member is no EOF block.  SAMv1 §4.1.2 fixes the marker's 28 bytes: its payload is the empty fixed-Huffman block
	// 03 00, not the stored 01 00 00 ff ff.  The two share the head up to BSIZE and the all-zero trailer, both inflate to nothing, and a
	// reader that looks for the marker finds only the one.
	snprintf(g_what, sizeof g_what, "empty stored member against the EOF block");
	{
		const uint8_t none = 0;
		uint8_t *m = (uint8_t *)malloc(31);
		CHECK(m != nullptr);
		bamfmt::bgzf_head(m, 31);
		CHECK(bamfmt::bgzf_stored(m + 18, &none, 0) == 5);
		bamfmt::bgzf_trailer(m + 23, 0, 0);
		const uint8_t *eof = bamfmt::kBgzfEof;
		CHECK(sizeof bamfmt::kBgzfEof == 28);
		CHECK(memcmp(m, eof, 16) == 0);                                       // the head
		CHECK(rd16(m + 16) == 30 && rd16(eof + 16) == 27);                    // BSIZE - 1: 31 and 28 bytes
		CHECK(m[18] == 1 && m[19] == 0 && m[20] == 0 && m[21] == 0xff && m[22] == 0xff);
		CHECK(eof[18] == 3 && eof[19] == 0);                                  // BFINAL = 1, BTYPE = 01, the end-of-block code
		CHECK(memcmp(m + 23, eof + 20, 8) == 0 && rd32(eof + 20) == 0 && rd32(eof + 24) == 0);
		check_member(m, 31, &none, 0);
		check_member(eof, 28, &none, 0);
		free(m);
	}
	printf("ok: %ld checks\n", g_checks);
	return 0;
}
