// sk_bamfmt.h — BAM and BGZF format bits that the library (sk_bamfile.cpp) and the hosts (sam_main.cpp, host_common.cpp) read or write.
// Plain C++: the hosts are built with g++.
#pragma once
#include <stdint.h>

#include <vector>

namespace bamfmt {

// a little-endian u32 at any address
inline uint32_t le32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

// the BGZF end-of-file marker: an empty member (SAMv1 §4.1.2)
constexpr uint8_t kBgzfEof[28] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0, 0x1b, 0, 0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0};

// Header::from_template + Writer (htslib sam_hdr_write): the text up to its first NUL, trailing '\n's stripped and one appended when
// anything is left; the reference list as read (htslib would rebuild it from the @SQ lines: DESIGN.md §10).  h: "BAM\1" .. the end of
// the reference list, as its reader checked it.
inline std::vector<uint8_t> rewrite_header(const std::vector<uint8_t> &h)
{
	const uint32_t l_text = le32(h.data() + 4);
	const uint8_t *text = h.data() + 8;
	size_t n = 0;
	while (n < l_text && text[n] != 0) n++;
	while (n > 0 && text[n - 1] == '\n') n--;
	const uint32_t l_new = n ? (uint32_t)n + 1 : 0;
	std::vector<uint8_t> o(h.begin(), h.begin() + 4);
	for (int k = 0; k < 4; k++) o.push_back((uint8_t)(l_new >> (8 * k)));
	o.insert(o.end(), text, text + n);
	if (n) o.push_back('\n');
	o.insert(o.end(), h.begin() + 8 + (ptrdiff_t)l_text, h.end());
	return o;
}

}  // namespace bamfmt
