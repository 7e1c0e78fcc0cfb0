// sk_bamfmt.h — BAM and BGZF format bits that the library (sk_bamfile*.cpp) and the hosts (sam_*.cpp, host_common.cpp) read or write.
// Plain C++: the hosts are built with g++.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

namespace bamfmt {

// a little-endian u32 at any address
inline uint32_t le32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

// the BGZF end-of-file marker: an empty member (SAMv1 §4.1.2)
constexpr uint8_t kBgzfEof[28] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0, 0x1b, 0, 0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0};

// A BGZF member (SAMv1 §4.1): the gzip head whose 'BC' extra field carries BSIZE - 1 at 16..17, a DEFLATE payload from 18 on, then
// CRC32 and ISIZE of the bytes it inflates to.  Which payload a member gets is its writer's decision, and so is the CRC's computation.
constexpr uint8_t kBgzfHead[16] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0};

// the 18 bytes of head of a member of bsize bytes in all (head, payload and trailer: at most 65536)
inline void bgzf_head(uint8_t *m, size_t bsize)
{
	memcpy(m, kBgzfHead, 16);
	m[16] = (uint8_t)((bsize - 1) & 0xff);
	m[17] = (uint8_t)((bsize - 1) >> 8);
}

// a payload of one stored block (BFINAL = 1, BTYPE = 00; LEN, ~LEN, the bytes) at p; its length, len + 5
inline size_t bgzf_stored(uint8_t *p, const uint8_t *src, uint32_t len)
{
	p[0] = 1;
	p[1] = (uint8_t)(len & 0xff); p[2] = (uint8_t)(len >> 8);
	p[3] = (uint8_t)(~len & 0xff); p[4] = (uint8_t)((~len >> 8) & 0xff);
	memcpy(p + 5, src, len);
	return (size_t)len + 5;
}

// the 8 bytes behind the payload
inline void bgzf_trailer(uint8_t *t, uint32_t crc, uint32_t isize)
{
	for (int k = 0; k < 4; k++) { t[k] = (uint8_t)(crc >> (8 * k)); t[4 + k] = (uint8_t)(isize >> (8 * k)); }
}

// Header::from_template + Writer (htslib sam_hdr_write): the text up to its first NUL, trailing '\n's stripped and one appended when
// anything is left; the reference list as read (htslib would rebuild it from the @SQ lines: DESIGN.md §10).  h: "BAM\1" .. the end of
// the reference list, as its reader checked it.  more: whole lines behind the text (Header::push_comment, `sam discard tail artifacts`).
inline std::vector<uint8_t> rewrite_header(const std::vector<uint8_t> &h, const uint8_t *more = nullptr, size_t n_more = 0)
{
	const uint32_t l_text = le32(h.data() + 4);
	const uint8_t *text = h.data() + 8;
	size_t n = 0;
	while (n < l_text && text[n] != 0) n++;
	while (n > 0 && text[n - 1] == '\n') n--;
	const uint32_t l_new = (n ? (uint32_t)n + 1 : 0) + (uint32_t)n_more;
	std::vector<uint8_t> o(h.begin(), h.begin() + 4);
	for (int k = 0; k < 4; k++) o.push_back((uint8_t)(l_new >> (8 * k)));
	o.insert(o.end(), text, text + n);
	if (n) o.push_back('\n');
	if (n_more) o.insert(o.end(), more, more + n_more);
	o.insert(o.end(), h.begin() + 8 + (ptrdiff_t)l_text, h.end());
	return o;
}

// The reference list of a BAM header (SAMv1 §4.2: magic, l_text, text, n_ref, then per reference l_name, name, l_ref), read from the
// first `have` bytes of a stream of `total` bytes; no byte at or beyond `have` is read.  kBad: no BAM magic, a name of more than 2^20
// bytes (the hosts' reader refuses such a header), or a field that ends beyond `total`; kMore: a field ends beyond `have`; kOk: `end` is
// where the list ends — the first record's offset — and refs holds, per reference, where its name lies in h and the two lengths.
// n_ref is the header's count as far as it was read, -1 where that exceeds 0x7fffffff.
struct RefList {
	enum Status { kOk, kMore, kBad };
	struct Ref { uint64_t name_off; uint32_t l_name, l_ref; };
	uint64_t end = 0;
	int32_t n_ref = -1;
	std::vector<Ref> refs;
	Status parse(const uint8_t *h, uint64_t have, uint64_t total)
	{
		end = 0; n_ref = -1; refs.clear();
		Status st = kOk;
		auto need = [&](uint64_t upto) { if (upto > have) { st = upto > total ? kBad : kMore; return false; } return true; };
		if (!need(12)) return st;
		if (memcmp(h, "BAM\1", 4) != 0) return kBad;
		uint64_t o = 8 + (uint64_t)le32(h + 4);
		if (!need(o + 4)) return st;
		const uint32_t n = le32(h + o);
		n_ref = n <= 0x7fffffffu ? (int32_t)n : -1;
		o += 4;
		for (uint32_t r = 0; r < n; r++) {
			if (!need(o + 4)) return st;
			const uint32_t l_name = le32(h + o);
			if (l_name > (1u << 20)) return kBad;
			if (!need(o + 4 + (uint64_t)l_name + 4)) return st;
			refs.push_back(Ref{o + 4, l_name, le32(h + o + 4 + l_name)});
			o += 4 + (uint64_t)l_name + 4;
		}
		end = o;
		return kOk;
	}
	// reference r's name as the hosts' reader keeps it: one trailing NUL dropped, other bytes kept
	std::string name(const uint8_t *h, size_t r) const
	{
		std::string s(reinterpret_cast<const char *>(h) + refs[r].name_off, refs[r].l_name);
		if (!s.empty() && s.back() == '\0') s.pop_back();
		return s;
	}
	std::vector<std::string> names(const uint8_t *h) const
	{
		std::vector<std::string> v;
		for (size_t r = 0; r < refs.size(); r++) v.push_back(name(h, r));
		return v;
	}
};

}  // namespace bamfmt
