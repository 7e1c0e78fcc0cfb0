// sam_bamio.cpp — BAM in and out for the `sam` commands (sam_host.h says what each piece is): BamStream walks the BGZF/BAM container
// itself (SAMv1 §4.2: BGZF is a series of gzip members; after the header every record is block_size:u32 + a 32-byte fixed core), BamOut
// writes BAM to stdout, HostBamRewrite is the two around a BAM-writing command's own per-record loop; and the helpers more than one
// command file uses.
#include <fcntl.h>
#include <unistd.h>
#include <zlib.h>

#include <new>

#include "sam_host.h"

void check(int rc, const char *what)
{
	if (rc != SK_OK) error("%s failed: %s", what, sk_last_error(host::gpu()));
}

int64_t cigar_end_pos(const uint8_t *cigar, uint32_t n_cigar, int64_t pos, bool *bad)
{
	for (uint32_t k = 0; k < n_cigar; k++) {
		const uint32_t op = le32(cigar + 4 * k), code = op & 15;
		if (code > 8 && bad) *bad = true;
		if (code == 0 || code == 2 || code == 3 || code == 7 || code == 8) pos += op >> 4;
	}
	return pos;
}

std::vector<std::string> split_tabs(const std::string &t)
{
	std::vector<std::string> cols;
	for (size_t a = 0;;) {
		const size_t b = t.find('\t', a);
		cols.push_back(t.substr(a, b == std::string::npos ? b : b - a));
		if (b == std::string::npos) return cols;
		a = b + 1;
	}
}

BamStream::BamStream(const std::string &path, bool keep_header) : path_(path)
{
	int fd = 0;
	if (path != "-") fd = open(path.c_str(), O_RDONLY);
	if (fd < 0) error("Cannot open BAM file '%s'", path.c_str());
	bz_.reset(new host::BgzfStream(fd, true));
	uint8_t h[8];
	auto keep = [&](const uint8_t *p, size_t n) { if (keep_header) header_raw.insert(header_raw.end(), p, p + n); };
	if (!get(h, 8) || memcmp(h, "BAM\1", 4) != 0) open_fail();
	keep(h, 8);
	if (keep_header) {
		const uint32_t l_text = le32(h + 4);
		for (uint32_t done = 0; done < l_text;) {                 // (in steps: a damaged l_text runs into the end of the data first)
			const uint32_t step = std::min<uint32_t>(l_text - done, 16u << 20);
			header_raw.resize(header_raw.size() + step);
			if (!get(header_raw.data() + header_raw.size() - step, step)) open_fail();
			done += step;
		}
	} else if (!skip(le32(h + 4))) open_fail();
	if (!get(h, 4)) open_fail();
	keep(h, 4);
	const uint32_t n_ref = le32(h);
	for (uint32_t i = 0; i < n_ref; i++) {
		if (!get(h, 4)) open_fail();
		keep(h, 4);
		const uint32_t l_name = le32(h);
		if (l_name > (1u << 20)) open_fail();               // a reference name of megabytes is a damaged header, not an allocation to attempt
		std::string name(l_name, '\0');
		if (l_name && !get(reinterpret_cast<uint8_t *>(&name[0]), l_name)) open_fail();
		keep(reinterpret_cast<const uint8_t *>(name.data()), l_name);
		if (!name.empty() && name.back() == '\0') name.pop_back();
		names.push_back(name);
		if (!get(h, 4)) open_fail();
		keep(h, 4);
	}
}

bool BamStream::next(BamCore &c, bool want_end)
{
	Var v;
	if (!next_core(c, v)) return false;
	const uint32_t l_read_name = v.l_read_name, n_cigar = v.n_cigar;
	uint32_t rest = le32(head) - 32;
	if (want_end && rest >= l_read_name + 4 * n_cigar) {
		var_.resize(l_read_name + 4 * n_cigar);
		if (!need(var_.data(), var_.size())) return false;
		rest -= (uint32_t)var_.size();
		c.end_pos = (int32_t)cigar_end_pos(var_.data() + l_read_name, n_cigar, c.pos);
	}
	return skip(rest);
}

bool BamStream::next_chunk(std::vector<BamCore> &out, bool want_end)
{
	out.clear();
	if (!err_.empty()) return false;
	if (!want_end) {
		recs_.clear();
		if (bz_->bam_records(recs_) > 0) {
			out.resize(recs_.size());
			for (size_t i = 0; i < recs_.size(); i++) {
				const host::BgzfStream::BamRec &r = recs_[i];
				BamCore &c = out[i];
				c.tid = r.tid; c.pos = r.pos; c.flag = r.flag; c.mtid = r.mtid; c.mpos = r.mpos; c.tlen = r.tlen; c.end_pos = r.pos; c.mapq = r.mapq;
			}
			return true;
		}
	}
	BamCore c;
	if (!next(c, want_end)) return false;
	out.push_back(c);
	return true;
}

bool BamStream::next_full(BamCore &c, Var &v, std::vector<uint8_t> &body)
{
	if (!next_core(c, v)) return false;
	const uint32_t rest = le32(head) - 32;
	// htslib bam_read1: a record whose variable part cannot hold its own fields is invalid
	if (v.l_read_name < 1 || v.l_seq > 0x7fffffffu || v.aux_off() > rest) return rd_fail("Invalid BAM record.");
	// the record's size comes from the file: take it in steps, so that a damaged size field runs into the end of the data
	// ("BAM file ended prematurely.") instead of into one allocation of gigabytes
	body.clear();
	for (uint32_t done = 0; done < rest;) {
		const uint32_t step = std::min<uint32_t>(rest - done, 16u << 20);
		try { body.resize((size_t)done + step); } catch (const std::bad_alloc &) { return rd_fail("Invalid BAM record."); }
		if (!need(body.data() + done, step)) return false;
		done += step;
	}
	return true;
}

inline bool BamStream::next_core(BamCore &c, Var &v)
{
	if (!err_.empty()) return false;
	const long r = bz_->read(head, 36);
	if (r == 0) return false;
	if (r < 0) return rd_fail("Invalid BAM record.");
	if (r < 4) return rd_fail("BAM file ended prematurely.");
	if (le32(head) < 32) return rd_fail("Invalid BAM record.");
	if (r < 36 && !need(head + r, (size_t)(36 - r))) return false;
	const uint8_t *core = head + 4;
	c.tid = (int32_t)le32(core + 0);
	c.pos = (int32_t)le32(core + 4);
	v.l_read_name = core[8];
	c.mapq = core[9];
	v.n_cigar = (uint32_t)core[12] | ((uint32_t)core[13] << 8);
	c.flag = (uint16_t)(core[14] | (core[15] << 8));
	v.l_seq = le32(core + 16);
	c.mtid = (int32_t)le32(core + 20);
	c.mpos = (int32_t)le32(core + 24);
	c.tlen = (int32_t)le32(core + 28);
	c.end_pos = c.pos;
	return true;
}

inline bool BamStream::get(uint8_t *dst, size_t n)
{
	size_t got = 0;
	while (got < n) {
		const long r = bz_->read(dst + got, n - got);
		if (r <= 0) return false;
		got += (size_t)r;
	}
	return true;
}

inline bool BamStream::need(uint8_t *dst, size_t n)
{
	size_t got = 0;
	while (got < n) {
		const long r = bz_->read(dst + got, n - got);
		if (r < 0) return rd_fail("Invalid BAM record.");
		if (r == 0) return rd_fail("BAM file ended prematurely.");
		got += (size_t)r;
	}
	return true;
}

inline bool BamStream::skip(uint32_t n)                                     // need() without a destination
{
	size_t got = 0;
	while (got < n) {
		const long r = bz_->skip(n - got);
		if (r < 0) return rd_fail("Invalid BAM record.");
		if (r == 0) return rd_fail("BAM file ended prematurely.");
		got += (size_t)r;
	}
	return true;
}

int64_t fill_batch(BamStream &bam, Columns &col, bool want_end, bool extra)
{
	col.clear();
	while (col.more && col.flag.size() < kBatchRecords && (col.more = bam.next_chunk(col.chunk, want_end)))
		for (const BamCore &c : col.chunk) col.push(c, extra);
	return (int64_t)col.flag.size();
}

std::string expand_home(const std::string &path)      // PathArgs::get_path, src/common.rs:28-38
{
	if (!path.empty() && path[0] == '~')
		if (const char *home = getenv("HOME")) return std::string(home) + path.substr(1);
	return path;
}

std::vector<std::string> header_names(const uint8_t *h, uint64_t len)
{
	bamfmt::RefList refs;
	(void)refs.parse(h, len, len);
	return refs.names(h);
}

bool file_path_wanted(const std::string &path) { return path != "-" && !getenv("SEQKIT_HOST_INFLATE"); }

bool bamfile_trace() { static const bool on = getenv("SK_BAMFILE_TRACE") != nullptr; return on; }

uint64_t file_window_bytes()
{
	static const uint64_t window = [] { const char *ev = getenv("SK_BAMFILE_WINDOW"); return ev ? (uint64_t)strtoull(ev, nullptr, 10) : (uint64_t)0; }();
	return window;
}

bool parse_i64(const std::string &s, int64_t &out)          // str::parse::<i64>()
{
	const char *p = s.c_str();
	bool neg = false;
	if (*p == '+' || *p == '-') { neg = *p == '-'; p++; }
	uint64_t v;
	if (!host::parse_uint(p, neg ? 9223372036854775808ull : 9223372036854775807ull, v)) return false;
	out = neg ? (int64_t)(0 - v) : (int64_t)v;
	return true;
}

void BamOut::flush()
{
	if (buf_.empty()) return;
	const size_t n = buf_.size(), nblk = (n + SK_DEFLATE_MAX_IN - 1) / SK_DEFLATE_MAX_IN;
	buf_.resize(n + 8, 0);                                       // (the device reads whole dwords)
	std::vector<sk_deflate_block> blocks(nblk);
	for (size_t i = 0; i < nblk; i++) { blocks[i].in_off = i * SK_DEFLATE_MAX_IN; blocks[i].in_len = (uint32_t)std::min<size_t>(SK_DEFLATE_MAX_IN, n - i * SK_DEFLATE_MAX_IN); blocks[i].reserved = 0; }
	std::vector<uint64_t> off(nblk + 1);
	static const bool here = [] { const char *e = getenv("SEQKIT_GPU_DEFLATE"); return e && atoi(e) == 0; }();
	if (level_ && here) deflate_here(blocks, off);
	else if (level_) {
		comp_.resize(nblk * SK_DEFLATE_MAX_MEMBER);
		check(sk_bgzf_deflate(host::gpu(), buf_.data(), n, blocks.data(), (int64_t)nblk, comp_.data(), comp_.size(), off.data()), "sk_bgzf_deflate");
	} else {
		comp_.resize(nblk * (SK_DEFLATE_MAX_IN + 31));
		size_t at = 0;
		for (size_t i = 0; i < nblk; i++) {
			const uint32_t len = blocks[i].in_len, bsize = len + 31;
			uint8_t *m = comp_.data() + at;
			bamfmt::bgzf_head(m, bsize);
			const size_t clen = bamfmt::bgzf_stored(m + 18, buf_.data() + blocks[i].in_off, len);
			const uint32_t crc = (uint32_t)crc32(crc32(0L, Z_NULL, 0), buf_.data() + blocks[i].in_off, len);
			bamfmt::bgzf_trailer(m + 18 + clen, crc, len);
			at += bsize;
		}
		off[nblk] = at;
	}
	write_all(comp_.data(), (size_t)off[nblk]);
	buf_.clear();
}

void BamOut::finish()
{
	if (done_) return;
	done_ = true;
	flush();
	write_all(bamfmt::kBgzfEof, sizeof bamfmt::kBgzfEof);
}

void BamOut::write_all(const uint8_t *p, size_t n)
{
	while (n) {
		const ssize_t w = ::write(1, p, n);
		if (w <= 0) error("Output stream closed unexpectedly.");
		p += w; n -= (size_t)w;
	}
}

// (SEQKIT_GPU_DEFLATE=0, the gzip writers' switch: level 1 is deflated here by zlib instead — the inflated stream is the same, and a
// command without --uncompressed can then be run where there is no device)
void BamOut::deflate_here(const std::vector<sk_deflate_block> &blocks, std::vector<uint64_t> &off)
{
	comp_.resize(blocks.size() * SK_DEFLATE_MAX_MEMBER);
	size_t at = 0;
	for (size_t i = 0; i < blocks.size(); i++) {
		const uint32_t len = blocks[i].in_len;
		const uint8_t *src = buf_.data() + blocks[i].in_off;
		uint8_t *m = comp_.data() + at;
		z_stream z;
		memset(&z, 0, sizeof z);
		if (deflateInit2(&z, 6, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) error("zlib: deflateInit2 failed");
		z.next_in = const_cast<uint8_t *>(src); z.avail_in = len;
		z.next_out = m + 18; z.avail_out = SK_DEFLATE_MAX_MEMBER - 26;
		const int zr = deflate(&z, Z_FINISH);
		uint32_t clen = (uint32_t)z.total_out;
		deflateEnd(&z);
		if (zr != Z_STREAM_END) clen = (uint32_t)bamfmt::bgzf_stored(m + 18, src, len);   // (it does not fit a member: stored)
		const uint32_t bsize = clen + 26, crc = (uint32_t)crc32(crc32(0L, Z_NULL, 0), src, len);
		bamfmt::bgzf_head(m, bsize);
		bamfmt::bgzf_trailer(m + 18 + clen, crc, len);
		at += bsize;
	}
	off[blocks.size()] = at;
}

static BamOut *g_bam_out = nullptr;
static void finish_bam_out() { if (g_bam_out) g_bam_out->finish(); }    // a panic unwinds through the Writer's drop: what was written stays valid BAM

void finish_at_exit(BamOut *out)
{
	g_bam_out = out;
	host::at_exit_flush(finish_bam_out);
}

void HostBamRewrite::start(const uint8_t *more, size_t n_more)
{
	finish_at_exit(&out);
	const std::vector<uint8_t> hdr = bamfmt::rewrite_header(bam.header_raw, more, n_more);
	out.put(hdr.data(), hdr.size());
	out.flush();
}

// (sam merge: its loop has raised every input's error by now, the first's among them; the call here finds none)
void HostBamRewrite::close() { bam.raise_deferred(); out.finish(); g_bam_out = nullptr; }

bool find_rx(const uint8_t *a, size_t n, const uint8_t *&val, size_t &vl)
{
	size_t o = 0;
	while (o + 3 <= n) {
		const uint8_t t0 = a[o], t1 = a[o + 1], ty = a[o + 2];
		size_t v = o + 3, e;
		if (ty == 'A' || ty == 'c' || ty == 'C') e = v + 1;
		else if (ty == 's' || ty == 'S') e = v + 2;
		else if (ty == 'i' || ty == 'I' || ty == 'f') e = v + 4;
		else if (ty == 'Z' || ty == 'H') {
			const void *z = v < n ? memchr(a + v, 0, n - v) : nullptr;
			if (!z) return false;
			e = (size_t)((const uint8_t *)z - a) + 1;
		} else if (ty == 'B') {
			if (v + 5 > n) return false;
			const uint8_t sub = a[v];
			const uint32_t cnt = le32(a + v + 1);
			const size_t es = (sub == 'c' || sub == 'C') ? 1 : (sub == 's' || sub == 'S') ? 2 : (sub == 'i' || sub == 'I' || sub == 'f') ? 4 : 0;
			if (!es) return false;
			e = v + 5 + (size_t)cnt * es;
		} else return false;
		if (e > n) return false;
		if (t0 == 'R' && t1 == 'X') {
			if (ty != 'Z' && ty != 'H') return false;
			val = a + v; vl = e - v - 1;
			return true;
		}
		o = e;
	}
	return false;
}

void renamed_record(std::vector<uint8_t> &rec, const uint8_t *head, const std::string &name, const uint8_t *tail, size_t n_tail, const std::vector<uint8_t> &app)
{
	const uint32_t bs = (uint32_t)(32 + name.size() + 1 + n_tail + app.size());
	rec.assign(head, head + 36);
	for (int k = 0; k < 4; k++) rec[k] = (uint8_t)(bs >> (8 * k));
	rec[12] = (uint8_t)(name.size() + 1);
	rec.insert(rec.end(), name.begin(), name.end());
	rec.push_back(0);
	rec.insert(rec.end(), tail, tail + n_tail);
	rec.insert(rec.end(), app.begin(), app.end());
}
