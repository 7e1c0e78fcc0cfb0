// sk_capi_bam.cpp — the C-ABI of include/seqkit_hip.h, the BAM entry points over columns and streams: flag / tlen, inflate, walk and
// deflate, `sam fragments`, `sam count`, `sam statistics --on-target`, sequence() and the draw of `sam subsample`.  (The calls that
// take a BAM file by its path: sk_bamfile*.cpp.)
#include <algorithm>

#include "sk_bamfmt.h"
#include "sk_ctx.h"

// Each reference's regions in the order of their starts (stable, as `sam count` sorts them; src/sam_statistics.rs:51-53 sorts unstably,
// and this is one of the orders that may give): order[i] is the caller's entry at place i, s[i] its start, pm[i] the running maximum
// of the ends up to it (from `lowest` on).
template <class T>
static std::vector<int32_t> regions_by_start(int n_chr, const int32_t *chr_off, const T *rstart, const T *rend, T lowest, std::vector<T> &s, std::vector<T> &pm)
{
	std::vector<int32_t> order((size_t)chr_off[n_chr]);
	s.resize(order.size()); pm.resize(order.size());
	for (size_t i = 0; i < order.size(); i++) order[i] = (int32_t)i;
	for (int k = 0; k < n_chr; k++) {
		std::stable_sort(order.begin() + chr_off[k], order.begin() + chr_off[k + 1], [&](int32_t x, int32_t y) { return rstart[x] < rstart[y]; });
		T run = lowest;
		for (int32_t i = chr_off[k]; i < chr_off[k + 1]; i++) {
			s[(size_t)i] = rstart[order[(size_t)i]];
			pm[(size_t)i] = run = std::max(run, rend[order[(size_t)i]]);
		}
	}
	return order;
}

extern "C" {

// ---- BAM -------------------------------------------------------------------------------------------
int sk_bam_flag_tlen_dev(sk_ctx *c, const uint16_t *flag, const int32_t *tid, const int32_t *mtid, const int32_t *tlen,
                         int64_t n, int32_t max_frag, uint64_t *out)
{
	if (!c) return SK_ERR_INVALID;
	if (n < 0 || max_frag < 0) return fail(c, SK_ERR_INVALID, "n = %lld, max_frag = %d", (long long)n, max_frag);
	if (n == 0) return SK_OK;
	if (!flag || !tid || !mtid || !tlen || !out) return fail(c, SK_ERR_INVALID, "NULL column or out");
	if (int r = bind(c)) return r;
	SK_HIP(c, sk::launch_bam_flag_tlen(flag, tid, mtid, tlen, n, max_frag, (unsigned long long *)out, 1, 1, c->n_cu, c->stream));
	return SK_OK;
}

int sk_bam_flag_tlen(sk_ctx *c, const uint16_t *flag, const int32_t *tid, const int32_t *mtid, const int32_t *tlen,
                     int64_t n, int32_t max_frag, uint64_t counters[3], uint64_t *hist, uint64_t *hist_total)
{
	if (!c) return SK_ERR_INVALID;
	if (n < 0 || max_frag < 0) return fail(c, SK_ERR_INVALID, "n = %lld, max_frag = %d", (long long)n, max_frag);
	if (n == 0) return SK_OK;
	if (!flag) return fail(c, SK_ERR_INVALID, "flag is NULL");
	if (hist && (!tid || !mtid || !tlen)) return fail(c, SK_ERR_INVALID, "histogram needs tid, mtid and tlen");
	if (!counters && !hist) return fail(c, SK_ERR_INVALID, "nothing to do");
	if (int r = bind(c)) return r;
	const size_t nout = 4 + (hist ? (size_t)max_frag + 1 : 0);
	const Dir core = hist ? kIn : kDev;                           // counters alone read the flags only
	uint16_t *dflag;
	int32_t *dtid, *dmtid, *dtlen;
	Stage cols;
	cols.add(dflag, 2, kIn, flag); cols.add(dtid, 4, core, tid); cols.add(dmtid, 4, core, mtid); cols.add(dtlen, 4, core, tlen);
	ChunkPipe pipe(c, cols);
	if (int r = pipe.begin(n, rows_per_chunk(pipe_chunk((size_t)4 << 20), 1, n), nout * 8)) return r;
	unsigned long long *dout = (unsigned long long *)pipe.tail();
	SK_HIP(c, hipMemsetAsync(dout, 0, nout * 8, c->stream));
	SK_HIP(c, hipStreamSynchronize(c->stream));                   // both lanes add into dout
	for (; pipe.more(); pipe.next()) {
		if (int r = pipe.stage_in()) return r;
		SK_HIP(c, sk::launch_bam_flag_tlen(dflag, dtid, dmtid, dtlen, pipe.nr, max_frag, dout, counters ? 1 : 0, hist ? 1 : 0, c->n_cu, pipe.st()));
	}
	if (int r = pipe.end()) return r;
	std::vector<uint64_t> h(nout);
	SK_HIP(c, hipMemcpy(h.data(), dout, nout * 8, hipMemcpyDeviceToHost));
	if (counters) for (int i = 0; i < 3; i++) counters[i] += h[i];
	if (hist) {
		if (hist_total) *hist_total += h[3];
		for (size_t i = 0; i <= (size_t)max_frag; i++) hist[i] += h[4 + i];
	}
	return SK_OK;
}

// ---- B1 on the device (sk_inflate.hip) -----------------------------------------------------------------------------
int sk_bgzf_inflate_dev(sk_ctx *c, const uint8_t *comp, const sk_bgzf_block *blocks, int64_t n_blocks, uint8_t *out, uint32_t *status, int check_crc)
{
	if (!c) return SK_ERR_INVALID;
	if (n_blocks < 0) return fail(c, SK_ERR_INVALID, "n_blocks = %lld", (long long)n_blocks);
	if (n_blocks == 0) return SK_OK;
	if (!comp || !blocks || !out || !status) return fail(c, SK_ERR_INVALID, "NULL comp, blocks, out or status");
	if (!aligned16(out)) return fail(c, SK_ERR_INVALID, "out must be 16-byte aligned");
	if ((uintptr_t)blocks & 7u) return fail(c, SK_ERR_INVALID, "blocks must be 8-byte aligned");
	if (int r = bind(c)) return r;
	SK_HIP(c, sk::launch_bgzf_inflate(comp, blocks, n_blocks, out, status, check_crc, c->n_cu, c->stream));
	return SK_OK;
}

int sk_bam_walk_dev(sk_ctx *c, const uint8_t *stream, uint64_t stream_len, const uint64_t *block_end, int64_t n, uint64_t first_record, int32_t n_ref,
                    uint64_t *entry, uint64_t *exit_scratch, uint32_t *nrec_scratch, int max_rounds, int *verified, uint64_t *n_records, int *rounds)
{
	if (!c || !verified) return SK_ERR_INVALID;
	*verified = 0;
	if (n_records) *n_records = 0;
	if (rounds) *rounds = 0;
	if (n < 0) return fail(c, SK_ERR_INVALID, "n = %lld", (long long)n);
	if (n == 0) { *verified = first_record == stream_len; return SK_OK; }
	if (!stream || !block_end || !entry || !exit_scratch || !nrec_scratch) return fail(c, SK_ERR_INVALID, "NULL stream, block_end, entry or scratch");
	if (int r = bind(c)) return r;
	uint32_t *changed = nrec_scratch + n;
	SK_HIP(c, sk::launch_bam_walk(stream, stream_len, block_end, entry, exit_scratch, nrec_scratch, n, first_record, changed, 0, n_ref, c->stream));
	int r_done = 1;
	for (;; r_done++) {
		SK_HIP(c, hipMemsetAsync(changed, 0, 4, c->stream));
		// (the first round behind the walk: blocks whose entry is not their predecessor's exit guess a record start and walk from it)
		if (r_done == 1) SK_HIP(c, sk::launch_bam_walk(stream, stream_len, block_end, entry, exit_scratch, nrec_scratch, n, first_record, changed, 2, n_ref, c->stream));
		SK_HIP(c, sk::launch_bam_walk(stream, stream_len, block_end, entry, exit_scratch, nrec_scratch, n, first_record, changed, 1, n_ref, c->stream));
		uint32_t ch = 0;
		SK_HIP(c, hipMemcpyAsync(&ch, changed, 4, hipMemcpyDeviceToHost, c->stream));
		SK_HIP(c, hipStreamSynchronize(c->stream));
		if (ch == 0) break;
		if (r_done >= max_rounds) { if (rounds) *rounds = r_done; return SK_OK; }      // did not settle: not verified
	}
	if (rounds) *rounds = r_done;
	// settled: every entry is its predecessor's exit.  The chain is the file's when it also ends where the stream ends (and no walk met a record it could not take)
	std::vector<uint64_t> ex((size_t)n);
	std::vector<uint32_t> nr((size_t)n);
	SK_HIP(c, hipMemcpy(ex.data(), exit_scratch, (size_t)n * 8, hipMemcpyDeviceToHost));
	SK_HIP(c, hipMemcpy(nr.data(), nrec_scratch, (size_t)n * 4, hipMemcpyDeviceToHost));
	uint64_t total = 0;
	for (int64_t i = 0; i < n; i++) {
		if (ex[(size_t)i] >= ~0ull - 2ull) return SK_OK;
		total += nr[(size_t)i];
	}
	const uint64_t last = ex[(size_t)n - 1] < first_record ? first_record : ex[(size_t)n - 1];
	if (last != stream_len) return SK_OK;
	*verified = 1;
	if (n_records) *n_records = total;
	return SK_OK;
}

int sk_bam_walk_reduce_dev(sk_ctx *c, const uint8_t *stream, uint64_t stream_len, const uint64_t *block_end, const uint64_t *entry, int64_t n,
                           int32_t max_frag, int want_counters, int want_hist, uint64_t *out)
{
	if (!c) return SK_ERR_INVALID;
	if (n < 0 || max_frag < 0) return fail(c, SK_ERR_INVALID, "n = %lld, max_frag = %d", (long long)n, max_frag);
	if (n == 0) return SK_OK;
	if (!stream || !block_end || !entry || !out) return fail(c, SK_ERR_INVALID, "NULL stream, block_end, entry or out");
	if (int r = bind(c)) return r;
	SK_HIP(c, sk::launch_bam_walk_reduce(stream, stream_len, block_end, entry, n, max_frag, want_counters, want_hist, (unsigned long long *)out, c->stream));
	return SK_OK;
}


// ---- F2 on the device (sk_deflate.hip) -------------------------------------------------------------------------------
int sk_bgzf_deflate_dev(sk_ctx *c, const uint8_t *in, const sk_deflate_block *blocks, int64_t n_blocks, uint8_t *slots, uint32_t slot_stride,
                        uint32_t *tokens, uint32_t *result, uint32_t *crc)
{
	if (!c) return SK_ERR_INVALID;
	if (n_blocks < 0) return fail(c, SK_ERR_INVALID, "n_blocks = %lld", (long long)n_blocks);
	if (n_blocks == 0) return SK_OK;
	if (!in || !blocks || !slots || !tokens || !result || !crc) return fail(c, SK_ERR_INVALID, "NULL in, blocks, slots, tokens, result or crc");
	if (slot_stride < SK_DEFLATE_SLOT || (slot_stride & 3u) || ((uintptr_t)slots & 3u)) return fail(c, SK_ERR_INVALID, "slot_stride = %u (>= %d, a multiple of 4), slots 4-byte aligned", slot_stride, SK_DEFLATE_SLOT);
	if (int r = bind(c)) return r;
	SK_HIP(c, sk::launch_bgzf_deflate(in, blocks, n_blocks, slots, slot_stride, tokens, result, crc, c->n_cu, c->stream));
	return SK_OK;
}

int sk_bgzf_deflate(sk_ctx *c, const uint8_t *in, size_t in_bytes, const sk_deflate_block *blocks, int64_t n_blocks, uint8_t *out, size_t out_cap, uint64_t *out_off)
{
	if (!c) return SK_ERR_INVALID;
	if (n_blocks < 0 || !out_off) return fail(c, SK_ERR_INVALID, "n_blocks = %lld, out_off %p", (long long)n_blocks, (void *)out_off);
	out_off[0] = 0;
	if (n_blocks == 0) return SK_OK;
	if (!in || !blocks || !out) return fail(c, SK_ERR_INVALID, "NULL in, blocks or out");
	for (int64_t i = 0; i < n_blocks; i++)
		if (blocks[i].in_len > SK_DEFLATE_MAX_IN || blocks[i].in_off + blocks[i].in_len > in_bytes)
			return fail(c, SK_ERR_INVALID, "block %lld: %u bytes at %llu of %zu (at most %d a block)", (long long)i, blocks[i].in_len, (unsigned long long)blocks[i].in_off, in_bytes, SK_DEFLATE_MAX_IN);
	if (int r = bind(c)) return r;
	const size_t n = (size_t)n_blocks;
	const size_t b_slots = n * (size_t)SK_DEFLATE_SLOT;
	uint8_t *d_in, *d_slots;
	sk_deflate_block *d_blk;
	uint32_t *d_tok, *d_res, *d_crc;
	passmem::Layout ws;
	ws.add(d_in, in_bytes + 8); ws.add(d_blk, n * sizeof(sk_deflate_block)); ws.add(d_slots, b_slots);
	ws.add(d_tok, n * (size_t)SK_DEFLATE_MAX_IN * 4); ws.add(d_res, n * 8); ws.add(d_crc, n * 4);
	if (int r = ensure_ws(c, ws.total())) return r;
	ws.carve(c->ws.get());
	// a pinned landing area for the slots (the ctx keeps it, a quarter larger than the call that made it grow asked for)
	int krc = SK_OK;
	const size_t have = sk::ctx_kept_bytes(c, sk::kKeepDeflatePin);
	uint8_t *pin = (uint8_t *)sk::ctx_keep(c, sk::kKeepDeflatePin, have >= b_slots ? have : passmem::up(b_slots) + (passmem::up(b_slots) >> 2), true, &krc);
	if (!pin) return krc;
	SK_HIP(c, hipMemcpyAsync(d_in, in, in_bytes, hipMemcpyHostToDevice, c->stream));
	SK_HIP(c, hipMemsetAsync(d_in + in_bytes, 0, 8, c->stream));
	SK_HIP(c, hipMemcpyAsync(d_blk, blocks, n * sizeof(sk_deflate_block), hipMemcpyHostToDevice, c->stream));
	SK_HIP(c, sk::launch_bgzf_deflate(d_in, d_blk, n_blocks, d_slots, SK_DEFLATE_SLOT, d_tok, d_res, d_crc, c->n_cu, c->stream));
	std::vector<uint32_t> res(2 * n), crc(n);
	SK_HIP(c, hipMemcpyAsync(res.data(), d_res, n * 8, hipMemcpyDeviceToHost, c->stream));
	SK_HIP(c, hipMemcpyAsync(crc.data(), d_crc, n * 4, hipMemcpyDeviceToHost, c->stream));
	SK_HIP(c, hipMemcpyAsync(pin, d_slots, b_slots, hipMemcpyDeviceToHost, c->stream));
	SK_HIP(c, hipStreamSynchronize(c->stream));
	size_t at = 0;
	for (size_t i = 0; i < n; i++) {
		const uint32_t len = blocks[i].in_len, pay = res[2 * i];
		const bool stored = pay >= len + 5u || pay + 26u > SK_DEFLATE_MAX_MEMBER;
		const size_t clen = stored ? (size_t)len + 5 : pay;
		const size_t bsize = 18 + clen + 8;
		if (at + bsize > out_cap) return fail(c, SK_ERR_INVALID, "out_cap = %zu is too small (block %zu ends at %zu)", out_cap, i, at + bsize);
		uint8_t *m = out + at;
		bamfmt::bgzf_head(m, bsize);
		if (stored) bamfmt::bgzf_stored(m + 18, in + blocks[i].in_off, len);
		else memcpy(m + 18, pin + i * (size_t)SK_DEFLATE_SLOT, pay);
		bamfmt::bgzf_trailer(m + 18 + clen, crc[i], len);
		at += bsize;
		out_off[i + 1] = at;
	}
	return SK_OK;
}

// ---- f2: sam fragments filter ----------------------------------------------------------------------------------
int sk_bam_fragments_dev(sk_ctx *c, const uint16_t *flag, const int32_t *tid, const int32_t *mtid, const int32_t *tlen,
                         int64_t n, int64_t min_size, int64_t max_size, uint8_t *keep_bits, uint64_t *kept)
{
	if (!c) return SK_ERR_INVALID;
	if (n < 0) return fail(c, SK_ERR_INVALID, "n = %lld", (long long)n);
	if (n == 0) return SK_OK;
	if (!flag || !tid || !mtid || !tlen || !keep_bits || !kept) return fail(c, SK_ERR_INVALID, "NULL column or output");
	if (!aligned16(flag) || !aligned16(tid) || !aligned16(mtid) || !aligned16(tlen)) return fail(c, SK_ERR_INVALID, "columns must be 16-byte aligned");
	if (int r = bind(c)) return r;
	SK_HIP(c, sk::launch_bam_fragments(flag, tid, mtid, tlen, n, min_size, max_size, keep_bits, (unsigned long long *)kept, c->n_cu, c->stream));
	return SK_OK;
}

int sk_bam_fragments(sk_ctx *c, const uint16_t *flag, const int32_t *tid, const int32_t *mtid, const int32_t *tlen,
                     int64_t n, int64_t min_size, int64_t max_size, uint8_t *keep_bits, uint64_t *kept)
{
	if (!c) return SK_ERR_INVALID;
	if (n < 0) return fail(c, SK_ERR_INVALID, "n = %lld", (long long)n);
	if (n == 0) return SK_OK;
	if (!flag || !tid || !mtid || !tlen || !keep_bits) return fail(c, SK_ERR_INVALID, "NULL column or output");
	if (int r = bind(c)) return r;
	uint16_t *dflag;
	int32_t *dtid, *dmtid, *dtlen;
	uint8_t *dbits;
	Stage cols;
	cols.add(dflag, 2, kIn, flag); cols.add(dtid, 4, kIn, tid); cols.add(dmtid, 4, kIn, mtid); cols.add(dtlen, 4, kIn, tlen);
	cols.add_bits(dbits, 1, kOut, keep_bits);                     // one bit per row: a lane stores the byte of its 8 rows, clipped at the chunk's last
	ChunkPipe pipe(c, cols);
	if (int r = pipe.begin(n, rows_per_chunk(pipe_chunk((size_t)4 << 20), 8, n), 8)) return r;      // whole bytes of keep_bits per chunk
	unsigned long long *dkept = (unsigned long long *)pipe.tail();
	SK_HIP(c, hipMemsetAsync(dkept, 0, 8, c->stream));
	SK_HIP(c, hipStreamSynchronize(c->stream));                   // both lanes add into dkept
	for (; pipe.more(); pipe.next()) {
		if (int r = pipe.stage_in()) return r;
		SK_HIP(c, sk::launch_bam_fragments(dflag, dtid, dmtid, dtlen, pipe.nr, min_size, max_size, dbits, dkept, c->n_cu, pipe.st()));
		if (int r = pipe.stage_out()) return r;
	}
	if (int r = pipe.end()) return r;
	uint64_t k = 0;
	SK_HIP(c, hipMemcpy(&k, dkept, 8, hipMemcpyDeviceToHost));
	if (kept) *kept += k;
	return SK_OK;
}

// ---- f2 (second half): sam count ---------------------------------------------------------------------------------
int sk_count_set_regions(sk_ctx *c, int n_chr, const int32_t *chr_off, const uint32_t *rstart, const uint32_t *rend,
                         const int32_t *ridx, int64_t n_entries, int64_t n_counts)
{
	if (!c) return SK_ERR_INVALID;
	if (n_chr < 0 || n_entries < 0 || n_counts < n_entries || n_counts > 0x7fffffff || !chr_off || (n_entries > 0 && (!rstart || !rend)))
		return fail(c, SK_ERR_INVALID, "sk_count_set_regions: bad arguments");
	const int64_t n_regions = n_entries;
	if (chr_off[0] != 0 || chr_off[n_chr] != n_regions) return fail(c, SK_ERR_INVALID, "chr_off must run from 0 to n_entries");
	for (int k = 0; k < n_chr; k++) if (chr_off[k] > chr_off[k + 1]) return fail(c, SK_ERR_INVALID, "chr_off must not decrease");
	if (int r = bind(c)) return r;
	std::vector<uint32_t> s, pm, e((size_t)n_regions);
	std::vector<int32_t> ix = regions_by_start<uint32_t>(n_chr, chr_off, rstart, rend, 0u, s, pm);
	for (int64_t i = 0; i < n_regions; i++) {
		const int32_t o = ix[(size_t)i];
		e[(size_t)i] = rend[o];
		ix[(size_t)i] = ridx ? ridx[o] : o;
		if (ix[(size_t)i] < 0 || ix[(size_t)i] >= n_counts) return fail(c, SK_ERR_INVALID, "ridx out of range");
	}
	SK_HIP(c, hipStreamSynchronize(c->stream));
	c->cnt = sk_ctx::CountRegions{};
	const size_t b_reg = (size_t)n_regions * 4 + 4, b_cnt = passmem::up((size_t)n_counts * 4 + 4);
	passmem::Layout tab;
	tab.add(c->cnt.chr_off, (size_t)(n_chr + 1) * 4); tab.add(c->cnt.rstart, b_reg); tab.add(c->cnt.rend, b_reg); tab.add(c->cnt.rpmax, b_reg);
	tab.add(c->cnt.ridx, b_reg); tab.add(c->cnt.region_frags, b_cnt);
	hipError_t he = c->cnt.d.alloc(tab.total());
	if (he != hipSuccess) return fail(c, SK_ERR_NOMEM, "region tables: %s", hipGetErrorString(he));
	tab.carve(c->cnt.d.get());
	SK_HIP(c, hipMemcpyAsync(c->cnt.chr_off, chr_off, (size_t)(n_chr + 1) * 4, hipMemcpyHostToDevice, c->stream));
	if (n_regions) {
		SK_HIP(c, hipMemcpyAsync(c->cnt.rstart, s.data(), (size_t)n_regions * 4, hipMemcpyHostToDevice, c->stream));
		SK_HIP(c, hipMemcpyAsync(c->cnt.rend, e.data(), (size_t)n_regions * 4, hipMemcpyHostToDevice, c->stream));
		SK_HIP(c, hipMemcpyAsync(c->cnt.rpmax, pm.data(), (size_t)n_regions * 4, hipMemcpyHostToDevice, c->stream));
		SK_HIP(c, hipMemcpyAsync(c->cnt.ridx, ix.data(), (size_t)n_regions * 4, hipMemcpyHostToDevice, c->stream));
	}
	SK_HIP(c, hipMemsetAsync(c->cnt.region_frags, 0, b_cnt, c->stream));
	SK_HIP(c, hipStreamSynchronize(c->stream));              // the staging vectors go out of scope
	c->cnt.n_chr = n_chr;
	c->cnt.n_regions = n_counts;
	return SK_OK;
}

static int count_args(sk_ctx *c, sk::CountArgs &a, const uint16_t *flag, const uint8_t *mapq, const int32_t *tid, const int32_t *mtid,
                      const int32_t *pos, const int32_t *mpos, const int32_t *tlen, const int32_t *end_pos, int64_t n,
                      uint8_t min_mapq, uint32_t max_frag_len, int single_end, int center)
{
	if (!c->cnt.d) return fail(c, SK_ERR_INVALID, "sk_count_set_regions has not been called");
	if (n < 0) return fail(c, SK_ERR_INVALID, "n = %lld", (long long)n);
	if (n > 0 && (!flag || !mapq || !tid || !pos || (single_end ? !end_pos : (!mtid || !mpos || !tlen)))) return fail(c, SK_ERR_INVALID, "NULL column");
	a.flag = flag; a.mapq = mapq; a.tid = tid; a.mtid = mtid; a.pos = pos; a.mpos = mpos; a.tlen = tlen; a.end_pos = end_pos;
	a.n = n; a.min_mapq = min_mapq; a.max_frag_len = max_frag_len; a.single_end = single_end ? 1 : 0; a.center = center ? 1 : 0;
	a.n_chr = c->cnt.n_chr; a.chr_off = c->cnt.chr_off; a.rstart = c->cnt.rstart; a.rend = c->cnt.rend; a.rpmax = c->cnt.rpmax; a.ridx = c->cnt.ridx;
	a.counts = c->cnt.region_frags;
	return SK_OK;
}

int sk_count_add_dev(sk_ctx *c, const uint16_t *flag, const uint8_t *mapq, const int32_t *tid, const int32_t *mtid, const int32_t *pos,
                     const int32_t *mpos, const int32_t *tlen, const int32_t *end_pos, int64_t n, uint8_t min_mapq, uint32_t max_frag_len,
                     int single_end, int center)
{
	if (!c) return SK_ERR_INVALID;
	sk::CountArgs a;
	if (int r = count_args(c, a, flag, mapq, tid, mtid, pos, mpos, tlen, end_pos, n, min_mapq, max_frag_len, single_end, center)) return r;
	if (n == 0) return SK_OK;
	if (int r = bind(c)) return r;
	SK_HIP(c, sk::launch_bam_count(a, c->n_cu, c->stream));
	return SK_OK;
}

int sk_count_add(sk_ctx *c, const uint16_t *flag, const uint8_t *mapq, const int32_t *tid, const int32_t *mtid, const int32_t *pos,
                 const int32_t *mpos, const int32_t *tlen, const int32_t *end_pos, int64_t n, uint8_t min_mapq, uint32_t max_frag_len,
                 int single_end, int center)
{
	if (!c) return SK_ERR_INVALID;
	sk::CountArgs a;
	if (int r = count_args(c, a, flag, mapq, tid, mtid, pos, mpos, tlen, end_pos, n, min_mapq, max_frag_len, single_end, center)) return r;
	if (n == 0) return SK_OK;
	if (int r = bind(c)) return r;
	Stage cols;
	// (a column the caller leaves out — the other mode's — is carved all the same: the kernel is handed no NULL)
	auto col4 = [&](const int32_t *&dev, const int32_t *host) { cols.add(dev, 4, host ? kIn : kDev, host); };
	cols.add(a.flag, 2, kIn, flag); cols.add(a.mapq, 1, kIn, mapq);
	col4(a.tid, tid); col4(a.mtid, mtid); col4(a.pos, pos); col4(a.mpos, mpos); col4(a.tlen, tlen); col4(a.end_pos, end_pos);
	ChunkPipe pipe(c, cols);
	if (int r = pipe.begin(n, rows_per_chunk(pipe_chunk((size_t)2 << 20), 1, n))) return r;
	for (; pipe.more(); pipe.next()) {
		a.n = pipe.nr;
		if (int r = pipe.stage_in()) return r;
		SK_HIP(c, sk::launch_bam_count(a, c->n_cu, pipe.st()));
	}
	return pipe.end();
}

int sk_count_get(sk_ctx *c, uint32_t *region_frags)
{
	if (!c) return SK_ERR_INVALID;
	if (!c->cnt.d) return fail(c, SK_ERR_INVALID, "sk_count_set_regions has not been called");
	if (c->cnt.n_regions > 0 && !region_frags) return fail(c, SK_ERR_INVALID, "region_frags is NULL");
	if (int r = bind(c)) return r;
	SK_HIP(c, hipStreamSynchronize(c->stream));
	if (c->cnt.n_regions) SK_HIP(c, hipMemcpy(region_frags, c->cnt.region_frags, (size_t)c->cnt.n_regions * 4, hipMemcpyDeviceToHost));
	return SK_OK;
}

// ---- S2: sam statistics --on-target ---------------------------------------------------------------------------------
int sk_on_target_set_regions(sk_ctx *c, int n_chr, const int32_t *chr_off, const int64_t *rstart, const int64_t *rend, int64_t n_entries)
{
	if (!c) return SK_ERR_INVALID;
	if (n_chr < 0 || n_entries < 0 || n_entries > 0x7fffffff || !chr_off || (n_entries > 0 && (!rstart || !rend)))
		return fail(c, SK_ERR_INVALID, "sk_on_target_set_regions: bad arguments");
	if (chr_off[0] != 0 || chr_off[n_chr] != n_entries) return fail(c, SK_ERR_INVALID, "chr_off must run from 0 to n_entries");
	for (int k = 0; k < n_chr; k++) if (chr_off[k] > chr_off[k + 1]) return fail(c, SK_ERR_INVALID, "chr_off must not decrease");
	if (int r = bind(c)) return r;
	std::vector<int64_t> s, pm;
	regions_by_start<int64_t>(n_chr, chr_off, rstart, rend, INT64_MIN, s, pm);
	SK_HIP(c, hipStreamSynchronize(c->stream));
	c->ot = sk_ctx::TargetRegions{};
	const size_t b_cnt = passmem::up(6 * 8);
	passmem::Layout tab;
	tab.add(c->ot.chr_off, (size_t)(n_chr + 1) * 4); tab.add(c->ot.rstart, (size_t)n_entries * 8 + 8); tab.add(c->ot.rpmax, (size_t)n_entries * 8 + 8);
	tab.add(c->ot.counters, b_cnt);
	hipError_t he = c->ot.d.alloc(tab.total());
	if (he != hipSuccess) return fail(c, SK_ERR_NOMEM, "target region tables: %s", hipGetErrorString(he));
	tab.carve(c->ot.d.get());
	SK_HIP(c, hipMemcpyAsync(c->ot.chr_off, chr_off, (size_t)(n_chr + 1) * 4, hipMemcpyHostToDevice, c->stream));
	if (n_entries) {
		SK_HIP(c, hipMemcpyAsync(c->ot.rstart, s.data(), (size_t)n_entries * 8, hipMemcpyHostToDevice, c->stream));
		SK_HIP(c, hipMemcpyAsync(c->ot.rpmax, pm.data(), (size_t)n_entries * 8, hipMemcpyHostToDevice, c->stream));
	}
	SK_HIP(c, hipMemsetAsync(c->ot.counters, 0, b_cnt, c->stream));
	SK_HIP(c, hipStreamSynchronize(c->stream));              // the staging vectors go out of scope
	c->ot.n_chr = n_chr;
	return SK_OK;
}

static int on_target_args(sk_ctx *c, sk::TargetArgs &a, const uint16_t *flag, const int32_t *tid, const int32_t *mtid, const int32_t *pos,
                          const int32_t *mpos, const int32_t *tlen, const int32_t *end_pos, int64_t n, int64_t max_frag_len)
{
	if (!c->ot.d) return fail(c, SK_ERR_INVALID, "sk_on_target_set_regions has not been called");
	if (n < 0) return fail(c, SK_ERR_INVALID, "n = %lld", (long long)n);
	if (n > 0 && (!flag || !tid || !mtid || !pos || !mpos || !tlen || !end_pos)) return fail(c, SK_ERR_INVALID, "NULL column");
	a.flag = flag; a.tid = tid; a.mtid = mtid; a.pos = pos; a.mpos = mpos; a.tlen = tlen; a.end_pos = end_pos;
	a.n = n; a.max_frag_len = max_frag_len;
	a.n_chr = c->ot.n_chr; a.chr_off = c->ot.chr_off; a.rstart = c->ot.rstart; a.rpmax = c->ot.rpmax; a.out = c->ot.counters;
	return SK_OK;
}

int sk_on_target_add_dev(sk_ctx *c, const uint16_t *flag, const int32_t *tid, const int32_t *mtid, const int32_t *pos, const int32_t *mpos,
                         const int32_t *tlen, const int32_t *end_pos, int64_t n, int64_t max_frag_len)
{
	if (!c) return SK_ERR_INVALID;
	sk::TargetArgs a;
	if (int r = on_target_args(c, a, flag, tid, mtid, pos, mpos, tlen, end_pos, n, max_frag_len)) return r;
	if (n == 0) return SK_OK;
	if (int r = bind(c)) return r;
	SK_HIP(c, sk::launch_bam_target(a, c->n_cu, c->stream));
	return SK_OK;
}

int sk_on_target_add(sk_ctx *c, const uint16_t *flag, const int32_t *tid, const int32_t *mtid, const int32_t *pos, const int32_t *mpos,
                     const int32_t *tlen, const int32_t *end_pos, int64_t n, int64_t max_frag_len)
{
	if (!c) return SK_ERR_INVALID;
	sk::TargetArgs a;
	if (int r = on_target_args(c, a, flag, tid, mtid, pos, mpos, tlen, end_pos, n, max_frag_len)) return r;
	if (n == 0) return SK_OK;
	if (int r = bind(c)) return r;
	Stage cols;
	cols.add(a.flag, 2, kIn, flag); cols.add(a.tid, 4, kIn, tid); cols.add(a.mtid, 4, kIn, mtid); cols.add(a.pos, 4, kIn, pos);
	cols.add(a.mpos, 4, kIn, mpos); cols.add(a.tlen, 4, kIn, tlen); cols.add(a.end_pos, 4, kIn, end_pos);
	ChunkPipe pipe(c, cols);
	if (int r = pipe.begin(n, rows_per_chunk(pipe_chunk((size_t)2 << 20), 1, n))) return r;
	for (; pipe.more(); pipe.next()) {
		a.n = pipe.nr;
		if (int r = pipe.stage_in()) return r;
		SK_HIP(c, sk::launch_bam_target(a, c->n_cu, pipe.st()));
	}
	return pipe.end();
}

int sk_on_target_get(sk_ctx *c, uint64_t out[6])
{
	if (!c) return SK_ERR_INVALID;
	if (!c->ot.d) return fail(c, SK_ERR_INVALID, "sk_on_target_set_regions has not been called");
	if (!out) return fail(c, SK_ERR_INVALID, "out is NULL");
	if (int r = bind(c)) return r;
	SK_HIP(c, hipStreamSynchronize(c->stream));
	SK_HIP(c, hipMemcpy(out, c->ot.counters, 6 * 8, hipMemcpyDeviceToHost));
	return SK_OK;
}

// ---- f4: sam to fastq sequence() ---------------------------------------------------------------------------------
static int bam_sequence_check(sk_ctx *c, const uint8_t *seq4, int seq4_stride, const uint8_t *qual, int stride, const uint16_t *flag, int64_t n,
                              uint8_t *out)
{
	if (n < 0) return fail(c, SK_ERR_INVALID, "n = %lld", (long long)n);
	if (stride < 4 || (stride & 3) || seq4_stride < 4 || (seq4_stride & 3) || 2 * (int64_t)seq4_stride < stride || stride > 65532)
		return fail(c, SK_ERR_INVALID, "stride = %d, seq4_stride = %d: multiples of 4 with 2*seq4_stride >= stride wanted", stride, seq4_stride);
	if (n > 0 && (!seq4 || !qual || !flag || !out)) return fail(c, SK_ERR_INVALID, "NULL matrix or column");
	return SK_OK;
}

int sk_bam_sequence_dev(sk_ctx *c, const uint8_t *seq4, int seq4_stride, const uint8_t *qual, int stride, const uint16_t *len,
                        const uint16_t *flag, int64_t n, uint8_t min_baseq, uint8_t *out)
{
	if (!c) return SK_ERR_INVALID;
	if (int r = bam_sequence_check(c, seq4, seq4_stride, qual, stride, flag, n, out)) return r;
	if (n == 0) return SK_OK;
	if (((uintptr_t)seq4 | (uintptr_t)qual | (uintptr_t)out) & 3u) return fail(c, SK_ERR_INVALID, "matrices must be 4-byte aligned");
	if (int r = bind(c)) return r;
	SK_HIP(c, sk::launch_bam_sequence(seq4, seq4_stride, qual, stride, len, flag, n, min_baseq, out, c->n_cu, c->stream));
	return SK_OK;
}

int sk_bam_sequence(sk_ctx *c, const uint8_t *seq4, int seq4_stride, const uint8_t *qual, int stride, const uint16_t *len,
                    const uint16_t *flag, int64_t n, uint8_t min_baseq, uint8_t *out)
{
	if (!c) return SK_ERR_INVALID;
	if (int r = bam_sequence_check(c, seq4, seq4_stride, qual, stride, flag, n, out)) return r;
	if (n == 0) return SK_OK;
	if (int r = bind(c)) return r;
	const uint8_t *dseq, *dq;
	uint8_t *dout;
	const uint16_t *dlen, *dflag;
	Stage cols;
	cols.add(dseq, seq4_stride, kIn, seq4); cols.add(dq, stride, kIn, qual); cols.add(dout, stride, kOut, out);
	cols.add(dlen, 2, kIn, len); cols.add(dflag, 2, kIn, flag);
	ChunkPipe pipe(c, cols);
	if (int r = pipe.begin(n, cols.rows_for_bytes(pipe_chunk(kPipeChunkBytes), 1, n))) return r;
	for (; pipe.more(); pipe.next()) {
		if (int r = pipe.stage_in()) return r;
		SK_HIP(c, sk::launch_bam_sequence(dseq, seq4_stride, dq, stride, dlen, dflag, pipe.nr, min_baseq, dout, c->n_cu, pipe.st()));
		if (int r = pipe.stage_out()) return r;
	}
	return pipe.end();
}

// ---- sam subsample: the draw (include/seqkit_hip.h; host code, no device) ----------------------------------------
int sk_subsample_keep(uint64_t seed, uint64_t draw, float fraction)
{
	if (!(fraction >= 0.0f && fraction <= 1.0f)) return SK_ERR_INVALID;
	return sk::subsample_keeps(seed, draw, sk::subsample_threshold(fraction)) ? 1 : 0;
}

}  // extern "C"
