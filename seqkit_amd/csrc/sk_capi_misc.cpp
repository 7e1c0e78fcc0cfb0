// sk_capi_misc.cpp — the C-ABI of include/seqkit_hip.h, what stands apart from barcodes and BAM: `fasta gc content` over a resident
// genome, and the barcode census (sk_census.hip).
#include <algorithm>

#include "sk_ctx.h"

extern "C" {

// ---- fasta gc content -------------------------------------------------------------------------------------------
int sk_gc_set_genome(sk_ctx *c, const uint8_t *genome, int64_t genome_len)
{
	if (!c) return SK_ERR_INVALID;
	if (genome_len < 0 || (genome_len > 0 && !genome)) return fail(c, SK_ERR_INVALID, "sk_gc_set_genome: bad arguments");
	if (int r = bind(c)) return r;
	SK_HIP(c, hipStreamSynchronize(c->stream));
	c->genome = sk_ctx::Genome{};
	hipError_t e = c->genome.d.alloc((size_t)genome_len + 32);
	if (e != hipSuccess) return fail(c, SK_ERR_NOMEM, "genome of %lld bytes: %s", (long long)genome_len, hipGetErrorString(e));
	if (genome_len) SK_HIP(c, hipMemcpy(c->genome.d.get(), genome, (size_t)genome_len, hipMemcpyHostToDevice));
	SK_HIP(c, hipDeviceSynchronize());     // the ctx streams are non-blocking: make the upload visible to them (as sk_set_barcodes does)
	c->genome.len = genome_len;
	return SK_OK;
}

int sk_gc_count(sk_ctx *c, const int64_t *start, const int64_t *len, int64_t n_regions, uint64_t *gc, uint64_t *total)
{
	if (!c) return SK_ERR_INVALID;
	if (!c->genome.d) return fail(c, SK_ERR_INVALID, "sk_gc_set_genome has not been called");
	if (n_regions < 0 || n_regions > 0x7fffffff) return fail(c, SK_ERR_INVALID, "n_regions = %lld", (long long)n_regions);
	if (n_regions == 0) return SK_OK;
	if (!start || !len || !gc || !total) return fail(c, SK_ERR_INVALID, "NULL argument");
	if (int r = bind(c)) return r;
	// regions -> segments of at most 64 KiB, one wave each
	const int64_t kSeg = 64 * 1024;
	std::vector<int64_t> sstart;
	std::vector<int32_t> slen, sreg;
	for (int64_t i = 0; i < n_regions; i++) {
		if (start[i] < 0 || len[i] < 0 || start[i] > c->genome.len || len[i] > c->genome.len - start[i])
			return fail(c, SK_ERR_INVALID, "region %lld = [%lld, +%lld) leaves the genome (%lld bytes)", (long long)i, (long long)start[i], (long long)len[i], (long long)c->genome.len);
		for (int64_t o = 0; o < len[i]; o += kSeg) {
			sstart.push_back(start[i] + o);
			slen.push_back((int32_t)std::min<int64_t>(kSeg, len[i] - o));
			sreg.push_back((int32_t)i);
		}
	}
	const size_t ns = sstart.size();
	unsigned long long *dout;
	int64_t *dstart;
	int32_t *dlen, *dreg;
	passmem::Layout ws;
	ws.add(dout, (size_t)n_regions * 16); ws.add(dstart, ns * 8 + 8); ws.add(dlen, ns * 4 + 4); ws.add(dreg, ns * 4 + 4);
	if (int r = ensure_ws(c, ws.total())) return r;
	ws.carve(c->ws.get());
	SK_HIP(c, hipMemsetAsync(dout, 0, (size_t)n_regions * 16, c->stream));
	if (ns) {
		SK_HIP(c, hipMemcpyAsync(dstart, sstart.data(), ns * 8, hipMemcpyHostToDevice, c->stream));
		SK_HIP(c, hipMemcpyAsync(dlen, slen.data(), ns * 4, hipMemcpyHostToDevice, c->stream));
		SK_HIP(c, hipMemcpyAsync(dreg, sreg.data(), ns * 4, hipMemcpyHostToDevice, c->stream));
		SK_HIP(c, sk::launch_gc_count(c->genome.d.get(), dstart, dlen, dreg, (int64_t)ns, dout, c->n_cu, c->stream));
	}
	std::vector<uint64_t> h((size_t)n_regions * 2);
	SK_HIP(c, hipMemcpyAsync(h.data(), dout, (size_t)n_regions * 16, hipMemcpyDeviceToHost, c->stream));
	SK_HIP(c, hipStreamSynchronize(c->stream));
	for (int64_t i = 0; i < n_regions; i++) { gc[i] = h[(size_t)2 * i]; total[i] = h[(size_t)2 * i + 1]; }
	return SK_OK;
}

// ---- f3: barcode census ----------------------------------------------------------------------------------------
static_assert(sizeof(sk_census_entry) == sizeof(sk::CensusEntry), "sk_census_entry layout");

static int census_ready(sk_ctx *c)
{
	if (c->census) return SK_OK;
	SK_HIP(c, sk::census_create(&c->census, c->stream));
	return SK_OK;
}

int sk_census_reset(sk_ctx *c)
{
	if (!c) return SK_ERR_INVALID;
	if (int r = bind(c)) return r;
	if (!c->census) return census_ready(c);
	SK_HIP(c, sk::census_reset(c->census, c->n_cu, c->stream));
	return SK_OK;
}

static int census_check(sk_ctx *c, const uint8_t *bc, int bc_stride, int L, int64_t n)
{
	if (n < 0) return fail(c, SK_ERR_INVALID, "n = %lld", (long long)n);
	if (L < 0 || L > sk::kMaxCensusLen) return fail(c, SK_ERR_INVALID, "census barcode length %d (0..%d)", L, sk::kMaxCensusLen);
	if (bc_stride < L || bc_stride < 1 || bc_stride > 64) return fail(c, SK_ERR_INVALID, "bc_stride = %d (1..64), L = %d", bc_stride, L);
	if (n > 0 && !bc) return fail(c, SK_ERR_INVALID, "bc is NULL");
	return SK_OK;
}

int sk_census_add_dev(sk_ctx *c, const uint8_t *bc, int bc_stride, int L, int64_t n, const int32_t *assign, int64_t row_base)
{
	if (!c) return SK_ERR_INVALID;
	if (int r = census_check(c, bc, bc_stride, L, n)) return r;
	if (n == 0) return SK_OK;
	if (!aligned16(bc)) return fail(c, SK_ERR_INVALID, "bc must be 16-byte aligned");
	if (int r = bind(c)) return r;
	if (int r = census_ready(c)) return r;
	SK_HIP(c, sk::census_add(c->census, bc, bc_stride, L, n, assign, row_base, c->n_cu, c->stream));
	return SK_OK;
}

int sk_census_add(sk_ctx *c, const uint8_t *bc, int bc_stride, int L, int64_t n, const int32_t *assign, int64_t row_base)
{
	if (!c) return SK_ERR_INVALID;
	if (int r = census_check(c, bc, bc_stride, L, n)) return r;
	if (n == 0) return SK_OK;
	if (int r = bind(c)) return r;
	if (int r = census_ready(c)) return r;
	// one stream, one half: inserts of two lanes in flight would change which row is recorded as a key's first
	uint8_t *dbc;
	int32_t *dassign;
	Stage cols;
	cols.add(dbc, bc_stride, kIn, bc); cols.add(dassign, 4, kIn, assign);
	cols.plan(cols.rows_for_bytes(pipe_chunk((size_t)64 << 20), 1, n), 0, 1);
	if (int r = ensure_ws(c, cols.total())) return r;
	cols.carve(c->ws.get());
	for (int64_t o = 0; o < n; o += cols.chunk()) {
		const int64_t nr = cols.rows_at(o, n);
		SK_HIP(c, hipMemcpyAsync(dbc, bc + o * (int64_t)bc_stride, (size_t)nr * bc_stride, hipMemcpyHostToDevice, c->stream));
		if (assign) SK_HIP(c, hipMemcpyAsync(dassign, assign + o, (size_t)nr * 4, hipMemcpyHostToDevice, c->stream));
		SK_HIP(c, sk::census_add(c->census, dbc, bc_stride, L, nr, dassign, row_base + o, c->n_cu, c->stream));
		SK_HIP(c, hipStreamSynchronize(c->stream));
	}
	return SK_OK;
}

int sk_census_stats(sk_ctx *c, uint64_t stats[4])
{
	if (!c || !stats) return SK_ERR_INVALID;
	if (int r = bind(c)) return r;
	if (int r = census_ready(c)) return r;
	uint64_t s[4];
	SK_HIP(c, sk::census_stats(c->census, s, c->stream));
	if (s[3] != 0) return fail(c, SK_ERR_HIP, "census table overflow (%llu rows lost)", (unsigned long long)s[3]);
	stats[0] = s[0]; stats[1] = s[1]; stats[2] = s[2]; stats[3] = sk::census_slots(c->census);
	return SK_OK;
}

int sk_census_count_hist(sk_ctx *c, uint64_t hist[64])
{
	if (!c || !hist) return SK_ERR_INVALID;
	if (int r = bind(c)) return r;
	if (int r = census_ready(c)) return r;
	SK_HIP(c, sk::census_count_hist(c->census, hist, c->n_cu, c->stream));
	return SK_OK;
}

int sk_census_entries(sk_ctx *c, uint64_t min_count, sk_census_entry *out, uint64_t cap, uint64_t *total)
{
	if (!c || !total || (cap && !out)) return SK_ERR_INVALID;
	if (int r = bind(c)) return r;
	if (int r = census_ready(c)) return r;
	SK_HIP(c, sk::census_entries(c->census, min_count, reinterpret_cast<sk::CensusEntry *>(out), cap, total, c->n_cu, c->stream));
	return SK_OK;
}

}  // extern "C"
