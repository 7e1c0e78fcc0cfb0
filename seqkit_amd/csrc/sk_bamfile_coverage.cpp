// sk_bamfile_coverage.cpp — sk_bam_file_coverage (include/seqkit_hip.h) behind the front half of sk_bamfile.cpp.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "sk_bamfile.h"

using namespace bamfile;

// ---- sam coverage histogram (include/seqkit_hip.h: sk_bam_file_coverage) ---
// The front half, then the passes of sk_bamcoverage.hip.  The host's part: the references' lengths out of the header (base = their
// running sum), the caller's intervals merged per reference for the mark pass, and, from the bits that pass leaves, the target
// intervals as events of their own behind the records'.  The events — two key and two kind buffers for the sort, 24 B per event, the
// idle key buffer taking the running sums behind the sort, and the scratch of the sort and the scan — lie in the device buffer of the
// compressed file where they fit (idle once the stream is verified), else in ctx slot kKeepPassWork.
extern "C" int sk_bam_file_coverage(sk_ctx *c, const char *path, int mode, const int64_t *targets, int64_t n_targets, uint64_t hist[SK_COVERAGE_BINS],
                                    uint64_t *n_positions, uint64_t *n_dropped, int64_t *n_counted, int *handled, double info[8])
{
	Cleanup cl;
	Front fr;
	if (int r = file_call_open(c, path, "sk_bam_file_coverage", handled, info, cl, fr, [&] {
		    if (n_positions) *n_positions = 0;
		    if (n_dropped) *n_dropped = 0;
		    if (n_counted) *n_counted = 0;
		    if (!hist) return sk::ctx_fail(c, SK_ERR_INVALID, "hist = NULL");
		    memset(hist, 0, (size_t)SK_COVERAGE_BINS * 8);
		    if (mode < 0 || mode > 2) return sk::ctx_fail(c, SK_ERR_INVALID, "mode = %d", mode);
		    if (n_targets < 0 || (n_targets > 0 && !targets)) return sk::ctx_fail(c, SK_ERR_INVALID, "n_targets = %lld", (long long)n_targets);
		    return (int)SK_OK;
	    }))
		return r;
	if (!fr.ready) return SK_OK;
	const double t_stage = now_ms();
	hipStream_t st = sk::ctx_stream(c);
	const int64_t nb = fr.nb;
	if (fr.n_ref < 0) BF_LEAVE(21);
	const size_t n_ref = (size_t)fr.n_ref;
	// ---- the references' lengths
	std::vector<uint64_t> base(n_ref + 1, 0);
	for (size_t r = 0; r < n_ref; r++) base[r + 1] = base[r] + fr.refs.refs[r].l_ref;
	auto l_ref = [&](size_t r) { return (int64_t)(base[r + 1] - base[r]); };
	// ---- the caller's intervals, merged per reference (mode 1: they are the targets as they come)
	struct Iv { int64_t ref, beg, end; };
	std::vector<Iv> iv;
	if (mode != 0)
		for (int64_t k = 0; k < n_targets; k++) {
			const Iv v{targets[3 * k], std::max<int64_t>(targets[3 * k + 1], 0), targets[3 * k + 2]};
			if (v.ref >= 0 && (uint64_t)v.ref < n_ref && v.beg < v.end) iv.push_back(v);
		}
	std::vector<uint32_t> ioff;
	std::vector<int64_t> ibeg, iend;
	if (mode == 2) {
		std::sort(iv.begin(), iv.end(), [](const Iv &a, const Iv &b) { return a.ref != b.ref ? a.ref < b.ref : a.beg < b.beg; });
		std::vector<Iv> merged;
		for (const Iv &v : iv) {
			if (!merged.empty() && merged.back().ref == v.ref && v.beg <= merged.back().end) merged.back().end = std::max(merged.back().end, v.end);
			else merged.push_back(v);
		}
		iv.swap(merged);
		if (iv.size() >= 0xffffffffull) BF_LEAVE(21);
		ioff.assign(n_ref + 1, 0);
		for (const Iv &v : iv) { ioff[(size_t)v.ref + 1]++; ibeg.push_back(v.beg); iend.push_back(v.end); }
		for (size_t r = 0; r < n_ref; r++) ioff[r + 1] += ioff[r];
	}
	// ---- the small device arrays, one allocation: base, the blocks' runs, the intervals, the histogram and its totals, the bits, the words
	const size_t n_words = (n_ref + 31) / 32, n_iv = ibeg.size();
	const size_t a_base = up((n_ref + 1) * 8), a_runs = up((uint64_t)(nb + 1) * 8), a_iv = up(n_iv * 8 + 8), a_ioff = up((n_ref + 1) * 4), a_hist = up((SK_COVERAGE_BINS + 2) * 8);
	const size_t a_bits = up(n_words * 4 + 4);
	uint8_t *sm = nullptr;
	if (hipMalloc((void **)&sm, a_base + a_runs + 2 * a_iv + a_ioff + a_hist + 2 * a_bits + 256) != hipSuccess) { (void)hipGetLastError(); BF_LEAVE(21); }
	cl.dev.push_back(sm);
	uint64_t *d_base = (uint64_t *)sm, *d_runs = (uint64_t *)(sm + a_base);
	int64_t *d_ibeg = (int64_t *)(sm + a_base + a_runs), *d_iend = (int64_t *)(sm + a_base + a_runs + a_iv);
	uint32_t *d_ioff = (uint32_t *)(sm + a_base + a_runs + 2 * a_iv);
	uint64_t *d_hist = (uint64_t *)(sm + a_base + a_runs + 2 * a_iv + a_ioff), *d_tot = d_hist + SK_COVERAGE_BINS;
	uint8_t *zeroed = sm + a_base + a_runs + 2 * a_iv + a_ioff + a_hist;        // has, hit, counted, decline
	uint32_t *d_has = (uint32_t *)zeroed, *d_hit = (uint32_t *)(zeroed + a_bits);
	uint64_t *d_counted = (uint64_t *)(zeroed + 2 * a_bits);
	uint32_t *d_decline = (uint32_t *)(d_counted + 1);
	BF_HIP(hipMemsetAsync(zeroed, 0, 2 * a_bits + 256, st));
	BF_HIP(hipMemcpyAsync(d_base, base.data(), (n_ref + 1) * 8, hipMemcpyHostToDevice, st));
	if (mode == 2) {
		BF_HIP(hipMemcpyAsync(d_ioff, ioff.data(), (n_ref + 1) * 4, hipMemcpyHostToDevice, st));
		if (n_iv) {
			BF_HIP(hipMemcpyAsync(d_ibeg, ibeg.data(), n_iv * 8, hipMemcpyHostToDevice, st));
			BF_HIP(hipMemcpyAsync(d_iend, iend.data(), n_iv * 8, hipMemcpyHostToDevice, st));
		}
	}
	sk::CovArgs a{};
	a.n_ref = fr.n_ref; a.base = d_base; a.ioff = mode == 2 ? d_ioff : nullptr; a.ibeg = d_ibeg; a.iend = d_iend;
	a.bruns = d_runs; a.has = d_has; a.hit = d_hit; a.counted = (unsigned long long *)d_counted; a.decline = d_decline;
	// ---- mark: the runs, the counted records, the references' bits; the file is served or left here
	BF_HIP(sk::launch_bam_cov_mark(fr.d_out, fr.d_bend, fr.d_entry, nb, a, st));
	uint64_t R = 0, counted = 0;
	std::vector<uint32_t> has(n_words + 1, 0), hit(n_words + 1, 0);
	BF_HIP(hipMemcpyAsync(&R, d_runs + nb, 8, hipMemcpyDeviceToHost, st));
	BF_HIP(hipMemcpyAsync(&counted, d_counted, 8, hipMemcpyDeviceToHost, st));
	if (n_words) {
		BF_HIP(hipMemcpyAsync(has.data(), d_has, n_words * 4, hipMemcpyDeviceToHost, st));
		BF_HIP(hipMemcpyAsync(hit.data(), d_hit, n_words * 4, hipMemcpyDeviceToHost, st));
	}
	BF_LEAVE_DECLINED(d_decline, 0);                                    // (8 invalid record: info[5] = -38)
	// ---- the targets, cut to their references
	std::vector<uint64_t> tkey;
	std::vector<uint32_t> tkind;
	auto target = [&](size_t r, int64_t beg, int64_t end) {
		end = std::min(end, l_ref(r));
		if (beg >= end) return;
		tkey.push_back(base[r] + (uint64_t)beg); tkind.push_back(sk::kCovInsideUp);
		tkey.push_back(base[r] + (uint64_t)end); tkind.push_back(sk::kCovInsideDown);
	};
	auto bit = [](const std::vector<uint32_t> &v, size_t r) { return (v[r >> 5] >> (r & 31)) & 1u; };
	if (mode == 0) { for (size_t r = 0; r < n_ref; r++) if (bit(has, r)) target(r, 0, l_ref(r)); }
	else for (const Iv &v : iv) if (mode == 1 || bit(hit, (size_t)v.ref)) target((size_t)v.ref, v.beg, v.end);
	const uint64_t T = tkey.size(), E = 2 * R + T;
	if (E >= ((uint64_t)1 << 32)) BF_LEAVE(21);
	uint64_t tot[2] = {0, 0};
	if (T) {                                                            // (without a target no position is asked for)
		int bits = 1;
		while (bits < 64 && (base[n_ref] >> bits)) bits++;
		passmem::SortBufs sb;                                             // (idx: the events' kinds)
		BF_HIP(pass_temp(sb, E, bits, st, [&](size_t *b) { return sk::bam_cov_scan(nullptr, b, nullptr, nullptr, E, st); }));
		passmem::Layout L;
		L.add(sb.key, E * 8 + 8); L.add(sb.idx, E * 4 + 4); L.add(sb.temp, sb.temp_bytes);
		const passmem::Placement pl = passmem::place(0, L.total(), fr.fsize + 64, false);
		uint8_t *own = nullptr;
		if (!pass_memory(c, pl, own)) BF_LEAVE(21);
		char events[48];
		snprintf(events, sizeof events, "%llu events", (unsigned long long)E);
		pl.trace(fr.who, events, "the compressed file's buffer");
		L.carve(pl.scratch_at(own, fr.d_comp));
		uint32_t **kind = sb.idx;
		// ---- the events, sorted; the running sums; the histogram
		BF_HIP(sk::launch_bam_cov_emit(fr.d_out, fr.d_bend, fr.d_entry, nb, a, sb.key[0], kind[0], st));
		BF_HIP(hipMemcpyAsync(sb.key[0] + 2 * R, tkey.data(), T * 8, hipMemcpyHostToDevice, st));
		BF_HIP(hipMemcpyAsync(kind[0] + 2 * R, tkind.data(), T * 4, hipMemcpyHostToDevice, st));
		int cur = 0;
		size_t tb = sb.temp_bytes;
		BF_HIP(sk::bam_sort_pairs(sb.temp, &tb, sb.key, sb.idx, E, bits, &cur, st));
		int64_t *sums = (int64_t *)sb.key[cur ^ 1];
		tb = sb.temp_bytes;
		BF_HIP(sk::bam_cov_scan(sb.temp, &tb, kind[cur], sums, E, st));
		BF_HIP(sk::launch_bam_cov_hist(sb.key[cur], sums, E, d_hist, d_tot, sk::ctx_n_cu(c), st));
		BF_HIP(hipMemcpyAsync(hist, d_hist, (size_t)SK_COVERAGE_BINS * 8, hipMemcpyDeviceToHost, st));
		BF_HIP(hipMemcpyAsync(tot, d_tot, 16, hipMemcpyDeviceToHost, st));
		BF_HIP(hipStreamSynchronize(st));
	}
	if (n_positions) *n_positions = tot[0];
	if (n_dropped) *n_dropped = tot[1];
	if (n_counted) *n_counted = (int64_t)counted;
	*handled = 1;
	char tail[160];
	snprintf(tail, sizeof tail, "; %llu counted, %llu runs, %llu target intervals, %llu positions", (unsigned long long)counted, (unsigned long long)R,
	         (unsigned long long)(T / 2), (unsigned long long)tot[0]);
	file_call_close(fr, "mark + emit + sort + scan + histogram", t_stage, tail, info);
	return SK_OK;
}
