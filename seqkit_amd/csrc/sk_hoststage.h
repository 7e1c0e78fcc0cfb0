// sk_hoststage.h — what a host-pointer entry point (sk_capi_*.cpp; sk_ctx.h: ChunkPipe) stages through the ctx's workspace: the call's columns, each stated
// once with its bytes per row, its direction and the caller's pointer.  From that one list: the rows of a chunk, the bytes of a
// workspace half, where every column's region lies in it, and what is copied in before the launch and out behind it.  Plain C++,
// nothing of the device: tests/cpp/hoststage_test.cpp carves heap memory with it.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include "sk_passmem.h"

namespace hoststage {

using passmem::up;

// Rows per chunk: the budget in whole granules, one granule at least; a batch below that is one chunk, n rounded up to the granule.
inline int64_t rows_per_chunk(uint64_t budget_rows, int64_t granule, int64_t n)
{
	int64_t chunk = (int64_t)(budget_rows / (uint64_t)granule) * granule;
	if (chunk < granule) chunk = granule;
	if (chunk > n) chunk = (n + granule - 1) / granule * granule;
	return chunk;
}

enum Dir { kIn, kOut, kDev };     // copied in before the launch; copied out behind it; only carved (the kernel's own, or a column this mode does not read)

// The columns of one call, in the order they are carved and copied.  add() names the device pointer that carve() sets.  A kIn / kOut
// column whose host pointer is NULL is absent: it counts in per_row() (the budgets count it), has no region and no copy, and its
// device pointer is set to NULL.  plan() fixes the rows of a chunk: `lanes` halves of half() bytes, then a tail every chunk shares.
class Stage {
	struct Col { void *ptr; void (*set)(void *ptr, uint8_t *at); uint8_t *host; uint64_t row_bits; Dir dir; size_t at; };
	static const int kMax = 16;
	Col c_[kMax];
	int n_ = 0, lanes_ = 2;
	int64_t chunk_ = 0;
	size_t half_ = 0, tail_ = 0;
	static bool absent(const Col &c) { return c.dir != kDev && !c.host; }
	static size_t bytes(const Col &c, int64_t rows) { return (size_t)(((uint64_t)rows * c.row_bits + 7) >> 3); }

public:
	template <class T> void add_bits(T *&dev, uint64_t row_bits, Dir dir, const void *host = nullptr)
	{
		if (n_ == kMax) abort();
		c_[n_++] = Col{&dev, [](void *ptr, uint8_t *at) { *(T **)ptr = (T *)at; }, (uint8_t *)host, row_bits, dir, 0};
	}
	template <class T> void add(T *&dev, uint64_t row_bytes, Dir dir, const void *host = nullptr) { add_bits(dev, row_bytes * 8, dir, host); }

	size_t per_row() const { uint64_t b = 0; for (int i = 0; i < n_; i++) b += c_[i].row_bits; return (size_t)(b >> 3); }
	int64_t rows_for_bytes(uint64_t budget_bytes, int64_t granule, int64_t n) const { return rows_per_chunk(budget_bytes / (per_row() ? per_row() : 1), granule, n); }

	void plan(int64_t chunk, size_t tail = 0, int lanes = 2)
	{
		chunk_ = chunk; lanes_ = lanes; tail_ = up(tail); half_ = 0;
		for (int i = 0; i < n_; i++) { c_[i].at = half_; if (!absent(c_[i])) half_ += up(bytes(c_[i], chunk)); }
	}
	int64_t chunk() const { return chunk_; }
	int64_t rows_at(int64_t r0, int64_t n) const { return n - r0 < chunk_ ? n - r0 : chunk_; }
	size_t half() const { return half_; }
	size_t tail_at() const { return (size_t)lanes_ * half_; }
	size_t total() const { return tail_at() + tail_; }

	void carve(uint8_t *half_base) const { for (int i = 0; i < n_; i++) c_[i].set(c_[i].ptr, absent(c_[i]) ? nullptr : half_base + c_[i].at); }
	// f(offset in the half, bytes): every region as `rows` rows fill it
	template <class F> void each_region(int64_t rows, F f) const { for (int i = 0; i < n_; i++) if (!absent(c_[i])) f(c_[i].at, bytes(c_[i], rows)); }
	// f(offset in the half, the caller's pointer at row r0, bytes): the copies of one direction for rows [r0, r0 + nr)
	template <class F> void each_copy(Dir dir, int64_t r0, int64_t nr, F f) const
	{
		for (int i = 0; i < n_; i++) if (c_[i].dir == dir && c_[i].host) f(c_[i].at, c_[i].host + (((uint64_t)r0 * c_[i].row_bits) >> 3), bytes(c_[i], nr));
	}
};

}  // namespace hoststage
