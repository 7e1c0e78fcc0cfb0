// sk_passmem.h — the working memory of a file call's record passes (sk_bamfile_out.cpp, sk_bamfile_coverage.cpp): the regions of one
// buffer, each stated once with its size; where the buffer lies; the trace line that says so; and the sort's double buffers.  Plain
// C++, nothing of the device: tests/cpp/passmem_test.cpp carves heap memory with it.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>

namespace passmem {

inline size_t up(uint64_t v) { return (size_t)((v + 255) & ~(uint64_t)255); }   // to the next multiple of 256

// The regions of one buffer, in the order they are added, each on a multiple of 256 bytes from its start.  add() names the pointer
// (or the pair of pointers: two regions of one size) that carve() sets once the buffer is there; total(): the buffer's bytes.
class Layout {
	struct Region { void *ptr; void (*set)(void *ptr, uint8_t *at); size_t at; };
	static const int kMax = 16;
	Region r_[kMax];
	int n_ = 0;
	size_t total_ = 0;

public:
	template <class T> void add(T *&p, uint64_t bytes)
	{
		if (n_ == kMax) abort();
		r_[n_++] = Region{&p, [](void *ptr, uint8_t *at) { *(T **)ptr = (T *)at; }, total_};
		total_ += up(bytes);
	}
	template <class T> void add(T *(&p)[2], uint64_t bytes) { add(p[0], bytes); add(p[1], bytes); }
	size_t total() const { return total_; }
	void carve(uint8_t *base) const { for (int i = 0; i < n_; i++) r_[i].set(r_[i].ptr, base + r_[i].at); }
};

// Where a call's memory lies.  `kept` bytes are read by the windows later, `scratch` bytes only by the call's own passes: the scratch
// goes into a buffer that is idle by then (`borrow_bytes` of it; the compressed file's) when it fits there and the caller lets it,
// else behind the kept head in the call's own buffer, which is own_bytes() long (0: the call needs none).  The kept head is always at
// the start of the own buffer.
struct Placement {
	size_t kept = 0, scratch = 0;
	bool borrowed = false;
	size_t own_bytes() const { return kept + (borrowed ? 0 : scratch); }
	uint8_t *scratch_at(uint8_t *own, uint8_t *borrow) const { return borrowed ? borrow : own + kept; }
	// "<who>: [<prefix>, ]<scratch> bytes of scratch in <the borrowed buffer's name | its own buffer>", under SK_BAMFILE_TRACE
	void trace(const char *who, const char *prefix, const char *borrowed_name) const
	{
		if (!getenv("SK_BAMFILE_TRACE")) return;
		fprintf(stderr, "%s: %s%s%zu bytes of scratch in %s\n", who, prefix, *prefix ? ", " : "", scratch, borrowed ? borrowed_name : "its own buffer");
	}
};
inline Placement place(size_t kept, size_t scratch, uint64_t borrow_bytes, bool never_borrow)
{
	Placement p;
	p.kept = up(kept); p.scratch = scratch;
	p.borrowed = !never_borrow && borrow_bytes >= scratch;
	return p;
}

// The double buffers of a key-value sort (sk_internal.h: bam_sort_pairs swaps between them) and the scratch bytes the sort and the
// call's scans ask for: want() takes each one's answer.
struct SortBufs {
	uint64_t *key[2] = {nullptr, nullptr};
	uint32_t *idx[2] = {nullptr, nullptr};
	void *temp = nullptr;
	size_t temp_bytes = 0;
	void want(size_t bytes) { temp_bytes = std::max(temp_bytes, bytes); }
};

}  // namespace passmem
