// sam_pairing.h — what `sam to` (sam_reads.cpp) does with the windows of the two file calls that serve it, apart from the device and the
// sinks, so that a stand-alone program can run it (tests/cpp/pairing_test.cpp): the loop over the windows of sk_bam_file_pairs, whose
// texts arrive paired and in output order, and the pairing of src/sam_to_fastq.rs:113-137 on the host over the windows of
// sk_bam_file_reads, whose texts arrive in file order.  `next(&w)` fills the next window (w.n == 0: the end); `write(stream, p, n)`
// takes n bytes for stream 0 (first mates), 1 (last mates) or 2 (the single stream).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/seqkit_hip.h"

namespace pairing {

template <class Next, class Write>
inline void write_pair_windows(Next next, Write write)
{
	sk_bam_pairs_window w;
	for (;;) {
		next(&w);
		if (w.n == 0) break;
		write((int)w.stream, reinterpret_cast<const char *>(w.text), (size_t)w.bytes);
	}
}

// the same loop over the windows of sk_bam_file_pairs_gz, whose bytes are finished BGZF members: `write(stream, p, n)` takes them as they are
template <class Next, class Write>
inline void write_member_windows(Next next, Write write)
{
	sk_bam_pairs_gz_window w;
	for (;;) {
		next(&w);
		if (w.n == 0) break;
		write((int)w.stream, w.bgzf, (size_t)w.bytes);
	}
}

// The reference's HashMap<Box<str>, Box<str>> (:97-98) over the device path's records, its leftovers listed in insertion order: a flat open-addressing table keyed by the device's 64-bit qname key (names compared
// byte for byte on a key match), the pending names and texts in an arena that is compacted when most of it is dead.  Same semantics:
// a second insert under a name replaces the text and keeps its order; after a removal a new insert takes a new order number.
struct PendingTexts {
	struct Slot { uint64_t key, order, at; uint32_t name_len, text_len; bool used; };
	std::vector<Slot> slots = std::vector<Slot>(1024);
	size_t count = 0;
	uint64_t next = 0, live = 0;
	std::vector<char> arena;                                        // name then text, per entry
	size_t mask() const { return slots.size() - 1; }
	int64_t find(uint64_t key, const uint8_t *name, uint32_t len) const
	{
		for (size_t i = key & mask();; i = (i + 1) & mask()) {
			const Slot &e = slots[i];
			if (!e.used) return -1;
			if (e.key == key && e.name_len == len && memcmp(arena.data() + e.at, name, len) == 0) return (int64_t)i;
		}
	}
	const char *text(const Slot &e) const { return arena.data() + e.at + e.name_len; }
	void put(Slot &e, const uint8_t *name, uint32_t len, const uint8_t *t, uint32_t tl)
	{
		e.at = arena.size(); e.name_len = len; e.text_len = tl;
		arena.insert(arena.end(), name, name + len);
		arena.insert(arena.end(), t, t + tl);
		live += (uint64_t)len + tl;
	}
	void insert(uint64_t key, const uint8_t *name, uint32_t len, const uint8_t *t, uint32_t tl)
	{
		const int64_t f = find(key, name, len);
		if (f >= 0) { Slot &e = slots[(size_t)f]; live -= (uint64_t)e.name_len + e.text_len; put(e, name, len, t, tl); }
		else {
			if ((count + 1) * 2 > slots.size()) grow();
			size_t i = key & mask();
			while (slots[i].used) i = (i + 1) & mask();
			Slot &e = slots[i];
			e.used = true; e.key = key; e.order = next++;
			put(e, name, len, t, tl);
			count++;
		}
		if (arena.size() > ((size_t)64 << 20) && arena.size() > 4 * live) compact();
	}
	void erase(size_t i)                                            // backward-shift deletion (linear probing)
	{
		live -= (uint64_t)slots[i].name_len + slots[i].text_len;
		slots[i].used = false;
		count--;
		for (size_t j = (i + 1) & mask(); slots[j].used; j = (j + 1) & mask()) {
			const size_t home = slots[j].key & mask();
			// slot j may move to the hole at i when its home does not lie cyclically in (i, j]
			if (((j - home) & mask()) >= ((j - i) & mask())) { slots[i] = slots[j]; slots[j].used = false; i = j; }
		}
	}
	void grow()
	{
		std::vector<Slot> old(slots.size() * 2);
		old.swap(slots);
		for (const Slot &e : old)
			if (e.used) { size_t i = e.key & mask(); while (slots[i].used) i = (i + 1) & mask(); slots[i] = e; }
	}
	void compact()
	{
		std::vector<char> a;
		a.reserve((size_t)live + (1 << 20));
		for (Slot &e : slots)
			if (e.used) { const uint64_t at = a.size(); a.insert(a.end(), arena.begin() + (ptrdiff_t)e.at, arena.begin() + (ptrdiff_t)(e.at + e.name_len + e.text_len)); e.at = at; }
		arena.swap(a);
	}
	std::vector<const Slot *> in_order() const
	{
		std::vector<const Slot *> v;
		v.reserve(count);
		for (const Slot &e : slots) if (e.used) v.push_back(&e);
		std::sort(v.begin(), v.end(), [](const Slot *a, const Slot *b) { return a->order < b->order; });
		return v;
	}
};

template <class Next, class Write>
inline void pair_on_host(Next next, Write write)
{
	PendingTexts reads_1, reads_2;
	sk_bam_reads_window w;
	for (;;) {
		next(&w);
		if (w.n == 0) break;
		for (int64_t j = 0; j < w.n; j++) {
			const char *t = reinterpret_cast<const char *>(w.text + w.text_off[j]);
			const uint32_t tl = (uint32_t)(w.text_off[j + 1] - w.text_off[j]);
			const uint8_t kind = w.kind[j];
			if (kind == 0) { write(2, t, tl); continue; }                                                        // :114-115
			const uint8_t *nm = w.names + w.name_off[j];
			const uint32_t nl = w.name_off[j + 1] - w.name_off[j];
			PendingTexts &mates = kind == 1 ? reads_2 : reads_1, &mine = kind == 1 ? reads_1 : reads_2;      // :116-130
			const int64_t f = mates.find(w.key[j], nm, nl);
			if (f >= 0) {
				const PendingTexts::Slot &e = mates.slots[(size_t)f];
				if (kind == 1) { write(0, t, tl); write(1, mates.text(e), e.text_len); }
				else { write(0, mates.text(e), e.text_len); write(1, t, tl); }
				mates.erase((size_t)f);
			} else mine.insert(w.key[j], nm, nl, reinterpret_cast<const uint8_t *>(t), tl);
		}
	}
	for (const PendingTexts *m : {&reads_1, &reads_2})                                                          // :133-137
		for (const PendingTexts::Slot *e : m->in_order()) write(2, m->text(*e), e->text_len);
}

}  // namespace pairing
